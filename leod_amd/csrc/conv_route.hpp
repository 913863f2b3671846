// Routing of the dense convolutions (k_conv.hip): one description (ConvProb), one router (conv_route).  The five entry points
// (leod_conv_nhwc_fwd / _dgrad / _wgrad, leod_stem_conv_fwd / _wgrad), the grouped 3x3 calls, the workspace queries and leod_conv_route all
// go through conv_route; launch_conv<E> (k_conv.hip) holds the only switch that launches.  Same shape as LinearProb -> linear_route ->
// launch_linear<E> in linear_common.hpp.
#pragma once
#include "gemm16.hpp"
#include "conv3.hpp"
#include "stem.hpp"

enum ConvEntry : int { CE_FWD = 0, CE_DGRAD, CE_WGRAD, CE_STEM_FWD, CE_STEM_WGRAD, CE_COUNT };
// the flags of leod_conv_route: what the entry points read off their pointers
enum : int { CF_BIAS = 1, CF_COLSTATS = 2, CF_BN = 4, CF_PACK = 8, CF_WS = 16, CF_DBIAS = 32, CF_ACCUMULATE = 64, CF_U8 = 128, CF_ALIGN4 = 256 };

// A convolution problem, fully described.  Sizes as the entry takes them: H, W the conv's INPUT map (the dgrad's dx, the stem's stored
// frame), N output channels, Hp x Wp the padded frame of the stem entries (= H x W elsewhere).
struct ConvProb {
    int entry;                      // ConvEntry
    int B, H, W, Cin, N, ks, stride, pad, Hp, Wp;
    bool bias, colstats, bn, pack, ws, dbias, accumulate;     // bias | colstats | eval BatchNorm | wpack | ws | dbias given; dx +=
    bool u8, align4;                // stem input: uint8 voxels | address a multiple of 4
    int Ho() const { return (Hp + 2 * pad - ks) / stride + 1; }
    int Wo() const { return (Wp + 2 * pad - ks) / stride + 1; }
    int M() const { return entry == CE_DGRAD ? B * H * W : B * Ho() * Wo(); }                       // rows of the contraction's output
    int K() const { return ks * ks * (entry == CE_DGRAD ? N : Cin); }                               // its length (wgrad: columns of dW)
};
static inline ConvProb conv_prob(int entry, int B, int H, int W, int Cin, int N, int ks, int stride, int pad, int flags, int Hp = 0, int Wp = 0) {
    const bool stem = entry == CE_STEM_FWD || entry == CE_STEM_WGRAD;
    ConvProb p{};
    p.entry = entry; p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.N = N; p.ks = ks; p.stride = stride; p.pad = pad;
    p.Hp = stem && Hp > 0 ? Hp : H; p.Wp = stem && Wp > 0 ? Wp : W;
    p.bias = flags & CF_BIAS; p.colstats = flags & CF_COLSTATS; p.bn = flags & CF_BN; p.pack = flags & CF_PACK; p.ws = flags & CF_WS;
    p.dbias = flags & CF_DBIAS; p.accumulate = flags & CF_ACCUMULATE; p.u8 = flags & CF_U8; p.align4 = flags & CF_ALIGN4;
    return p;
}

// Route codes (include/leod_hip.h lists them for callers).  A code names kernel template, instantiation and weight-operand source; it is read
// together with the entry (17448 is gemm_lds_kernel<4, 48> on the im2col loader of the forward, or on the transposed one of the dgrad).
//   110 / 120              conv3s1_kernel, stride 1 / 2: direct 3x3 from the LDS halo, per-tap 16-bit weight pack (110: also the stride-1 dgrad)
//   220                    conv3s2_dgrad_kernel: direct stride-2 dgrad, per-tap bf16 weight pack
//   300 + c                wgradw_kernel configuration c (1x1, pixel rows)                     } the codes of leod_linear_wgrad_route
//   400 + 10 TN + 4        wgrad16_kernel<TN, 4> on pixel rows (1x1)                           }
//   500                    direct 3x3 weight gradient into the workspace + reduce (conv3_wgrad_launch)
//   600 + NT / 610 + NT    stem forward: stem_fwd_bf16_kernel<NT> (bf16 patch, NT 2 | 3) / stem_u8_fwd_kernel<NT> (uint8 patch, NT 1..4)
//   620 + NT / 630 + NT    stem weight gradient: stem_wgrad_bf16_kernel (NT 1..3; 4 = two slices of <2>) / stem_u8_wgrad_kernel<NT>
//   700 / 800 / 900 + 10 TN + 4     wgrad16_kernel<TN, 4> on the im2col loader XConvNHWC / XStemNCHW<uint8> / XStemNCHW<float>
//   1x1 forward and dgrad are Linear layers over the pixel rows, with the codes of leod_linear_route -- except that the wide code carries
//   the NT digit here (3043 where leod_linear_route says 3003): launch_conv takes every template argument from the code
//   3000 + 10 NT + NTW     gemm_wide_bf16_kernel<NTW> (RG_WIDE; NT: the column tiling the weight loader is built with)
//   4000 / 5000 + 100 NT + KCH      gemm_lds_kernel<NT, KCH> on the two-phase / plain row loader (RG_TWO_PHASE / RG_PLAIN)
//   6000 + 10 NT + KS      gemm16_kernel<NT, KS> (register-direct; KS = 4: K split over the waves)
//   ks > 1 and the stem's generic path, 10000 L + form:  L = 1 im2col of an NHWC map, 2 parity classes of a stride-2 dgrad ("live taps"),
//                                                        3 / 4 im2col of the NCHW uint8 / fp32 frame (stem)
//   L7000 + 100 NT + KCH   gemm_lds_kernel<NT, KCH> on the K-contiguous fp32 weight pack (conv_pack_kernel)
//   L8000 + 100 NT + KCH   gemm_lds_kernel<NT, KCH> on the weights in their native layout
//   L9000 + 10 NT + KS     gemm16_kernel<NT, KS> on the weights in their native layout
//   0                      nothing to do (no rows);    < 0    LEOD_ERR_*: what the entry returns
enum : int { CR_DIRECT3 = 100, CR_DIRECT3_S2_DGRAD = 220, CR_WGRADW = 300, CR_WGRAD16 = 400, CR_WGRAD3 = 500, CR_STEM_FWD16 = 600, CR_STEM_FWD8 = 610,
             CR_STEM_WGRAD16 = 620, CR_STEM_WGRAD8 = 630, CR_WGRAD16_CONV = 700, CR_WGRAD16_STEM8 = 800, CR_WGRAD16_STEMF = 900, CR_GEMM16 = 6000,
             CR_LOADER = 10000, CR_LDS_PACKED = 7000, CR_LDS_NATIVE = 8000, CR_REG_NATIVE = 9000 };
static inline bool conv_route_reads_pack(int route) { return route == CR_DIRECT3 + 10 || route == CR_DIRECT3 + 20 || route == CR_DIRECT3_S2_DGRAD ||
                                                             (route >= CR_LOADER && route % CR_LOADER / 1000 == CR_LDS_PACKED / 1000); }

// implicit GEMM [M, K] x [K, nout] on loader family L: LDS-staged for large M (coalesced operands; on the packed weights when a pack buffer
// is offered), else register-direct
static inline int conv_gemm_route(int L, bool pack, int M, int K, int nout) {
    const int nt = pick_nt(nout), nbn = cdiv(nout, 16 * nt);
    if (!use_gemm_lds(M, nbn)) return L * CR_LOADER + CR_REG_NATIVE + 10 * nt + (gemm16_ksplit(M, K, nbn) ? 4 : 1);
    return L * CR_LOADER + (pack ? CR_LDS_PACKED : CR_LDS_NATIVE) + 100 * nt + gemm_lds_kch(K);
}
// 1x1 / stride 1: a Linear layer over the pixel rows (trans: the dgrad reads W transposed)
static inline int conv_rows_route(bool trans, int M, int K, int nout) {
    const int nt = pick_nt(nout), nbn = cdiv(nout, 16 * nt);
    if (!use_gemm_lds(M, nbn)) return CR_GEMM16 + 10 * nt + (gemm16_ksplit(M, K, nbn) ? 4 : 1);
    const int kind = rows_gemm_kind(M, K, nout, nt, trans, false, FMT_F32, false, false, false, false);
    return kind < RG_TWO_PHASE ? RG_WIDE + 10 * nt + (kind - RG_WIDE) : kind + 100 * nt + gemm_lds_kch(K);
}
// weight-gradient GEMM dW[N][K] on wgrad16_kernel<TN, 4>: base + 10 TN + 4
static inline int conv_wgrad16_route(int base, int M, int N, int K) {
    if (M <= 0) return 0;
    if (!wgrad_rows16b_ok(N, N, K)) return LEOD_ERR_ARG;
    return base + 10 * (N % 48 == 0 ? 3 : N % 64 == 0 ? 4 : N % 32 == 0 ? 2 : 1) + 4;
}
// the LDS-resident uint8 patch kernels of the stem (k_conv.hip; dedicated to the RVT stem geometry): patch_ok = the patch fits their staging
static inline bool stem_u8_supported(const ConvProb& p, bool patch_ok) {
    return p.stride == 4 && p.pad == 3 && p.N <= 64 && !(p.N & 15) && !(p.W & 3) && patch_ok && p.align4 && ((long)p.Cin * p.H * p.W) % 4 == 0;
}

// The one routing function of the dense convolutions: the described problem -> the kernel that runs it, as a route code.  It launches nothing
// and reads no device memory.  Precision: every predicate below reads leod_precision() (the same in and out of a LeodFwdScope), none reads
// leod_opfmt(); the operand format of a forward launch (bf16 / fp16) is picked by the launchers and is not part of the code.
static int conv_route(const ConvProb& p) {
    const int B = p.B, H = p.H, W = p.W, Cin = p.Cin, N = p.N, ks = p.ks, stride = p.stride, pad = p.pad;
    if (stride <= 0) return LEOD_ERR_ARG;            // (before any output size is computed: the queries must not fault)
    const bool bf = leod_precision() == 1, k1 = ks == 1 && stride == 1 && pad == 0, k3 = ks == 3 && pad == 1;
    switch (p.entry) {
    case CE_FWD: {
        if (Cin & 3) return LEOD_ERR_ARG;
        // PAFPN / head 3x3 convs in the 16-bit modes: direct convolution from an LDS-resident input halo (k_conv3.hip)
        // (eval mode: the folded BatchNorm + SiLU run in the direct kernel's row epilogue -- the pseudo-label pass spent a third of its
        // device time in the implicit-GEMM form of these convs)
        const bool direct = k3 && !p.bias && !(p.bn && p.colstats) && p.pack;
        if (direct && stride == 1 && conv3s1_supported(H, W, Cin, N)) return CR_DIRECT3 + 10;
        if (direct && stride == 2 && conv3s2_fwd_supported(B, H, W, Cin, N)) return CR_DIRECT3 + 20;
        if (k1) return conv_rows_route(false, p.M(), p.K(), N);
        // scratch given: the weights are repacked K-contiguous first (N*Cin*ks*ks floats, a few microseconds), then the B operand is a
        // plain row-major matrix like a Linear weight
        return conv_gemm_route(1, p.pack, p.M(), p.K(), N);
    }
    case CE_DGRAD: {
        if (N & 3) return LEOD_ERR_ARG;
        const int M = p.M();
        if (k3 && stride == 1 && p.pack && conv3s1_supported(H, W, N, Cin)) return CR_DIRECT3 + 10;
        if (k3 && stride == 2 && p.pack && conv3s2_dgrad_supported(H, W, Cin, N)) return CR_DIRECT3_S2_DGRAD;
        const int Q = B * (H / 2) * (W / 2);
        if (k3 && stride == 2 && !(H & 1) && !(W & 1) && Q % 16 == 0) {
            // live-tap formulation: rows grouped by input parity class, 2.25 taps per pixel on average instead of 9
            if (Q % 128 == 0) return conv_gemm_route(2, p.pack, M, 4 * N, Cin);     // a (64|128)-row workgroup must not mix classes
            const int nt = pick_nt(Cin), nbn = cdiv(Cin, 16 * nt);
            return 2 * CR_LOADER + CR_REG_NATIVE + 10 * nt + (gemm16_ksplit(M, 4 * N, nbn) ? 4 : 1);
        }
        if (k1) return conv_rows_route(true, M, p.K(), Cin);
        return conv_gemm_route(1, p.pack, M, p.K(), Cin);
    }
    case CE_WGRAD: {
        const int M = p.M(), K = p.K();
        if (k1) {
            // 1 x 1 convs are Linear layers over the pixel rows: the wave-tiled weight gradient of the Linear layers for the large maps in
            // bf16 mode (22 -> 15, 28 -> 23, 18 -> 12 us on the PAFPN shapes; fp32 mode: 24 -> 28, 22 -> 26 us, not used)
            if (bf && use_wgradw(M)) {
                if (!wgrad_rows16b_ok(N, N, K)) return LEOD_ERR_ARG;
                return CR_WGRADW + wgradw_cfg(XRows{nullptr, (long)Cin, nullptr, nullptr, nullptr, nullptr, 0, 0}, M, N, K);
            }
            return conv_wgrad16_route(CR_WGRAD16, M, N, K);
        }
        if (k3 && !p.dbias && p.ws && conv3_wgrad_supported(H, W, Cin, N, stride)) return CR_WGRAD3;
        return conv_wgrad16_route(CR_WGRAD16_CONV, M, N, K);
    }
    case CE_STEM_FWD: {
        if ((Cin * ks * ks) & 3) return LEOD_ERR_ARG;
        if (ks < 1 || ks > 15) return LEOD_ERR_UNSUPPORTED;
        const int nt16 = N / 16 >= 1 && N / 16 <= 3 ? N / 16 : 4;
        if (ks == 7 && p.u8 && bf && stem_fwd_bf16_supported(p.align4, Cin, H, W, N, stride, pad)) return CR_STEM_FWD16 + nt16;     // k_stem.hip: bf16 patch, weights resident in LDS
        // LDS-resident uint8 patch kernel; anything else takes the generic path
        if (ks == 7 && p.u8 && stem_u8_supported(p, Cin * 19 * 72 <= 60000)) return CR_STEM_FWD8 + nt16;
        return conv_gemm_route(p.u8 ? 3 : 4, false, p.M(), Cin * ks * ks, N);
    }
    case CE_STEM_WGRAD: {
        if (ks < 1 || ks > 15) return LEOD_ERR_UNSUPPORTED;
        const int nt16 = N / 16 >= 1 && N / 16 <= 3 ? N / 16 : 4;
        if (ks == 7 && p.u8 && bf && stem_wgrad_bf16_supported(p.align4, Cin, H, W, N, stride, pad)) return CR_STEM_WGRAD16 + nt16;    // k_stem.hip
        if (ks == 7 && p.u8 && stem_u8_supported(p, Cin * 19 * 18 <= 27 * 256)) return CR_STEM_WGRAD8 + nt16;
        return conv_wgrad16_route(p.u8 ? CR_WGRAD16_STEM8 : CR_WGRAD16_STEMF, p.M(), N, Cin * ks * ks);
    }
    }
    return LEOD_ERR_ARG;
}

// n problems of one (Cin -> N) 3x3 / stride-1 / pad-1 geometry can share a launch when there are 1..8 of them and every member routes to
// `want` (the direct kernel of the entry; B does not enter those routes)
static inline bool conv_group_routes_to(int want, int entry, int flags, int n, const int* H, const int* W, int Cin, int N) {
    if (n < 1 || n > 8 || !H || !W) return false;
    for (int k = 0; k < n; ++k)
        if (conv_route(conv_prob(entry, 1, H[k], W[k], Cin, N, 3, 1, 1, flags)) != want) return false;
    return true;
}
