// Token-row contractions of the RVT backbone: weight gradients of the Linear layers and their per-stream workspace.  All tensors channels-last ("rows" = tokens of an NHWC map).
// C-ABI declared in include/leod_hip.h.
#include "linear_common.hpp"
#include "wgrad_bf16.hpp"
#include "wgrad_dma.hpp"

// Workspace of the weight-gradient kernels for launches on `stream` (wgrad_bf16.hpp: partial tiles, leod_workspace_bytes() bytes, 16-byte
// aligned, caller-owned and alive until replaced; ws == NULL withdraws it).
LEOD_API long leod_workspace_bytes() { return (long)kWgwScratchBytes; }
LEOD_API int leod_set_workspace(void* ws, long bytes, hipStream_t stream) {
    if (ws && (bytes <= 0 || (reinterpret_cast<uintptr_t>(ws) & 15))) return LEOD_ERR_ARG;
    wgrad_wide_register_scratch(stream, ws, (size_t)(bytes > 0 ? bytes : 0));
    return LEOD_OK;
}

// Profiling aid (LEOD_FAMILY_MARKERS=1, used by the PMC passes of tools/pmc_bench_traffic.sh only): one-thread marker kernels in front of
// and behind every launch of the roofline family, so that tools/roofline_traffic.py sums the HBM counters of exactly the dispatches the
// event probe of bench.py brackets (the kernel names alone do not separate the Linear weight gradients from the 1x1-conv ones).
__global__ void leod_family_marker_kernel(int begin) { (void)begin; }
struct FamilyMarker {
    hipStream_t s; bool on;
    explicit FamilyMarker(hipStream_t st) : s(st) {
        static const bool env = getenv("LEOD_FAMILY_MARKERS") && atoi(getenv("LEOD_FAMILY_MARKERS"));
        on = env;
        if (on) hipLaunchKernelGGL(leod_family_marker_kernel, dim3(1), dim3(1), 0, s, 1);
    }
    ~FamilyMarker() { if (on) hipLaunchKernelGGL(leod_family_marker_kernel, dim3(1), dim3(1), 0, s, 0); }
};

// The one routing function of the Linear weight gradients: the fully described problem -> the kernel that runs it, as a route code.
// LDS-DMA kernel (wgrad_dma.hpp), then the register-staged wide kernel (wgrad_bf16.hpp), then wgradw_kernel, then the tile ladder of
// wgrad16_kernel.  It launches nothing and reads no device memory (of xl only the mode, the strides, K1 and WHETHER stats / x2 are set):
//   100 + T           LDS-DMA kernel on T x T blocks of 16 columns (T = 4, 6, 8)
//   200 + combo       wide kernel, combo 1..16 of wgrad_wide_combo
//   300 + cfg         wgradw_kernel, cfg 1..5 of wgradw_cfg
//   400 + 10 TN + TK  wgrad16_kernel<TN, TK>
//   0                 M <= 0: nothing to launch (LEOD_OK);   < 0: LEOD_ERR_*
// dma = false: the LDS-DMA kernel is not available (launch_linear_wgrad: its workspace could not be had) -- where the problem goes then.
enum : int { WGR_NONE = 0, WGR_DMA = 100, WGR_WIDE = 200, WGR_WGRADW = 300, WGR_LADDER = 400 };
static int wgrad_route(const XRows& xl, long lddy, int dyfmt, int M, int N, int K, bool dma = true) {
    const int xm = xl.x_mode();
    const bool x16 = xm == XM_BF16 || xm == XM_F16; // 16-bit rows (the attention output; fp16 in precision mode 16f): the bf16-MFMA kernels only
    if (x16 && (xl.stats || xl.x2)) return LEOD_ERR_ARG;
    if (dma && wgrad_dma_ok(xl, lddy, M, N, K, dyfmt)) return WGR_DMA + wgd_tile(N, K);
    if (use_wgrad_wide(xl, lddy, M, N, K, dyfmt)) return WGR_WIDE + wgrad_wide_combo(xl, N, K, dyfmt);
    if (x16) return LEOD_ERR_UNSUPPORTED;
    if (M <= 0) return WGR_NONE;
    if (!wgrad_rows16b_ok(lddy, N, K)) return LEOD_ERR_ARG;
    const bool f32 = leod_precision() != 1;         // 16-bit tensors exist in the 16-bit precision modes only
    if (use_wgradw(M)) return (f32 && (dyfmt || xm == XM_GELU16)) ? LEOD_ERR_ARG : WGR_WGRADW + wgradw_cfg(xl, M, N, K);
    if (f32 && dyfmt) return LEOD_ERR_ARG;
    if (N % 48 == 0 && K % 48 == 0) return WGR_LADDER + 33;
    // the fp16 pre-activation had an entry point of its own, whose ladder ended here; it is reachable (any M < 8192 with widths that
    // are not multiples of 48), so that mode keeps its tile
    if (xm == XM_GELU16) return WGR_LADDER + 44;
    if (N % 32 == 0 && K % 32 == 0 && (N % 64 || K % 64)) return WGR_LADDER + 22;
    if (N >= 64 && K >= 64) return WGR_LADDER + 44;
    if (K >= 64) return WGR_LADDER + 14;
    if (N >= 64) return WGR_LADDER + 41;
    return WGR_LADDER + 11;
}
// ... and the switch that launches what wgrad_route decided
static int launch_linear_wgrad(int route, const float* dy, long lddy, int dyfmt, const XRows& xl, float* dW, float* dbias, int M, int N, int K,
                               hipStream_t stream) {
    if (route <= 0) return route;                   // WGR_NONE == LEOD_OK
    const long ldw = (long)K;
    if (route < WGR_WIDE) {
        // the one condition wgrad_route cannot know: no workspace is registered for the stream and none can be allocated (the stream is
        // being captured, or hipMalloc failed) -- nothing was launched, and the problem takes the route it has without this kernel
        const int rc = launch_wgrad_dma(route - WGR_DMA, dy, lddy, xl, dW, ldw, dbias, M, N, K, stream, dyfmt);
        return rc != LEOD_ERR_UNSUPPORTED ? rc : launch_linear_wgrad(wgrad_route(xl, lddy, dyfmt, M, N, K, false), dy, lddy, dyfmt, xl, dW, dbias, M, N, K, stream);
    }
    if (route < WGR_WGRADW) return launch_wgrad_wide(route - WGR_WIDE, dy, lddy, xl, dW, ldw, dbias, M, N, K, stream);
    if (route < WGR_LADDER) return launch_wgradw_as(route - WGR_WGRADW, dy, lddy, xl, dW, ldw, dbias, M, N, K, stream, dyfmt);
    switch (route - WGR_LADDER) {
        case 33: return launch_wgrad16<3, 3>(dy, lddy, xl, dW, ldw, dbias, M, N, K, stream, dyfmt);
        case 22: return launch_wgrad16<2, 2>(dy, lddy, xl, dW, ldw, dbias, M, N, K, stream, dyfmt);
        case 44: return launch_wgrad16<4, 4>(dy, lddy, xl, dW, ldw, dbias, M, N, K, stream, dyfmt);
        case 14: return launch_wgrad16<1, 4>(dy, lddy, xl, dW, ldw, dbias, M, N, K, stream, dyfmt);
        case 41: return launch_wgrad16<4, 1>(dy, lddy, xl, dW, ldw, dbias, M, N, K, stream, dyfmt);
        case 11: return launch_wgrad16<1, 1>(dy, lddy, xl, dW, ldw, dbias, M, N, K, stream, dyfmt);
    }
    return LEOD_ERR_ARG;
}

// what leod_linear_wgrad takes at all: the (dy_fmt, x_fmt) vocabulary and which of stats / ln_w + ln_b / x2 go with which x_fmt
static bool wgrad_formats_ok(int dy_fmt, int x_fmt, bool has_stats, bool has_ln_wb, bool has_x2) {
    if ((dy_fmt != 0 && dy_fmt != 1) || !xm_valid(x_fmt)) return false;
    if ((x_fmt == XM_LN) != has_stats || (x_fmt == XM_LN && !has_ln_wb)) return false;
    if (x_fmt == XM_GELU16 && (has_x2 || dy_fmt)) return false;             // fp32 dy, no concat: all that the former entry of this mode took
    return true;
}

// dW[N,K] += dy[M,N]^T @ X[M,K] ; dbias[N] += colsum(dy).  dy_fmt: 0 fp32 rows, 1 bf16 rows.  x_fmt (XMode): what x holds and how X comes
// from it -- 0 fp32 rows, 1 fp32 rows through LayerNorm (stats + ln_w + ln_b), 2 fp16 pre-activation through GELU, 3 bf16 rows, 4 fp16
// rows; x_fmt 0 / 1 also as [x | x2] (x2 fp32, K1 columns of x).
LEOD_API int leod_linear_wgrad(const float* dy, long lddy, const float* x, long ldx, const float* stats,
                               const float* ln_w, const float* ln_b, const float* x2, long ldx2, int K1,
                               float* dW, float* dbias, int M, int N, int K, int dy_fmt, int x_fmt, hipStream_t stream) {
    if (!dy || !x || !dW || !wgrad_formats_ok(dy_fmt, x_fmt, stats != nullptr, ln_w && ln_b, x2 != nullptr)) return LEOD_ERR_ARG;
    FamilyMarker fm(stream);
    XRows xl{x, ldx, stats, ln_w, ln_b, x2, ldx2, K1};
    xl.set_mode(x_fmt);
    return launch_linear_wgrad(wgrad_route(xl, lddy, dy_fmt, M, N, K), dy, lddy, dy_fmt, xl, dW, dbias, M, N, K, stream);
}

// The route leod_linear_wgrad takes for this problem in the current precision mode, without launching anything: the code of wgrad_route
// above (100 + T LDS-DMA, 200 + combo wide, 300 + cfg wgradw, 400 + 10 TN + TK wgrad16, 0 nothing to do, < 0 the error the call returns).
// has_stats: stats, ln_w and ln_b are given; has_x2: x2 is given.  leod_linear_wgrad switches on the same value; it leaves a 100 + T route
// only when no workspace is registered for its stream and none can be allocated (stream capture): register one (leod_set_workspace).
LEOD_API int leod_linear_wgrad_route(int M, int N, int K, long lddy, long ldx, long ldx2, int K1, int dy_fmt, int x_fmt, int has_stats,
                                     int has_x2) {
    if (!wgrad_formats_ok(dy_fmt, x_fmt, has_stats != 0, has_stats != 0, has_x2 != 0)) return LEOD_ERR_ARG;
    static const float given = 0.f;                  // a non-NULL address: wgrad_route tests stats / x2 for presence only
    XRows xl{&given, ldx, has_stats ? &given : nullptr, has_stats ? &given : nullptr, has_stats ? &given : nullptr,
             has_x2 ? &given : nullptr, ldx2, K1};
    xl.set_mode(x_fmt);
    return wgrad_route(xl, lddy, dy_fmt, M, N, K);
}

// n <= 4 Linear weight gradients of ONE row count M in one preparation launch, one contraction launch and one reduce launch (the LDS-DMA
// kernel of wgrad_dma.hpp with a problem table): the four weight gradients of an attention block -- qkv and fc1 from LayerNorm inputs, proj
// from the 16-bit attention rows, fc2 through GELU of the fp16 pre-activation (maxvit.py:110-118,252-270) -- which the block's backward
// issues together.  dy_fmt[k]: 0 fp32 rows, 1 bf16 rows.  x_fmt[k]: 0 fp32 rows, 1 fp32 rows through LayerNorm (stats / ln_w / ln_b of
// problem k), 2 fp16 pre-activation through GELU, 3 bf16 rows, 4 fp16 rows.  Dense rows (strides N[k] / K[k]).
// LEOD_ERR_UNSUPPORTED: not coverable (precision mode, row count, widths) -- nothing was launched, run the problems singly.
//
// The route of the group, from the integers alone (leod_linear_wgrad_group_route): WGR_DMA + T where it launches, on T x T blocks of 16
// columns; per problem in order LEOD_ERR_ARG for an x_fmt outside the vocabulary, then LEOD_ERR_UNSUPPORTED outside the coverage; the bound
// of the 16-bit operand copies (kWgdOperandBytes) last.  It launches nothing and reads no device memory.
static int wgrad_group_route(int n, int M, const int* N, const int* K, const int* dy_fmt, const int* x_fmt) {
    if (n < 1 || n > 4 || !N || !K || !dy_fmt || !x_fmt) return LEOD_ERR_ARG;
    int T = 0;
    size_t need = 0;
    for (int k = 0; k < n; ++k) {
        if (!xm_valid(x_fmt[k])) return LEOD_ERR_ARG;
        const int t = wgd_tile(N[k], K[k]);
        if (leod_precision() != 1 || !t || (T && t != T) || M < 8192 || (M % kWgdRC) || M > (t == 6 ? 60000 : 400000) || (N[k] & 7) || (K[k] & 7))
            return LEOD_ERR_UNSUPPORTED;
        T = t;
        need += (size_t)M * ((dy_fmt[k] ? 0 : N[k]) + (xm_is_mfma_operand(x_fmt[k]) ? 0 : K[k])) * 2;
    }
    return need > kWgdOperandBytes ? LEOD_ERR_UNSUPPORTED : WGR_DMA + T;
}
LEOD_API int leod_linear_wgrad_group_route(int n, int M, const int* N, const int* K, const int* dy_fmt, const int* x_fmt) {
    return wgrad_group_route(n, M, N, K, dy_fmt, x_fmt);
}
LEOD_API int leod_linear_wgrad_group(int n, const void* const* dy, const int* dy_fmt, const void* const* x, const int* x_fmt,
                                     const float* const* stats, const float* const* ln_w, const float* const* ln_b, float* const* dW,
                                     float* const* dbias, int M, const int* N, const int* K, hipStream_t stream) {
    if (!dy || !x || !dW) return LEOD_ERR_ARG;
    const int route = wgrad_group_route(n, M, N, K, dy_fmt, x_fmt);
    if (route < 0) return route;
    WgdHostProb hp[4];
    for (int k = 0; k < n; ++k) {
        if (!dy[k] || !x[k] || !dW[k]) return LEOD_ERR_ARG;
        XRows xl{reinterpret_cast<const float*>(x[k]), (long)K[k], nullptr, nullptr, nullptr, nullptr, 0, 0};
        if (x_fmt[k] == XM_LN) {
            if (!stats || !ln_w || !ln_b || !stats[k] || !ln_w[k] || !ln_b[k]) return LEOD_ERR_ARG;
            xl.stats = stats[k]; xl.ln_w = ln_w[k]; xl.ln_b = ln_b[k];
        }
        xl.set_mode(x_fmt[k]);
        hp[k] = WgdHostProb{dy[k], (long)N[k], xl, dW[k], (long)K[k], dbias ? dbias[k] : nullptr, N[k], K[k], dy_fmt[k] ? 1 : 0};
    }
    FamilyMarker fm(stream);
    switch (route - WGR_DMA) {
        case 6: return launch_wgrad_dma_group_t<6, 64, 3>(n, hp, M, stream);
        case 8: return launch_wgrad_dma_group_t<8, 64, 2>(n, hp, M, stream);
        case 4: return launch_wgrad_dma_group_t<4, 64, 3>(n, hp, M, stream);
    }
    return LEOD_ERR_ARG;
}

// 1: an attention block of this geometry may keep its attention output O and the gradient dO as bf16 rows in precision mode bf16 --
// every kernel that touches them has a 16-bit path: the bf16-tile attention kernels, proj forward (LDS-staged GEMM), the dgrad of proj
// (row epilogue) and the proj weight gradient (wide kernel)
extern "C" int leod_partition_attn_o16_ok(int B, int H, int W, int C, int heads, int ph, int pw);
LEOD_API int leod_attn_block_o16_ok(int B, int H, int W, int C, int heads, int ph, int pw) {
    const long M = (long)B * H * W;
    if (M > 0x7fffffffL || !leod_partition_attn_o16_ok(B, H, W, C, heads, ph, pw)) return 0;
    XRows xl{}; xl.ld = C; xl.set_mode(XM_BF16);
    return (C % 8 == 0) && use_gemm_lds((int)M, cdiv(C, 16 * pick_nt(C))) && use_wgrad_wide(xl, (long)C, (int)M, C, C, 0);
}
