// Short 1x1 / stride-1 convolutions of the PAFPN and the head stems: up to 4 independent problems Out[m][n] = sum_k A[m][k] * W(n, k) over
// pixel rows in ONE launch, every operand of a tile in flight at once.
//
// The LDS-staged GEMM (gemm_lds_kernel, gemm16.hpp) walks K in chunks of 48 / 64 with one register prefetch and two barriers per chunk: a
// chunk costs about one memory round trip, which four resident workgroups per CU hide at stage sizes.  The neck / head problems (2 560 ..
// 40 960 rows, K <= 384) fill the 256 CUs once or twice, so their K / 48 dependent round trips are the launch.  Here a workgroup issues
// EVERY global load of its A tile and its W tile for the whole K before its first wait, rounds them to the operand format on the way into
// LDS, passes ONE barrier and runs all MFMAs: no load depends on a barrier or on another load.
//
//   forward (TRANS = false): W as stored, [N][K]; operands in the forward format of the launch (OF: bf16, or fp16 in mode 16f), activations
//       saturated like gemm_lds_kernel's A rows; the BatchNorm column statistics of leod_conv_nhwc_fwd ([R][2][N] doubles, 16-row fragment f
//       adds into replica f & (R - 1), one fp32 fold per fragment before the atomics)
//   dgrad (TRANS = true): W[k][n] read transposed (k = the conv's output channel, n = its input channel), bf16 operands, optional Out +=
// fp32 master weights are rounded in the kernel; fp32 accumulation on the 16-bit 16x16x16 MFMA; fp32 output rows.
//
// A group computes BIT FOR BIT what its members compute through their single-call routes (conv_rows_route): ascending k where that route is
// LDS-staged or register-direct on one wave, the four interleaved partial sums of gemm16_kernel<NT, 4> where it splits K over its waves; the
// statistics in the order and with the (un)fused squares of that route's epilogue (EpStore::run, or EpStore's row epilogue, which is called
// as it stands).  Grouping therefore changes no value of a training step -- a last-bit change of one BatchNorm statistic is enough to flip a
// SimOTA assignment of the full-size 16-bit step (tests/test_bf16_class_gpu.py compares its plans against eager steps).
//
// Tile: 16 RF rows (RF = 2 | 4, per problem) x 48 columns, 256 threads.  LDS: operands (K + 8)-strided 16-bit rows as in gemm_lds_kernel,
// at most 62.7 KB (RF = 2, K = 384; RF = 4 is offered up to K = 192: 45 KB), so that a workgroup co-resides with the weight-gradient lane.
// The grid is the concatenation of the problems' tiles, each problem's tiles in the XCD-aware order of gemm_lds_kernel.  Every workgroup
// runs alone to completion.
#pragma once
#include "conv_route.hpp"

constexpr int C1_MAX = 4;               // problems per launch
constexpr int C1_NT = 3, C1_BN = 16 * C1_NT;
constexpr int C1_KMAX = 384, C1_NMAX = 384, C1_MMAX = 65536;
constexpr int C1_BST = 16 * 16 + 16;    // 16-bit elements per [16 k][16 n] block of transposed weights (gemm_lds_kernel's layout)
constexpr int C1_LDO = C1_BN + 4;       // fp32 row stride of the output tile that aliases the operands

struct C1Prob {
    const float* a; const float* w; float* out; double* stats;
    int M, K, N;                        // rows, contraction length, output columns
    int rep, acc;                       // statistics replicas (power of two); dgrad: Out +=
    int rf;                             // 16-row fragments per workgroup: 2 | 4
    int ks4, rowstats;                  // the summation orders of the member's single-call route (launch_conv1x1_group)
    int nbn, tile0;                     // column blocks; first workgroup of the problem (a multiple of 8)
};
struct C1Group { C1Prob p[C1_MAX]; int n; };

static inline size_t c1_lds_bytes(bool trans, int rf, int K) {
    const size_t a = (size_t)16 * rf * (K + 8) * 2;
    const size_t b = trans ? (size_t)(K / 16) * C1_NT * C1_BST * 2 : (size_t)C1_BN * (K + 8) * 2;
    const size_t o = (size_t)16 * rf * C1_LDO * 4;
    return a + b > o ? a + b : o;
}

// v * v rounded on its own: EpStore::run, the statistics of the register-direct single calls, adds unfused squares (a packed add of
// (v, v * v)), the row epilogue of the LDS-staged ones fused ones (v_pk_fma_f32); the grouped kernel says which it means
__device__ __forceinline__ float c1_square(float v) {
#pragma clang fp contract(off)
    return v * v;
}

// The statistics of a member whose single call is LDS-staged come out of that call's OWN row epilogue (EpStore::run_rows_full / run_rows on
// the wave's part of the fp32 tile): the same source gives the same fused products in the same order.  NTV: the wave's column tiles.
struct C1Cols { int n; __device__ __forceinline__ int col(int, int, int) const { return n; } };
template <int NTV>
__device__ __forceinline__ void c1_row_epilogue(const EpStore& ep, const float* sw, int n, int row0, int lane, int M) {
    const C1Cols bl{n};
    // gemm_lds_kernel takes the branch-free body where its 64-row workgroup lies inside the matrix
    if ((row0 & ~63) + 64 <= M) ep.template run_rows_full<6, NTV, C1Cols>(sw, C1_LDO, bl, row0, 0, lane, RowPre{});
    else ep.template run_rows<NTV, C1Cols>(sw, C1_LDO, bl, row0, 0, lane, M);
}

// one tile of problem pr.  KK: the contraction length at compile time (the step's 48 / 96 / 192 / 384: constant slot decode), 0: pr.K
template <int OF, bool TRANS, int RF, int KK>
__device__ __forceinline__ void c1_tile(const C1Prob& pr, int local, unsigned short* __restrict__ smem16) {
    constexpr int BM = 16 * RF, NT = C1_NT, BN = C1_BN, BN4 = BN / 4, KCAP = KK ? KK : C1_KMAX;
    constexpr int SA = (BM * KCAP / 4 + 255) / 256, SB = (BN * KCAP / 4 + 255) / 256;
    constexpr int WPR = 4 / RF, TW = (NT + WPR - 1) / WPR;        // waves per row fragment, column tiles per wave
    constexpr int BST = C1_BST, LDO = C1_LDO;
    const int K = KK ? KK : pr.K, K4 = K >> 2, LD = K + 8;
    const int M = pr.M, N = pr.N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int per = 8 * pr.nbn;
    const int grp = local / per, rem = local - grp * per;
    const int brow0 = (grp * 8 + (rem & 7)) * BM, n0 = (rem >> 3) * BN;
    if (brow0 >= M) return;                                     // workgroup-uniform (padding of the last group of 8 row tiles)
    unsigned short* __restrict__ a16 = smem16;
    unsigned short* __restrict__ b16 = smem16 + BM * LD;
    // ---- every global load of the tile, unconditional on clamped addresses: all in flight together ------------------------------
    f4 ra[SA], rb[SB];
    [[maybe_unused]] f4 rc[4];
#pragma unroll
    for (int p = 0; p < SA; ++p) {
        const int e = min(tid + 256 * p, BM * K4 - 1), r = e / K4, k4 = e - r * K4;
        ra[p] = ld4(pr.a + (long)min(brow0 + r, M - 1) * K + 4 * k4);
    }
#pragma unroll
    for (int p = 0; p < SB; ++p) {
        if constexpr (!TRANS) {
            const int e = min(tid + 256 * p, BN * K4 - 1), nl = e / K4, k4 = e - nl * K4;
            rb[p] = ld4(pr.w + (long)min(n0 + nl, N - 1) * K + 4 * k4);
        } else {
            const int e = min(tid + 256 * p, K * BN4 - 1), kl = e / BN4, n4 = (e - kl * BN4) * 4;
            rb[p] = ld4(pr.w + (long)kl * N + min(n0 + n4, N - 4));
        }
    }
    // the wave's part of the tile: row fragment rfw, column tiles ct0 .. ct0 + TW (those below NT).  Epilogue lane (i, q): columns 4 i .. 4 i + 3
    // of that span, rows q, q + 4, q + 8, q + 12 of the fragment
    const int rfw = wave % RF, ct0 = (wave / RF) * TW;
    const int row0 = brow0 + 16 * rfw, col = n0 + 16 * ct0 + 4 * i;
    const bool col_ok = i < 4 * min(TW, NT - ct0) && col < N;
    if constexpr (TRANS) {                                       // Out +=: the old values travel with the operands (no accumulate: one hot line)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float* old = pr.out + (long)min(row0 + q + 4 * p, M - 1) * N + min(col, N - 4);
            rc[p] = ld4(pr.acc ? old : pr.w);
        }
    }
    // ---- round to the operand format on the way into LDS ---------------------------------------------------------------------------
    const s4 zero = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < SA; ++p) {
        const int e = tid + 256 * p, r = e / K4, k4 = e - r * K4;
        if (e < BM * K4) *reinterpret_cast<s4*>(a16 + r * LD + 4 * k4) = brow0 + r < M ? pack16<OF>(ra[p]) : zero;
    }
#pragma unroll
    for (int p = 0; p < SB; ++p) {
        const int e = tid + 256 * p;
        if constexpr (!TRANS) {
            const int nl = e / K4, k4 = e - nl * K4;
            if (e < BN * K4) *reinterpret_cast<s4*>(b16 + nl * LD + 4 * k4) = n0 + nl < N ? pack16_raw<OF>(rb[p]) : zero;
        } else {
            const int kl = e / BN4, n4 = (e - kl * BN4) * 4;
            if (e < K * BN4)
                *reinterpret_cast<s4*>(b16 + ((kl >> 4) * NT + (n4 >> 4)) * BST + (kl & 15) * 16 + (n4 & 15)) = n0 + n4 < N ? pack16_raw<OF>(rb[p]) : zero;
        }
    }
    __syncthreads();
    // ---- all MFMAs: wave = (row fragment, group of TW column tiles) ------------------------------------------------------------------
    f4 acc[TW];
    int tcl[TW];                                                   // a wave past the last column tile repeats it and discards the result
#pragma unroll
    for (int j = 0; j < TW; ++j) { acc[j] = zero4(); tcl[j] = min(ct0 + j, NT - 1); }
    {
        typedef __attribute__((address_space(3))) s4 lds_s4;
        const unsigned short* __restrict__ pa = a16 + (16 * rfw + i) * LD + 4 * q;
        const unsigned short* __restrict__ pb = b16 + (TRANS ? (4 * q + (i >> 2)) * 16 + 4 * (i & 3) : i * LD + 4 * q);
        auto step = [&](int c, f4 (&d)[TW]) {
            const s4 av = *reinterpret_cast<const s4*>(pa + 16 * c);
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                s4 bv;
                if constexpr (TRANS) bv = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(pb + (c * NT + tcl[j]) * BST));
                else bv = *reinterpret_cast<const s4*>(pb + 16 * tcl[j] * LD + 16 * c);
                d[j] = mfma16_16<OF>(av, bv, d[j]);
            }
        };
        if (RF == 2 && pr.ks4) {
            // the order of gemm16_kernel<NT, 4>: chunk c into the sum of wave c & 3, then s0 + ((s1 + s2) + s3) -- four short MFMA chains
            f4 part[3][TW];
#pragma unroll
            for (int w = 0; w < 3; ++w)
#pragma unroll
                for (int j = 0; j < TW; ++j) part[w][j] = zero4();
            if constexpr (KK != 0) {
#pragma unroll
                for (int c = 0; c < KK / 16; ++c) {
                    if ((c & 3) == 0) step(c, acc); else step(c, part[(c & 3) - 1]);
                }
            } else {
                const int nc = K >> 4;
                for (int c = 0; c < nc; c += 4) {
                    step(c, acc);
                    if (c + 1 < nc) step(c + 1, part[0]);
                    if (c + 2 < nc) step(c + 2, part[1]);
                    if (c + 3 < nc) step(c + 3, part[2]);
                }
            }
#pragma unroll
            for (int j = 0; j < TW; ++j) acc[j] += (part[0][j] + part[1][j]) + part[2][j];
        } else if constexpr (KK != 0) {
#pragma unroll 3
            for (int c = 0; c < KK / 16; ++c) step(c, acc);
        } else {
            for (int c = 0; c < (K >> 4); ++c) step(c, acc);
        }
    }
    double* const cs = pr.stats ? pr.stats + (pr.rep > 1 ? (size_t)((row0 >> 4) & (pr.rep - 1)) * 2 * N : 0) : nullptr;
    // ---- column statistics of the fragment in the order of EpStore::run (register-direct single calls): rows 4 q .. 4 q + 3 per lane, then
    // the four row groups.  Rows past M are zero rows: they add nothing
    if constexpr (!TRANS) {
        if (cs && !pr.rowstats) {
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                const int n = n0 + 16 * (ct0 + j) + i;
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float v = acc[j][r]; s1 += v; s2 += c1_square(v); }
                s1 = quad16_sum(s1); s2 = quad16_sum(s2);
                if (q == 0 && ct0 + j < NT && n < N && row0 < M) { atomicAdd(cs + n, (double)s1); atomicAdd(cs + N + n, (double)s2); }
            }
        }
    }
    // ---- output rows through an fp32 tile on top of the operands: 16-byte stores of whole row segments; a wave reads back what it wrote ----
    float* __restrict__ so = reinterpret_cast<float*>(smem16);
    __syncthreads();                                               // everyone is done with the operands
#pragma unroll
    for (int j = 0; j < TW; ++j)
        if (ct0 + j < NT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) so[(16 * rfw + 4 * q + r) * LDO + 16 * (ct0 + j) + i] = acc[j][r];
        }
    __syncthreads();
    if constexpr (!TRANS) {
        if (cs && pr.rowstats) {                                   // workgroup-uniform
            if (row0 < M) {                                        // wave-uniform, like ntv
                EpStore ep{};
                ep.out = pr.out; ep.ld = N; ep.N = N; ep.colstats = pr.stats; ep.stat_rep = pr.rep; ep.act = ACT_NONE;
                const float* sw = so + 16 * rfw * LDO + 16 * ct0;
                const int ntv = min(TW, NT - ct0), n = n0 + 16 * ct0;
                if (ntv == 3) c1_row_epilogue<3>(ep, sw, n, row0, lane, M);
                else if (ntv == 2) c1_row_epilogue<2>(ep, sw, n, row0, lane, M);
                else c1_row_epilogue<1>(ep, sw, n, row0, lane, M);
            }
            return;
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int lr = q + 4 * p;
        if (col_ok && row0 + lr < M) {
            f4 v = *reinterpret_cast<const f4*>(so + (16 * rfw + lr) * LDO + 16 * ct0 + 4 * i);
            if constexpr (TRANS) { if (pr.acc) v += rc[p]; }
            *reinterpret_cast<f4*>(pr.out + (long)(row0 + lr) * N + col) = v;
        }
    }
}

template <int OF, bool TRANS>
__global__ __launch_bounds__(256, 2) void conv1x1_short_kernel(C1Group g) {
    extern __shared__ __attribute__((aligned(16))) unsigned short c1_smem[];
    const int bid = blockIdx.x;
    C1Prob pr = g.p[0];
#pragma unroll
    for (int j = 1; j < C1_MAX; ++j)
        if (j < g.n && bid >= g.p[j].tile0) pr = g.p[j];
    const int local = bid - pr.tile0;
    // workgroup-uniform: one body per (row fragments, contraction length) of the step's shapes, the run-time-K body for the rest
    if (pr.rf == 4) {                                            // offered for K = 48 | 96 | 192 only (c1_rf)
        if (pr.K == 48) c1_tile<OF, TRANS, 4, 48>(pr, local, c1_smem);
        else if (pr.K == 96) c1_tile<OF, TRANS, 4, 96>(pr, local, c1_smem);
        else c1_tile<OF, TRANS, 4, 192>(pr, local, c1_smem);
    } else if (pr.K == 48) c1_tile<OF, TRANS, 2, 48>(pr, local, c1_smem);
    else if (pr.K == 96) c1_tile<OF, TRANS, 2, 96>(pr, local, c1_smem);
    else if (pr.K == 192) c1_tile<OF, TRANS, 2, 192>(pr, local, c1_smem);
    else if (pr.K == 384) c1_tile<OF, TRANS, 2, 384>(pr, local, c1_smem);
    else c1_tile<OF, TRANS, 2, 0>(pr, local, c1_smem);
}

// ---- routing: the only place that decides ------------------------------------------------------------------------------------------------
// Route code of a group: 1 followed by one digit per member, the member's row fragments per workgroup (2: 32-row tiles, 4: 64-row tiles) --
// 12, 14, 122, 1422, ...  M, K, N: rows, contraction length and output columns of each member's GEMM (dgrad: K = the conv's output channels,
// N = its input channels).
enum : int { C1E_FWD = 0, C1E_DGRAD = 1 };
// 64-row tiles halve the W traffic of the long maps; they fit the LDS bound up to K = 192 and leave the short maps too few workgroups.
// A group computes bit for bit what its members compute through their single-call routes (conv_rows_route): same operand rounding, same
// order of the fp32 sums of outputs and statistics.  Members whose single call splits K over four waves (6000 + 10 NT + 4) keep that order
// on 32-row tiles; the wide-tile kernel (3000 + ..) contracts 32 k per MFMA, which this kernel cannot reproduce: refused.
constexpr int C1_LONG = 8192;            // rows from which a map counts as long
static inline bool c1_single_ks4(int single) { return single >= CR_GEMM16 && single % 10 == 4; }
static inline int c1_rf(int M, int K, int single) { return M >= C1_LONG && (K == 48 || K == 96 || K == 192) && !c1_single_ks4(single) ? 4 : 2; }
static int conv1x1_group_route(int entry, int n, const int* M, const int* K, const int* N, int flags) {
    if ((entry != C1E_FWD && entry != C1E_DGRAD) || n < 1 || n > C1_MAX || !M || !K || !N) return LEOD_ERR_ARG;
    if (flags & ~(CF_COLSTATS | CF_ACCUMULATE)) return LEOD_ERR_ARG;
    if (leod_precision() != 1) return LEOD_ERR_UNSUPPORTED;     // 16-bit modes only
    int code = 1;
    for (int k = 0; k < n; ++k) {
        if (M[k] < 1 || M[k] > C1_MMAX || K[k] < 16 || K[k] > C1_KMAX || (K[k] & 15) || N[k] < 16 || N[k] > C1_NMAX || (N[k] & 15))
            return LEOD_ERR_UNSUPPORTED;
        const int single = conv_rows_route(entry == C1E_DGRAD, M[k], K[k], N[k]);
        if (single >= RG_WIDE && single < RG_TWO_PHASE) return LEOD_ERR_UNSUPPORTED;
        code = 10 * code + c1_rf(M[k], K[k], single);
    }
    // A member of C1_LONG rows or more is not faster here than through its single call (tools/kbench_conv1x1.py on this kernel,
    // profiles/r18_a_kbench_conv1x1_before_last_refusal.txt: forward 16.9 / 11.5 / 13.4 / 17.3 / 13.8 / 22.6 us single against 18.4 / 11.2 / 12.7 / 17.7 / 13.3 /
    // 23.9 here -- the statistics epilogue of the LDS-staged calls is most of both; input gradients 4.6 - 10.2 us single against 4.4 - 14.1 in
    // the first version, ..._first.txt).  Long members gain only by the launch they share: forward next to any other member (pairs on one
    // map 33.1 -> 28.1, 26.6 -> 18.5, 34.1 -> 29.4 us), input gradients next to a short one (the three stems 23.9 -> 19.1 us).
    bool any_short = false;
    for (int k = 0; k < n; ++k) any_short |= M[k] < C1_LONG;
    if (!any_short && (entry == C1E_DGRAD || n == 1)) return LEOD_ERR_UNSUPPORTED;
    return code;
}

// what the route decided, launched: g holds pointers, sizes, replicas and accumulate flags; the tiling comes from the code
template <bool TRANS>
static int launch_conv1x1_group(int route, C1Group& g, hipStream_t s) {
    if (route <= 0) return route;
    int tiles = 0;
    size_t lds = 0;
    int div = 1;
    for (int k = 1; k < g.n; ++k) div *= 10;
    for (int k = 0; k < g.n; ++k, div /= 10) {
        C1Prob& p = g.p[k];
        p.rf = route / div % 10;
        if (p.rf != 2 && p.rf != 4) return LEOD_ERR_ARG;
        const int single = conv_rows_route(TRANS, p.M, p.K, p.N);
        p.ks4 = c1_single_ks4(single);
        p.rowstats = single < CR_GEMM16;
        p.nbn = cdiv(p.N, C1_BN);
        p.tile0 = tiles;
        tiles += cdiv(cdiv(p.M, 16 * p.rf), 8) * 8 * p.nbn;
        const size_t need = c1_lds_bytes(TRANS, p.rf, p.K);
        lds = need > lds ? need : lds;
    }
    if (lds > 65536) return LEOD_ERR_ARG;
    LEOD_BY_OPFMT16_IF(!TRANS, hipLaunchKernelGGL((conv1x1_short_kernel<OF, TRANS>), dim3(tiles), dim3(256), lds, s, g));
    return leod_launch_status();
}
