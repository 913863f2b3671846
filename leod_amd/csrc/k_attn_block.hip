// The attention half of a MaxViT block in ONE launch (RVT stages 1-2, 16-bit precision modes):
//     y = x + gamma * (softmax(q k^T d^-1/2) v  W_proj^T + b_proj),   (q | k | v) = LN(x) W_qkv^T + b_qkv
// Reference: maxvit.py:185-270 (PartitionAttentionCl: norm1 -> partition attention -> ls1 -> residual), :343-354 (SelfAttentionCl).
//
// The three launches it replaces (ln_linear_bf16_fwd -> partition_attn_fwd -> linear_lsres_bf16_fwd) are bandwidth-limited at these
// stages and exchange qkv [M,3C] and O [M,C] through HBM and read x twice.  Here a persistent workgroup owns whole partitions (80 tokens,
// all heads): x is read once, qkv / O / lse / stats are written once (and only when the caller keeps them for a backward pass), y once.
// The rounding points are those of the three launches: LN(x), the weights, qkv, P and O are rounded to the 16-bit operand format of the
// precision mode (bf16, or fp16 in mode 16f), every accumulation, the statistics, the softmax and the residual are fp32.
//
// Workgroup = 10 waves = (half hl, 16-token tile qt).  W_qkv, W_proj (16-bit), the biases, gamma and the LayerNorm affine stay in LDS for
// the life of the workgroup.  Per partition, with one region R of LDS used three times (fp32 x tile, 16-bit qkv tile, fp32 proj tile):
//   1. x rows (coalesced, prefetched into registers during the previous partition) -> R as fp32; they wait for the residual in LDS where
//      a second workgroup per CU still fits (C = 48), else in registers (C = 96)
//   2. every wave: LayerNorm of its 16 rows from R, in the MFMA operand layout -> 16-bit fragments in registers; stats
//   3. qkv^T = W_qkv LN(x)^T: lane (token i, group rg) ends up with 4 consecutive columns -> one 8-byte store into the qkv tile in R
//   4. coalesced copy of the qkv tile to HBM; attention per (head, tile) as attn_fwd_lds16_kernel (k_attn.hip), heads in pairs, with
//      O^T = V^T P^T so that O goes to its LDS tile in 8-byte stores; lse
//   5. coalesced copy of the O tile to HBM; (O W_proj^T + b) gamma -> R as fp32
//   6. y = x + R, coalesced
#include "attn_route.hpp"
#include "attn_common.hpp"

template <int C, int HEADS>
struct ABL {                                                 // geometry and the LDS image (offsets in dwords)
    static constexpr int D = 24, PT = 5, TOK = 16 * PT, NWAVE = 2 * PT, NTHR = 64 * NWAVE;
    static_assert(C == HEADS * D && HEADS % 2 == 0, "two heads per pass, head dimension 24");
    static constexpr int N3 = 3 * C, KC = C / 16;
    static constexpr int LD = C + 8;                         // 16-bit elements per weight / O row: a 4 * odd dword stride (conflict-free 8-byte fragments)
    static constexpr int SD = A16L<D, HEADS>::SD;            // dwords per row of the qkv tile
    static constexpr int SX = C + 4;                         // floats per row of the fp32 x / proj tile
    static_assert(SX <= SD, "the fp32 tiles live in the qkv tile's region");
    static constexpr int OFF_Q = 0;                          // region R: TOK rows of SD dwords + 8 zeroed slack dwords
    static constexpr int OFF_O = OFF_Q + TOK * SD + 8;       // O tile [TOK][LD] 16-bit
    static constexpr int OFF_WQ = OFF_O + TOK * LD / 2;      // W_qkv [3C][LD] 16-bit
    static constexpr int OFF_WP = OFF_WQ + N3 * LD / 2;      // W_proj [C][LD] 16-bit
    static constexpr int OFF_F = OFF_WP + C * LD / 2;        // fp32: b_qkv [3C], b_proj [C], gamma [C], ln_w [C], ln_b [C]
    static constexpr int OFF_ROW = OFF_F + N3 + 4 * C;       // int srow[2][TOK]: the token rows of this partition and of the next one
    // The x rows wait for the residual in registers, or, where a second workgroup per CU still fits with them (C = 48, whose register budget
    // at two workgroups per CU is 96), in LDS: every thread reads back the float4s it wrote itself
    static constexpr int OFF_XR = OFF_ROW + 2 * TOK;
    static constexpr bool XRES_LDS = (OFF_XR + TOK * C) * 4 * 2 <= 160 * 1024;
    static constexpr int DWORDS = OFF_XR + (XRES_LDS ? TOK * C : 0);
    static_assert(OFF_O % 4 == 0 && OFF_WQ % 4 == 0 && OFF_WP % 4 == 0 && OFF_F % 4 == 0 && OFF_XR % 4 == 0, "16-byte aligned tiles");
    static_assert(DWORDS * 4 <= 160 * 1024, "one CU's LDS");
};

// OF: 1 = bf16 operands and rows, 2 = fp16 (precision mode 16f).  SAVE: qkv / o16 / lse / stats are written (else not touched: inference).
// LN = false: norm1 is the identity (the first block of a stage, maxvit_rnn.py:164-166): x itself is rounded to the operand format, no stats.
template <int C, int HEADS, int OF, bool SAVE, bool LN>
__global__ __launch_bounds__(640, C == 48 ? 5 : 3) void attn_block_fwd_kernel(
        const float* __restrict__ x, const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps,
        const float* __restrict__ Wqkv, const float* __restrict__ bqkv, const float* __restrict__ Wproj, const float* __restrict__ bproj,
        const float* __restrict__ gamma, float* __restrict__ y, unsigned short* __restrict__ qkv, unsigned short* __restrict__ o16,
        float* __restrict__ lse, float* __restrict__ stats, AttnGeom g, float scale, int nparts) {
    typedef ABL<C, HEADS> L;
    constexpr int D = L::D, PT = L::PT, TOK = L::TOK, NTHR = L::NTHR, N3 = L::N3, KC = L::KC, LD = L::LD, SD = L::SD, SX = L::SX;
    constexpr int F = C / 4, NX = (TOK * F + NTHR - 1) / NTHR;          // float4s of an x row, float4s of the x tile per thread
    extern __shared__ __attribute__((aligned(16))) unsigned sm[];
    unsigned* sq = sm + L::OFF_Q;
    float* sx = reinterpret_cast<float*>(sq);
    unsigned short* sqh = reinterpret_cast<unsigned short*>(sq);
    unsigned short* so = reinterpret_cast<unsigned short*>(sm + L::OFF_O);
    unsigned short* swq = reinterpret_cast<unsigned short*>(sm + L::OFF_WQ);
    unsigned short* swp = reinterpret_cast<unsigned short*>(sm + L::OFF_WP);
    float* sbq = reinterpret_cast<float*>(sm + L::OFF_F);
    float* sbp = sbq + N3; float* sg = sbp + C; float* slw = sg + C; float* slb = slw + C;
    f4* sxres = reinterpret_cast<f4*>(sm + L::OFF_XR);
    int* srows = reinterpret_cast<int*>(sm + L::OFF_ROW);       // rows fit an int: M < 2^31 (attn_block_kernel_route)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the (half, tile) index math lives in scalar registers
    const int i = lane & 15, rg = lane >> 4;
    const int hl = wave / PT, qt = wave - hl * PT;

    // ---- resident operands: weights rounded to the operand format once per workgroup -------------------------------------------------
    for (int e = tid; e < N3 * F; e += NTHR) {
        const int n = e / F, k4 = (e - n * F) * 4;
        *reinterpret_cast<s4*>(&swq[n * LD + k4]) = pack16_raw<OF>(ld4(Wqkv + (long)n * C + k4));
    }
    for (int e = tid; e < C * F; e += NTHR) {
        const int n = e / F, k4 = (e - n * F) * 4;
        *reinterpret_cast<s4*>(&swp[n * LD + k4]) = pack16_raw<OF>(ld4(Wproj + (long)n * C + k4));
    }
    for (int e = tid; e < N3; e += NTHR) sbq[e] = bqkv ? bqkv[e] : 0.f;
    for (int e = tid; e < C; e += NTHR) {
        sbp[e] = bproj ? bproj[e] : 0.f; sg[e] = gamma ? gamma[e] : 1.f;
        if (LN) { slw[e] = ln_w[e]; slb[e] = ln_b[e]; }
    }
    // the v fragments of the last head read 8 elements past the last row of the tile (into discarded output columns): keep them finite
    if (tid < 8) sq[TOK * SD + tid] = 0u;

    // the x tile of a partition in registers: float4 e = tid + j NTHR of the [TOK][F] tile (threads beyond it re-read its last row)
    auto load_x = [&](const int* rows, f4 (&v)[NX]) {
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const int e = tid + j * NTHR, tok = min(e / F, TOK - 1), f = e - (e / F) * F;
            v[j] = ld4(x + (long)rows[tok] * C + 4 * f);
        }
    };
    if (tid < TOK) srows[tid] = (int)token_row(g, blockIdx.x, tid);     // gridDim.x <= nparts
    __syncthreads();
    f4 xr[NX];
    load_x(srows, xr);
    int buf = 0;

    for (int p = blockIdx.x; p < nparts; p += gridDim.x) {
        // ---- 1. x tile -> region R (and, where it waits there, its place for the residual) ------------------------------------------------
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const int e = tid + j * NTHR, tok = e / F, f = e - tok * F;
            if (e < TOK * F) *reinterpret_cast<f4*>(&sx[tok * SX + 4 * f]) = xr[j];
            if (L::XRES_LDS && e < TOK * F) sxres[e] = xr[j];
        }
        const int* srow = srows + buf * TOK;
        if (tid < TOK) srows[(buf ^ 1) * TOK + tid] = (int)token_row(g, min(p + (int)gridDim.x, nparts - 1), tid);
        __syncthreads();
        // the next partition's rows are requested now (one workgroup per CU: nothing else hides the latency), or, where the register budget
        // of two workgroups per CU is tight and the other workgroup keeps the CU busy, just before the attention (step 4)
        f4 xn[NX];
        if (!L::XRES_LDS) load_x(srows + (buf ^ 1) * TOK, xn);

        // ---- 2. LayerNorm of rows 16 qt + i in operand layout (lane (i, rg) holds columns 16 c + 4 rg .. +3): two-pass statistics
        //         as in rowstream48_kernel, the 16-bit fragments stay in registers -----------------------------------------------------
        s4 a16[KC];
        {
            const float* xp = sx + (16 * qt + i) * SX + 4 * rg;
            f4 a[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) a[c] = *reinterpret_cast<const f4*>(xp + 16 * c);
            if constexpr (LN) {
                float sum = 0.f;
#pragma unroll
                for (int c = 0; c < KC; ++c) sum += (a[c][0] + a[c][1]) + (a[c][2] + a[c][3]);
                sum = quad16_sum(sum);
                const float mean = sum * (1.0f / C);
                float var = 0.f;
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    const f4 dv = a[c] - mean;
                    var += (dv[0] * dv[0] + dv[1] * dv[1]) + (dv[2] * dv[2] + dv[3] * dv[3]);
                }
                var = quad16_sum(var);
                const float rstd = rsqrtf(var * (1.0f / C) + eps);
                if (SAVE && hl == 0) {                            // the 4 lanes of a row write the same pair
                    float2 st; st.x = mean; st.y = rstd;
                    *reinterpret_cast<float2*>(stats + 2 * (long)srow[16 * qt + i]) = st;
                }
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    const f4 lw = *reinterpret_cast<const f4*>(slw + 16 * c + 4 * rg), lb = *reinterpret_cast<const f4*>(slb + 16 * c + 4 * rg);
                    a16[c] = pack16<OF>((a[c] - mean) * rstd * lw + lb);
                }
            } else {
#pragma unroll
                for (int c = 0; c < KC; ++c) a16[c] = pack16<OF>(a[c]);
            }
        }
        __syncthreads();                                      // every wave has its fragments: R becomes the qkv tile

        // ---- 3. qkv^T tile (16 columns x 16 tokens) = W_qkv rows (A operand) x LN(x)^T (B operand): accumulator register r of lane
        //         (i, rg) is column 16 t + 4 rg + r of token i; the two halves split the column tiles -----------------------------------
        {
            constexpr int NT = N3 / 16, T0 = (NT + 1) / 2;
            const int t0 = hl ? T0 : 0, nt = hl ? NT - T0 : T0;
#pragma unroll
            for (int tt = 0; tt < T0; ++tt) {
                if (tt >= nt) break;
                const int t = t0 + tt;
                f4 acc = zero4();
#pragma unroll
                for (int c = 0; c < KC; ++c)
                    acc = mfma16_16<OF>(*reinterpret_cast<const s4*>(&swq[(16 * t + i) * LD + 16 * c + 4 * rg]), a16[c], acc);
                acc = acc + *reinterpret_cast<const f4*>(sbq + 16 * t + 4 * rg);
                *reinterpret_cast<s4*>(&sqh[(16 * qt + i) * (2 * SD) + 16 * t + 4 * rg]) = pack16<OF>(acc);
            }
        }
        __syncthreads();

        // ---- 4. qkv rows to HBM (whole rows, 16 bytes per lane); attention of (head 2 hp + hl, query tile qt) -------------------------
        if (SAVE) {
            constexpr int U = N3 / 8;
            for (int e = tid; e < TOK * U; e += NTHR) {
                const int tok = e / U, f = e - tok * U;
                *reinterpret_cast<u4v_*>(qkv + (long)srow[tok] * N3 + 8 * f) = *reinterpret_cast<const u4v_*>(sq + tok * SD + 4 * f);
            }
        }
        if (L::XRES_LDS) load_x(srows + (buf ^ 1) * TOK, xn);
#pragma unroll
        for (int hp = 0; hp < HEADS / 2; ++hp) {
            const int h = 2 * hp + hl;
            const int hq = h * 3 * D / 2, hk = hq + D / 2, hv = hq + D;                  // dword offsets of this head's q | k | v
            const s8v qf = a16_mask<D>(a16_frag(sq, 16 * qt + i, SD, hq, rg), rg);
            f4 s[PT];                                         // S^T: keys 16 mt + 4 rg + r along the registers, query i
#pragma unroll
            for (int mt = 0; mt < PT; ++mt) s[mt] = mfma32_16<OF>(a16_frag(sq, 16 * mt + i, SD, hk, rg), qf, zero4());
            float mx = -INFINITY;
#pragma unroll
            for (int mt = 0; mt < PT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[mt][r] *= scale;
                    mx = fmaxf(mx, s[mt][r]);
                }
            mx = quad16_max(mx);
            float sum = 0.f;
#pragma unroll
            for (int mt = 0; mt < PT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = fast_exp(s[mt][r] - mx);
                    s[mt][r] = e;
                    sum += e;
                }
            sum = quad16_sum(sum);
            const float inv = 1.0f / sum;
            if (SAVE && rg == 0) lse[(long)srow[16 * qt + i] * HEADS + h] = mx + logf(sum);
            // O^T = V^T P^T: register r of lane (i, rg) is column 16 ct + 4 rg + r of query i
            f4 o0 = zero4(), o1 = zero4();
#pragma unroll
            for (int mt = 0; mt < PT; ++mt) {
                const s4 pa = pack16_raw<OF>(s[mt] * inv);
                o0 = mfma16_16<OF>(a16_tfrag(sq, 16 * mt, SD, hv, i, rg), pa, o0);
                o1 = mfma16_16<OF>(a16_tfrag(sq, 16 * mt, SD, hv + 8, i, rg), pa, o1);
            }
            unsigned short* orow = so + (16 * qt + i) * LD + h * D + 4 * rg;
            *reinterpret_cast<s4*>(orow) = pack16<OF>(o0);
            if (rg < 2) *reinterpret_cast<s4*>(orow + 16) = pack16<OF>(o1);               // columns 16 .. 23 of d = 24
        }
        __syncthreads();                                      // O tile complete, R free

        // ---- 5. O rows to HBM; (O W_proj^T + b) gamma -> R (fp32), transposed product as in step 3 ------------------------------------
        if (SAVE) {
            constexpr int U = C / 8;
            for (int e = tid; e < TOK * U; e += NTHR) {
                const int tok = e / U, f = e - tok * U;
                *reinterpret_cast<u4v_*>(o16 + (long)srow[tok] * C + 8 * f) = *reinterpret_cast<const u4v_*>(so + tok * LD + 8 * f);
            }
        }
        {
            constexpr int NT = C / 16, T0 = (NT + 1) / 2;
            const int t0 = hl ? T0 : 0, nt = hl ? NT - T0 : T0;
            s4 of[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) of[c] = *reinterpret_cast<const s4*>(&so[(16 * qt + i) * LD + 16 * c + 4 * rg]);
#pragma unroll
            for (int tt = 0; tt < T0; ++tt) {
                if (tt >= nt) break;
                const int t = t0 + tt;
                f4 acc = zero4();
#pragma unroll
                for (int c = 0; c < KC; ++c)
                    acc = mfma16_16<OF>(*reinterpret_cast<const s4*>(&swp[(16 * t + i) * LD + 16 * c + 4 * rg]), of[c], acc);
                const f4 v = (acc + *reinterpret_cast<const f4*>(sbp + 16 * t + 4 * rg)) * *reinterpret_cast<const f4*>(sg + 16 * t + 4 * rg);
                *reinterpret_cast<f4*>(&sx[(16 * qt + i) * SX + 16 * t + 4 * rg]) = v;
            }
        }
        __syncthreads();

        // ---- 6. y = x + gamma * proj, whole rows ---------------------------------------------------------------------------------------
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const int e = tid + j * NTHR, tok = e / F, f = e - tok * F;
            if (e < TOK * F) {
                const f4 xv = L::XRES_LDS ? sxres[e] : xr[j];
                *reinterpret_cast<f4*>(y + (long)srow[tok] * C + 4 * f) = xv + *reinterpret_cast<const f4*>(&sx[tok * SX + 4 * f]);
            }
        }
        __syncthreads();                                      // R is read out before the next x tile lands in it
#pragma unroll
        for (int j = 0; j < NX; ++j) xr[j] = xn[j];
        buf ^= 1;
    }
}

struct AttnBlockArgs {
    const float* x; const float* ln_w; const float* ln_b; float eps; const float* Wqkv; const float* bqkv; const float* Wproj;
    const float* bproj; const float* gamma; float* y; void* qkv16; void* o16; float* lse; float* stats;
};

template <int C, int HEADS, int OF, bool SAVE, bool LN>
static void launch_attn_block_kernel(const AttnBlockArgs& a, const AttnGeom& g, hipStream_t s) {
    typedef ABL<C, HEADS> L;
    constexpr int LDS = L::DWORDS * 4;
    const int nparts = g.B * (g.H / g.ph) * (g.W / g.pw);
    const int per_cu = (160 * 1024) / LDS;                    // resident workgroups per CU (LDS: 2 at C = 48, 1 at C = 96)
    const int grid = min(nparts, 256 * per_cu);
    const float scale = 1.0f / sqrtf((float)g.d);
    auto kern = attn_block_fwd_kernel<C, HEADS, OF, SAVE, LN>;
    static bool attr_set = false;
    if (!attr_set) { hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS); attr_set = true; }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(L::NTHR), LDS, s, a.x, a.ln_w, a.ln_b, a.eps, a.Wqkv, a.bqkv, a.Wproj, a.bproj, a.gamma, a.y,
                       reinterpret_cast<unsigned short*>(a.qkv16), reinterpret_cast<unsigned short*>(a.o16), a.lse, a.stats, g, scale, nparts);
}
template <int C, int HEADS>
static int launch_attn_block(const AttnBlockArgs& a, const AttnGeom& g, hipStream_t s) {
    LEOD_BY_OPFMT16({
        if (a.ln_w) { if (a.qkv16) launch_attn_block_kernel<C, HEADS, OF, true, true>(a, g, s); else launch_attn_block_kernel<C, HEADS, OF, false, true>(a, g, s); }
        else { if (a.qkv16) launch_attn_block_kernel<C, HEADS, OF, true, false>(a, g, s); else launch_attn_block_kernel<C, HEADS, OF, false, false>(a, g, s); }
    });
    return leod_launch_status();
}

// Whether a block of this geometry takes the one-launch forward in the current precision mode (flags: 1 = norm1 has weight and bias), or
// the error code that says it does not: a query, nothing is launched.  Codes: include/leod_hip.h.
LEOD_API int leod_attn_block_fwd_route(int B, int H, int W, int C, int heads, int ph, int pw, int flags) {
    return attn_block_fwd_route(B, H, W, C, heads, ph, pw, flags);
}

// y[M,C] = x + gamma * (attention(LN(x) W_qkv^T + b_qkv) W_proj^T + b_proj) on the window (window = 1) or grid partitions of ph x pw
// tokens of the NHWC map x.  qkv16 [M,3C] / o16 [M,C] (16-bit rows of the precision mode), lse [M,heads], stats [M,2] are written when
// given (all or none; stats only with a LayerNorm, ln_w = ln_b = NULL means norm1 is the identity): what the three-launch path leaves behind for the backward pass.
LEOD_API int leod_attn_block_fwd(const float* x, const float* ln_w, const float* ln_b, float eps, const float* Wqkv, const float* bqkv,
                                 const float* Wproj, const float* bproj, const float* gamma, float* y, void* qkv16, void* o16, float* lse,
                                 float* stats, int B, int H, int W, int C, int heads, int ph, int pw, int window, hipStream_t stream) {
    LeodFwdScope fwd_scope;                                   // forward contractions: fp16 operands in precision mode 16f
    if (!x || !Wqkv || !Wproj || !y || !ln_w != !ln_b) return LEOD_ERR_ARG;                     // ln_w = ln_b = NULL: norm1 is the identity
    // the saved tensors: all or none (stats exist only with a LayerNorm)
    if (!!qkv16 != !!o16 || !!qkv16 != !!lse || !!stats != (qkv16 && ln_w)) return LEOD_ERR_ARG;
    const int route = attn_block_kernel_route(B, H, W, C, heads, ph, pw);
    if (route <= 0) return route;
    const AttnGeom g{B, H, W, C, heads, C / heads, ph, pw, window, 0};
    const AttnBlockArgs a{x, ln_w, ln_b, eps, Wqkv, bqkv, Wproj, bproj, gamma, y, qkv16, o16, lse, stats};
    if (C == 48) return launch_attn_block<48, 2>(a, g, stream);
    return launch_attn_block<96, 4>(a, g, stream);
}
