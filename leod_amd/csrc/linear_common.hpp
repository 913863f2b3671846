// Shared by the token-row contraction translation units (k_linear.hip: fp32-tensor forward; k_linear16.hip: 16-bit-tensor forward;
// k_linear_bwd.hip: input gradients; k_linear_wgrad.hip: weight gradients): tile pickers and the wave-autonomous row-streaming kernels.
// The entry points were one file until round 5; it took 7+ minutes to compile on its own, the four files build in parallel.
#pragma once
#include <type_traits>

#define LEOD_SHADOW_KERNELS 1        // bf16-shadow weight loaders for the Linear layers (gemm16.hpp: BLRows16 / BLTrans16)
#include "gemm16.hpp"

static inline EpStore ep_store(float* out, long ld, int N) {
    EpStore e{};
    e.out = out; e.ld = ld; e.N = N; e.act = ACT_NONE;
    return e;
}

// ---------------------------------------------------------------------------------------------------------------------
// Wave-autonomous row-streaming GEMM for the short contractions of stages 1 and 2 (K = 48: N = 144 / 192, K = 96: N = 288 / 384
// in column slabs: LN -> qkv, LN -> fc1 + GELU).  A 64 x 48 workgroup of the LDS-staged GEMM lives ~11 us for 36 MFMAs per wave (operand loads, barrier, MFMAs, barrier,
// transposition, barrier, stores: two serialized memory latencies) and 4 of them per CU keep only ~2.5 TB/s in flight.  Here the
// whole weight matrix stays in LDS for the life of a persistent workgroup, every WAVE streams its own 16-row tiles with the A
// fragments loaded straight into the MFMA operand layout two tiles ahead, and the only LDS traffic besides the B fragments is a
// wave-private 16 x 64 transposition tile for 16-byte row stores -- no workgroup barrier after the prologue.
// ---------------------------------------------------------------------------------------------------------------------
// K = 16 * KC.  A workgroup owns the NTT column tiles of slab blockIdx.y (its weights: NTT*16 x K floats in LDS); the slabs of
// one row range get workgroup ids that differ by a multiple of 8, i.e. run on the same XCD and re-read the rows from its L2.
// DG = 0: forward (W [Ntot][K]; optional LayerNorm on load, optional exact-GELU second output).
// DG = 1 / 2: dgrad of a Linear, dx = (dy * kscale) @ W with W [K][Ntot] (read transposed into LDS once per workgroup); ln_w
// carries kscale (may be NULL), DG = 2 multiplies by gelu'(aux) with aux = out2 [M][Ntot] (the pre-activation), loaded at the
// START of the tile so that its wait falls behind the tile's MFMAs.
// BF (precision mode bf16): the resident weights are rounded to bf16 ONCE in the prologue (rows of K + 8 bf16: a 4 * odd dword
// stride keeps the ds_read_b64 fragment reads conflict-free), the streamed A fragments are packed in registers, and one
// v_mfma_f32_16x16x16_bf16 replaces the four fp32 MFMAs of a 16-k chunk.
// UF (precision mode bf16, stages 1-2 of the MLP): the pre-activation u is kept ONCE, as fp16 -- ACT stores only fp16(u) through out2
// (no fp32 u, no gelu(u) copy: 2 instead of 8 bytes per hidden element; its consumers apply GELU / GELU' on load), DG = 2 reads it back.
// OB: the output (the gradient du of the dgrad through GELU) is stored as bf16 -- both of its consumers (dgrad of fc1, fc1 weight
// gradient) feed it to bf16 MFMAs, so nothing changes numerically and 4 -> 2 bytes move on the write and on both reads.
// BF / OB are operand / output formats: 0 = fp32, 1 = bf16, 2 = fp16 (forward launches of precision mode 16f: weights and rows packed to fp16,
// the qkv rows stored as fp16)
template <int KC, int NTT, bool LN, bool ACT, int DG = 0, int BF = 0, bool UF = false, int OB = 0>
__global__ __launch_bounds__(256, (KC == 3 && NTT <= 9) ? 3 : 2) void rowstream48_kernel(const float* __restrict__ x, long ldx, float* __restrict__ stats_out,
                                                             const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps,
                                                             const float* __restrict__ W, const float* __restrict__ bias,
                                                             float* __restrict__ out, float* __restrict__ out2, int M, int Ntot) {
    constexpr int K = 16 * KC, LD = K + 8, N = NTT * 16, LDO = 68, NG = (NTT + 3) / 4;
    const int n0 = blockIdx.y * N;                              // first column of this slab
    W += DG ? (long)n0 : (long)n0 * K;
    if (bias) bias += n0;
    if (OB) out = reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(out) + n0);
    else if (!(ACT && UF)) out += n0;
    unsigned short* u16 = reinterpret_cast<unsigned short*>(out2) + n0;      // UF: the fp16 pre-activation [M][Ntot]
    if ((ACT || DG == 2) && !UF) out2 += n0;
    __shared__ __attribute__((aligned(16))) float sW[BF ? (N * LD) / 2 : N * LD];
    __shared__ __attribute__((aligned(16))) float sO[4][16 * LDO];
    unsigned short* sWh = reinterpret_cast<unsigned short*>(sW);        // BF: [N][LD] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    if (DG == 0) {
        for (int e = tid; e < N * (K / 4); e += 256) {
            const int n = e / (K / 4), k4 = (e - n * (K / 4)) * 4;
            if constexpr (BF) *reinterpret_cast<s4*>(&sWh[n * LD + k4]) = pack16_raw<BF>(ld4(W + (long)n * K + k4));
            else *reinterpret_cast<f4*>(&sW[n * LD + k4]) = ld4(W + (long)n * K + k4);
        }
    } else {
        for (int e = tid; e < K * (N / 4); e += 256) {
            const int k = e / (N / 4), n4 = (e - k * (N / 4)) * 4;
            const f4 w = ld4(W + (long)k * Ntot + n4);
            if constexpr (BF) {
                const s4 wh = pack16_raw<BF>(w);
#pragma unroll
                for (int j = 0; j < 4; ++j) sWh[(n4 + j) * LD + k] = (unsigned short)wh[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) sW[(n4 + j) * LD + k] = w[j];
            }
        }
    }
    // everything a tile needs besides its own rows is loaded ONCE: a global load inside the tile loop makes the compiler wait
    // for vmcnt(0) at its first use, i.e. for every prefetched fragment and every store still in flight
    f4 lw[KC], lb[KC], bv[NG];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        lw[c] = (LN || (DG && ln_w)) ? ld4(ln_w + 16 * c + 4 * q) : f4{1.f, 1.f, 1.f, 1.f};
        lb[c] = LN ? ld4(ln_b + 16 * c + 4 * q) : zero4();
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int n = 64 * g + 4 * i;
        bv[g] = (bias && n < N) ? ld4(bias + n) : zero4();
    }
    __syncthreads();
    const int ntiles = (M + 15) / 16;
    const int stride = gridDim.x * 4;
    float* so = sO[wave];
    struct Frag { f4 a[KC]; };
    // branch-free: out-of-range tiles / rows read the last row again (never stored), so the loads carry no select and the
    // compiler has no reason to wait for them before their first real use two tiles later
    auto load = [&](Frag& f, int tile) {
        const long row = min((long)tile * 16 + i, (long)M - 1);
        const float* p = x + row * ldx + 4 * q;
#pragma unroll
        for (int c = 0; c < KC; ++c) f.a[c] = ld4(p + 16 * c);
    };
    // FULL tiles store unconditionally: a store behind a branch is invisible to the compiler's vmcnt bookkeeping, which then
    // waits for (nearly) everything in flight before the next tile's first MFMA
    auto compute = [&](const Frag& f, int tile, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const long row0 = (long)tile * 16;
        // LayerNorm statistics of row i from the fragments themselves (the row's 48 values sit in the 4 lanes i, i+16, i+32,
        // i+48): two-pass mean / variance like the reference's LayerNorm, (mean, rstd) kept for the backward pass
        float mean = 0.f, rstd = 1.f;
        if (LN) {
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < KC; ++c) sum += (f.a[c][0] + f.a[c][1]) + (f.a[c][2] + f.a[c][3]);
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            mean = sum * (1.0f / K);
            float var = 0.f;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const f4 d = f.a[c] - mean;
                var += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
            }
            var += __shfl_xor(var, 16, 64);
            var += __shfl_xor(var, 32, 64);
            rstd = rsqrtf(var * (1.0f / K) + eps);
            if (blockIdx.y == 0 && (FULL || row0 + i < M)) {  // the 4 lanes of a row write the same pair (no q == 0 branch)
                float2 st; st.x = mean; st.y = rstd;
                *reinterpret_cast<float2*>(stats_out + 2 * (row0 + i)) = st;
            }
        }
        // dgrad through GELU: this tile's slice of the pre-activation, in the lane layout of the row stores below
        f4 ug[DG == 2 ? NTT : 1];
        if (DG == 2) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (NTT - 4 * g >= 4) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const long row = FULL ? row0 + q + 4 * p : min(row0 + q + 4 * p, (long)M - 1);
                        if constexpr (UF) ug[4 * g + p] = unpack_h16(*reinterpret_cast<const s4*>(u16 + row * Ntot + 64 * g + 4 * i));
                        else ug[4 * g + p] = ld4(out2 + row * Ntot + 64 * g + 4 * i);
                    }
                } else {
                    const long row = FULL ? row0 + (lane >> 2) : min(row0 + (lane >> 2), (long)M - 1);
                    if constexpr (UF) ug[4 * g] = unpack_h16(*reinterpret_cast<const s4*>(u16 + row * Ntot + 64 * g + 4 * (lane & 3)));
                    else ug[4 * g] = ld4(out2 + row * Ntot + 64 * g + 4 * (lane & 3));
                }
            }
        }
        f4 acc[NTT];
#pragma unroll
        for (int t = 0; t < NTT; ++t) acc[t] = zero4();
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            f4 av = f.a[c];
            if (LN) av = (av - mean) * rstd * lw[c] + lb[c];
            if (DG) av = av * lw[c];
            if constexpr (BF) {
                const s4 pa = pack16<BF>(av);
#pragma unroll
                for (int t = 0; t < NTT; ++t)
                    acc[t] = mfma16_16<BF>(pa, *reinterpret_cast<const s4*>(&sWh[(16 * t + i) * LD + 16 * c + 4 * q]), acc[t]);
            } else {
#pragma unroll
            for (int t = 0; t < NTT; ++t) {
                const f4 b = *reinterpret_cast<const f4*>(&sW[(16 * t + i) * LD + 16 * c + 4 * q]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t] = mfma16(av[j], b[j], acc[t]);
            }
            }
        }
        auto emit = [&](long row, int n, f4 v, const f4& u) {
            if (!FULL && row >= M) return;
            if (DG == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] *= gelu_erf_grad(u[j]);
            }
            if constexpr (ACT && UF) { *reinterpret_cast<s4*>(u16 + row * Ntot + n) = pack_h16(v); return; }
            if constexpr (OB) { *reinterpret_cast<s4*>(reinterpret_cast<unsigned short*>(out) + row * Ntot + n) = pack16<OB>(v); return; }
            *reinterpret_cast<f4*>(out + row * Ntot + n) = v;
            if (ACT) {
                f4 ge;
#pragma unroll
                for (int j = 0; j < 4; ++j) ge[j] = gelu_erf(v[j]);
                *reinterpret_cast<f4*>(out2 + row * Ntot + n) = ge;
            }
        };
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int nt_g = NTT - 4 * g >= 4 ? 4 : NTT - 4 * g;              // column tiles of this group (compile time after unroll)
            // wave-private tile: LDS operations of one wave execute in order, so only the COMPILER must keep write -> read ->
            // write order (no fence: it would drain vmcnt, i.e. the prefetched fragments and the stores in flight)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int t = 4 * g; t < NTT && t < 4 * g + 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) so[(4 * q + r) * LDO + 16 * (t - 4 * g) + i] = acc[t][r];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            if (nt_g == 4) {                                                 // 64 columns: lane = (4 rows q + 4p) x 16-byte column i
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int lr = q + 4 * p;
                    emit(row0 + lr, 64 * g + 4 * i, *reinterpret_cast<const f4*>(&so[lr * LDO + 4 * i]) + bv[g], ug[DG == 2 ? 4 * g + p : 0]);
                }
            } else {                                                         // 16 columns: every lane stores one (row, 16-byte column)
                const int lr = lane >> 2, c4 = lane & 3;
                const f4 b4 = {__shfl(bv[g][0], c4, 64), __shfl(bv[g][1], c4, 64), __shfl(bv[g][2], c4, 64), __shfl(bv[g][3], c4, 64)};
                emit(row0 + lr, 64 * g + 4 * c4, *reinterpret_cast<const f4*>(&so[lr * LDO + 4 * c4]) + b4, ug[DG == 2 ? 4 * g : 0]);
            }
        }
    };
    static_assert(NTT % 4 == 0 || NTT % 4 == 1, "remainder groups of 2 or 3 column tiles are not laid out");
    const int nfull = M / 16;
    int tile = blockIdx.x * 4 + wave;
    Frag f0, f1, f2;
    load(f0, tile);
    load(f1, tile + stride);
    const std::true_type full{};
    while (true) {
        load(f2, tile + 2 * stride);
        if (tile >= nfull) break;
        compute(f0, tile, full); tile += stride;
        load(f0, tile + 2 * stride);
        if (tile >= nfull) { f0 = f1; break; }
        compute(f1, tile, full); tile += stride;
        load(f1, tile + 2 * stride);
        if (tile >= nfull) { f0 = f2; break; }
        compute(f2, tile, full); tile += stride;
    }
    if (tile == nfull && (M & 15)) compute(f0, tile, std::false_type{});       // the ragged last tile, on whichever wave owns it
}

// ---------------------------------------------------------------------------------------------------------------------
// The same streaming scheme for the wide-input, 48-column-output contractions of stage 1 (K = 144 / 192 -> 48):
//   MODE 0: out = res + gamma * (A W^T + bias)      W [48][K]   (fc2 + LayerScale + residual, maxvit.py:268-269)
//   MODE 1: out = A W                                W [K][48]   (dgrad of fc1 / qkv)
//   MODE 2: MODE 1 followed by the LayerNorm backward of the producer in the same epilogue (maxvit.py:267-269: x -> norm ->
//           Linear): dn = A W never leaves the registers; in accumulator layout a lane holds columns 16t + i of rows 4q + r, so
//           the two row means are one 16-lane reduction each, dx = rstd (dn w - mean(dn w) - xhat mean(dn w xhat)) + dres goes
//           through the transposition tile, and dgamma / dbeta accumulate per lane over all tiles (one atomic per column and
//           wave at the end).  xin / stats / dres of the tile are loaded before its MFMAs.
// One wave = one 16-row tile; 48 output columns = 12 float4 per row = 3 per lane (idx = 64 p + lane -> row idx / 12,
// column idx % 12); the residual slice of the tile is loaded before its MFMAs.
// ---------------------------------------------------------------------------------------------------------------------
// AF = 1 (MODE 0, precision mode bf16): x is the fp16 pre-activation of the MLP hidden, A = gelu(x) evaluated on the fragments.
// AF = 2 (MODE 1 / 2): x is a bf16 gradient (du / dqkv): its fragments ARE the MFMA operands.
// NTN = output column tiles: 3 (48 columns, stage 1: 4 waves, two workgroups per CU) or 6 (96 columns, stage 2, bf16 mode with
// 16-bit A rows only: 8 waves, the 75 KB weight tile allows one workgroup per CU).
template <int KC, int MODE, int BF = 0, int AF = 0, int NTN = 3>
__global__ __launch_bounds__(NTN == 3 ? 256 : 512, NTN == 3 ? 2 : 1) void rowstream_narrow_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                  const float* __restrict__ bias, const float* __restrict__ gamma,
                                                                  const float* __restrict__ res, float* __restrict__ out, int M,
                                                                  const float* __restrict__ xin = nullptr,
                                                                  const float* __restrict__ stats = nullptr,
                                                                  float* __restrict__ dgamma = nullptr, float* __restrict__ dbeta = nullptr) {
    constexpr int K = 16 * KC, LD = K + 8, N = 16 * NTN, LDO = N + 4, NWV = NTN == 3 ? 4 : 8, NTHR = 64 * NWV, F4R = N / 4;
    __shared__ __attribute__((aligned(16))) float sW[BF ? (N * LD) / 2 : N * LD];
    __shared__ __attribute__((aligned(16))) float sO[NWV][16 * LDO];
    unsigned short* sWh = reinterpret_cast<unsigned short*>(sW);        // BF: [N][LD] bf16 (see rowstream48_kernel)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    if (MODE == 0) {
        for (int e = tid; e < N * (K / 4); e += NTHR) {
            const int n = e / (K / 4), k4 = (e - n * (K / 4)) * 4;
            if constexpr (BF) *reinterpret_cast<s4*>(&sWh[n * LD + k4]) = pack16_raw<BF>(ld4(W + (long)n * K + k4));
            else *reinterpret_cast<f4*>(&sW[n * LD + k4]) = ld4(W + (long)n * K + k4);
        }
    } else {
        for (int e = tid; e < K * (N / 4); e += NTHR) {
            const int k = e / (N / 4), n4 = (e - k * (N / 4)) * 4;
            const f4 w = ld4(W + (long)k * N + n4);
            if constexpr (BF) {
                const s4 wh = pack16_raw<BF>(w);
#pragma unroll
                for (int j = 0; j < 4; ++j) sWh[(n4 + j) * LD + k] = (unsigned short)wh[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) sW[(n4 + j) * LD + k] = w[j];
            }
        }
    }
    int lr[NTN], c4[NTN];
    f4 b4[NTN], g4[NTN];
#pragma unroll
    for (int p = 0; p < NTN; ++p) {
        const int idx = 64 * p + lane;
        lr[p] = idx / F4R; c4[p] = idx - lr[p] * F4R;
        b4[p] = (MODE == 0 && bias) ? ld4(bias + 4 * c4[p]) : zero4();
        g4[p] = (MODE == 0 && gamma) ? ld4(gamma + 4 * c4[p]) : f4{1.f, 1.f, 1.f, 1.f};
    }
    float lnw[NTN], agam[NTN], abet[NTN];
#pragma unroll
    for (int t = 0; t < NTN; ++t) { lnw[t] = 1.f; agam[t] = 0.f; abet[t] = 0.f; }
    if (MODE == 2) {
#pragma unroll
        for (int t = 0; t < NTN; ++t) lnw[t] = gamma[16 * t + i];                 // LayerNorm weight of column 16t + i
    }
    __syncthreads();
    const int stride = gridDim.x * NWV;
    float* so = sO[wave];
    typedef typename std::conditional<AF != 0, s4, f4>::type AFrag;
    struct Frag { AFrag a[KC]; };
    auto load = [&](Frag& f, int tile) {
        const long row = min((long)tile * 16 + i, (long)M - 1);
        if constexpr (AF) {
            const unsigned short* p = reinterpret_cast<const unsigned short*>(x) + row * K + 4 * q;
#pragma unroll
            for (int c = 0; c < KC; ++c) f.a[c] = *reinterpret_cast<const s4*>(p + 16 * c);
        } else {
            const float* p = x + row * K + 4 * q;
#pragma unroll
            for (int c = 0; c < KC; ++c) f.a[c] = ld4(p + 16 * c);
        }
    };
    auto compute = [&](const Frag& f, int tile, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const long row0 = (long)tile * 16;
        f4 r4[NTN];
        if (MODE == 0 || (MODE == 2 && res)) {
#pragma unroll
            for (int p = 0; p < NTN; ++p) {
                const long row = FULL ? row0 + lr[p] : min(row0 + lr[p], (long)M - 1);
                r4[p] = ld4(res + row * N + 4 * c4[p]);
            }
        }
        float xi[NTN][4], mean[4], rstd[4];
        if (MODE == 2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = FULL ? row0 + 4 * q + r : min(row0 + 4 * q + r, (long)M - 1);
                const float2 st = *reinterpret_cast<const float2*>(stats + 2 * row);
                mean[r] = st.x; rstd[r] = st.y;
#pragma unroll
                for (int t = 0; t < NTN; ++t) xi[t][r] = xin[row * N + 16 * t + i];
            }
        }
        f4 acc[NTN];
#pragma unroll
        for (int t = 0; t < NTN; ++t) acc[t] = zero4();
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            if constexpr (BF) {
                s4 pa;
                if constexpr (AF == 2) pa = f.a[c];
                else if constexpr (AF == 1) {
                    f4 u = unpack_h16(f.a[c]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) u[j] = gelu_erf(u[j]);
                    pa = pack16<BF>(u);
                } else pa = pack16<BF>(f.a[c]);
#pragma unroll
                for (int t = 0; t < NTN; ++t)
                    acc[t] = mfma16_16<BF>(pa, *reinterpret_cast<const s4*>(&sWh[(16 * t + i) * LD + 16 * c + 4 * q]), acc[t]);
            } else if constexpr (AF == 0) {
#pragma unroll
            for (int t = 0; t < NTN; ++t) {
                const f4 b = *reinterpret_cast<const f4*>(&sW[(16 * t + i) * LD + 16 * c + 4 * q]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t] = mfma16(f.a[c][j], b[j], acc[t]);
            }
            }
        }
        if (MODE == 2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = FULL || row0 + 4 * q + r < M;
                float s1 = 0.f, s2 = 0.f, xh[NTN], gw[NTN];
#pragma unroll
                for (int t = 0; t < NTN; ++t) {
                    const float dn = live ? acc[t][r] : 0.f;
                    xh[t] = (xi[t][r] - mean[r]) * rstd[r];
                    gw[t] = dn * lnw[t];
                    agam[t] += dn * xh[t]; abet[t] += dn;
                    s1 += gw[t]; s2 += gw[t] * xh[t];
                }
                s1 = row16_sum(s1) * (1.0f / N);
                s2 = row16_sum(s2) * (1.0f / N);
#pragma unroll
                for (int t = 0; t < NTN; ++t) acc[t][r] = (gw[t] - s1 - xh[t] * s2) * rstd[r];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // wave-private tile: compiler ordering only (see above)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < NTN; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) so[(4 * q + r) * LDO + 16 * t + i] = acc[t][r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int p = 0; p < NTN; ++p) {
            f4 v = *reinterpret_cast<const f4*>(&so[lr[p] * LDO + 4 * c4[p]]);
            if (MODE == 0) v = r4[p] + g4[p] * (v + b4[p]);
            if (MODE == 2 && res) v = v + r4[p];
            if (FULL || row0 + lr[p] < M) *reinterpret_cast<f4*>(out + (row0 + lr[p]) * N + 4 * c4[p]) = v;
        }
    };
    const int nfull = M / 16;
    int tile = blockIdx.x * NWV + wave;
    const std::true_type full{};
    if constexpr (NTN == 3) {                                 // fragments two tiles ahead (three register sets)
        Frag f0, f1, f2;
        load(f0, tile);
        load(f1, tile + stride);
        while (true) {
            load(f2, tile + 2 * stride);
            if (tile >= nfull) break;
            compute(f0, tile, full); tile += stride;
            load(f0, tile + 2 * stride);
            if (tile >= nfull) { f0 = f1; break; }
            compute(f1, tile, full); tile += stride;
            load(f1, tile + 2 * stride);
            if (tile >= nfull) { f0 = f2; break; }
            compute(f2, tile, full); tile += stride;
        }
        if (tile == nfull && (M & 15)) compute(f0, tile, std::false_type{});
    } else {                                                  // 96 columns: one tile ahead (two sets: a third would spill), 8 waves per CU
        Frag f0, f1;
        load(f0, tile);
        while (true) {
            load(f1, tile + stride);
            if (tile >= nfull) break;
            compute(f0, tile, full); tile += stride;
            load(f0, tile + stride);
            if (tile >= nfull) { f0 = f1; break; }
            compute(f1, tile, full); tile += stride;
        }
        if (tile == nfull && (M & 15)) compute(f0, tile, std::false_type{});
    }
    if (MODE == 2) {                                         // column sums of this wave: over the 4 row groups, then one atomic
#pragma unroll
        for (int t = 0; t < NTN; ++t) {
            float a = agam[t], b = abet[t];
            a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
            b += __shfl_xor(b, 16, 64); b += __shfl_xor(b, 32, 64);
            if (q == 0) { atomicAdd(dgamma + 16 * t + i, a); atomicAdd(dbeta + 16 * t + i, b); }
        }
    }
}
static inline bool use_rowstream_narrow(int M, int Kc, int Nout) {
    return M >= 16384 && Nout == 48 && (Kc == 144 || Kc == 192);
}
// stage 2 of RVT-S in precision mode bf16: 16-bit A rows (fp16 hidden, bf16 du / dqkv), 288 / 384 -> 96 columns
static inline bool use_rowstream_narrow96(int M, int Kc, int Nout) {
    return leod_precision() == 1 && M >= 16384 && Nout == 96 && (Kc == 288 || Kc == 384);
}
// (K, N) -> column tiles per slab; 0 = shape not covered.  K = 48: the whole N (9 / 12 tiles); K = 96: slabs of 9 (N = 288) or
// 8 (N = 384) tiles, so that weights + wave tiles of two workgroups fit the 160 KB of a CU
static inline int rowstream_slab(int M, int N, int K) {
    if (M < 16384) return 0;
    if (K == 48 && (N == 144 || N == 192)) return N / 16;                    // RVT-S stage 1
    if (K == 96) return N == 288 ? 9 : (N == 384 ? 8 : 0);       // RVT-S stage 2
    if (K == 64) return N == 192 ? 12 : (N == 256 ? 8 : 0);      // RVT-B stage 1 (qkv whole, fc1 in two slabs)
    return 0;
}
// the grids of the two streaming kernels, for every launch of them
static inline dim3 rowstream48_grid(int KC, int NTT, int M, int Nout) {
    const int per_cu = (KC == 3 && NTT <= 9) ? 3 : 2;        // resident workgroups per CU (registers / LDS): one wave of them
    const int slabs = Nout / (16 * NTT);
    return dim3(min(cdiv(cdiv(M, 16), 4), max(8, (256 * per_cu / slabs) & ~7)), slabs);   // x a multiple of 8: slabs of a row range share an XCD
}
static inline dim3 rowstream_narrow_grid(int M, int NTN) {       // one 16-row tile per wave; NTN = 3: 4 waves, two workgroups per CU, 6: 8 waves, one
    return dim3(NTN == 3 ? min(cdiv(cdiv(M, 16), 4), 256 * 2) : min(cdiv(cdiv(M, 16), 8), 256));
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward and input-gradient entry points of the Linear layers: one description (LinearProb), one router (linear_route), one launch
// switch (launch_linear).  What differs between the entry points is the data of kLinearEntry.
// ---------------------------------------------------------------------------------------------------------------------
enum LinearEntry : int { LE_LN_LINEAR = 0, LE_LSRES, LE_LN_GELU16, LE_LN_BF16, LE_LSRES_BF16, LE_LSRES_GELU16, LE_DGRAD, LE_DGRAD_LNBWD, LE_DGRAD_GELU16, LE_COUNT };
constexpr unsigned rs_bit(int KC, int NTT) { return 1u << ((KC == 3 ? 0 : KC == 6 ? 2 : 4) + (NTT == 9 || (KC == 4 && NTT == 12) ? 0 : 1)); }
constexpr unsigned kRsFc1 = rs_bit(3, 12) | rs_bit(6, 8) | rs_bit(4, 8), kRsQkv = rs_bit(3, 9) | rs_bit(6, 9) | rs_bit(4, 12);
struct LinearEntryInfo {
    bool dgrad, lsres;              // reads W[N][K] transposed (BLTrans) | EpLsRes epilogue (else EpStore)
    int kc_mask, lda_mask;          // alignment of the contraction length and the A row stride: LEOD_ERR_ARG
    int needs16;                    // what the entry returns in precision mode f32 (0: it runs there)
    unsigned rs_pairs;              // the (KC, NTT) pairs of rowstream48_kernel it is instantiated for
    bool rs_commits, rs_ln_only;    // a shape rowstream_slab covers never tries the GEMMs | only with LayerNorm
    bool narrow, narrow96, generic16, gemm16;   // rowstream_narrow 48 / 96 columns; 16-bit store: widths % 4; register-direct gemm16 (else refuse)
};
constexpr LinearEntryInfo kLinearEntry[LE_COUNT] = {
    /* leod_ln_linear_fwd           */ {false, false, 3, 3, 0, kRsFc1 | kRsQkv, false, false, false, false, false, true},
    /* leod_linear_lsres_fwd        */ {false, true, 3, 0, 0, 0, false, false, true, false, false, true},
    /* leod_ln_linear_gelu16_fwd    */ {false, false, 0, 0, LEOD_ERR_UNSUPPORTED, kRsFc1, true, false, false, false, true, false},
    /* leod_ln_linear_bf16_fwd      */ {false, false, 0, 0, LEOD_ERR_UNSUPPORTED, kRsQkv, true, true, false, false, true, false},
    /* leod_linear_lsres_bf16_fwd   */ {false, true, 7, 0, LEOD_ERR_ARG, 0, false, false, false, false, false, false},
    /* leod_linear_lsres_gelu16_fwd */ {false, true, 3, 0, LEOD_ERR_ARG, 0, false, false, true, true, false, true},
    /* leod_linear_dgrad            */ {true, false, 3, 3, 0, kRsFc1, false, false, true, false, false, true},
    /* leod_linear_dgrad_lnbwd      */ {true, false, 0, 0, 0, 0, false, false, true, true, false, false},
    /* leod_linear_dgrad_gelu16     */ {true, false, 0, 0, LEOD_ERR_ARG, kRsFc1, true, false, false, false, true, false},
};

// A forward or input-gradient problem, fully described: out[M, nout] = A[M, kc] (x) W, W[nout][kc] forward, W[kc][nout] dgrad.
struct LinearProb {
    int entry;                      // LinearEntry
    int M, kc, nout;                // rows, contraction length, output columns
    int a_fmt; long lda; bool a_dense;          // RowFmt of the A rows, their stride, lda == kc
    bool ln, stats;                 // LayerNorm on load | (mean, rstd) can be had (stats_out of a forward, the saved ones of a backward)
    bool kscale;
    int act, aux_fmt, out_fmt;      // ACT_NONE | ACT_GELU_DUAL | ACT_MUL_GELU_GRAD, RowFmt of aux and of the stored rows
    bool tout;                      // EpLsRes: t is wanted too
    bool dx2, colsum, accumulate, dres, out_dense; int nsplit;  // leod_linear_dgrad's extras: each bars the streaming kernels
};
// from the integers and flags of the C ABI (leod_linear_route has the same arguments): a16 / out16 = the entry's 16-bit option for the A rows
// (dy_fmt, dy_bf16) / the stored rows (dx_fmt, out_bf16), ldo the stride of the stored rows
enum : int { LF_LN = 1, LF_STATS = 2, LF_KSCALE = 4, LF_AUX = 8, LF_TOUT = 16, LF_DX2 = 32, LF_COLSUM = 64, LF_ACCUMULATE = 128, LF_DRES = 256 };
static LinearProb linear_prob(int entry, int M, int N, int K, long lda, long ldo, int a16, int out16, int flags, int nsplit) {
    const LinearEntryInfo& e = kLinearEntry[entry];
    const bool h16 = leod_opfmt() == 2;             // forward launch of precision mode 16f: the 16-bit activations are fp16
    LinearProb p{};
    p.entry = entry; p.M = M; p.kc = e.dgrad ? N : K; p.nout = e.dgrad ? K : N;
    p.lda = lda; p.a_dense = lda == p.kc; p.out_dense = ldo == p.nout;
    p.a_fmt = entry == LE_LSRES_BF16 ? (h16 ? FMT_F16 : FMT_BF16) : entry == LE_LSRES_GELU16 ? FMT_F16PRE : a16 ? FMT_BF16 : FMT_F32;
    p.out_fmt = entry == LE_LN_GELU16 ? FMT_F16PRE : entry == LE_LN_BF16 ? (h16 ? FMT_F16PRE : FMT_BF16) : out16 ? FMT_BF16 : FMT_F32;
    p.ln = flags & LF_LN; p.stats = flags & LF_STATS; p.kscale = flags & LF_KSCALE; p.tout = flags & LF_TOUT;
    p.act = (flags & LF_AUX) ? (e.dgrad ? ACT_MUL_GELU_GRAD : ACT_GELU_DUAL) : ACT_NONE;
    p.aux_fmt = entry == LE_DGRAD_GELU16 ? FMT_F16PRE : FMT_F32;
    p.dx2 = flags & LF_DX2; p.colsum = flags & LF_COLSUM; p.accumulate = flags & LF_ACCUMULATE; p.dres = flags & LF_DRES; p.nsplit = nsplit;
    return p;
}

// The one routing function of the Linear forward / dgrad entries: the described problem -> the kernel that runs it, as a route code.
// Row-streaming kernels first (stages 1-2), then the LDS-staged GEMMs (rows_gemm_kind, gemm16.hpp), then the register-direct one.  It
// launches nothing and reads no device memory; the operand format (fp32 / bf16 / fp16) is the precision mode's and not part of the code:
//   1000 + 100 KC + NTT    rowstream48_kernel<KC, NTT>: contraction 16 KC, slabs of NTT column tiles
//   2000 + KC              rowstream_narrow_kernel<KC>: KC = 9 / 12 -> 48 columns, 18 / 24 -> 96 columns
//   3000 + NTW             gemm_wide_bf16_kernel<NTW> (3 | 4)
//   4000 + 100 NT + KCH    gemm_lds_kernel<NT, KCH> with the two-phase loader ALRowsM (KCH 48 | 64)
//   5000 + 100 NT + KCH    gemm_lds_kernel<NT, KCH> with the plain loader ALRows
//   6000 + 10 NT + KS      gemm16_kernel<NT, KS> (KS = 4: K split over the waves, else 1)
//   0                      M <= 0: nothing to do, the entry returns LEOD_OK
//   < 0                    LEOD_ERR_*: what the entry returns
enum : int { LR_RS48 = 1000, LR_NARROW = 2000, LR_WIDE = RG_WIDE, LR_LDS2P = RG_TWO_PHASE, LR_LDS = RG_PLAIN, LR_GEMM16 = 6000 };
static int linear_route(const LinearProb& p) {
    const LinearEntryInfo& e = kLinearEntry[p.entry];
    const bool bf = leod_precision() == 1, a_bf16 = p.a_fmt == FMT_BF16;
    const int M = p.M, kc = p.kc, nout = p.nout;
    if ((kc & e.kc_mask) || (p.lda & e.lda_mask)) return LEOD_ERR_ARG;
    if (e.needs16 && !bf) return e.needs16;
    if (p.entry == LE_DGRAD_LNBWD) {                // the narrow kernel with the LayerNorm backward in its epilogue, or nothing
        if (M <= 0) return 0;
        if (a_bf16 && use_rowstream_narrow96(M, kc, nout)) return LR_NARROW + kc / 16;
        if (!use_rowstream_narrow(M, kc, nout)) return LEOD_ERR_UNSUPPORTED;
        return (a_bf16 && !bf) ? LEOD_ERR_ARG : LR_NARROW + kc / 16;         // bf16 dy in mode f32: refused only after the narrow test
    }
    const int nt = pick_nt(nout), nbn = cdiv(nout, 16 * nt);
    const bool lds = use_gemm_lds(M, nbn) && (!p.ln || p.stats), out16 = p.out_fmt != FMT_F32;
    const bool extras = p.dx2 || p.colsum || p.accumulate || p.dres || p.nsplit > 0;
    if (p.entry == LE_DGRAD) {                      // dx_fmt = 1 runs on the LDS path or not at all
        if (out16 && (!bf || extras || p.act || (nout & 3) || !lds)) return LEOD_ERR_UNSUPPORTED;
        if (p.dres && (p.nsplit > 0 || p.accumulate)) return LEOD_ERR_ARG;
    }
    if (M <= 0) return 0;                           // no rows: every entry returns LEOD_OK, also those that have no kernel for small M
    if (!a_bf16 && p.a_dense && p.out_dense && !extras && (!p.ln || p.stats) && !(p.entry == LE_DGRAD && out16)) {
        if (e.narrow && !p.tout && !p.kscale && !p.act) {
            if (e.narrow96 && kc == 384 && use_rowstream_narrow96(M, kc, nout)) return LR_NARROW + 24;
            if (use_rowstream_narrow(M, kc, nout)) return LR_NARROW + kc / 16;
        }
        if (const int slab = (e.rs_pairs && (p.ln || !e.rs_ln_only)) ? rowstream_slab(M, nout, kc) : 0) {
            if (e.rs_pairs & rs_bit(kc / 16, slab)) return LR_RS48 + 100 * (kc / 16) + slab;
            if (e.rs_commits) return LEOD_ERR_UNSUPPORTED;
        }
    }
    if (e.generic16 && ((kc | nout) & 3)) return LEOD_ERR_UNSUPPORTED;
    if (lds) {
        const int kind = rows_gemm_kind(M, kc, nout, nt, e.dgrad, e.lsres, p.a_fmt, p.ln, p.stats, p.kscale, p.act == ACT_MUL_GELU_GRAD);
        return kind < RG_TWO_PHASE ? kind : kind + 100 * nt + gemm_lds_kch(kc);
    }
    return e.gemm16 ? LR_GEMM16 + 10 * nt + (gemm16_ksplit(M, kc, nbn) ? 4 : 1) : LEOD_ERR_UNSUPPORTED;
}

// the device pointers of a problem (what LinearProb only knows the presence of)
struct LinearArgs {
    const void* a; const float* ln_w; const float* ln_b; float eps; const float* kscale;    // A rows, LayerNorm on load, per-k scale
    const float* W; const float* bias; const float* gamma; const float* res;                // EpLsRes: gamma, res (lnbwd: LayerNorm weight, dres)
    void* out; long ldo; void* out2; long ld2;      // stored rows; second output: gelu(out) | t | dx2
    float* stats; const void* aux;                  // (mean, rstd): written by a forward, read by lnbwd | pre-activation of ACT_MUL_GELU_GRAD
    float* colsum; const float* dres;               // leod_linear_dgrad
    const float* xin; float* dgamma; float* dbeta;  // leod_linear_dgrad_lnbwd
};
// ... and the switch that launches what linear_route decided.  E (LinearEntry) is a template argument so that a translation unit holds
// the kernels of its own entries only.  Not a route: the launchers replace fp32 weights by their 16-bit shadow (bl_shadow_ptr) when the
// weights lie in a registered buffer whose shadow is fresh -- a loader type picked from runtime state, same values, same kernel family.
template <int E, int KC, int NTT>
static int launch_rowstream48(const LinearProb& p, const LinearArgs& a, hipStream_t s) {
    const dim3 grid = rowstream48_grid(KC, NTT, p.M, p.nout);
    const float* x = reinterpret_cast<const float*>(a.a);
    float* out = reinterpret_cast<float*>(a.out); float* out2 = reinterpret_cast<float*>(a.out2);
    float* aux = reinterpret_cast<float*>(const_cast<void*>(a.aux));
#define RS48(LNV, ACTV, DGV, BFV, UFV, OBV, ...) \
    hipLaunchKernelGGL((rowstream48_kernel<KC, NTT, LNV, ACTV, DGV, BFV, UFV, OBV>), grid, dim3(256), 0, s, x, p.lda, __VA_ARGS__, p.M, p.nout)
#define RS48_FWD(LNV, ACTV, BFV, UFV, OBV, ST, OUT, OUT2) RS48(LNV, ACTV, 0, BFV, UFV, OBV, ST, a.ln_w, a.ln_b, a.eps, a.W, a.bias, OUT, OUT2)
#define RS48_DG(DGV, BFV, UFV, OBV) RS48(false, false, DGV, BFV, UFV, OBV, nullptr, a.kscale, nullptr, 0.f, a.W, nullptr, out, aux)
    if constexpr (E == LE_LN_LINEAR) {              // the kernel derives (mean, rstd) itself and leaves them in stats
        LEOD_BY_OPFMT({
            if (p.ln && out2) RS48_FWD(true, true, OF, false, 0, a.stats, out, out2);
            else if (p.ln) RS48_FWD(true, false, OF, false, 0, a.stats, out, nullptr);
            else if (out2) RS48_FWD(false, true, OF, false, 0, nullptr, out, out2);
            else RS48_FWD(false, false, OF, false, 0, nullptr, out, nullptr);
        });
    } else if constexpr (E == LE_LN_GELU16) { LEOD_BY_OPFMT16(RS48_FWD(true, true, OF, true, 0, a.stats, nullptr, out));
    } else if constexpr (E == LE_LN_BF16) { LEOD_BY_OPFMT16(RS48_FWD(true, false, OF, false, OF, a.stats, out, nullptr));
    } else if constexpr (E == LE_DGRAD) {
        if (leod_precision() == 1) { if (aux) RS48_DG(2, 1, false, 0); else RS48_DG(1, 1, false, 0); }
        else { if (aux) RS48_DG(2, 0, false, 0); else RS48_DG(1, 0, false, 0); }
    } else if constexpr (E == LE_DGRAD_GELU16) {
        if (p.out_fmt == FMT_BF16) RS48_DG(2, 1, true, 1); else RS48_DG(2, 1, true, 0);
    }
#undef RS48_DG
#undef RS48_FWD
#undef RS48
    return leod_launch_status();
}
template <int E, int KC>
static int launch_rowstream_narrow(const LinearProb& p, const LinearArgs& a, hipStream_t s) {
    constexpr int NTN = KC >= 18 ? 6 : 3;
    const dim3 grid = rowstream_narrow_grid(p.M, NTN);
#define NARROW(MODEV, BFV, AFV) hipLaunchKernelGGL((rowstream_narrow_kernel<KC, MODEV, BFV, AFV, NTN>), grid, dim3(NTN == 3 ? 256 : 512), 0, s, reinterpret_cast<const float*>(a.a), \
                                                   a.W, a.bias, a.gamma, a.res, reinterpret_cast<float*>(a.out), p.M, a.xin, a.stats, a.dgamma, a.dbeta)
    if constexpr (E == LE_LSRES) { LEOD_BY_OPFMT(NARROW(0, OF, 0)); }
    else if constexpr (E == LE_LSRES_GELU16) { LEOD_BY_OPFMT16(NARROW(0, OF, 1)); }
    else if constexpr (E == LE_DGRAD) { LEOD_BY_OPFMT_IF(false, NARROW(1, OF, 0)); }
    else if constexpr (E == LE_DGRAD_LNBWD) {
        if (p.a_fmt == FMT_BF16) NARROW(2, 1, 2);
        else if constexpr (NTN == 3) { if (leod_precision() == 1) NARROW(2, 1, 0); else NARROW(2, 0, 0); }
    }
#undef NARROW
    return leod_launch_status();
}
template <int E>
static int launch_linear(int route, const LinearProb& p, const LinearArgs& a, hipStream_t s) {
    if (route <= 0) return route;
    static constexpr LinearEntryInfo e = kLinearEntry[E];
    const int par = route % 1000;
    if (route < LR_NARROW) {
#define RS_CASE(KCV, NTTV) if constexpr ((e.rs_pairs & rs_bit(KCV, NTTV)) != 0) { if (par == 100 * KCV + NTTV) return launch_rowstream48<E, KCV, NTTV>(p, a, s); }
        RS_CASE(3, 9) RS_CASE(3, 12) RS_CASE(6, 9) RS_CASE(6, 8) RS_CASE(4, 12) RS_CASE(4, 8)
#undef RS_CASE
        return LEOD_ERR_ARG;
    }
    if (route < LR_WIDE) {
        if constexpr (e.narrow) {
            if (par == 9) return launch_rowstream_narrow<E, 9>(p, a, s);
            if (par == 12) return launch_rowstream_narrow<E, 12>(p, a, s);
        }
        if constexpr (e.narrow96) {
            if (par == 24) return launch_rowstream_narrow<E, 24>(p, a, s);
            if constexpr (E == LE_DGRAD_LNBWD) { if (par == 18) return launch_rowstream_narrow<E, 18>(p, a, s); }
        }
        return LEOD_ERR_ARG;
    }
    if constexpr (E != LE_DGRAD_LNBWD) {
        typedef typename std::conditional<e.dgrad, BLTrans, BLRows>::type BL;
        const int M = p.M, kc = p.kc, nout = p.nout;
        ALRows al{}; al.x = reinterpret_cast<const float*>(a.a); al.ld = p.lda; al.ln_w = a.ln_w; al.ln_b = a.ln_b; al.eps = a.eps;
        al.kscale = a.kscale; al.stats_out = a.stats; al.K = kc; al.fmt = p.a_fmt;
        auto launch = [&](const auto& ep) {
            int rc = LEOD_OK;
            if (route < LR_GEMM16) {                // LayerNorm on load: the LDS-staged kernels read (mean, rstd) that a launch of their own leaves in stats
                if (p.ln) { rc = launch_row_stats(al.x, p.lda, a.stats, M, kc, a.eps, s); if (rc) return rc; al.stats_in = a.stats; }
                const int kind = route < LR_LDS2P ? route : route / 1000 * 1000;
                DISPATCH_NT(pick_nt(nout), { BL bl{a.W, (long)(e.dgrad ? nout : kc), nout, NT}; rc = launch_gemm_lds<NT>(kind, al, bl, ep, M, kc, cdiv(nout, 16 * NT), s); });
            } else if constexpr (e.gemm16) {
                DISPATCH_NT(pick_nt(nout), { BL bl{a.W, (long)(e.dgrad ? nout : kc), nout, NT}; rc = launch_gemm16<NT>(al, bl, ep, M, kc, cdiv(nout, 16 * NT), s); });
            } else rc = LEOD_ERR_ARG;
            return rc;
        };
        if constexpr (e.lsres) return launch(EpLsRes{reinterpret_cast<float*>(a.out), reinterpret_cast<float*>(a.out2), a.res, a.bias, a.gamma, (long)nout, nout});
        else {
            EpStore ep = ep_store(reinterpret_cast<float*>(a.out), a.ldo, nout);
            ep.bias = a.bias; ep.out_fmt = p.out_fmt; ep.out2 = reinterpret_cast<float*>(a.out2); ep.ld2 = a.ld2; ep.nsplit = p.nsplit;
            ep.act = p.act; ep.aux = reinterpret_cast<const float*>(a.aux); ep.ldaux = nout; ep.aux_fmt = p.aux_fmt;
            ep.accumulate = p.accumulate; ep.colsum = a.colsum; ep.addsrc = a.dres;
            return launch(ep);
        }
    }
    return LEOD_ERR_ARG;
}
