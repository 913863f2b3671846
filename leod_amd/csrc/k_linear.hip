// Token-row contractions of the RVT backbone, forward with fp32 tensors: LayerNorm->Linear(+GELU), Linear->LayerScale+residual, the fused ConvLSTM cell.  All tensors channels-last ("rows" = tokens of an NHWC map).
// C-ABI declared in include/leod_hip.h.
#include "linear_common.hpp"

// out[M,N] = LN(x)[M,K] @ W[N,K]^T + bias ; optionally also out_act = gelu(out)
// ln_w == NULL -> no LayerNorm.  stats_out (optional) [M,2] = (mean, rstd) for the backward pass.
// Reference: models/layers/maxvit/maxvit.py:267-269 (norm1 -> qkv, :347) and :110-118 (norm2 -> fc1 -> GELU)
LEOD_API int leod_ln_linear_fwd(const float* x, long ldx, const float* ln_w, const float* ln_b, float eps,
                                const float* W, const float* bias, float* out, float* out_act, float* stats_out,
                                int M, int N, int K, hipStream_t stream) {
    LeodFwdScope fwd_scope;                                   // forward contraction: fp16 operands in precision mode 16f
    if (!x || !W || !out) return LEOD_ERR_ARG;
    const LinearProb p = linear_prob(LE_LN_LINEAR, M, N, K, ldx, N, 0, 0, (ln_w ? LF_LN : 0) | (stats_out ? LF_STATS : 0) | (out_act ? LF_AUX : 0), 0);
    LinearArgs a{}; a.a = x; a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps; a.W = W; a.bias = bias; a.out = out; a.ldo = N; a.out2 = out_act; a.ld2 = N;
    a.stats = stats_out;
    return launch_linear<LE_LN_LINEAR>(linear_route(p), p, a, stream);
}

// t = a @ W^T + bias ; tout = t (optional) ; out = res + gamma * t        (maxvit.py:268-269, LayerScale :51-53)
LEOD_API int leod_linear_lsres_fwd(const float* a, const float* W, const float* bias, const float* gamma,
                                   const float* res, float* out, float* tout, int M, int N, int K, hipStream_t stream) {
    LeodFwdScope fwd_scope;                                   // forward contraction: fp16 operands in precision mode 16f
    if (!a || !W || !res || !out) return LEOD_ERR_ARG;
    const LinearProb p = linear_prob(LE_LSRES, M, N, K, K, N, 0, 0, tout ? LF_TOUT : 0, 0);
    LinearArgs g{}; g.a = a; g.W = W; g.bias = bias; g.gamma = gamma; g.res = res; g.out = out; g.ldo = N; g.out2 = tout;
    return launch_linear<LE_LSRES>(linear_route(p), p, g, stream);
}

// The kernel one of the nine Linear forward / dgrad entries runs for a problem in the current precision mode, without launching anything:
// the code of linear_route (linear_common.hpp: 1000 + 100 KC + NTT rowstream48, 2000 + KC rowstream_narrow, 3000 + NTW wide tile,
// 4000 / 5000 + 100 NT + KCH LDS-staged with the two-phase / plain loader, 6000 + 10 NT + KS gemm16, < 0 the error the call returns).
// entry: 0 ln_linear_fwd, 1 linear_lsres_fwd, 2 ln_linear_gelu16_fwd, 3 ln_linear_bf16_fwd, 4 linear_lsres_bf16_fwd,
// 5 linear_lsres_gelu16_fwd, 6 linear_dgrad, 7 linear_dgrad_lnbwd, 8 linear_dgrad_gelu16.  M, N, K as the entry takes them; lda / ldo:
// strides of the A rows (x, a, dy) and of the stored rows; a16 / out16: dy_fmt | dy_bf16 / dx_fmt | out_bf16; flags: 1 ln_w, 2 stats_out |
// stats, 4 kscale, 8 out_act | aux_u, 16 tout, 32 dx2, 64 colsum, 128 accumulate, 256 dres.  The entries switch on the same value.
LEOD_API int leod_linear_route(int entry, int M, int N, int K, long lda, long ldo, int a16, int out16, int flags, int nsplit) {
    if (entry < 0 || entry >= LE_COUNT) return LEOD_ERR_ARG;
    if (kLinearEntry[entry].dgrad) return linear_route(linear_prob(entry, M, N, K, lda, ldo, a16, out16, flags, nsplit));
    LeodFwdScope fwd_scope;
    return linear_route(linear_prob(entry, M, N, K, lda, ldo, a16, out16, flags, nsplit));
}

// Fused ConvLSTM cell (models/layers/rnn.py:37-70, dws_conv=False): gates = [x | h_prev] @ W[4C,2C]^T + b,
// (f,i,o) = sigmoid, g = tanh, c = f*c_prev + i*g, h = o*tanh(c).  h_prev/c_prev NULL = zero state.
// gates_out (optional) [M,4,C] keeps the post-activation gates for the backward pass.
LEOD_API int leod_convlstm_fwd(const float* x, const float* h_prev, const float* c_prev, const float* W,
                               const float* bias, float* h_out, float* c_out, float* gates_out, int M, int C,
                               hipStream_t stream) {
    LeodFwdScope fwd_scope;                                   // forward contraction: fp16 operands in precision mode 16f
    if (!x || !W || !bias || !h_out || !c_out || (C & 15)) return LEOD_ERR_ARG;
    ALConcat2 al{x, (long)C, C, h_prev, (long)C};
    BLGates bl{W, (long)2 * C, C};
    EpLstm ep{bias, c_prev, h_out, c_out, gates_out, C};
    // a zero initial state contributes nothing: stop the contraction at K = C
    const int K = h_prev ? 2 * C : C;
    if (use_gemm_lds(M, C / 16)) return launch_gemm_lds<4>(al, bl, ep, M, K, C / 16, stream);
    return launch_gemm16<4>(al, bl, ep, M, K, C / 16, stream);
}
