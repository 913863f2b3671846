// Token-row contractions of the RVT backbone, forward entry points of the 16-bit precision modes whose inputs / outputs are 16-bit rows (fp16 MLP hidden, bf16 / fp16 qkv and attention output).  All tensors channels-last ("rows" = tokens of an NHWC map).
// C-ABI declared in include/leod_hip.h.
#include "linear_common.hpp"

// ---------------------------------------------------------------------------------------------------------------------
// Precision mode bf16, stages 1-2: the MLP hidden u = LN(x) W1^T + b1 is stored ONCE as fp16 (as the reference does under
// autocast); fc2, the dgrad through GELU and the fc2 weight gradient evaluate GELU / GELU' on load.  8 -> 2 bytes per hidden
// element in the forward pass, 4 -> 2 on each of its three reads.
// Generic 16-bit producers (round 3: stages 3-4 and every geometry the row-streaming kernels do not cover): the LDS-staged / wide-tile
// GEMMs with a 16-bit row epilogue, fp16 for the MLP hidden pre-activation, bf16 (fp16 in precision mode 16f) for qkv.
// ---------------------------------------------------------------------------------------------------------------------
// u16[M,N] = fp16(LN(x) W^T + bias); stats_out [M,2].  LEOD_ERR_UNSUPPORTED where no 16-bit kernel covers (M, N, K)
// -- the caller then uses leod_ln_linear_fwd with its fp32 (u, gelu(u)) pair.
LEOD_API int leod_ln_linear_gelu16_fwd(const float* x, const float* ln_w, const float* ln_b, float eps, const float* W, const float* bias,
                                       void* u16, float* stats_out, int M, int N, int K, hipStream_t stream) {
    LeodFwdScope fwd_scope;                                   // forward contraction: fp16 operands in precision mode 16f
    if (!x || !W || !u16 || !ln_w || !stats_out) return LEOD_ERR_ARG;
    const LinearProb p = linear_prob(LE_LN_GELU16, M, N, K, K, N, 0, 0, LF_LN | LF_STATS, 0);
    LinearArgs a{}; a.a = x; a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps; a.W = W; a.bias = bias; a.out = u16; a.ldo = N; a.stats = stats_out;
    return launch_linear<LE_LN_GELU16>(linear_route(p), p, a, stream);
}

// out16[M,N] = bf16(LN(x) W^T + bias) (the qkv rows of stages 1-2: q, k, v only ever enter bf16 MFMAs); stats_out [M,2]; ln_w may be NULL
// (plain rows).  The stored rows are the attention kernels' MFMA operands: bf16, or fp16 in precision mode 16f
LEOD_API int leod_ln_linear_bf16_fwd(const float* x, const float* ln_w, const float* ln_b, float eps, const float* W, const float* bias,
                                     void* out16, float* stats_out, int M, int N, int K, hipStream_t stream) {
    LeodFwdScope fwd_scope;                                   // forward contraction: fp16 operands in precision mode 16f
    if (!x || !W || !out16 || (ln_w && !stats_out)) return LEOD_ERR_ARG;
    const LinearProb p = linear_prob(LE_LN_BF16, M, N, K, K, N, 0, 0, (ln_w ? LF_LN : 0) | (stats_out ? LF_STATS : 0), 0);
    LinearArgs a{}; a.a = x; a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps; a.W = W; a.bias = bias; a.out = out16; a.ldo = N; a.stats = stats_out;
    return launch_linear<LE_LN_BF16>(linear_route(p), p, a, stream);
}

// out = res + gamma * (a16 W^T + bias) with bf16 rows a16 (fp16 in precision mode 16f: proj + LayerScale + residual on the attention output)
LEOD_API int leod_linear_lsres_bf16_fwd(const void* a16, const float* W, const float* bias, const float* gamma, const float* res,
                                        float* out, int M, int N, int K, hipStream_t stream) {
    LeodFwdScope fwd_scope;                                   // forward contraction: fp16 operands in precision mode 16f
    if (!a16 || !W || !res || !out) return LEOD_ERR_ARG;
    const LinearProb p = linear_prob(LE_LSRES_BF16, M, N, K, K, N, 0, 0, 0, 0);
    LinearArgs a{}; a.a = a16; a.W = W; a.bias = bias; a.gamma = gamma; a.res = res; a.out = out; a.ldo = N;
    return launch_linear<LE_LSRES_BF16>(linear_route(p), p, a, stream);
}

// out = res + gamma * (gelu(u16) W^T + bias)     (fc2 + LayerScale + residual on the fp16 pre-activation)
LEOD_API int leod_linear_lsres_gelu16_fwd(const void* u16, const float* W, const float* bias, const float* gamma, const float* res,
                                          float* out, int M, int N, int K, hipStream_t stream) {
    LeodFwdScope fwd_scope;                                   // forward contraction: fp16 operands in precision mode 16f
    if (!u16 || !W || !res || !out) return LEOD_ERR_ARG;
    const LinearProb p = linear_prob(LE_LSRES_GELU16, M, N, K, K, N, 0, 0, 0, 0);
    LinearArgs a{}; a.a = u16; a.W = W; a.bias = bias; a.gamma = gamma; a.res = res; a.out = out; a.ldo = N;
    return launch_linear<LE_LSRES_GELU16>(linear_route(p), p, a, stream);
}
