// Token-row contractions of the RVT backbone: input gradients (dgrad) of the Linear layers, plain / through GELU / with the LayerNorm backward of the producer in the epilogue.  All tensors channels-last ("rows" = tokens of an NHWC map).
// C-ABI declared in include/leod_hip.h.
#include "linear_common.hpp"

// dx[M,K] (=|+=) (dy[M,N] * kscale[N]) @ W[N,K]          (dgrad of y = x W^T).  dy_fmt: 0 fp32 rows, 1 bf16 rows; dx_fmt: 0 fp32, 1 dx is
// written as bf16 rows (row-epilogue kernels only)
//   aux_u != NULL : dx *= gelu'(aux_u[M,K])                (through GELU, maxvit.py:107)
//   nsplit > 0    : columns >= nsplit go to dx2[M, K-nsplit] (ConvLSTM: [dx | dh_prev])
//   colsum != NULL: colsum[K] += column sums of the stored dx (bias gradient of the producer)
LEOD_API int leod_linear_dgrad(const float* dy, long lddy, const float* kscale, const float* W, float* dx, long lddx,
                               float* dx2, long lddx2, int nsplit, const float* aux_u, float* colsum,
                               int accumulate, const float* dres, int M, int N, int K, int dy_fmt, int dx_fmt, hipStream_t stream) {
    if (!dy || !W || !dx || (dy_fmt != 0 && dy_fmt != 1) || (dx_fmt != 0 && dx_fmt != 1)) return LEOD_ERR_ARG;
    const int flags = (kscale ? LF_KSCALE : 0) | (aux_u ? LF_AUX : 0) | (dx2 ? LF_DX2 : 0) | (colsum ? LF_COLSUM : 0) | (accumulate ? LF_ACCUMULATE : 0) | (dres ? LF_DRES : 0);
    const LinearProb p = linear_prob(LE_DGRAD, M, N, K, lddy, lddx, dy_fmt, dx_fmt, flags, nsplit);
    LinearArgs a{}; a.a = dy; a.kscale = kscale; a.W = W; a.out = dx; a.ldo = lddx; a.out2 = dx2; a.ld2 = lddx2; a.aux = aux_u; a.colsum = colsum; a.dres = dres;
    return launch_linear<LE_DGRAD>(linear_route(p), p, a, stream);
}

// dx[M,K] = LayerNorm backward of (dy[M,N] @ W[N,K]) in one pass: dn = dy W stays in registers, dx = rstd (dn w - mean(dn w) -
// xhat mean(dn w xhat)) (+ dres), dgamma[K] += sum_m dn xhat, dbeta[K] += sum_m dn   (x[M,K] = the LayerNorm input, stats[M,2] =
// its saved (mean, rstd)).  Covers K = 48 with N = 144 / 192 and M >= 16384 (stage 1; bf16 dy in precision mode bf16: also K = 96 with
// N = 288 / 384); LEOD_ERR_UNSUPPORTED otherwise -- the caller then runs leod_linear_dgrad + leod_layernorm_bwd.
LEOD_API int leod_linear_dgrad_lnbwd(const float* dy, const float* W, const float* x, const float* stats, const float* ln_w,
                                     const float* dres, float* dx, float* dgamma, float* dbeta, int M, int N, int K, int dy_bf16,
                                     hipStream_t stream) {
    if (!dy || !W || !x || !stats || !ln_w || !dx || !dgamma || !dbeta) return LEOD_ERR_ARG;
    const LinearProb p = linear_prob(LE_DGRAD_LNBWD, M, N, K, N, K, dy_bf16, 0, LF_STATS | (dres ? LF_DRES : 0), 0);
    LinearArgs a{}; a.a = dy; a.W = W; a.gamma = ln_w; a.res = dres; a.out = dx; a.ldo = K; a.stats = const_cast<float*>(stats); a.xin = x; a.dgamma = dgamma; a.dbeta = dbeta;
    return launch_linear<LE_DGRAD_LNBWD>(linear_route(p), p, a, stream);
}

// du[M,K] = ((dy[M,N] * kscale[N]) @ W[N,K]) * gelu'(u16[M,K])      (dgrad of fc2 through GELU, fp16 pre-activation; the row-streaming
// kernel on the stage 1-2 shapes, else (stages 3-4) the LDS-staged / wide-tile dgrad with gelu'(fp16 u) and the 16-bit store in the row epilogue)
LEOD_API int leod_linear_dgrad_gelu16(const float* dy, const float* kscale, const float* W, const void* u16, void* dx,
                                      int M, int N, int K, int out_bf16, hipStream_t stream) {
    if (!dy || !W || !u16 || !dx) return LEOD_ERR_ARG;
    const LinearProb p = linear_prob(LE_DGRAD_GELU16, M, N, K, N, K, 0, out_bf16, (kscale ? LF_KSCALE : 0) | LF_AUX, 0);
    LinearArgs a{}; a.a = dy; a.kscale = kscale; a.W = W; a.out = dx; a.ldo = K; a.aux = u16;
    return launch_linear<LE_DGRAD_GELU16>(linear_route(p), p, a, stream);
}
