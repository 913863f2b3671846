/* leod_hip.h -- C ABI of libleod_hip.so: the hand-written gfx950 (MI355X / CDNA4) kernels behind the
 * LEOD hot path (RVT recurrent backbone fwd/bwd, YOLOX head + SimOTA + losses, pseudo-label NMS).
 *
 * The reference (Wuziyi616/LEOD) is 100 % Python and has no FFI; each entry point below replaces the
 * ATen / torchvision call sequence of the cited reference lines (paths relative to the reference
 * root).  The reference-side binding is the ctypes stub in leod_amd/_lib.py.
 *
 * Conventions
 *   - plain C symbols, raw DEVICE pointers, explicit sizes; no torch types, no global state;
 *   - every call only enqueues work on `stream` (hipStream_t passed as void*): it never allocates,
 *     never synchronises and is re-entrant across streams; scratch is caller-provided;
 *   - return 0 on success, <0 on error: -1 bad argument, -2 launch failure, -3 unsupported shape;
 *   - activations are fp32 "rows": a row is one token/pixel of a channels-last (NHWC) map,
 *     M = B*H*W rows, contiguous channels.  "+=" outputs accumulate (parameter gradients).
 */
#ifndef LEOD_HIP_H
#define LEOD_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef void* leod_stream_t; /* hipStream_t */

const char* leod_version(void);

/* Precision of the contractions (process-wide; set before the first step).
 * 0: fp32 end to end -- v_mfma_f32_16x16x4_f32, bitwise an fp32 fmaf chain, the mode the parity tests pin against the fp32 oracle.
 * 2 ("16f"): the reference's mixed precision (Lightning precision=16 = fp16 autocast + GradScaler, train.py:236-243): the FORWARD
 *    contractions (GEMM, conv, attention, ConvLSTM, stem) take fp16 operands for v_mfma_f32_16x16x16_f16 / 16x16x32_f16 with fp32
 *    accumulation, and the 16-bit tensors the forward pass stores (qkv, attention output, MLP hidden, LSTM gates) are fp16; the GRADIENT
 *    contractions take bf16 operands (fp32's exponent range: no loss scaler) and gradient rows (dqkv, du, dO, gate gradients) are bf16.
 * 1 ("bf16", Lightning bf16-mixed): bf16 operands and bf16 rows in both directions.
 * In both 16-bit modes LayerNorm / BatchNorm statistics, softmax, the residual stream, LSTM state, SimOTA cost, losses and the optimiser
 * stay fp32.  Wherever a comment below says "precision mode bf16" it means "modes 1 and 2"; the parameters called *_bf16 that describe
 * FORWARD-stored activation rows (qkv, the attention output) carry fp16 rows in mode 2. */
int leod_set_precision(int mode);
int leod_get_precision(void);

/* ---- backbone: MaxViT block pieces (models/layers/maxvit/maxvit.py) ------------------------------ */

/* out[M,N] = LN(x)[M,K] W[N,K]^T + bias (LN skipped when ln_w == NULL); out_act (optional) = gelu_erf(out);
 * stats_out (optional) [M,2] = (mean, rstd).  Replaces norm1->qkv (maxvit.py:267,347) and norm2->fc1->GELU (:110-118,269). */
int leod_ln_linear_fwd(const float* x, long ldx, const float* ln_w, const float* ln_b, float eps, const float* W,
                       const float* bias, float* out, float* out_act, float* stats_out, int M, int N, int K,
                       leod_stream_t stream);

/* t = a[M,K] W[N,K]^T + bias ; tout (optional) = t ; out = res + gamma * t.
 * Replaces proj / fc2 followed by LayerScale and the residual add (maxvit.py:51-53,268-269,353). */
int leod_linear_lsres_fwd(const float* a, const float* W, const float* bias, const float* gamma, const float* res,
                          float* out, float* tout, int M, int N, int K, leod_stream_t stream);

/* Partition attention core on the interleaved qkv rows [M,3C] of an NHWC map (head h owns columns
 * [h*3d,(h+1)*3d) = q|k|v): out[M,C] = softmax(q k^T d^-1/2) v within each window (window=1) or grid
 * (window=0) partition of ph x pw tokens; lse (optional) [M,heads].  Replaces window/grid_partition + SelfAttentionCl
 * core + *_reverse (maxvit.py:252-265,273-304,347-352). */
int leod_partition_attn_fwd(const float* qkv, float* out, float* lse, int B, int H, int W, int C, int heads, int ph,
                            int pw, int window, int qkv_bf16, leod_stream_t stream);
/* dqkv[M,3C] from dout[M,C]; dsum [M,heads] scratch. */
int leod_partition_attn_bwd(const float* qkv, const float* dout, const float* lse, float* dsum, float* dqkv, int B,
                            int H, int W, int C, int heads, int ph, int pw, int window, int qkv_bf16, int dqkv_bf16,
                            leod_stream_t stream);
/* Precision mode bf16: q, k, v only ever enter bf16 MFMAs and dqkv's consumers feed bf16 MFMAs, so both tensors may live in HBM as
 * bf16 (qkv_bf16 / dqkv_bf16 above: the pointers then address bf16 elements) where the LDS attention kernels cover the geometry --
 * 1 from this query; leod_ln_linear_bf16_fwd produces the bf16 qkv rows. */
int leod_partition_attn_16bit_ok(int B, int H, int W, int C, int heads, int ph, int pw);
/* Bit 1 of qkv_bf16 in the two attention calls above: the attention output `out` (forward) is written / its gradient `dout` (backward)
 * is read as bf16 rows [M,C] -- valid where leod_partition_attn_o16_ok returns 1 (bf16-tile kernels).  leod_attn_block_o16_ok adds the
 * conditions of the block's other consumers (leod_linear_lsres_bf16_fwd, dx_fmt 1 of leod_linear_dgrad = dx written as bf16 rows,
 * x_fmt 3 of leod_linear_wgrad = x holds bf16 rows): the reference's autocast holds both tensors in 16 bits as well
 * (maxvit.py:185-270 under train.py:236-243). */
int leod_partition_attn_o16_ok(int B, int H, int W, int C, int heads, int ph, int pw);
int leod_attn_block_o16_ok(int B, int H, int W, int C, int heads, int ph, int pw);
/* Which kernels leod_partition_attn_fwd (entry 0) / leod_partition_attn_bwd (entry 1) run for this geometry in the current precision mode
 * -- a query: nothing is launched, no memory is read.  The calls themselves switch on the same value, so the two cannot differ.
 * flags, what the call is told about its tensors: 1 qkv rows are 16-bit (bit 0 of qkv_bf16), 2 O (forward) / dO (backward) rows are 16-bit
 * (bit 1 of qkv_bf16), 4 dqkv is written as bf16 (dqkv_bf16; backward only).  Code = 10000 F + 100 PT + D, PT = ceil(ph pw / 16):
 *   F = 1   register-direct fp32 kernels, one launch forward, q pass then kv pass backward; D = 16 ceil(d / 16)
 *   F = 2   LDS kernels on fp32 tiles; D = d (24 | 32)
 *   F = 3   LDS kernels on 16-bit tiles; D = d (24 | 32)
 *   0       no partitions: nothing to launch;    -1 / -3: what the call returns for these arguments (NULL pointers apart)
 * The bf16 / fp16 operand format inside a family follows from the precision mode and is not part of the code.
 * leod_partition_attn_16bit_ok / _o16_ok are derivations: forward and backward with the 16-bit flags both route to F = 3. */
int leod_partition_attn_route(int entry, int B, int H, int W, int C, int heads, int ph, int pw, int flags);
/* The attention half of a block in one launch (16-bit precision modes, RVT stages 1-2: 80-token partitions, (C, heads) = (48, 2) | (96, 4)):
 * y[M,C] = x + gamma * (attn(LN(x) W_qkv^T + b_qkv) W_proj^T + b_proj), i.e. leod_ln_linear_bf16_fwd -> leod_partition_attn_fwd ->
 * leod_linear_lsres_bf16_fwd with the same rounding points (maxvit.py:185-270,343-354).  qkv16 [M,3C] / o16 [M,C] (16-bit rows of the
 * precision mode), lse [M,heads] and stats [M,2] are each written when non-NULL -- what the three calls leave for the backward pass; all
 * NULL is the inference case (x in, y out); qkv16, o16 and lse come all or none.  ln_w = ln_b = NULL: norm1 is the identity (the first block
 * of a stage, maxvit_rnn.py:164-166), stats is then NULL as well.  b_qkv, b_proj and gamma may be NULL.  -3 where the kernel does not cover
 * the geometry or mode.
 * leod_attn_block_fwd_route: whether a BLOCK takes this call -- a query, nothing is launched, no memory is read.  flags: 1 = norm1 is a
 * LayerNorm with weight and bias, 2 = norm1 is the identity.  40000 + 100 PT + D (40524) where the kernel covers the geometry in the current
 * precision mode, one of the two flags is set and leod_attn_block_o16_ok holds (the block then saves the same 16-bit qkv / O as its
 * three-launch path); 0: no partitions; -1 / -3 otherwise (mode f32, padded partitions, other (C, heads), a norm1 without weight and bias,
 * O kept as fp32): the block runs the three calls. */
int leod_attn_block_fwd_route(int B, int H, int W, int C, int heads, int ph, int pw, int flags);
int leod_attn_block_fwd(const float* x, const float* ln_w, const float* ln_b, float eps, const float* Wqkv, const float* bqkv,
                        const float* Wproj, const float* bproj, const float* gamma, float* y, void* qkv16, void* o16, float* lse,
                        float* stats, int B, int H, int W, int C, int heads, int ph, int pw, int window, leod_stream_t stream);
int leod_linear_lsres_bf16_fwd(const void* a16, const float* W, const float* bias, const float* gamma, const float* res, float* out,
                               int M, int N, int K, leod_stream_t stream);
/* out16[M,N] = bf16(LN(x) W^T + bias), stats_out [M,2]; -3 unless the row-streaming kernel covers (M, N, K) in precision mode bf16. */
int leod_ln_linear_bf16_fwd(const float* x, const float* ln_w, const float* ln_b, float eps, const float* W, const float* bias,
                            void* out16, float* stats_out, int M, int N, int K, leod_stream_t stream);

/* Precision mode bf16, stages 1-2 of the MLP (maxvit.py:110-118): the hidden pre-activation u = LN(x) W1^T + b1 is stored ONCE,
 * as fp16 [M,N] (as the reference does under autocast, train.py:236-243; clamped to the fp16 range); the three consumers below
 * apply GELU / GELU' while loading it.  leod_ln_linear_gelu16_fwd returns -3 where the row-streaming kernel does not cover (M, N, K): callers then use
 * leod_ln_linear_fwd and its fp32 (u, gelu(u)) pair.  u16: device pointer to fp16 elements. */
int leod_ln_linear_gelu16_fwd(const float* x, const float* ln_w, const float* ln_b, float eps, const float* W, const float* bias,
                              void* u16, float* stats_out, int M, int N, int K, leod_stream_t stream);
int leod_linear_lsres_gelu16_fwd(const void* u16, const float* W, const float* bias, const float* gamma, const float* res, float* out,
                                 int M, int N, int K, leod_stream_t stream);
int leod_linear_dgrad_gelu16(const float* dy, const float* kscale, const float* W, const void* u16, void* dx, int M, int N, int K,
                             int out_bf16, leod_stream_t stream);
/* (the fc2 weight gradient on u16 is x_fmt 2 of leod_linear_wgrad / leod_linear_wgrad_group) */

/* n <= 4 Linear weight gradients of ONE row count M in one preparation, one contraction and one reduce launch (LDS-DMA kernel with a problem
 * table): dW_k [N_k, K_k] += dy_k^T X_k, dbias_k += colsum(dy_k).  The four weight gradients of an attention block, which its backward issues
 * together (maxvit.py:110-118,252-270).  Host arrays of length n.  dy_fmt: 0 fp32 rows, 1 bf16 rows; x_fmt: 0 fp32 rows, 1 fp32 rows through
 * LayerNorm (stats_k [M,2], ln_w_k, ln_b_k), 2 fp16 pre-activation through GELU, 3 bf16 rows, 4 fp16 rows; dense rows.
 * -3: not coverable (precision mode f32, M outside 8192 .. 60 000 / 400 000 or not a multiple of 64, widths of different tile classes):
 * nothing was launched, run the problems singly. */
int leod_linear_wgrad_group(int n, const void* const* dy, const int* dy_fmt, const void* const* x, const int* x_fmt,
                            const float* const* stats, const float* const* ln_w, const float* const* ln_b, float* const* dW,
                            float* const* dbias, int M, const int* N, const int* K, leod_stream_t stream);
/* Whether leod_linear_wgrad_group launches for these n problems of M rows in the current precision mode -- a query: nothing is launched, no
 * memory is read.  The call itself switches on the same value, so the two cannot differ.
 *   100 + T   the LDS-DMA kernel on T x T blocks of 16 columns (104 / 106 / 108: the codes of leod_linear_wgrad_route)
 *   -1 / -3   what the call returns for these arguments (NULL data pointers apart), its checks in their order: n outside 1 .. 4 or a NULL
 *             array -1; then per problem, in order, an x_fmt outside 0 .. 4 -1, then -3 for precision mode f32, widths of no tile class or of
 *             another class than the problems before, M < 8192, M not a multiple of 64, M above 60 000 (T = 6) / 400 000, a width that is
 *             no multiple of 8; last -3 where the 16-bit copies of the fp32 operands exceed the library's 600 MiB. */
int leod_linear_wgrad_group_route(int n, int M, const int* N, const int* K, const int* dy_fmt, const int* x_fmt);

/* The whole MLP of a MaxViT block in one row-streaming launch (maxvit.py:110-118, 268-269), precision mode bf16, K = 48 / H = 192 (stage 1
 * of RVT-S / -T), M >= 16384:  z[M,K] = y + g2 * (gelu(LN(y) W1^T + b1) W2^T + b2) with the hidden in registers (csrc/k_mlp.hip).
 * u16 [M,H] fp16 + stats [M,2] (both or neither): what the backward pass reads back (training).  -3: not covered -- the caller runs
 * leod_ln_linear_gelu16_fwd + leod_linear_lsres_gelu16_fwd. */
int leod_mlp_fwd_fused(const float* y, const float* ln_w, const float* ln_b, float eps, const float* W1, const float* b1, const float* W2,
                       const float* b2, const float* g2, float* out, void* u16, float* stats, int M, int H, int K, leod_stream_t stream);

/* Backward of that MLP along the activation path, one launch: u is recomputed from y, du = ((dz g2) W2) gelu'(u) is written as bf16 rows
 * (du16 [M,H], optional: the fc1 weight gradient reads it), dy = dz + LayerNorm-backward(du W1), dgamma / dbeta [K] += (norm2).
 * stats [M,2] = the (mean, rstd) of the forward pass.  Replaces leod_linear_dgrad_gelu16 + leod_linear_dgrad_lnbwd where it applies
 * (same coverage as leod_mlp_fwd_fused; -3 otherwise). */
int leod_mlp_bwd_dgrad_fused(const float* dz, const float* y, const float* stats, const float* ln_w, const float* ln_b, const float* W1,
                             const float* b1, const float* W2, const float* g2, float* dy, void* du16, float* dgamma, float* dbeta, int M,
                             int H, int K, leod_stream_t stream);
/* Whether leod_mlp_fwd_fused (entry 0) / leod_mlp_bwd_dgrad_fused (entry 1) run for this problem in the current precision mode -- a query:
 * nothing is launched, no memory is read.  The calls themselves switch on the same value, so the two cannot differ.
 *   7000 + 100 (K / 16) + H / 16   the one-launch kernel: 7312 for (K, H) = (48, 192), 7416 for (64, 256), in the 16-bit precision modes
 *                                  with M >= 16384
 *   -3                             everything else: what the call returns (NULL pointers apart);    -1: an entry other than 0 / 1 */
int leod_mlp_fused_route(int entry, int M, int H, int K);

/* Fused ConvLSTM cell, DWSConvLSTM2d.forward with dws_conv=False (models/layers/rnn.py:37-70):
 * gates = [x|h_prev] W[4C,2C]^T + b, (f,i,o)=sigmoid, g=tanh, c=f*c_prev+i*g, h=o*tanh(c).
 * h_prev/c_prev NULL = zero state; gates_out (optional) [M,4,C] post-activation gates. */
int leod_convlstm_fwd(const float* x, const float* h_prev, const float* c_prev, const float* W, const float* bias,
                      float* h_out, float* c_out, float* gates_out, int M, int C, leod_stream_t stream);
/* dgates[M,4,C] (pre-activation), dc_prev (optional) from dh + dh2 (both optional: gradient of h_t from the layers
 * above and from timestep t+1) and dc_next (optional). */
int leod_convlstm_gates_bwd(const float* dh, const float* dh2, const float* dc_next, const float* gates, const float* c_prev,
                            const float* c_t, float* dgates, float* dc_prev, int M, int C, leod_stream_t stream);

/* The ConvLSTM recurrence of a whole sequence in ONE launch per direction (same cell as leod_convlstm_fwd, unrolled over the L
 * timesteps of modules/detection.py:188-226): one workgroup carries 16 rows through all T timesteps with its slice of the weights
 * resident in registers.  leod_convlstm_seq_mode(C): 1 = xin is x_seq [T,M,C] (fused [x|h] contraction), 2 / 3 = xin is the
 * time-batched projection gx [T,M,4C] = x W_x^T + b computed by the caller, 0 = not available for this C / precision mode
 * (callers then loop leod_convlstm_fwd).  hbuf, cbuf [T+1,M,C]: slot 0 = incoming state (zero_state: taken as zeros, not read),
 * slots 1..T are written; gates_out [T,M,4,C] optional -- without it (inference: no backward pass will read the history) only slot T of cbuf
 * is written. */
int leod_convlstm_seq_mode(int C);
/* mode 3 (C = 192 / 256 / 384 / 512 in the 16-bit precision modes: the weight slice of a wave does not fit its registers): like mode 2, and the waves
 * stream their MFMA B fragments from a fragment-ordered bf16 copy of W_h -- leod_convlstm_seq_pack writes it (once per step, shared by
 * forward and backward) into a buffer of leod_convlstm_seq_pack_bytes(C) bytes, passed as wpack (NULL in modes 1 / 2). */
long leod_convlstm_seq_pack_bytes(int C);
int leod_convlstm_seq_pack(const float* W, void* wpack, int C, leod_stream_t stream);
int leod_convlstm_seq_fwd(const float* xin, int x_is_projection, float* hbuf, float* cbuf, const float* W, const float* bias,
                          float* gates_out, const void* wpack, int M, int C, int T, int zero_state, int gates16, leod_stream_t stream);
/* Backward through time of the same: dh_seq [T,M,C] (optional) gradients of every h_t from above, dc_last [M,C] (optional);
 * writes dgates_out [T,M,4C] (pre-activation; dx = dgates W_x and the weight gradient are one GEMM each over all T*M rows)
 * and optionally dh0 / dc0 [M,C].  gates [T,M,4,C] and cbuf [T+1,M,C] as the forward call wrote them; zero_state: c_0 is taken as zeros
 * and slot 0 of cbuf is not read, on every route (slots 1..T are read; hbuf is not needed).  LEOD_ERR_UNSUPPORTED (-3) when the weight
 * slice does not fit the registers. */
int leod_convlstm_seq_bwd(const float* dh_seq, const float* dc_last, const float* gates, const float* cbuf, const float* W,
                          float* dgates_out, float* dh0, float* dc0, const void* wpack, int M, int C, int T, int zero_state,
                          int gates16, leod_stream_t stream);
/* gates16 (both calls above; precision mode bf16 only, leod_convlstm_seq_gates16_ok(C) != 0): gates_out / gates point to fp16 storage in
 * the sequence kernels' own lane-linear layout (T x ceil(M / 16) * 16 x 4C halfs, written and read by these two calls only), dgates_out to
 * bf16 rows [T][M][4C] -- the reference's autocast holds the gates in 16 bits as well (rnn.py:58-62 under train.py:236-243). */
int leod_convlstm_seq_gates16_ok(int C);
/* Which kernel leod_convlstm_seq_fwd (entry 0) / leod_convlstm_seq_bwd (entry 1) run for this channel count in the current precision
 * mode -- a query: nothing is launched, no memory is read.  The calls themselves switch on the same value.
 * flags, what the call is given: 1 xin is the hoisted projection (x_is_projection), 2 gates16, 4 a wpack.
 *   forward    1000 + C   fused [x | h] contraction, weights resident in registers
 *              2000 + C   hoisted projection, weights resident in registers
 *              3000 + C   hoisted projection, weights streamed from the pack
 *   backward   3000 + C   streamed from the pack
 *              4000 + C   weights resident in registers
 *   -1 / -3: what the call returns for these arguments (NULL pointers and M, T <= 0 apart); -3 from the backward (precision mode f32 at
 *   C = 192 among others) tells the caller to run the per-timestep kernels.
 * leod_convlstm_seq_mode, leod_convlstm_seq_gates16_ok, leod_convlstm_seq_pack_bytes and the check of leod_convlstm_seq_pack are derivations. */
int leod_convlstm_seq_route(int entry, int C, int flags);

/* dy_fmt 1 (here and in leod_linear_wgrad; dy_bf16 of leod_linear_dgrad_lnbwd): dy points to bf16 elements -- in precision mode bf16 the
 * wide gradients du (out_bf16 of leod_linear_dgrad_gelu16) and dqkv are stored as the bf16 their consumers feed to the MFMAs anyway.
 * dy_fmt 0: fp32 rows.  dx_fmt: 0 fp32, 1 dx is written as bf16 rows (precision mode bf16, plain dgrad without dx2 / colsum / accumulate /
 * dres / aux_u / nsplit on the LDS-staged kernels; -3 otherwise).
 * dx (=|+=) (dy[M,N]*kscale[N]) W[N,K] ; optional: multiply by gelu'(aux_u[M,K]); route columns >= nsplit to dx2;
 * colsum[K] += column sums of the result; dres [M,K] (optional, leading dimension lddx): dx = dres + result (the second gradient source of a
 * residual branch, so that no separate add kernel runs).  Autograd of the Linear layers above. */
int leod_linear_dgrad(const float* dy, long lddy, const float* kscale, const float* W, float* dx, long lddx, float* dx2,
                      long lddx2, int nsplit, const float* aux_u, float* colsum, int accumulate, const float* dres, int M, int N,
                      int K, int dy_fmt, int dx_fmt, leod_stream_t stream);
/* Workspace of the weight-gradient calls below for launches on `stream` (precision mode bf16: the per-workgroup partial tiles that a second
 * kernel adds up -- 1024 workgroups adding to the same dW addresses with atomics were 130 us of a 200 us launch): leod_workspace_bytes()
 * bytes, 16-byte aligned, owned by the caller and kept alive until replaced (ws == NULL withdraws it).  Without a registered workspace
 * the library allocates one per stream on first use, or falls back to the atomic epilogue while the stream is being captured.
 * (No counterpart in the reference: torch's autograd owns the cuBLAS workspaces there.) */
long leod_workspace_bytes(void);
int leod_set_workspace(void* ws, long bytes, leod_stream_t stream);
/* dW[N,K] += dy^T X ; dbias[N] += colsum(dy).  dy_fmt: 0 fp32 rows, 1 bf16 rows.  x_fmt, as in leod_linear_wgrad_group: what x points to
 * and how X comes from it -- 0 fp32 rows, 1 fp32 rows through LayerNorm (stats [M,2], ln_w, ln_b: all three, and stats only here),
 * 2 fp16 pre-activation through GELU (fp32 dy, no x2), 3 bf16 rows, 4 fp16 rows (3 / 4: no x2; -3 where no bf16-MFMA kernel covers the
 * shape).  x2 != NULL: X = [x | x2] with K1 columns from x and fp32 x2.  -1 for any other combination. */
int leod_linear_wgrad(const float* dy, long lddy, const float* x, long ldx, const float* stats, const float* ln_w,
                      const float* ln_b, const float* x2, long ldx2, int K1, float* dW, float* dbias, int M, int N,
                      int K, int dy_fmt, int x_fmt, leod_stream_t stream);
/* Which kernel leod_linear_wgrad runs for this problem in the current precision mode -- a query: nothing is launched, no memory is read.
 * has_stats: stats, ln_w and ln_b are given; has_x2: x2 is given.  The call itself switches on the same value, so the two cannot differ.
 *   100 + T            LDS-DMA kernel, T x T blocks of 16 columns per workgroup (T = 4, 6, 8)
 *   200 + c            register-staged wide kernel, instantiation c = 1 .. 16
 *   300 + c            wgradw kernel, configuration c = 1 .. 5 (48 x 48, 192 x 48, 48 x 192, 96 x 96 with 32-row chunks, 96 x 96 with 16-row chunks)
 *   400 + 10 TN + TK   wgrad16 kernel on TN x TK blocks of 16 columns (33, 22, 44, 14, 41, 11)
 *   0                  M <= 0: nothing to do;    -1 / -3: what leod_linear_wgrad returns for these arguments (NULL pointers apart)
 * One thing is not known before the launch: a 100 + T problem on a stream that has no registered workspace while none can be allocated
 * (the stream is being captured) runs on the route it would have without the LDS-DMA kernel.  Register a workspace first
 * (leod_set_workspace) and the answer is what runs. */
int leod_linear_wgrad_route(int M, int N, int K, long lddy, long ldx, long ldx2, int K1, int dy_fmt, int x_fmt, int has_stats,
                            int has_x2);
/* The same query for the nine Linear forward / input-gradient calls: which kernel the call runs in the current precision mode, or the
 * negative error it returns (NULL pointers apart).  entry: 0 leod_ln_linear_fwd, 1 leod_linear_lsres_fwd, 2 leod_ln_linear_gelu16_fwd,
 * 3 leod_ln_linear_bf16_fwd, 4 leod_linear_lsres_bf16_fwd, 5 leod_linear_lsres_gelu16_fwd, 6 leod_linear_dgrad, 7 leod_linear_dgrad_lnbwd,
 * 8 leod_linear_dgrad_gelu16.  M, N, K as that call takes them; lda / ldo: row strides of its input rows (x, a, dy) and of the rows it
 * stores; a16 / out16: its dy_fmt or dy_bf16 / dx_fmt or out_bf16 (0 where it has none); nsplit as leod_linear_dgrad; flags, the optional
 * pointers that are given: 1 ln_w, 2 stats_out or stats, 4 kscale, 8 out_act or aux_u, 16 tout, 32 dx2, 64 colsum, 128 accumulate, 256 dres.
 *   1000 + 100 KC + NTT   row-streaming kernel, contraction of 16 KC, slabs of NTT blocks of 16 columns
 *   2000 + KC             narrow row-streaming kernel, contraction of 16 KC into 48 (KC 9, 12) or 96 (KC 18, 24) columns
 *   3000 + NTW            persistent wide-tile kernel, workgroups of 64 NTW columns (NTW 3, 4)
 *   4000 + 100 NT + KCH   LDS-staged kernel, NT blocks of 16 columns, K chunks of KCH (48, 64), two-phase row loader
 *   5000 + 100 NT + KCH   the same with the plain row loader
 *   6000 + 10 NT + KS     register-direct kernel, K split over KS waves (1, 4)
 *   0                     M <= 0 with valid arguments: nothing to do, the call returns 0 */
int leod_linear_route(int entry, int M, int N, int K, long lda, long ldo, int a16, int out16, int flags, int nsplit);

/* LayerNorm over channels (eps 1e-5), maxvit.py:172-178 and its autograd. */
int leod_layernorm_fwd(const float* x, const float* w, const float* b, float* y, float* stats, int M, int C, float eps,
                       leod_stream_t stream);
int leod_layernorm_bwd(const float* dn, const float* x, const float* stats, const float* w, const float* dres, float* dx,
                       float* dw, float* db, int M, int C, float eps, leod_stream_t stream);
/* LayerScale autograd: dt = gamma*dz ; dgamma += sum_m dz*t (maxvit.py:45-53). */
int leod_layerscale_bwd(const float* dz, const float* t, const float* gamma, float* dt, float* dgamma, int M, int C,
                        leod_stream_t stream);
/* LayerScale autograd without the stored pre-scale tensor t = h W^T + b (maxvit.py:45-53, :268-269): from the UN-scaled
 * weight gradient G[N,K] = dz^T h and s[N] = colsum(dz) of the Linear in front of the LayerScale:
 * dW += diag(gamma) G ; db += gamma*s ; dgamma[n] += sum_k W[n,k] G[n,k] + b[n] s[n]. */
int leod_layerscale_finalize(const float* W, const float* b, const float* gamma, const float* G, const float* s, float* dW,
                             float* db, float* dgamma, int N, int K, leod_stream_t stream);

/* ---- convolutions (implicit GEMM, NHWC) --------------------------------------------------------- */

/* Stem conv of stage 1 straight from the raw NCHW event tensor (uint8 or fp32, H x W unpadded; reads outside are
 * the zero padding of utils/padding.py:32-58 up to Hp x Wp): ConvDownsampling_Cf2Cl.conv, maxvit.py:160-176. */
int leod_stem_conv_fwd(const void* x, int x_is_u8, const float* w, float* y, int B, int Cin, int H, int W, int Hp, int Wp,
                       int N, int ks, int stride, int pad, leod_stream_t stream);
int leod_stem_conv_wgrad(const float* dy, const void* x, int x_is_u8, float* dw, int B, int Cin, int H, int W, int Hp,
                         int Wp, int N, int ks, int stride, int pad, leod_stream_t stream);
/* y = conv(x NHWC, w[N,Cin,ks,ks]) (+bias); colstats (optional) [stat_rep,2,N] double += (sum, sumsq) for training BatchNorm,
 * spread over stat_rep replicas (power of two, 0/1 = one copy; the caller zero-fills, leod_bn_silu_fwd folds them);
 * bn_w != NULL: eval BatchNorm folded + SiLU (network_blocks.py:29-54; yolo_pafpn.py:109-140; yolo_head.py:208-222).
 * wpack (optional scratch, N*Cin*ks*ks floats): the call first writes a K-contiguous copy of w there and contracts
 * against that (the native [N][Cin][ks][ks] layout strides every weight float4 over 36 bytes).  wpack_valid != 0: wpack already
 * holds the packed copy this very call (same weights, geometry, direction, precision mode) wrote earlier and w has not changed since --
 * the pack launch is skipped (the weights change once per optimiser step, the PAFPN / head convs run 40 packs per step otherwise). */
int leod_conv_nhwc_fwd(const float* x, const float* w, const float* bias, float* y, double* colstats, int stat_rep, const float* bn_w,
                       const float* bn_b, const float* bn_rm, const float* bn_rv, float bn_eps, int B, int H, int W,
                       int Cin, int N, int ks, int stride, int pad, float* wpack, int wpack_valid, leod_stream_t stream);
int leod_conv_nhwc_dgrad(const float* dy, const float* w, float* dx, int accumulate, int B, int H, int W, int Cin, int N,
                         int ks, int stride, int pad, float* wpack, int wpack_valid, leod_stream_t stream);
/* dw[N,Cin,ks,ks] += weight gradient (dbias optional).  ws: scratch of leod_conv_nhwc_wgrad_workspace_floats(...) floats (may be
 * NULL when that is 0; with a workspace the 3x3 / stride-1 gradients of the bf16 mode are reduced without atomics). */
long leod_conv_nhwc_wgrad_workspace_floats(int B, int H, int W, int Cin, int N, int ks, int stride, int pad, int has_bias);
int leod_conv_nhwc_wgrad(const float* dy, const float* x, float* dw, float* dbias, float* ws, int B, int H, int W, int Cin, int N,
                         int ks, int stride, int pad, leod_stream_t stream);

/* Grouped 3x3 / stride-1 / pad-1 convolutions: n <= 8 independent problems of ONE (Cin, Cout) geometry in one launch -- the convs of equal
 * depth in the cls / reg towers of the three head levels (yolo_head.py:61-145,208-222).  All array arguments are HOST arrays of length n
 * (device pointers / sizes per problem); wpack[k] / wpack_valid[k] as in leod_conv_nhwc_fwd.  forward: y_k = conv(x_k, w_k) with the
 * BatchNorm (sum, sumsq) of y_k into colstats[k] ([stat_rep[k]][2][Cout] doubles, zeroed; NULL: none).  dgrad: dx_k (+)= the input
 * gradient from dy_k [B,H,W,N]; problems of one call must write different dx buffers.  -3: not coverable, run the problems singly. */
int leod_conv3x3_group_supported(int n, const int* H, const int* W, int Cin, int Cout);   /* 1: n in 1..8 and every map routes to 110 (leod_conv_route): the forward call covers them (dgrad: ask with (Cout, Cin)) */
int leod_conv3x3_group_fwd(int n, const float* const* x, const float* const* w, float* const* y, double* const* colstats,
                           const int* stat_rep, void* const* wpack, const int* wpack_valid, const int* B, const int* H, const int* W,
                           int Cin, int Cout, leod_stream_t stream);
int leod_conv3x3_group_dgrad(int n, const float* const* dy, const float* const* w, float* const* dx, const int* accumulate,
                             void* const* wpack, const int* wpack_valid, const int* B, const int* H, const int* W, int Cin, int N,
                             leod_stream_t stream);
/* weight gradients of the same problems: dw_k [N,Cin,3,3] += ... in one launch + one reduce launch; ws[k]: scratch of
 * leod_conv3x3_group_wgrad_workspace_floats(B[k], H[k], W[k], Cin, N) floats (0: not coverable -> -3 from the call) */
long leod_conv3x3_group_wgrad_workspace_floats(int B, int H, int W, int Cin, int N);
int leod_conv3x3_group_wgrad(int n, const float* const* dy, const float* const* x, float* const* dw, float* const* ws, const int* B,
                             const int* H, const int* W, int Cin, int N, leod_stream_t stream);

/* Grouped 1x1 / stride-1 convolutions over pixel rows: n <= 4 independent problems in ONE launch of the short-problem kernel, which has a
 * workgroup's operands for the whole contraction in flight at once -- the single layers of the PAFPN, conv1 | conv2 of a CSP layer on one
 * map, the three head stems.  All array arguments are HOST arrays of length n.  16-bit precision modes only.
 * leod_conv1x1_group_route: the kernel the call `entry` (0 leod_conv1x1_group_fwd, 1 leod_conv1x1_group_dgrad) runs for members of M[k] rows,
 * contraction length K[k] and N[k] output columns (dgrad: K = the conv's output channels, N = its input channels); flags: 2 colstats,
 * 64 accumulate.  A query: nothing is launched.  Covered: 1 <= M <= 65536, 16 <= K <= 384, 16 <= N <= 384, K and N multiples of 16.
 *   1 d_0 .. d_{n-1}       one launch; decimal digit d_k = row fragments per workgroup of member k (2: 32-row tiles, 4: 64-row tiles)
 *   -1                     bad arguments (n outside 1..4, NULL, unknown entry or flag);    -3    not covered: run the members singly
 * A group computes bit for bit what its members compute through leod_conv_nhwc_fwd / _dgrad.  Refused (-3) besides the coverage: a member
 * whose single call is the wide-tile kernel (leod_conv_route 3000 + ..); a group whose members all have 8192 rows or more, unless it is a
 * forward group of two or more -- such members are no faster here than alone (measured) and gain only by the launch they share.
 * The calls switch on the same value; < 0: nothing was launched and no output was touched.
 * forward: y_k [M][N] = x_k [M][Cin] w_k [N][Cin]^T with the BatchNorm (sum, sumsq) of y_k into colstats[k] ([stat_rep[k]][2][N] doubles,
 * zeroed; NULL: none), as leod_conv_nhwc_fwd leaves them.  dgrad: dx_k [M][Cin] (+)= dy_k [M][N] w_k; members of one call must write
 * different dx buffers. */
int leod_conv1x1_group_route(int entry, int n, const int* M, const int* K, const int* N, int flags);
int leod_conv1x1_group_fwd(int n, const float* const* x, const float* const* w, float* const* y, double* const* colstats,
                           const int* stat_rep, const int* M, const int* Cin, const int* N, leod_stream_t stream);
int leod_conv1x1_group_dgrad(int n, const float* const* dy, const float* const* w, float* const* dx, const int* accumulate,
                             const int* M, const int* Cin, const int* N, leod_stream_t stream);

/* Which kernel a dense-convolution call runs for this problem in the current precision mode, or the negative error it returns (NULL pointers
 * apart) -- a query: nothing is launched, no memory is read.  The calls themselves switch on the same value, so the two cannot differ.
 * entry: 0 leod_conv_nhwc_fwd, 1 leod_conv_nhwc_dgrad, 2 leod_conv_nhwc_wgrad, 3 leod_stem_conv_fwd, 4 leod_stem_conv_wgrad.  B, H, W, Cin,
 * N, ks, stride, pad as that call takes them (H, W: the conv's input map; the stem's stored frame).  Hp, Wp: the padded frame of the stem
 * entries (0: H, W); ignored by the others.  flags, what the call is given: 1 bias, 2 colstats, 4 bn_w (eval BatchNorm), 8 wpack, 16 ws,
 * 32 dbias, 64 accumulate, 128 x_is_u8, 256 the address of x is a multiple of 4 (stem).  A code is read together with the entry:
 *   110 / 120              direct 3x3 from the LDS halo, stride 1 / 2 (forward; 110 also the stride-1 dgrad); reads the 16-bit per-tap pack in wpack
 *   220                    direct stride-2 3x3 dgrad; reads the bf16 per-tap pack in wpack
 *   300 + c                1x1 weight gradient on the wgradw kernel, configuration c   (the codes of leod_linear_wgrad_route)
 *   400 + 10 TN + 4        1x1 weight gradient on the wgrad16 kernel, TN x 4 blocks of 16 columns
 *   500                    direct 3x3 weight gradient into the workspace ws + reduce
 *   600 + NT / 610 + NT    stem forward on the bf16 patch (NT = N / 16: 2, 3) / on the uint8 patch (NT 1..4)
 *   620 + NT / 630 + NT    stem weight gradient on the bf16 patch (NT 1..4; 4 runs as two slices of 32 channels) / on the uint8 patch
 *   700 / 800 / 900 + 10 TN + 4   wgrad16 kernel on the im2col loader of an NHWC map / the stem's uint8 frame / the stem's fp32 frame
 *   1x1 forward and dgrad run as Linear layers over the pixel rows, with the codes of leod_linear_route, except that the wide-tile code
 *   carries one more digit (3043 here is 3003 there):
 *   3000 + 10 NT + NTW     persistent wide-tile kernel, workgroups of 64 NTW columns (NT: column tiling of its weight loader)
 *   4000 / 5000 + 100 NT + KCH    LDS-staged kernel, NT blocks of 16 columns, K chunks of KCH, two-phase / plain row loader
 *   6000 + 10 NT + KS      register-direct kernel, K split over KS waves (1, 4)
 *   implicit GEMMs of ks > 1 and of the stem's generic path, 10000 L + form: L = 1 im2col of an NHWC map, 2 parity classes of a stride-2
 *   3x3 dgrad ("live taps"), 3 / 4 im2col of the stem's uint8 / fp32 frame;
 *   L7000 + 100 NT + KCH   LDS-staged kernel on the K-contiguous fp32 copy of the weights in wpack (the only GEMM form that reads wpack)
 *   L8000 + 100 NT + KCH   LDS-staged kernel on the weights in their native layout
 *   L9000 + 10 NT + KS     register-direct kernel on the weights in their native layout
 *   0                      no output rows: nothing to do;    -1 / -3: what the call returns for these arguments */
int leod_conv_route(int entry, int B, int H, int W, int Cin, int N, int ks, int stride, int pad, int flags, int Hp, int Wp);

/* Depthwise convolution (groups == channels) on NHWC maps, w[C,1,ks,ks]: the depthwise half of DWConv (network_blocks.py:57-76, selected
 * by `depthwise` at yolo_pafpn.py:37 / yolo_head.py:52) and conv3x3_dws of the ConvLSTM (models/layers/rnn.py:20-30,50-55).  Same epilogue
 * options as leod_conv_nhwc_fwd: +bias, colstats [stat_rep,2,C] double += (sum, sumsq), or eval BatchNorm folded + SiLU.  C % 4 == 0.
 * dgrad: dx[B,H,W,C] (+= when accumulate) from dy[B,Ho,Wo,C]; wgrad: dw[C,1,ks,ks] += , dbias[C] += (optional).  fp32 in every mode. */
int leod_dwconv_nhwc_fwd(const float* x, const float* w, const float* bias, float* y, double* colstats, int stat_rep, const float* bn_w,
                         const float* bn_b, const float* bn_rm, const float* bn_rv, float bn_eps, int B, int H, int W, int C,
                         int ks, int stride, int pad, leod_stream_t stream);
int leod_dwconv_nhwc_dgrad(const float* dy, const float* w, float* dx, int accumulate, int B, int H, int W, int C, int ks,
                           int stride, int pad, leod_stream_t stream);
int leod_dwconv_nhwc_wgrad(const float* dy, const float* x, float* dw, float* dbias, int B, int H, int W, int C, int ks,
                           int stride, int pad, leod_stream_t stream);

/* BatchNorm2d (batch statistics) + SiLU on rows and its autograd (network_blocks.py:47-51).  `count` = rows that
 * entered colstats/sums.  SyncBatchNorm: with count_dev (device scalar) the row count is count * count_dev[0] -- pass count =
 * rows per image and count_dev = images over all ranks (one all-reduced scalar per step), colstats/sums all-reduced.
 * sums of the backward pair: zero-filled double [rep][2][N]; the reduce kernel's workgroups spread their closing atomics over the rep
 * copies (rep >= 1, chosen by the caller from the row count), the apply kernel folds them. */
int leod_bn_silu_fwd(const float* z, const double* colstats, int stat_rep, const float* w, const float* b, float* y, float* save_mean,
                     float* save_rstd, float* run_mean, float* run_var, int M, int N, double count,
                     const double* count_dev, float eps, float momentum, leod_stream_t stream);
int leod_bn_silu_bwd_reduce(const float* dy, const float* z, const float* mean, const float* rstd, const float* w,
                            const float* b, double* sums, int rep, int M, int N, int lddy, leod_stream_t stream);
int leod_bn_silu_bwd_apply(const float* dy, const float* z, const float* mean, const float* rstd, const float* w,
                           const float* b, const double* sums, int rep, float* dz, float* dw, float* db, int M, int N, double count,
                           const double* count_dev, int lddy, leod_stream_t stream);

/* The three BatchNorm + SiLU launches above for n <= 8 layers of ONE channel count at once (the layers of equal depth over the head levels and
 * branches): every array argument is a HOST array of length n holding what the single call takes for layer k.  run_mean / run_var /
 * count_dev / lddy / dw / db may be NULL as arrays (none for any layer) or hold NULL / 0 entries. */
int leod_bn_silu_fwd_group(int n, const float* const* z, const double* const* colstats, const int* stat_rep, const float* const* w,
                           const float* const* b, float* const* y, float* const* save_mean, float* const* save_rstd, float* const* run_mean,
                           float* const* run_var, const int* M, int N, const double* count, const double* const* count_dev, float eps,
                           const float* momentum, leod_stream_t stream);
int leod_bn_silu_bwd_reduce_group(int n, const float* const* dy, const float* const* z, const float* const* mean, const float* const* rstd,
                                  const float* const* w, const float* const* b, double* const* sums, const int* rep, const int* M, int N,
                                  const int* lddy, leod_stream_t stream);
int leod_bn_silu_bwd_apply_group(int n, const float* const* dy, const float* const* z, const float* const* mean, const float* const* rstd,
                                 const float* const* w, const float* const* b, double* const* sums, const int* rep, float* const* dz,
                                 float* const* dw, float* const* db, const int* M, int N, const double* count,
                                 const double* const* count_dev, const int* lddy, leod_stream_t stream);

/* ---- YOLOX head tail (models/detection/yolox/models/yolo_head.py) --------------------------------- */

/* cls/reg/obj 1x1 prediction convs of one level + grid decode (:216-222,289-332): out_train = decoded boxes + logits,
 * out_infer = decoded boxes + sigmoid, both [B, A, 5+nc] written at anchor offset a0. */
int leod_head_pred_fwd(const float* cls_feat, const float* reg_feat, const float* cls_w, const float* cls_b,
                       const float* reg_w, const float* reg_b, const float* obj_w, const float* obj_b, float* out_train,
                       float* out_infer, int B, int h, int w, int Hd, int nc, int stride, int a0, int A, leod_stream_t stream);
/* gscale (optional): device scalar multiplied into d_raw (the seed gradient of the loss). */
int leod_head_pred_bwd(const float* d_raw, const float* cls_feat, const float* reg_feat, const float* cls_w,
                       const float* reg_w, const float* obj_w, float* d_cls_feat, float* d_reg_feat, float* d_cls_w,
                       float* d_cls_b, float* d_reg_w, float* d_reg_b, float* d_obj_w, float* d_obj_b, const float* gscale,
                       int B, int h, int w, int Hd, int nc, int a0, int A, leod_stream_t stream);

/* SimOTA (get_assignments / get_assignments_w_ignore / simota_matching, :606-774, :974-1148) for a whole batch:
 * outputs [B,A,5+nc] decoded boxes + logits, labels [B,Nmax,7] = (cls,cx,cy,w,h,obj,cls_conf) zero padded.
 * totals[3] int (caller-zeroed): sum num_fg, sum num_gt, status bit0 = some gt had no candidate anchor.
 * No limit on Nmax (boxes per frame) or A: the per-gt and per-candidate arrays live in LDS when they fit (Nmax <= 128,
 * candidates <= 10240) and in the workspace otherwise.  workspace = leod_simota_workspace_floats(B, Nmax, A) floats. */
long leod_simota_workspace_floats(int B, int Nmax, int A);
int leod_simota_assign(const float* outputs, const float* labels, float* workspace, unsigned char* fg_mask,
                       unsigned char* ignore_mask, int* matched_row, int* matched_valid_idx, float* pred_iou,
                       int* num_fg_img, int* totals, int B, int Nmax, int nc, int nlv, const int* hs, const int* ws,
                       const int* strides, float ignore_label, leod_stream_t stream);
/* Loss assembly (:547-597, losses.py:18-85) + gradient wrt the raw prediction-conv outputs (d_raw, optional).
 * sums[3] double caller-zeroed; losses[6] = loss, iou_loss, conf_loss, cls_loss, l1_loss(0), num_fg/num_gt. */
int leod_yolox_loss(const float* outputs, const float* labels, const unsigned char* fg_mask,
                    const unsigned char* ignore_mask, const int* matched_row, const float* pred_iou, const int* totals,
                    double* sums, float* losses, float* d_raw, int B, int Nmax, int nc, int nlv, const int* hs,
                    const int* ws, const int* strides, int focal, float reg_weight, float obj_weight, float cls_weight,
                    float grad_scale, leod_stream_t stream);
/* leod_yolox_loss under ``bbox_loss_weighting`` (_get_bbox_loss_weight, yolo_head.py:358-381; normalisation :550-553 / :928-931):
 * label_w [B,Nmax] = the configured expression of each label row's obj / cls / obj*cls confidence; the IoU and class terms of a
 * foreground anchor and their gradients are scaled by label_w[its box] / (mean of that over the batch's foreground anchors).
 * wsum[1] double caller-zeroed (the sum behind the mean). */
int leod_yolox_loss_weighted(const float* outputs, const float* labels, const unsigned char* fg_mask,
                             const unsigned char* ignore_mask, const int* matched_row, const float* pred_iou, const int* totals,
                             const float* label_w, double* wsum, double* sums, float* losses, float* d_raw, int B, int Nmax, int nc,
                             int nlv, const int* hs, const int* ws, const int* strides, int focal, float reg_weight,
                             float obj_weight, float cls_weight, float grad_scale, leod_stream_t stream);
/* ``ignore_bg_k`` (_get_highest_score_mask, yolo_head.py:335-356, applied at :541-542): marks in ignore_mask [B,A] the
 * int(#background anchors * k) highest objectness logits (outputs[...,4]) among each image's background anchors (fg_mask == 0), so
 * that leod_yolox_loss leaves them out of the objectness term.  Does nothing when any label row carries ignore_label: such a
 * batch takes the reference's get_losses_w_ignore, which has no such step.  0 < k <= 1; ties at the threshold go to the lowest
 * anchor indices (torch.topk leaves that order unspecified). */
int leod_bg_topk_ignore(const float* outputs, const float* labels, const unsigned char* fg_mask, unsigned char* ignore_mask,
                        int B, int Nmax, int A, int nc, double k, float ignore_label, leod_stream_t stream);

/* ---- post-processing (models/detection/yolox/utils/boxes.py:32-86; modules/utils/ssod.py:40-188) -- */

/* postprocess + torchvision-semantics batched NMS for B images at once.  nc>0: pred [B,A,5+nc] (cx,cy,w,h,obj,cls..),
 * boxes rewritten IN PLACE to xyxy; nc==0: pred [B,A,7] already (xyxy,obj,cls_conf,cls_id) (TTA merge).
 * det_out [B,max_det,7] in NMS order, det_cnt[B].  One workgroup per image keeps the candidates in LDS: all A anchors when
 * they fit (A <= 5040: Gen1, Gen4), else 4096 candidates; an image with more boxes above conf_thre than that is sorted and
 * suppressed in its slice of ``workspace`` (leod_postprocess_nms_workspace_bytes(B, A) bytes, 0 when never needed) -- the
 * reference has no candidate limit (boxes.py:53-80).  workspace == NULL: such an image reports det_cnt = -1. */
long leod_postprocess_nms_workspace_bytes(int B, int A);
int leod_postprocess_nms(float* pred, float* det_out, int* det_cnt, void* workspace, int B, int A, int nc, float conf_thre,
                         float nms_thre, int class_agnostic, int max_det, int vanilla_limit, leod_stream_t stream);
/* pred2label + filter_pred_boxes: det -> labels [B,max_det,8] = (0,x,y,w,h,cls,cls_conf,obj), lab_cnt[B]. */
int leod_pseudo_filter(const float* det, const int* det_cnt, float* lab, int* lab_cnt, int B, int max_det,
                       const float* obj_thr, const float* cls_thr, int nthr, int filter_boxes, float frame_w,
                       float frame_h, leod_stream_t stream);

/* ---- optimiser / input ----------------------------------------------------------------------------- */

/* value-clip + AdamW over flat buffers (modules/detection.py:485-518; train.py:236-237). g is scaled/clipped in place.
 * hp_dev (optional) = device float[4] {lr, 1-beta1^step, sqrt(1-beta2^step), grad_scale} overriding the host scalars, so a
 * captured hipGraph can be replayed with a new learning rate every step. */
int leod_adamw_clip_step(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int step, float clip_value, float grad_scale, const float* hp_dev,
                         leod_stream_t stream);
/* Per-segment statistics of an fp32 buffer g[n] in one segmented pass (two launches): for each of nseg segments (= the parameters of a
 * flat gradient buffer) stats[s] = {sum |g|, sum g*g, max |g|} over its FINITE elements (double[nseg][3]), nonfinite[s] = its number of
 * inf / NaN elements (classified by exponent bits), *total = their sum over all segments.  Elements outside every segment (the
 * alignment padding between parameters) are never read into a result.  Sums are accumulated in double from the first add; there are no
 * floating-point atomics, so results are bit-identical from run to run.  The reference computes grad.abs().mean() per parameter with one
 * reduction and one read-back each (callbacks/utils/visualization.py:5-23) and GradScaler's inf check per tensor (train.py:243).
 * Tables: seg [nseg][3] longs = {offset, length, index of the segment's first chunk}, once on the HOST (seg_host, validated on every call)
 * and once on the device (seg_dev); chunk_dev [nchunk][2] ints = {segment, chunk index within the segment}, a segment of length L owning
 * ceil(L / chunk_floats) consecutive chunks.  LEOD_ERR_ARG before any launch unless offsets are multiples of 4 floats, ascending and
 * disjoint, lengths >= 1, every segment inside g[0, n), first-chunk indices running sums that end at nchunk, g 16-byte aligned and
 * n < 2^31.  ws = caller-owned device scratch of the size leod_grad_stats_query reports.  nseg == 0: only *total = 0.
 * leod_grad_stats_query (host only, no launch): *chunk_floats = floats per chunk, *ws_bytes = scratch bytes for nchunk chunks. */
int leod_grad_stats_query(long nchunk, int* chunk_floats, long* ws_bytes);
int leod_grad_stats(const float* g, long n, const long* seg_host, const long* seg_dev, int nseg, const int* chunk_dev, long nchunk,
                    void* ws, double* stats, int* nonfinite, int* total, leod_stream_t stream);
/* leod_adamw_clip_step that is NOT taken when a gradient is non-finite (what GradScaler.step does under the reference's precision 16,
 * train.py:243), decided on the device: no host read-back.  nonfinite_total = the device total of leod_grad_stats over g; state =
 * device int[2] {applied, skipped}; scratch = device float[8] owned by the caller (per-step scalars + skip word, written here).
 * Launch one (one thread): total != 0 -> skip word set, ++skipped; else t = ++applied and {lr, 1-beta1^t, sqrt(1-beta2^t), grad_scale}
 * (double pow rounded to float, as the entry above) go to scratch.  Launch two: the AdamW body of the entry above with those scalars;
 * every thread returns at once on a skipped step, which leaves p, m, v AND g untouched, so moments and bias corrections do not advance.
 * The host cannot know the outcome: registered weight shadows are marked stale either way. */
int leod_adamw_clip_step_guarded(float* p, float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, float clip_value, float grad_scale, const int* nonfinite_total, int* state,
                                 float* scratch, leod_stream_t stream);
/* bf16 shadow of a flat fp32 parameter buffer (the reference keeps ONE copy of the weights and lets autocast convert them per op,
 * train.py:236-243 precision=16; here the Linear kernels of precision mode bf16 read a 16-bit copy made once per optimiser step).
 * leod_set_weight_shadow registers shadow16 (n bf16 values, caller-owned) for the n floats at base (shadow16 == NULL withdraws it);
 * leod_weight_shadow_refresh rounds the registered buffers whose shadow is stale (force != 0: all of them, flags untouched -- for a
 * launch that is being recorded into a step plan / hipGraph) and returns the number of launches; leod_adamw_clip_step on a registered
 * buffer and leod_weight_shadow_invalidate mark shadows stale (stale shadows are never read); leod_weight_shadow_pin(1) makes the
 * launchers read the shadows regardless of the flags while a step is being recorded behind a forced refresh. */
int leod_set_weight_shadow(const float* base, long n, void* shadow16);
/* fp16 copy (n values, caller-owned, 8-byte aligned; NULL withdraws it) of a buffer registered above: leod_weight_shadow_refresh writes it
 * next to the bf16 copy in precision mode 2 ("16f"), whose forward GEMMs read it (the gradient GEMMs keep reading the bf16 copy).
 * LEOD_ERR_ARG if base is not registered. */
int leod_set_weight_shadow_f16(const float* base, void* shadow_f16);
int leod_weight_shadow_refresh(int force, leod_stream_t stream);
int leod_weight_shadow_invalidate(void);
int leod_weight_shadow_pin(int on);
/* Options of the attention block that no shipped config enables (the shipped block is fused into the GEMM kernels and never comes here).
 * act: 0 gelu 1 silu / swish 2 relu 3 sigmoid 4 tanh 5 relu6 6 leaky_relu 7 elu 8 hard_sigmoid 9 hard_swish 10 mish 11 selu 12 celu 13 hard_mish
 * (`mlp_activation`, models/layers/maxvit/maxvit.py:357-365).  gated != 0 (GLU.forward, maxvit.py:80-82): p [M, 2 * inner] = (a | g),
 * h [M, inner] = a * act(g); gated == 0: p [M, inner], h = act(p).  The backward writes dp (same shape as p) from dh.  inner % 4 == 0. */
int leod_act_glu_fwd(const float* p, float* h, long M, int inner, int act, int gated, leod_stream_t stream);
int leod_act_glu_bwd(const float* p, const float* dh, float* dp, long M, int inner, int act, int gated, leod_stream_t stream);
/* Token masking of the first stage (recurrent_backbone/maxvit_rnn.py:190-192): x[m][:] = token where mask[m] (in place; x [M, C], mask
 * [M] bytes, token [C]); backward: dtoken[c] += sum of the masked rows of dx, which are then zeroed (in place). */
int leod_token_mask_fwd(float* x, const unsigned char* mask, const float* token, long M, int C, leod_stream_t stream);
int leod_token_mask_bwd(float* dx, const unsigned char* mask, float* dtoken, long M, int C, leod_stream_t stream);
/* out[i] = (i == idx) ? *g : 0 for i < n <= 64 (device scalar g): the gradient of one entry of the six-entry loss vector as a zero-padded vector. */
int leod_onehot_scale(const float* g, float* out, int n, int idx, leod_stream_t stream);
/* dst[0..3] = (a,b,c,d) on the device (launch-time scalars for a replayed hipGraph). */
int leod_set_scalars4(float* dst, float a, float b, float c, float d, leod_stream_t stream);
/* Recurrent-state plumbing as one launch per call (host arrays of up to 16 entries; pointers and sizes 16-byte aligned):
 * leod_rows_masked_zero -- tensors[k][b, :] = 0 where mask[b] (B rows of row_bytes[k] each): RNNStates.reset over the (h, c) of all
 *   stages, reference modules/utils/detection.py:60-75 (`t[mask] = 0` per tensor);
 * leod_copy_multi -- dst[k][:] = src[k][:]: the initial (h, c) of a stage into slot 0 of its sequence buffers
 *   (reference models/layers/rnn.py:53-60 takes them as h_and_c_previous). */
int leod_rows_masked_zero(void* const* tensors, const long* row_bytes, int n, const unsigned char* mask, int B, leod_stream_t stream);
int leod_copy_multi(void* const* dst, const void* const* src, const long* nbytes, int n, leod_stream_t stream);
/* Channel concatenation of two NHWC maps, the first optionally upsampled x2 (nearest) on the way: out [B,H,W,Ca+Cb] from a [B,H>>up,W>>up,Ca]
 * and b [B,H,W,Cb] -- torch.cat([upsample(a), b], 1) of the PAFPN top-down path (models/detection/yolox_extension/models/yolo_pafpn.py:113-123)
 * and the cat of CSPLayer (models/detection/yolox/models/network_blocks.py:160-166) as one launch; _bwd: da (summed over the 2 x 2 copies when
 * up = 1) and db from dout.  fp32, Ca % 4 == Cb % 4 == 0, up in {0, 1}. */
int leod_cat2_up_fwd(const float* a, const float* b, float* out, int B, int H, int W, int Ca, int Cb, int up, leod_stream_t stream);
int leod_cat2_up_bwd(const float* dout, float* da, float* db, int B, int H, int W, int Ca, int Cb, int up, leod_stream_t stream);
/* dst[idx[j], :] += src[j, :] for j < nsel, rows of row_floats floats (% 4 == 0), idx unique and in [0, nrows_dst): the gradient of the labelled
 * frames added into the gradient of a stage's output map (the `selected_indices` gather of BackboneFeatureSelector, modules/utils/detection.py:120-157,
 * differentiated).  No atomics: the indices of one call must be distinct. */
int leod_rows_index_add(float* dst, const float* src, const long* idx, int nsel, long row_floats, int nrows_dst, leod_stream_t stream);
/* hflip TTA input of the pseudo-label pass (modules/pseudo_labeler.py:469-470: cat([ev, flip(ev, -1)], batch dim)) in one pass:
 * frames[t] = [B, rows_per_sample, W] bytes (T device pointers in a HOST array), out = [T, 2B, rows_per_sample, W]:
 * out[t, b] = frames[t][b], out[t, B + b, r, x] = frames[t][b, r, W - 1 - x]. */
int leod_stack_hflip_u8(const void* const* frames, int T, void* out, int B, long rows_per_sample, int W, leod_stream_t stream);
/* StackedHistogram.construct (data/utils/representations.py:78-123): int64 events -> uint8 [2*bins,H,W]. */
int leod_voxelize_u8(const long* x, const long* y, const long* pol, const long* t, long n_events, int* counts_ws,
                     unsigned char* out, int bins, int H, int W, int count_cutoff, int fastmode, leod_stream_t stream);
/* MixedDensityEventStack.construct (data/utils/representations.py:132-221): int64 events (time sorted) -> int8 [bins,H,W]: polarity sums
 * (2*pol-1) in the logarithmic time bin floor(max(bins - log(t_norm)/log(1/2), 0)), running sum over the bins in int8 arithmetic, clamp to
 * +-count_cutoff (count_cutoff < 0 = none, <= 127).  counts_ws: bins*H*W int32 of scratch. */
int leod_mixed_density_i8(const long* x, const long* y, const long* pol, const long* t, long n_events, int* counts_ws,
                          signed char* out, int bins, int H, int W, int count_cutoff, leod_stream_t stream);
/* Recording ingestion (csrc/k_ingest.hip): the raw 8-byte records of a Prophesee .dat file (u32 t in microseconds; i32 with x in bits 0-13,
 * y in bits 14-27, p in bit 28), time sorted, to the stacked histograms of n_win windows.  Window w holds events win_off[w] ..
 * win_off[w+1]-1 (win_off: n_win + 1 ascending int64 offsets on the device); out[w] equals leod_voxelize_u8 on exactly those events
 * (t0 / t1 = the window's first / last event time; an empty window is all zeros).  ds2 != 0 (H and W even) writes [.., H/2, W/2] =
 * full[.., 1::2, 1::2] of the full-resolution histogram, what nearest-exact interpolation at scale 0.5 selects.  The windows are processed
 * ws_windows at a time: one clear, one count launch, one finalise launch per chunk; counts_ws holds ws_windows * 2*bins*Ho*Wo int32
 * (16-byte aligned for the packed finalise stores, else they go out byte-wise).  An event with x >= W or y >= H is skipped and added to *dropped (device counter the caller zeroes; may be NULL).
 * count_cutoff <= 0: none. */
int leod_voxelize_dat_windows(const void* records, long n_events, const long* win_off, int n_win, int* counts_ws, int ws_windows,
                              unsigned char* out, int bins, int H, int W, int ds2, int count_cutoff, int fastmode, long* dropped,
                              leod_stream_t stream);
/* Metavision RAW payloads (csrc/k_evt.hip; layouts and the project's rules: DESIGN.md section 1) -> the 8-byte .dat records above, in
 * stream order, one chunk of words per scan + emit pair.  fmt 2: EVT2, little-endian u32 words, type in bits 31:28 (0 / 1 CD_OFF / CD_ON:
 * low 6 time bits in 27:22, x in 21:11, y in 10:0; 8 EVT_TIME_HIGH: bits 27:0; A, E, F ignored; others unknown), t = (high << 6) | low.
 * fmt 3: EVT3, little-endian u16 words, type in bits 15:12 (0 ADDR_Y: y = bits 10:0; 2 ADDR_X: one event, x = bits 10:0, p = bit 11;
 * 3 VECT_BASE_X: base = bits 10:0, p = bit 11; 4 VECT_12 / 5 VECT_8: an event at base + i for every set bit i of bits 11:0 / 7:0 in
 * ascending i, then base += 12 / 8; 6 TIME_LOW, 8 TIME_HIGH: bits 11:0; 7, A, E, F ignored; others unknown),
 * t = ((wraps * 4096 + high) << 12) | low, one wrap where TIME_HIGH falls by 2048 or more.  Times are shifted by the file's first
 * TIME_HIGH (<< 12 / << 6); an event before every field it needs is set is dropped and counted; x and y are not range-checked.
 * state: 16 longs on the device, carried from chunk to chunk (all zero before the first chunk; state_out may be state_in):
 *   [0] valid bits (1 time high, 2 time low, 4 row, 8 vector base) [1] last TIME_HIGH [2] clock wraps [3] TIME_LOW [4] row [5] vector base
 *   [6] vector polarity [7] time base [8] events [9] early events [10] ignored words [11] unknown words [12] overflow: a shifted time
 *   outside [0, 2^32) was met (its record holds the low 32 bits) [13] fmt of the last chunk [14] events of the last chunk [15] 0.
 * leod_evt_query (host only): *tile_words = words per tile, *tiles_per_pass = tile summaries the scan workgroup takes per pass,
 *   *ws_bytes = workspace for a chunk of n_words words (any may be NULL).
 * leod_evt_scan: per-tile reduce + the one-workgroup scan (2 launches): fills ws and writes state_out, so state_out[14] sizes the output.
 * leod_evt_emit: same words, same ws; stores the records (out: 8-byte aligned, capacity in records; nothing is stored at or beyond
 *   capacity) and ORs the overflow flag into state_out[12].  words: 16-byte aligned; ws: 8-byte aligned.  -1 for bad arguments. */
int leod_evt_query(long n_words, int* tile_words, int* tiles_per_pass, long* ws_bytes);
int leod_evt_scan(const void* words, long n_words, int fmt, const long* state_in, long* state_out, void* ws, long ws_bytes,
                  leod_stream_t stream);
int leod_evt_emit(const void* words, long n_words, int fmt, const void* ws, long ws_bytes, void* out, long capacity, long* state_out,
                  leod_stream_t stream);
/* The way back (csrc/k_evtenc.hip; the rule: DESIGN.md section 1): the 8-byte .dat records above, in stream order, t non-decreasing ->
 * the words of a Metavision RAW payload in the layouts above, one chunk of records per scan + emit pair.  The words of a recording are
 * those of raw_events.encode_evt2 / encode_evt3 (leod_amd/data/utils/raw_events.py) on all its events at once, however it is cut into
 * chunks: the stream opens with TIME_HIGH = first_time_high (fmt 3: < 4096; fmt 2: < 2^27), which the first call writes whatever its
 * events are; TIME_HIGH where it changes (fmt 3: in steps of at most 1024) and before every high_period-th (1 .. 2^30) group; fmt 3:
 * TIME_LOW and ADDR_Y where they change; vectors (fmt 3 only): two or more consecutive events of one t, y, p with strictly ascending x
 * inside the 12 columns of the first are one VECT_BASE_X + VECT_12 (VECT_8 where 8 columns do).  fmt, vectors, high_period and
 * first_time_high must be the same in every call of a recording.  With vectors the last group of a chunk is held back in the state until
 * a later event closes it or final_chunk != 0 is given.  At most 2^31 - 1 events per call.
 * state: 32 longs on the device, carried from chunk to chunk (all zero before the first chunk; state_out must not be state_in, which is
 *   not modified):
 *   [0] the opening word is written [1] [2] [3] time high (not reduced to 12 bits), time low and row of the last group written
 *   [4] groups written (fmt 2: events) [5] events taken [6] words written [7] vector groups written [8] events held back (0 .. 12)
 *   [9] time of the last event taken [10] words of the last call (sizes its output) [11] records of the last call with x >= 2048 or
 *   y >= 2048, which no EVT word holds [12] position of the first of them in its chunk (-1: none) [13] position in its chunk of the first
 *   record of the last call whose time is below that of the record before it (-1: none; 0: below the last time of the chunk before)
 *   [14] [15] the two times around it [16] fmt [17] vectors [18] high_period [19] first_time_high [20 .. 31] the records held back.
 *   After a call that sets [11] or [13] the state and the words are of no use.
 * leod_evtenc_query (host only): *tile_events = events per tile, *ws_bytes = workspace for a chunk of n_events, *max_words = an upper
 *   bound of the words n_events events take in one call (any may be NULL).
 * leod_evtenc_scan: one memset, the marking and group-count launches (vectors only), the per-tile count and the one-workgroup scan: fills
 *   ws and writes state_out, so state_out[10] sizes the output.
 * leod_evtenc_emit: same arguments, same ws, the state_in of the scan; stores the words (out: 4-byte aligned, capacity in words; nothing
 *   is stored at or beyond capacity), one launch.  records, ws: 8-byte aligned.  -1 for bad arguments. */
int leod_evtenc_query(long n_events, int fmt, int* tile_events, long* ws_bytes, long* max_words);
int leod_evtenc_scan(const void* records, long n_events, int fmt, int vectors, int final_chunk, long high_period, long first_time_high,
                     const long* state_in, long* state_out, void* ws, long ws_bytes, leod_stream_t stream);
int leod_evtenc_emit(const void* records, long n_events, int fmt, int vectors, int final_chunk, long high_period, long first_time_high,
                     const long* state_in, const void* ws, long ws_bytes, void* out, long capacity, leod_stream_t stream);
/* Event noise filters (csrc/k_filter.hip; the rule: DESIGN.md section 1) on the 8-byte .dat records above, in stream order, t
 * non-decreasing.  An event with x >= W or y >= H is removed (outside); one on a pixel with mask[y * W + x] != 0 is removed (masked; mask
 * may be NULL); any other is kept iff an earlier event that passed these two tests lies on one of its 8 neighbour pixels, at most tau_us
 * before it (0 <= tau_us < 2^31), else it is removed (unsupported) -- and still supports later events; tau_us = -1 switches this third
 * test off.  At most 2^31 - 1 events per call.
 * state: 8 + H * W longs on the device, updated in place, carried from chunk to chunk: [0] seen [1] kept [2] outside [3] masked
 *   [4] unsupported [5] time of the last event seen (-1: none) [6] [7] 0; then the surface [H, W]: the last time per pixel (-1: never).
 *   A recording starts from zero counters and -1 everywhere else.
 * io: 4 longs on the device: [0] records kept by this call so far (in: 0; sizes the output) [1] position of the first event whose time
 *   is below that of the event before it (in: the largest long; stays so for a sorted chunk) [2] [3] the two times around it.
 * leod_event_filter_query (host only): *tile_events = records per tile of the compaction, *tiles_per_pass = tile counts the scan workgroup
 *   takes per pass, *table_bytes = the table that takes n_events records in one piece, *marks_bytes = the marks of a chunk of n_events.
 * leod_event_filter_scan: decides every record of the chunk; table (16-byte aligned): table_bytes of scratch, at least 1024 -- a chunk
 *   that needs more than it holds is cut at record boundaries into pieces of whole tiles that fit (that takes 8192 bytes or more), one
 *   memset and four launches each; marks (8-byte aligned) receives the chunk's decisions.
 * leod_event_filter_emit: same records, same marks; stores the kept records in order (out: 8-byte aligned, capacity in records; nothing
 *   is stored at or beyond capacity), one launch.
 * leod_event_pixel_counts: counts[y * W + x] += 1 for every event inside the sensor, *outside += the others (both on the device).
 * -1 for bad arguments. */
int leod_event_filter_query(long n_events, int* tile_events, int* tiles_per_pass, long* table_bytes, long* marks_bytes);
int leod_event_filter_scan(const void* records, long n_events, int H, int W, long tau_us, const unsigned char* mask, long* state,
                           void* table, long table_bytes, void* marks, long marks_bytes, long* io, leod_stream_t stream);
int leod_event_filter_emit(const void* records, long n_events, const void* marks, long marks_bytes, void* out, long capacity,
                           leod_stream_t stream);
int leod_event_pixel_counts(const void* records, long n_events, int H, int W, long* counts, long* outside, leod_stream_t stream);
/* Per-pixel event filters (csrc/k_pixfilter.hip; the rule: DESIGN.md section 1) on the same records, in stream order, t non-decreasing:
 * bounds and mask as above (outside, masked; such events touch no state); any other event is a candidate and updates its pixel's state,
 * whatever its verdict.  burst_us (-1: off; else 0 <= burst_us < 2^31): a candidate continues the burst of the candidate before it on
 * its pixel when the polarity is the same and it lies at most burst_us behind it; its position k is counted 1, 2, 3 (= 3 or later);
 * burst_keep 0 keeps k = 1 (trail), 1 keeps k = 2, 2 keeps k >= 2 (STC); the others are removed (burst).  lock (0: off; else 1..255) with
 * 1 <= p_min_us <= p_max_us < 2^31: a rising edge is an ON candidate that is the pixel's first or follows an OFF one; n_per counts
 * consecutive periods between rising edges within [p_min_us, p_max_us], saturates at lock, and is reset by a period outside the band or
 * by any candidate later than p_max_us behind the last edge; while n_per >= lock every candidate of the pixel is removed (flicker,
 * which is tested before burst).  At most 2^31 - 1 events per call.
 * state: 8 + 4 * H * W longs on the device, updated in place, carried from chunk to chunk: [0] seen [1] kept [2] outside [3] masked
 *   [4] flicker [5] burst [6] time of the last event seen (-1: none) [7] 0; then per pixel q at 8 + 4 * q: t_prev (time of the last
 *   candidate; -1: never), t_edge (time of the last rising edge; -1: none), p_prev + 2 * k_prev, n_per.  A recording starts from zero
 *   counters, [6] = -1 and {-1, -1, 0, 0} in every pixel.
 * io: as for leod_event_filter_scan.
 * leod_pixel_filter_query (host only): *tile_events = records per tile (of the sort and of the compaction), *tiles_per_pass = tile counts
 *   the scan workgroup takes per pass, *digit_bits = key bits per pass of the sort (ceil(ceil(log2(H * W)) / digit_bits) passes),
 *   *ws_bytes = the workspace that takes n_events records in one piece, *marks_bytes = the marks of a chunk of n_events (any may be NULL).
 * leod_pixel_filter_scan: decides every record of the chunk; ws (8-byte aligned): ws_bytes of scratch -- a chunk that needs more than it
 *   holds is cut at record boundaries into pieces of whole tiles that fit (the workspace of one tile, leod_pixel_filter_query(1, ...), is
 *   the least); marks (8-byte aligned) receives the chunk's decisions in the layout leod_event_filter_emit reads, which stores the kept
 *   records.  -1 for bad arguments. */
int leod_pixel_filter_query(long n_events, int H, int W, int* tile_events, int* tiles_per_pass, int* digit_bits, long* ws_bytes,
                            long* marks_bytes);
int leod_pixel_filter_scan(const void* records, long n_events, int H, int W, long burst_us, int burst_keep, long p_min_us, long p_max_us,
                           int lock, const unsigned char* mask, long* state, void* ws, long ws_bytes, void* marks, long marks_bytes,
                           long* io, leod_stream_t stream);
/* Filter survey (csrc/k_survey.hip; the definitions and identities: DESIGN.md section 1) on the same records, in stream order, t
 * non-decreasing: one pass that filters nothing and adds to integer histograms from which the counters of every filter above follow for
 * a whole list of thresholds.  edges_us (HOST array): n_edges strictly increasing values, 0 <= e < 2^31, 1 <= n_edges <= 64 (= K);
 * bin(d) = the number of edges < d.  Bounds and mask as above; any other event is a candidate.  p_min_us = p_max_us = 0: no flicker band
 * (run[] is not touched); else 1 <= p_min_us <= p_max_us < 2^31.  At most 2^31 - 1 events per call.
 * state: 8 + (5 * K + 262) + 4 * H * W longs on the device, updated in place, carried from chunk to chunk: [0] seen [1] candidates
 *   [2] outside [3] masked [4] time of the first event seen (-1: none) [5] time of the last event seen (-1: none) [6] [7] 0; then
 *   nb[K + 2] (d = t - the latest earlier candidate on one of the 8 neighbours; [K + 1]: none), same[K + 1] (d = t - t_prev where the
 *   pixel's previous candidate has the same polarity), sec_on[K + 1], sec_off[K + 1] (c = the `same` bin of a candidate, c' = that of its
 *   predecessor on the pixel, either INF where there is none: when c < c' and c < K, sec_on[c] += 1 and, if c' <= K, sec_off[c'] += 1),
 *   period[K + 1] (d = t - t_edge at every rising edge with an edge before it), run[256] (n_per of the anti-flicker rule with lock = 255,
 *   after every candidate; only with a band); then per pixel q four words: t_prev (time of the last candidate -- also the surface of the
 *   activity filter; -1: never), t_edge (time of the last rising edge; -1: none), p_prev + 2 * c_prev (c_prev: the `same` bin of the last
 *   candidate, 255 = INF), n_per.  A recording starts from zeros, [4] = [5] = -1 and {-1, -1, 510, 0} in every pixel.
 * io: as for leod_event_filter_scan ([0] is not used).
 * leod_survey_query (host only): *tile_events = records per tile of the sort, *digit_bits = key bits per pass of the sort
 *   (ceil(ceil(log2(H * W + 1)) / digit_bits) passes), *ws_bytes = the workspace that takes n_events records in one piece,
 *   *state_longs = the size of the state block (any may be NULL).
 * leod_survey_events: ws (8-byte aligned): ws_bytes of scratch -- a chunk that needs more than it holds is cut at record boundaries into
 *   pieces of whole tiles that fit (the workspace of one tile, leod_survey_query(1, ...), is the least); per piece four launches and three
 *   per pass of the sort.  -1 for bad arguments (edges included). */
int leod_survey_query(long n_events, int H, int W, int n_edges, int* tile_events, int* digit_bits, long* ws_bytes, long* state_longs);
int leod_survey_events(const void* records, long n_events, int H, int W, const long* edges_us, int n_edges, long p_min_us, long p_max_us,
                       const unsigned char* mask, long* state, void* ws, long ws_bytes, long* io, leod_stream_t stream);
/* Sensor fit (csrc/k_fit.hip; the rule: DESIGN.md section 1) on the same records, in stream order, t non-decreasing: events of a sensor
 * (Hs, Ws) onto a frame (Hd, Wd).  An event with x >= Ws or y >= Hs is removed (outside).  Any other is mapped, all in integers:
 * mirror (0 / 1): x = Ws - 1 - x; orient (0, 90, 180, 270 degrees clockwise): 90 (Hs - 1 - y, x), 180 (Ws - 1 - x, Hs - 1 - y),
 * 270 (y, Ws - 1 - x), giving (x', y') in an image (H', W') = (Hs, Ws), or (Ws, Hs) at 90 / 270; scale k: cell (x' / k, y' / k) of the
 * scaled image (H' / k, W' / k), an event of an incomplete edge cell is removed (cropped); place: xd = x' / k + ox, yd = y' / k + oy, an
 * event outside [0, Wd) x [0, Hd) is removed (cropped).  reduce 0 (pick): an event is kept iff x' % k == k / 2 and y' % k == k / 2, else
 * removed (skipped); 1 (sum): every event is kept; 2 (fire): per destination pixel an accumulator a takes the pixel's events in stream
 * order, a += +1 (ON, bit 28) or -1 (OFF); the event that brings a to +threshold or -threshold is kept and a = 0, any other is removed
 * (merged); threshold is read with reduce 2 only.  A kept record is stored with t and bits 28-31 unchanged and x, y replaced by xd, yd;
 * kept records stay in stream order.  At most 2^31 - 1 events per call.
 * Limits: Hs, Ws, Hd, Wd in [1, 16384] (so Hd * Wd <= 2^28, the bound of the per-pixel filter), k in [1, 64], |ox|, |oy| <= 16384,
 *   threshold in [1, 32767].
 * state: 8 + Hd * Wd longs on the device, updated in place, carried from chunk to chunk: [0] seen [1] kept [2] outside [3] cropped
 *   [4] skipped [5] merged [6] time of the last event seen (-1: none) [7] 0; then the accumulators [Hd, Wd] (touched by reduce 2 only).
 *   A recording starts from zeros and [6] = -1.
 * io: as for leod_event_filter_scan.
 * leod_event_fit_query (host only): *tile_events = records per tile (of the sort and of the compaction), *tiles_per_pass = tile counts the
 *   scan workgroup takes per pass, *digit_bits = key bits per pass of the sort (ceil(ceil(log2(Hd * Wd)) / digit_bits) passes),
 *   *ws_bytes = the workspace that takes n_events records in one piece (0 for reduce 0 and 1, which sort nothing), *marks_bytes = the marks
 *   of a chunk of n_events (any may be NULL).
 * leod_event_fit_scan: decides every record of the chunk; reduce 0 / 1: two launches, ws is not read (may be NULL); reduce 2: ws (8-byte
 *   aligned): ws_bytes of scratch -- a chunk that needs more than it holds is cut at record boundaries into pieces of whole tiles that
 *   fit (the workspace of one tile, leod_event_fit_query(1, ...), is the least), four launches and three per pass of the sort each;
 *   marks (8-byte aligned) receives the chunk's decisions (class 0 = kept, as leod_event_filter_emit reads them).
 * leod_event_fit_emit: same records, same geometry, same marks; stores the kept records in order with the mapped coordinates (out: 8-byte
 *   aligned, capacity in records; nothing is stored at or beyond capacity), one launch.  -1 for bad arguments. */
int leod_event_fit_query(long n_events, int Hd, int Wd, int reduce, int* tile_events, int* tiles_per_pass, int* digit_bits, long* ws_bytes,
                         long* marks_bytes);
int leod_event_fit_scan(const void* records, long n_events, int Hs, int Ws, int Hd, int Wd, int orient, int mirror, int k, int ox, int oy,
                        int reduce, int threshold, long* state, void* ws, long ws_bytes, void* marks, long marks_bytes, long* io,
                        leod_stream_t stream);
int leod_event_fit_emit(const void* records, long n_events, int Hs, int Ws, int Hd, int Wd, int orient, int mirror, int k, int ox, int oy,
                        int reduce, const void* marks, long marks_bytes, void* out, long capacity, leod_stream_t stream);
/* Video-to-events simulator (csrc/k_simulate.hip; the rule: DESIGN.md section 1): luma frames (uint8 [n_frames, H, W] on the device) with
 * their times (times_us: device long [n_frames], strictly increasing, above the time the state carries, below 2^32) -> .dat records, all
 * in integers.  lut (device int [256], values in [0, 2^24)) is the response table, theta_on / theta_off (device int [H, W], >= 1) the
 * thresholds.  Per pixel: a reference level m, the time t_keep of its last kept event (-1: none), the byte of the last frame.  The first
 * frame of a recording sets m = lut[v] and emits nothing.  Any later frame at t1, after one at t0, with l0 = lut[v before], l1 = lut[v],
 * D = t1 - t0: l1 > l0: for j = 1, 2, ... while m + j * theta_on <= l1 an ON candidate at t = t0 + max(1, D * (m + j * theta_on - l0) /
 * (l1 - l0)), then m += n * theta_on; l1 < l0: the same with OFF, levels m - j * theta_off >= l1, t = t0 + max(1, D * (l0 - (m - j *
 * theta_off)) / (l0 - l1)); l1 == l0: nothing.  A candidate is kept unless t_keep >= 0 and t - t_keep < refractory_us; a kept one sets
 * t_keep = t, a dropped one is counted and still moves m.  The records (t u32, x bits 0-13, y bits 14-27, ON = bit 28) come out ordered
 * by t, then pixel y * W + x, then j.  The caller checks the values (ops.simulate_check): the device clamps what would leave a buffer.
 * Limits: H, W in [1, 16384], H * W < 2^30, n_frames <= 65536 per call, refractory_us in [0, 2^32), (max lut - min lut) / min theta <=
 *   4096 (at most 4097 candidates per pixel and interval, as m may lag the value by theta - 1), at most 2^31 - 1 events per call.
 * state: *state_longs longs on the device, updated in place by leod_simulate_emit alone, carried from call to call: [0] frames seen
 *   [1] kept events [2] ON [3] OFF [4] refractory-dropped [5] time of the last frame (-1: none) [6], [7] 0; then {m, t_keep} per pixel;
 *   then the last frame's bytes, padded with zeros to a whole long.  A recording starts from zeros, [5] = -1 and every t_keep = -1.
 * counts: *count_longs + n_frames longs on the device (8-byte aligned), written by leod_simulate_count and read by leod_simulate_emit
 *   of the same arguments: kept events per tile of pixels, per pixel (32 bits each), and behind them per interval: counts[*count_longs
 *   + k] = the kept events of the interval that ends at frame k of the call (0 for the first frame of a recording).
 * leod_simulate_query (host only): *tile_pixels = pixels per tile (one lane a pixel), *digit_bits = key bits per pass of the sort
 *   (ceil(ceil(log2(t_end - t_base)) / digit_bits) passes), *state_longs, *count_longs as above, *ws_bytes = the workspace of a call that
 *   keeps n_events events (any may be NULL).
 * leod_simulate_count: one memset and one launch; writes counts, nothing else.
 * leod_simulate_emit: n_events = the sum of the call's interval counts, t_base = the time of the frame before the call's first interval
 *   (state [5], or times_us[0] for the first call of a recording), t_end = times_us[n_frames - 1]; ws (8-byte aligned, ws_bytes >= the
 *   query's; not read for n_events = 0); out: 8-byte aligned, capacity >= n_events records.  Four launches and three per pass of the
 *   sort (n_events = 0: three launches).  -1 for bad arguments. */
int leod_simulate_query(long n_events, int H, int W, int* tile_pixels, int* digit_bits, long* state_longs, long* count_longs,
                        long* ws_bytes);
int leod_simulate_count(const unsigned char* frames, int n_frames, int H, int W, const long* times_us, const int* lut, const int* theta_on,
                        const int* theta_off, long refractory_us, const long* state, long* counts, leod_stream_t stream);
int leod_simulate_emit(const unsigned char* frames, int n_frames, int H, int W, const long* times_us, const int* lut, const int* theta_on,
                       const int* theta_off, long refractory_us, long* state, long* counts, long t_base, long t_end, long n_events,
                       void* ws, long ws_bytes, void* out, long capacity, leod_stream_t stream);

/* Packed event frames (csrc/k_pack.hip; format: leod_amd/data/utils/packed.py).  A frame of E = C*H*W bytes is a blob:
 * {u32 n_masks, u32 n_values, 8 zero bytes}, ceil(E/4096) group entries {u64 l1, u32 mask_base, u32 value_base}, n_masks u64 block masks,
 * n_values non-zero bytes, zero padding to 16.
 * leod_unpack_frames_u8: out [n_slots, C, H, W]; slot i decodes the blob at blob + slot_off[i] (device int64; 16-byte aligned offsets;
 * negative, misaligned or out-of-extent = a frame of zeros); slot_flags (device int32, may be NULL) bit 0 = write the channel planes in
 * reverse order.  Every output byte is stored exactly once by one launch (no clear, no atomics).  nbytes is the extent of the blob buffer
 * (16-byte aligned): positions taken from blob contents are compared with it before they are read, so a malformed blob gives wrong frames
 * and no access outside [blob, blob + nbytes) or out.  -1 for bad arguments, -3 for E >= 2^31. */
int leod_unpack_frames_u8(const unsigned char* blob, long nbytes, const long* slot_off, const int* slot_flags, int n_slots,
                          unsigned char* out, int C, int H, int W, leod_stream_t stream);
/* Bytes of the largest blob a frame of E elements can take (every element non-zero), a multiple of 16; 0 for E < 1. */
long leod_pack_frame_stride(long E);
/* Encoder: frames [n, E] uint8 -> blob k at ws + k*stride (stride >= leod_pack_frame_stride(E), multiple of 16; ws 16-byte aligned) and its
 * size in bytes in sizes[k] (device int64).  Three launches: per-group counts, per-frame exclusive scan, masks and values.  The bytes are
 * those of the numpy codec. */
int leod_pack_frames_u8(const unsigned char* frames, int n, long E, unsigned char* ws, long stride, long* sizes, leod_stream_t stream);
/* Blob k from ws + k*stride to out + offsets[k] .. out + offsets[k+1] (device int64 [n+1], multiples of 16 within [0, out_bytes]; a frame
 * whose offsets do not fit is skipped). */
int leod_pack_compact_u8(const unsigned char* ws, long stride, const long* offsets, int n, unsigned char* out, long out_bytes,
                         leod_stream_t stream);

/* The same format on the HOST (csrc/packed_host.cpp; b and out are host pointers, no stream): what the frame store runs on every blob
 * before any decoder sees it, and the dense decoder of the loaders' host path; called through ctypes, so without the GIL.
 * leod_evp_validate: 0 = b[0 .. nbytes) is THE encoding of a frame of E elements, else the number (1 .. 12) of the first failed check of
 * packed.validate_frame (sizes, paddings, n_masks / n_values against the popcounts, mask_base / value_base against the running sums,
 * blocks and bits beyond E, empty masks, stored zeros).
 * leod_evp_decode: a validated blob -> out[C * HW] (contiguous); flip != 0 writes the channel planes in reverse order; indices are
 * still compared with their extents.  0, or -1 for bad arguments / a blob shorter than its counts say. */
int leod_evp_validate(const unsigned char* b, long nbytes, long E);
int leod_evp_decode(const unsigned char* b, long nbytes, int C, long HW, int flip, unsigned char* out);

/* On-device spatial augmentation of uint8 event representations src/dst [T,B,C,H,W] (data/utils/augmentor.py:216-331,
 * 390-401): per batch sample b, params[b] = {hflip, mode (0 none, 1 zoom-in, 2 zoom-out), x0, y0, win_h, win_w, tflip}
 * (7 ints); flip first, then the zoom with ATen's nearest-exact index rule; zoom-out leaves zeros outside the pasted
 * window.  tflip != 0 additionally applies time_flip_data (data/genx_utils/sequence_base.py:207-227): frames in reverse
 * order and the 2*bins channel planes of each frame reversed. */
int leod_augment_u8(const unsigned char* src, unsigned char* dst, const int* params, int T, int B, int C, int H, int W,
                    leod_stream_t stream);
/* The same pass with a rotation between the flip and the zoom (data/utils/augmentor.py:359-386,464-476: hflip -> rotate ->
 * zoom; torchvision rotate with NEAREST, expand=False, fill=None).  rot[b] = {cos a, sin a} of the sample's counter-clockwise
 * angle as fp32 (2 floats per sample); {1, 0} = no rotation for that sample.  Source index in fp32, one rounding per operation:
 * cx = 0.5*W - 0.5, cy = 0.5*H - 0.5, sx = rint(c*(x-cx) - s*(y-cy) + cx), sy = rint(s*(x-cx) + c*(y-cy) + cy) (round half to
 * even, as grid_sample(nearest) over affine_grid(align_corners=False)); pixels whose source falls outside the frame are 0.
 * Same refusals as leod_augment_u8, plus a NULL rot. */
int leod_augment_rot_u8(const unsigned char* src, unsigned char* dst, const int* params, const float* rot, int T, int B, int C,
                        int H, int W, leod_stream_t stream);

/* Prediction-video frames (csrc/k_render.hip; reference vis_pred.py:74-93 for the base image, :126-215 for what is drawn on it): the
 * event representation ev [L,C2,H,W] (uint8, or fp32 when ev_is_f32 != 0; counts >= 0, C2 = 2*bins) -> out [L, up*H, up*W, 3] uint8
 * RGB rows, up = 1 or 2.  A source pixel with any channel > 0 is 0.25, every other 1.0; bilinear x2 (align_corners=False), * 255, rounded
 * -- evaluated in integers: K = sum of the quarter weights wy*wx over the event taps, byte = (16320 - 765 K + 32) >> 6 (up = 1: 64 / 255).
 * Overlay items, drawn in the same pass in item order (the later item wins): items [n_items,8] int32 = {frame, kind, x, y, a, b, c, rgb}
 * sorted by frame, rgb = r | g<<8 | b<<16, coordinates in output pixels; frame_off [L+1] int32 = first item of every frame.
 * kind 0: rectangle outline, corners (x,y)-(a,b), thickness 1 <= c <= 65536 (pixels in [x-c/2, a+(c-1)/2] x [y-c/2, b+(c-1)/2] that are not in
 * [x+(c-1)/2+1, a-c/2-1] x [y+(c-1)/2+1, b-c/2-1]).  kind 1: one text line with bottom-left (x,y), integer scale 1 <= a <= 65536, bytes
 * text[b .. b+c-1] in the 5 x 7 font of leod_render_font (advance 6a; a byte outside 0x20-0x7E is a solid block).  Everything is clipped
 * to the frame.  ws: L*H*W bytes of scratch (the event mask).  n_items == 0: frame_off / items / text may be NULL.
 * An item whose thickness / scale lies outside [1, 65536] or whose kind is neither 0 nor 1 draws nothing; a text byte whose offset lies
 * outside [0, n_text) draws as a solid block (ops.render_frames refuses all of these before the upload).
 * Returns 0; -1 for up not in {1,2}, an odd C2, non-positive L / C2 / H / W, negative n_items / n_text, NULL ev / out / ws, or n_items > 0
 * with NULL frame_off / items; -3 for up*H or up*W above 32767; -2 if a launch failed. */
int leod_render_frames_u8(const void* ev, int ev_is_f32, unsigned char* out, int L, int C2, int H, int W, int up, const int* frame_off,
                          const int* items, int n_items, const unsigned char* text, int n_text, unsigned char* ws, leod_stream_t stream);
/* The renderer's font, copied to HOST memory dst[95*7]: glyphs of ASCII 0x20-0x7E, 7 rows each from the top, one byte per row, bit 4 =
 * leftmost of the 5 columns. */
int leod_render_font(unsigned char* dst);

/* Baseline JPEG of such frames (csrc/k_jpeg.hip; the reference hands its frames to an mp4 writer on the host, vis_pred.py:216-227): rgb
 * [n,H,W,3] uint8 -> n complete JFIF files back to back.  The stream is fixed: 4:4:4, the Annex K.1 quantisation
 * tables under the IJG rule for quality 1 .. 100, the Annex K.3 Huffman tables, one restart interval per row of 8 x 8 blocks, partial
 * blocks repeating the last column / row; colour conversion, DCT and quantisation in integers.  Two calls with the sizes between them:
 * leod_jpeg_scan transforms and codes the frames into ws and writes offsets[0 .. n] = base + the first byte of every file, offsets[n] = base +
 * all of them (device int64; the caller reads offsets[n] back, checks its buffer, and calls)
 * leod_jpeg_emit with the same n, H, W, quality, base and the untouched ws: it writes the files to out[0 .. offsets[n] - base) -- out is
 * where byte `base` of the blob goes, out_bytes the room from there; no byte at or behind out + out_bytes is written whatever ws holds.
 * leod_jpeg_query (host only): *ws_bytes = workspace of n frames (16-byte aligned; no more than n times that of one frame), *out_bound =
 * the most n files can take (header + 432 bytes per block and component + 2 per row), *header_bytes = bytes in front of a file's scan.
 * Outputs may be NULL.
 * Return 0; -1 for NULL pointers, n / H / W < 1, H or W above 65535, quality outside 1 .. 100, base < 0, a ws that is too small or not
 * 16-byte aligned; -2 if a launch failed. */
int leod_jpeg_query(int n, int H, int W, long* ws_bytes, long* out_bound, int* header_bytes);
int leod_jpeg_scan(const unsigned char* rgb, int n, int H, int W, int quality, void* ws, long ws_bytes, long* offsets, long base,
                   leod_stream_t stream);
int leod_jpeg_emit(const void* ws, long ws_bytes, int n, int H, int W, int quality, unsigned char* out, long out_bytes,
                   long base, leod_stream_t stream);

/* dgrad of a Linear fused with the LayerNorm backward of its producer (x -> norm -> Linear, maxvit.py:267-269,110-118):
 * dx[M,K] = LN-backward(dy[M,N] @ W[N,K]) (+ dres), dgamma[K] += sum dn*xhat, dbeta[K] += sum dn, with x[M,K] the LayerNorm
 * input and stats[M,2] its saved (mean, rstd).  Stage-1 shapes only (K = 48, N = 144 / 192, M >= 16384): returns -3
 * (unsupported shape) otherwise and the caller runs leod_linear_dgrad + leod_layernorm_bwd. */
int leod_linear_dgrad_lnbwd(const float* dy, const float* W, const float* x, const float* stats, const float* ln_w,
                            const float* dres, float* dx, float* dgamma, float* dbeta, int M, int N, int K, int dy_bf16,
                            leod_stream_t stream);

/* ---- launch plans (no counterpart in the reference: its answer to launch overhead is torch.compile(mode='reduce-overhead') = CUDA
 * graphs, config/model/maxvit_yolox/default.yaml:8-11, modules/detection.py:43-44) -----------------------------------------------
 * A plan replays a stream-captured hipGraph as plain stream launches from one C loop: hip_graph (hipGraph_t of a finished capture:
 * kernel / memset / 1-D memcpy nodes) is sorted topologically, its chains become lanes (lane 0 = the stream given to
 * leod_plan_launch, lanes 1 .. max_lanes-1 = streams owned by the plan), edges between lanes become event record / wait pairs.
 * ~3 us of host time per kernel, parallel branches stay parallel (hipGraphLaunch on ROCm 7.2: 8 us per node single-stream, and as
 * slow as eager Python launches once the graph forks).  The graph must outlive the plan (kernel argument blocks are borrowed).
 * leod_plan_create returns a handle > 0 or a negative error (-3: a node type a plan cannot replay; leod_plan_last_error() names it).
 * The library's own weight-pack kernels (conv3_pack_kernel, lstm_pack_kernel: they read parameters only) are taken out of the chain the capture
 * put them in and run on lane 1 from the start of the plan (LEOD_PLAN_HOIST=0: left where they were captured).
 * leod_plan_info: info[9] = kernels, memsets, memcpys, empty nodes, lanes, events, cross-lane waits, ops, collectives (kernel nodes that are
 * leod_comm_allreduce calls recorded during the capture: the replay issues the all-reduce on the op's lane). */
long leod_plan_create(void* hip_graph, int max_lanes);
/* Address ranges (start address as a long, length in bytes; n of them, copied) of PERSISTENT weight-pack buffers.  leod_plan_create moves a
 * weight-pack kernel (conv3_pack_kernel / lstm_pack_kernel) to the start of the plan -- dropping the stream-order edges of its capture --
 * only when the buffer it writes lies inside one of these ranges: a pack into a temporary of the captured step keeps its captured order
 * (that temporary may share its address with another temporary of the same capture). */
int leod_plan_set_hoist_ranges(const long* starts, const long* bytes, int n);
int leod_plan_launch(long plan, leod_stream_t stream);
/* The step's input tensor without a copy: every kernel of the plan that reads it (the stem convolution and its weight gradient register
 * themselves) and was captured with a pointer inside [captured_base, captured_base + bytes) reads new_base + the same offset from the next
 * launch on.  Returns the number of kernels re-pointed (0: none in this plan -- copy into the captured buffer instead), < 0 on error.  The
 * new buffer must stay alive and unchanged until the launches reading it have completed (the backward plan's stem weight gradient is the
 * last reader) -- what the reference's autograd requires of the event tensor too (modules/detection.py:196-207). */
int leod_plan_rebase_input(long plan, const void* captured_base, long bytes, const void* new_base);
/* leod_plan_launch without its closing join: `stream` does not wait for the plan's side lanes; leod_plan_join(plan, stream) makes it wait
 * later (before the plan is launched again and before anything reads what the side lanes wrote). */
int leod_plan_launch_nojoin(long plan, leod_stream_t stream);
int leod_plan_join(long plan, leod_stream_t stream);
int leod_plan_info(long plan, int* info);
int leod_plan_destroy(long plan);
int leod_plan_dump(long plan, const char* path); /* debug listing: lane, kernel, events per op in launch order */
const char* leod_plan_last_error(void);

/* ---- data-parallel exchange: the library's own RCCL communicator (csrc/k_comm.hip) ---------------------------------
 * The all-reduces of a data-parallel step -- SyncBatchNorm statistics of the detection head, gradient buckets (reference: Lightning's
 * DDP strategy with sync_batchnorm, train.py:131-133,247) -- enqueued on the caller's stream like kernels.  RCCL is resolved from the
 * process at run time (dlopen); without it every call returns -3.  Rank 0 draws an id and hands its 128 bytes to the other ranks (the
 * host side uses torch.distributed for that); leod_comm_init is collective and binds the CURRENT device.  One communicator per process. */
int leod_comm_unique_id(char* id128);
int leod_comm_init(const char* id128, int rank, int world);
int leod_comm_world(void);                                  /* ranks of the communicator, 0 = none */
/* buf[count] <- element-wise sum over ranks, in place.  dtype: 0 float, 1 double, 2 bf16.  On a stream that is being captured the call
 * records a marker kernel instead; a launch plan made of that capture (leod_plan_create) issues the all-reduce at that position of every
 * replay -- a hipGraph launched as such would NOT. */
int leod_comm_allreduce(void* buf, long count, int dtype, leod_stream_t stream);
int leod_comm_destroy(void);
const char* leod_comm_last_error(void);

/* ---- host-side C++ of the path (no GPU involved) ------------------------------------------------------------------
 * Tracking post-filter of the pseudo-label loop: linear-velocity tracklets, confidence-ordered greedy IoU association,
 * short-tracklet removal and in-painting of missed detections.  Replaces modules/tracking/linear.py:10-292,
 * modules/tracking/utils.py:7-96 and EventSeqData._track (modules/pseudo_labeler.py:201-258).
 * boxes [N,5] float32 (cx,cy,w,h,class) of the labelled frames concatenated in frame order; is_gt [N] (uint8);
 * frame_idx [F] strictly increasing; counts [F] boxes per labelled frame.  remove [N] (uint8) out: 1 = box on a finished
 * non-GT tracklet with fewer than min_track_len hits.  inpaint != 0: predicted boxes of the kept tracklets at their
 * missed frames -> inp_frame [inp_cap], inp_box [inp_cap,5], *n_inp (needed count; rc -3 if inp_cap is too small). */
int leod_track_filter(const float* boxes, const unsigned char* is_gt, const int* frame_idx, const int* counts, int F,
                      int img_h, int img_w, int min_track_len, double min_conf, double iou_threshold, double q,
                      unsigned char* remove, int inpaint, int* inp_frame, float* inp_box, int inp_cap, int* n_inp);

/* Detection evaluation of the validation / test loop: the COCO bbox protocol the reference delegates to pycocotools'
 * COCOeval / detectron2's COCOeval_opt (utils/evaluation/prophesee/metrics/coco_eval.py:121-139) over the image windows
 * built by the +-50 ms time matching (coco_eval.py:49-97).  gt_box [G,4] / dt_box [D,4] = (x,y,w,h) float32 rows of all
 * images concatenated, gt_off / dt_off [n_img+1] first row of every image, *_cls class ids in [0,n_cat), dt_score the
 * class confidences.  iou_thrs [T], rec_thrs [R] as np.linspace gives them.  Out: precision [T,R,n_cat,4,3] and recall
 * [T,n_cat,4,3] (area ranges all/small/medium/large, maxDets 1/10/100), -1 where COCOeval leaves them undefined. */
int leod_coco_eval(const float* gt_box, const int* gt_cls, const int* gt_off, const float* dt_box, const int* dt_cls,
                   const float* dt_score, const int* dt_off, int n_img, int n_cat, const double* iou_thrs, int T,
                   const double* rec_thrs, int R, double* precision, double* recall);

#ifdef __cplusplus
}
#endif
#endif /* LEOD_HIP_H */
