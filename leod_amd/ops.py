"""Thin tensor-level wrappers over the C ABI (include/leod_hip.h).

PyTorch is used here only as plumbing: device memory (``torch.empty``), the current HIP stream and
shape bookkeeping.  All arithmetic happens in libleod_hip.so; there is no fallback path -- every
function raises if its input is not a contiguous fp32 CUDA(HIP) tensor or the library is missing.

Convention: activations are channels-last.  2-D ``[M, C]`` "rows" and 4-D ``[B, H, W, C]`` maps are the
same memory.
"""
from typing import NamedTuple, Optional, Sequence, Tuple

import ctypes

import torch

from ._lib import lib, check, LeodHipError, DevPtr

F32 = torch.float32
UNSUPPORTED = -3            # what a ``*_route`` query answers where its entry point does not cover the problem (LEOD_ERR_UNSUPPORTED)


_LIB = None


def _l():
    """cached CDLL handle (attribute lookups on a CDLL are cached by ctypes after the first use)"""
    global _LIB
    if _LIB is None:
        _LIB = lib()
    return _LIB


try:
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:                                        # pragma: no cover
    _raw_stream = None


PRECISIONS = {'f32': 0, 'fp32': 0, 'float32': 0, 32: 0, '32': 0, '32-true': 0,
              'bf16': 1, 'bfloat16': 1, 'bf16-mixed': 1,
              '16f': 2, 'f16': 2, 'fp16': 2, 'float16': 2, 16: 2, '16': 2, '16-mixed': 2}
PRECISION_NAMES = {0: 'f32', 1: 'bf16', 2: '16f'}


def set_precision(mode) -> int:
    """'f32' (default): fp32 end to end, bit-tight against the fp32 oracle.
    '16f' (the reference's ``precision=16`` = fp16 autocast, train.py:236-243): the FORWARD contractions take fp16 operands (fp16 MFMA, fp32
    accumulation) and the 16-bit activations the forward pass leaves in HBM (qkv, attention output, MLP hidden) are fp16; the gradient
    contractions take bf16 operands (fp32's exponent range, so no loss scaler); statistics, softmax, residual stream, LSTM state,
    SimOTA cost, losses and optimiser in fp32.
    'bf16' (Lightning's ``bf16-mixed``): bf16 operands in both directions.
    Process-wide; returns the previous mode (0 / 1 / 2)."""
    prev = int(_l().leod_get_precision())
    check(_l().leod_set_precision(PRECISIONS[mode] if not isinstance(mode, bool) and mode in PRECISIONS else int(mode)), 'set_precision')
    return prev


def precision_from_config(training_cfg=None) -> str:
    """The mode a run asks for: ``LEOD_PRECISION`` (f32 | bf16 | 16f) if set, else the reference's ``training.precision`` key
    (config/general.yaml: 16 -> fp16 mixed precision = mode 16f; 'bf16' / 'bf16-mixed' -> bf16; 32 -> fp32)."""
    import os
    env = os.environ.get('LEOD_PRECISION')
    if env:
        return PRECISION_NAMES[PRECISIONS[env]]
    prec = None if training_cfg is None else training_cfg.get('precision', 32)
    return PRECISION_NAMES[PRECISIONS.get(str(prec).lower(), 0)]


def get_precision() -> str:
    return PRECISION_NAMES[int(_l().leod_get_precision())]


def is_16bit() -> bool:
    """One of the two mixed-precision modes ('bf16', '16f'): the 16-bit tensor layouts and kernel families are in use."""
    return int(_l().leod_get_precision()) != 0


def act16_dtype():
    """torch dtype of the 16-bit activation rows the forward pass stores (qkv, attention output): fp16 in mode 16f, else bf16.  Gradient
    rows (dqkv, du, dO, LSTM gate gradients) are bf16 in both modes; the MLP hidden pre-activation and the LSTM gates fp16 in both."""
    return torch.float16 if int(_l().leod_get_precision()) == 2 else torch.bfloat16


def _is16(t) -> bool:
    return t.dtype is torch.bfloat16 or t.dtype is torch.float16


def _stream():
    """raw hipStream_t of torch's current stream (the stream every kernel of this library is enqueued on)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


_KIND = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16', torch.float64: 'f64', torch.int32: 'i32', torch.int64: 'i64',
         torch.uint8: 'u8', torch.bool: 'bool', torch.int8: 'i8'}


def _p(t: Optional[torch.Tensor]):
    """device address + element kind: the typed pointer parameters of the binding (``_lib.DevPtr``) refuse a mismatching tensor"""
    return None if t is None else DevPtr(t.data_ptr(), _KIND.get(t.dtype, 'void'))


def _ck(t: Optional[torch.Tensor], dtype=F32, name='tensor'):
    """Loud input validation: device tensor, expected dtype, contiguous.  No fallback of any kind."""
    if t is None:
        return
    if t.dtype is not dtype or not t.is_cuda or not t.is_contiguous():
        if not t.is_cuda:
            raise LeodHipError(f'{name}: the LEOD HIP path needs device tensors (got {t.device}); there is no CPU fallback')
        if t.dtype != dtype:
            raise LeodHipError(f'{name}: expected {dtype}, got {t.dtype}')
        raise LeodHipError(f'{name}: expected a contiguous tensor, got strides {t.stride()}')


def _ck_dtype_dev(t: torch.Tensor, dtype=F32, name='tensor'):
    """``_ck`` without the contiguity requirement (for operands a kernel reads with an explicit row stride)."""
    if not t.is_cuda:
        raise LeodHipError(f'{name}: the LEOD HIP path needs device tensors (got {t.device}); there is no CPU fallback')
    if t.dtype != dtype:
        raise LeodHipError(f'{name}: expected {dtype}, got {t.dtype}')


def _empty(shape, like: torch.Tensor, dtype=F32):
    return torch.empty(shape, dtype=dtype, device=like.device)


# ---------------------------------------------------------------------------------------------------
# backbone pieces
# ---------------------------------------------------------------------------------------------------
def ln_linear_fwd(x, ln_w, ln_b, W, bias, want_act=False, want_stats=False, eps=1e-5, out_bf16=False):
    """x [.., K] -> out [.., N] = LN(x) W^T + b ; optional gelu(out), LN stats [M,2].
    With want_act in precision mode bf16 and a shape the row-streaming kernel covers (RVT stages 1-2) the result is
    (u as torch.float16, None, stats): pass that u to linear_lsres_fwd / linear_dgrad(aux_u=) / linear_wgrad(x=), which apply GELU."""
    for t, n in ((x, 'x'), (ln_w, 'ln_w'), (ln_b, 'ln_b'), (W, 'W'), (bias, 'bias')):
        _ck(t, name=n)
    K = x.shape[-1]
    N = W.shape[0]
    M = x.numel() // K
    ev = _probe('linear_gemm', 0, 0) if _PROBE is not None else None
    try:
        return _ln_linear_fwd(x, ln_w, ln_b, W, bias, want_act, want_stats, eps, out_bf16, K, N, M, ev)
    finally:
        if ev is not None:
            ev.record()


def _ln_linear_fwd(x, ln_w, ln_b, W, bias, want_act, want_stats, eps, out_bf16, K, N, M, ev):
    def tally(out_bytes_per_el, n_out=1):
        # algorithmic bytes: x once, W once, the output(s) at their stored width; 2 M N K flops
        if ev is not None:
            _PROBE.amend('linear_gemm', 4.0 * M * K + 4.0 * N * K + out_bytes_per_el * n_out * M * N, 2.0 * M * N * K,
                         2.0 * M * K + 4.0 * N * K + 2.0 * n_out * M * N)
    if out_bf16 and not want_act and linear_route(3, M, N, K, flags=3 if ln_w is not None else 0) != UNSUPPORTED:
        # the qkv rows in the 16-bit precision modes (consumed only by 16-bit MFMAs): stored in 16 bits where the kernels allow
        o16 = torch.empty(x.shape[:-1] + (N,), dtype=act16_dtype(), device=x.device)
        stats = _empty((M, 2), x) if ln_w is not None else None
        check(_l().leod_ln_linear_bf16_fwd(_p(x), _p(ln_w), _p(ln_b), eps, _p(W), _p(bias), _p(o16), _p(stats), M, N, K, _stream()),
              'ln_linear_bf16_fwd')
        tally(2.0)
        return o16, None, stats
    if want_act and want_stats and ln_w is not None and linear_route(2, M, N, K, flags=3) != UNSUPPORTED:
        # 16-bit precision modes: the hidden pre-activation is stored once, as fp16 (the reference's autocast dtype); consumers apply GELU on load
        u16 = torch.empty(x.shape[:-1] + (N,), dtype=torch.float16, device=x.device)
        stats = _empty((M, 2), x)
        check(_l().leod_ln_linear_gelu16_fwd(_p(x), _p(ln_w), _p(ln_b), eps, _p(W), _p(bias), _p(u16), _p(stats), M, N, K, _stream()),
              'ln_linear_gelu16_fwd')
        tally(2.0)
        return u16, None, stats
    out = _empty(x.shape[:-1] + (N,), x)
    act = _empty(out.shape, x) if want_act else None
    # always hand the kernel a statistics buffer: the LDS-staged GEMM reads precomputed (mean, rstd) from it
    stats = _empty((M, 2), x) if ln_w is not None else None
    check(_l().leod_ln_linear_fwd(_p(x), K, _p(ln_w), _p(ln_b), eps, _p(W), _p(bias), _p(out), _p(act), _p(stats),
                                   M, N, K, _stream()), 'ln_linear_fwd')
    tally(4.0, 2 if want_act else 1)
    return out, act, stats


def linear_lsres_fwd(a, W, bias, gamma, res, want_t=True, a_gelu=None):
    """out = res + gamma * (a W^T + b); also returns t = a W^T + b when want_t.
    a_gelu: ``a`` is the fp16 PRE-activation of the MLP hidden (the kernel applies GELU on load).  None: decided by the dtype as before
    mode 16f existed -- torch.float16 means pre-activation; callers that hand over plain fp16 rows (the attention output of mode 16f)
    say a_gelu=False."""
    for t, n in ((W, 'W'), (bias, 'bias'), (gamma, 'gamma'), (res, 'res')):
        _ck(t, name=n)
    K = a.shape[-1]
    N = W.shape[0]
    M = a.numel() // K
    # algorithmic bytes: a once (stored width), W, residual in, output out
    ev = _probe('linear_gemm', a.element_size() * M * K + 4.0 * N * K + (12.0 if want_t else 8.0) * M * N, 2.0 * M * N * K)
    try:
        return _linear_lsres_fwd(a, W, bias, gamma, res, want_t, K, N, M, a_gelu)
    finally:
        if ev is not None:
            ev.record()


def _linear_lsres_fwd(a, W, bias, gamma, res, want_t, K, N, M, a_gelu=None):
    if a.dtype is torch.float16 and a_gelu is not False:     # a = fp16 pre-activation: out = res + gamma * (gelu(a) W^T + b)
        _ck(a, torch.float16, 'a')
        if want_t:
            raise LeodHipError('linear_lsres_fwd: the fp16 pre-activation path does not return t')
        out = _empty(res.shape, res)
        check(_l().leod_linear_lsres_gelu16_fwd(_p(a), _p(W), _p(bias), _p(gamma), _p(res), _p(out), M, N, K, _stream()),
              'linear_lsres_gelu16_fwd')
        return out, None
    if _is16(a):                                             # a = 16-bit rows (the attention output: bf16, or fp16 in mode 16f)
        _ck(a, act16_dtype(), 'a')
        if want_t:
            raise LeodHipError('linear_lsres_fwd: the 16-bit-row path does not return t')
        out = _empty(res.shape, res)
        check(_l().leod_linear_lsres_bf16_fwd(_p(a), _p(W), _p(bias), _p(gamma), _p(res), _p(out), M, N, K, _stream()),
              'linear_lsres_bf16_fwd')
        return out, None
    _ck(a, name='a')
    out = _empty(res.shape, a)
    tout = _empty(res.shape, a) if want_t else None
    check(_l().leod_linear_lsres_fwd(_p(a), _p(W), _p(bias), _p(gamma), _p(res), _p(out), _p(tout), M, N, K,
                                      _stream()), 'linear_lsres_fwd')
    return out, tout


def mlp_fwd_fused(y, ln_w, ln_b, W1, b1, W2, b2, gamma, want_saved=False, eps=1e-5):
    """z = y + gamma * (gelu(LN(y) W1^T + b1) W2^T + b2) in ONE launch (csrc/k_mlp.hip) -> (z, u16 | None, stats | None), or None where
    the fused kernel does not cover the shape / precision mode (the caller then runs ln_linear_fwd + linear_lsres_fwd)."""
    K = y.shape[-1]
    H = W1.shape[0]
    M = y.numel() // K
    if mlp_fused_route(0, M, H, K) == UNSUPPORTED:
        return None
    for t, n in ((y, 'y'), (ln_w, 'ln_w'), (ln_b, 'ln_b'), (W1, 'W1'), (b1, 'b1'), (W2, 'W2'), (b2, 'b2'), (gamma, 'gamma')):
        _ck(t, name=n)
    out = _empty(y.shape, y)
    u16 = torch.empty(y.shape[:-1] + (H,), dtype=torch.float16, device=y.device) if want_saved else None
    stats = _empty((M, 2), y) if want_saved else None
    ev = _probe('linear_gemm', 8.0 * M * K + 4.0 * 2 * H * K + (2.0 * M * H if want_saved else 0.0), 4.0 * M * H * K)
    rc = _l().leod_mlp_fwd_fused(_p(y), _p(ln_w), _p(ln_b), eps, _p(W1), _p(b1), _p(W2), _p(b2), _p(gamma), _p(out), _p(u16), _p(stats),
                                 M, H, K, _stream())
    if ev is not None:
        ev.record()
    check(rc, 'mlp_fwd_fused')
    return out, u16, stats


def mlp_bwd_dgrad_fused(dz, y, stats, ln_w, ln_b, W1, b1, W2, gamma, dgamma, dbeta, want_du=True):
    """The activation-path backward of the fused MLP in ONE launch (csrc/k_mlp.hip) -> (dy, du bf16 | None), or None where it does not
    apply (the caller then runs linear_dgrad(aux_u=) + linear_dgrad_ln_bwd).  dgamma / dbeta accumulate norm2's gradients."""
    K = y.shape[-1]
    H = W1.shape[0]
    M = y.numel() // K
    if not BF16_GRADS or mlp_fused_route(1, M, H, K) == UNSUPPORTED:
        return None
    for t, n in ((dz, 'dz'), (y, 'y'), (stats, 'stats'), (ln_w, 'ln_w'), (ln_b, 'ln_b'), (W1, 'W1'), (b1, 'b1'), (W2, 'W2'),
                 (gamma, 'gamma'), (dgamma, 'dgamma'), (dbeta, 'dbeta')):
        _ck(t, name=n)
    dy = _empty(y.shape, y)
    du = torch.empty(y.shape[:-1] + (H,), dtype=torch.bfloat16, device=y.device) if want_du else None
    ev = _probe('linear_gemm', 12.0 * M * K + 4.0 * 2 * H * K + (2.0 * M * H if want_du else 0.0), 8.0 * M * H * K)
    rc = _l().leod_mlp_bwd_dgrad_fused(_p(dz), _p(y), _p(stats), _p(ln_w), _p(ln_b), _p(W1), _p(b1), _p(W2), _p(gamma), _p(dy), _p(du),
                                       _p(dgamma), _p(dbeta), M, H, K, _stream())
    if ev is not None:
        ev.record()
    check(rc, 'mlp_bwd_dgrad_fused')
    return dy, du


def partition_attn_fwd(qkv, heads, part, window, want_lse=False, out_bf16=False):
    """qkv [B,H,W,3C] -> out [B,H,W,C] (+ lse [B,H,W,heads]); out_bf16 (attn_block_o16_ok): out as bf16 rows."""
    q16 = _is16(qkv)
    _ck(qkv, act16_dtype() if q16 else F32, 'qkv')
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    out = torch.empty((B, H, W, C), dtype=act16_dtype() if out_bf16 else F32, device=qkv.device)
    lse = torch.empty((B, H, W, heads), dtype=F32, device=qkv.device) if want_lse else None
    check(_l().leod_partition_attn_fwd(_p(qkv), _p(out), _p(lse), B, H, W, C, heads, part[0], part[1],
                                        1 if window else 0, (1 if q16 else 0) | (2 if out_bf16 else 0), _stream()), 'partition_attn_fwd')
    return out, lse


def attn_block_o16_ok(B, H, W, C, heads, part) -> bool:
    """The attention output O and its gradient dO of this block geometry may live in HBM as bf16 rows (every consumer has a 16-bit path)."""
    return BF16_GRADS and bool(_l().leod_attn_block_o16_ok(B, H, W, C, heads, part[0], part[1]))


def partition_attn_16bit_ok(B, H, W, C, heads, part) -> bool:
    """qkv may be handed to partition_attn_fwd / _bwd as torch.bfloat16 (and dqkv comes back as bfloat16) for this geometry."""
    return BF16_GRADS and bool(_l().leod_partition_attn_16bit_ok(B, H, W, C, heads, part[0], part[1]))


def partition_attn_route(entry, B, H, W, C, heads, part, flags=0) -> int:
    """The kernels ``partition_attn_fwd`` (entry 0) / ``partition_attn_bwd`` (entry 1) run for this geometry in the current precision mode, or
    the negative error code they return (``leod_partition_attn_route`` in include/leod_hip.h lists the flags and the codes; nothing is launched).
    flags: 1 qkv is 16-bit, 2 out / dout is 16-bit, 4 dqkv comes back as bfloat16.  A query for tests and tools, not for the step path."""
    return int(_l().leod_partition_attn_route(entry, B, H, W, C, heads, part[0], part[1], flags))


ATTN_BLOCK_FUSED = True     # the attention half of a block in one launch where attn_block_fwd_route says so; False: always the three launches
ABF_LN_AFFINE, ABF_NO_NORM = 1, 2   # flags of ``attn_block_fwd_route`` (include/leod_hip.h): norm1 is a LayerNorm with weight and bias | the identity


def attn_block_fwd_route(B, H, W, C, heads, part, flags=ABF_LN_AFFINE) -> int:
    """Whether an attention block of this geometry runs ``attn_block_fwd`` in the current precision mode: a positive route code, or the
    negative error code that sends it to its three launches (``leod_attn_block_fwd_route``; nothing is launched; the step path: ``attn_block_routes``)."""
    return int(_l().leod_attn_block_fwd_route(B, H, W, C, heads, part[0], part[1], flags)) if BF16_GRADS else UNSUPPORTED


MLP_FUSED, MLP_PAIR16, MLP_PAIR32 = 'fused', 'pair16', 'pair32'


class BlockRoutes(NamedTuple):
    """What a MaxViT block of one geometry launches in one precision mode: every decision of ``functions.AttnBlockFn`` (``attn_block_routes``)."""
    attn: int               # code of ``attn_block_fwd`` where the attention half is ONE launch (ATTN_BLOCK_FUSED is read by the caller), else <= 0:
    q16: bool               # ... ln_linear_fwd + partition_attn_fwd + linear_lsres_fwd, qkv / dqkv rows in 16 bits
    o16: bool               # ... and O / dO rows (a one-launch block leaves the same tensors behind)
    mlp_fwd: str            # MLP_FUSED: mlp_fwd_fused | MLP_PAIR16: fp16 pre-activation (Linear entries 2 + 5) | MLP_PAIR32: fp32 pair (entries 0 + 1)
    mlp_bwd_fused: bool     # mlp_bwd_dgrad_fused, else linear_dgrad + linear_dgrad_ln_bwd
    ln2_fused: bool         # norm2's input gradient: dgrad + LayerNorm backward in one launch (Linear entry 7), else two calls
    ln1_fused: bool         # norm1's
    wgrads_grouped: bool    # the four weight gradients in one grouped launch (attn_block_wgrads), else singly

    @property
    def u16(self) -> bool:  # the MLP hidden is kept as ONE fp16 pre-activation; its consumers apply GELU on load
        return self.mlp_fwd != MLP_PAIR32


_BLOCK_ROUTES = {}


def attn_block_routes(B, H, W, C, heads, part, hidden, norm1=ABF_LN_AFFINE) -> BlockRoutes:
    """The routes of a block on the map [B,H,W,C] with an MLP of ``hidden`` units; norm1 as the flags of ``attn_block_fwd_route``.
    Host state only (nothing is launched); remembered per precision mode: the step path asks on every block."""
    mode = int(_l().leod_get_precision())
    key = (mode, BF16_GRADS, B, H, W, C, heads, part[0], part[1], hidden, norm1)
    r = _BLOCK_ROUTES.get(key)
    if r is None:
        if len(_BLOCK_ROUTES) > 4096:
            _BLOCK_ROUTES.clear()
        M, geom, ln1 = B * H * W, (B, H, W, C, heads, part), norm1 != ABF_NO_NORM
        q16 = partition_attn_16bit_ok(*geom)
        o16 = q16 and attn_block_o16_ok(*geom)
        q16 = q16 and linear_route(3, M, 3 * C, C, flags=3 if ln1 else 0) != UNSUPPORTED
        mlp_fwd = (MLP_FUSED if mlp_fused_route(0, M, hidden, C) > 0 else
                   MLP_PAIR16 if linear_route(2, M, hidden, C, flags=3) != UNSUPPORTED else MLP_PAIR32)
        u16 = mlp_fwd != MLP_PAIR32; du16 = u16 and BF16_GRADS                             # du leaves the dgrad through GELU' as bf16 rows
        r = BlockRoutes(attn_block_fwd_route(*geom, flags=norm1), q16, o16, mlp_fwd,
                        BF16_GRADS and mlp_fused_route(1, M, hidden, C) > 0,
                        linear_route(7, M, hidden, C, a16=int(du16), flags=2 | 256) > 0,
                        ln1 and linear_route(7, M, 3 * C, C, a16=int(q16), flags=2 | 256) > 0,
                        linear_wgrad_group_route(M, (C, hidden, C, 3 * C), (hidden, C, C, C), (0, int(du16), 0, int(q16)),      # fc2, fc1, proj, qkv
                                                 (2 if u16 else 0, 1, (4 if mode == 2 else 3) if o16 else 0, int(ln1))) > 0)     # as attn_block_wgrads
        _BLOCK_ROUTES[key] = r
    return r


def attn_block_fwd(x, ln_w, ln_b, qkv_w, qkv_b, proj_w, proj_b, gamma, heads, part, window, want_saved=False, eps=1e-5):
    """y = x + gamma * proj(attention(qkv(LN(x)))) on the partitions of the map x [B,H,W,C] in ONE launch (csrc/k_attn_block.hip)
    -> (y, qkv, stats, o, lse); the last four are what ln_linear_fwd / partition_attn_fwd leave for the backward pass (16-bit qkv and O
    rows of the precision mode; stats is None when ln_w and ln_b are None: norm1 is the identity) when want_saved, else None.  Raises where the kernel does not cover the geometry: ask
    ``attn_block_fwd_route`` first."""
    for t, n in ((x, 'x'), (ln_w, 'ln_w'), (ln_b, 'ln_b'), (qkv_w, 'qkv_w'), (qkv_b, 'qkv_b'), (proj_w, 'proj_w'), (proj_b, 'proj_b'),
                 (gamma, 'gamma')):
        _ck(t, name=n)
    B, H, W, C = x.shape
    M = B * H * W
    y = _empty(x.shape, x)
    qkv = o = lse = stats = None
    if want_saved:
        qkv = torch.empty((B, H, W, 3 * C), dtype=act16_dtype(), device=x.device)
        o = torch.empty((B, H, W, C), dtype=act16_dtype(), device=x.device)
        lse = _empty((B, H, W, heads), x)
        stats = _empty((M, 2), x) if ln_w is not None else None
    check(_l().leod_attn_block_fwd(_p(x), _p(ln_w), _p(ln_b), eps, _p(qkv_w), _p(qkv_b), _p(proj_w), _p(proj_b), _p(gamma), _p(y),
                                   _p(qkv), _p(o), _p(lse), _p(stats), B, H, W, C, heads, part[0], part[1], 1 if window else 0, _stream()),
          'attn_block_fwd')
    return y, qkv, stats, o, lse


def partition_attn_bwd(qkv, dout, lse, heads, part, window):
    q16 = _is16(qkv)
    _ck(qkv, act16_dtype() if q16 else F32, 'qkv')
    do16 = dout.dtype is torch.bfloat16                       # bf16 dO rows (attn_block_o16_ok)
    _ck(dout, torch.bfloat16 if do16 else F32, 'dout')
    _ck(lse, name='lse')
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    dqkv = torch.empty(qkv.shape, dtype=torch.bfloat16 if q16 else F32, device=qkv.device)     # 16-bit qkv <=> bf16 dqkv (partition_attn_16bit_ok)
    dsum = torch.empty(lse.shape, dtype=F32, device=qkv.device)
    check(_l().leod_partition_attn_bwd(_p(qkv), _p(dout), _p(lse), _p(dsum), _p(dqkv), B, H, W, C, heads, part[0],
                                        part[1], 1 if window else 0, (1 if q16 else 0) | (2 if do16 else 0), 1 if q16 else 0, _stream()), 'partition_attn_bwd')
    return dqkv


def convlstm_fwd(x, h_prev, c_prev, W, bias, want_gates=False, h_out=None, c_out=None, gates_out=None):
    """x/h_prev/c_prev [..,C] channels-last rows; W [4C,2C]; -> h, c, gates[M,4,C] (optionally into given buffers)."""
    for t, n in ((x, 'x'), (h_prev, 'h_prev'), (c_prev, 'c_prev'), (W, 'W'), (bias, 'bias'), (h_out, 'h_out'),
                 (c_out, 'c_out'), (gates_out, 'gates_out')):
        _ck(t, name=n)
    C = x.shape[-1]
    M = x.numel() // C
    h = _empty(x.shape, x) if h_out is None else h_out
    c = _empty(x.shape, x) if c_out is None else c_out
    gates = gates_out if gates_out is not None else (_empty((M, 4, C), x) if want_gates else None)
    check(_l().leod_convlstm_fwd(_p(x), _p(h_prev), _p(c_prev), _p(W), _p(bias), _p(h), _p(c), _p(gates), M, C,
                                  _stream()), 'convlstm_fwd')
    return h, c, gates


def convlstm_gates_bwd(dh, dc_next, gates, c_prev, c_t, want_dc_prev=True, dh2=None, dgates_out=None):
    for t, n in ((dh, 'dh'), (dc_next, 'dc_next'), (gates, 'gates'), (c_prev, 'c_prev'), (c_t, 'c_t'), (dh2, 'dh2'),
                 (dgates_out, 'dgates_out')):
        _ck(t, name=n)
    M, _, C = gates.shape
    dgates = _empty((M, 4 * C), gates) if dgates_out is None else dgates_out
    dc_prev = _empty(c_t.shape, gates) if want_dc_prev else None
    check(_l().leod_convlstm_gates_bwd(_p(dh), _p(dh2), _p(dc_next), _p(gates), _p(c_prev), _p(c_t), _p(dgates), _p(dc_prev),
                                        M, C, _stream()), 'convlstm_gates_bwd')
    return dgates, dc_prev


def convlstm_seq_mode(C: int) -> int:
    """0: no sequence kernel for this channel count / precision mode; 1: fused [x | h] contraction (xin = x_seq);
    2: the caller supplies the time-batched projection gx = x W_x^T + b; 3: as 2, and the kernels stream their weights from the
    ``convlstm_seq_pack`` buffer (leod_convlstm_seq_mode)."""
    return int(_l().leod_convlstm_seq_mode(int(C)))


def convlstm_seq_route(entry, C: int, flags=0) -> int:
    """The kernel ``convlstm_seq_fwd`` (entry 0) / ``convlstm_seq_bwd`` (entry 1) run for this channel count in the current precision mode, or
    the negative error code they return (``leod_convlstm_seq_route`` in include/leod_hip.h lists the codes; nothing is launched).
    flags: 1 xin is the hoisted projection, 2 fp16 gates, 4 a wpack is given.  A query for tests and tools, not for the step path."""
    return int(_l().leod_convlstm_seq_route(entry, int(C), flags))


def convlstm_seq_pack(W, C: int):
    """Mode 3 only: the fragment-ordered bf16 copy of W_h the sequence kernels stream (valid until the weights change) | None."""
    n = int(_l().leod_convlstm_seq_pack_bytes(int(C)))
    if n == 0:
        return None
    _ck(W, name='W')
    # a persistent buffer of the pack cache (never a temporary of the calling step: the launch plans run weight packs ahead of the captured
    # order, which is only sound for buffers no other kernel of the step ever writes), re-packed once per optimiser step
    buf, valid = PackCache.get(W, ('lstm', int(C)), (n + 3) // 4)
    wp = buf.view(torch.uint8)[:n]
    if not valid:
        check(_l().leod_convlstm_seq_pack(_p(W), _p(wp), int(C), _stream()), 'convlstm_seq_pack')
    return wp


def convlstm_gates16_ok(C: int) -> bool:
    """Precision mode bf16: the sequence kernels keep the gates as fp16 (their own layout) and emit bf16 gate-gradient rows."""
    return bool(_l().leod_convlstm_seq_gates16_ok(int(C)))


def convlstm_gates16_buffer(T: int, M: int, C: int, device):
    """fp16 gate storage for convlstm_seq_fwd / _bwd (opaque layout: only those two calls read it)."""
    return torch.empty((T, (M + 15) // 16 * 16, 4, C), dtype=torch.float16, device=device)


def convlstm_seq_fwd(xin, is_projection, hbuf, cbuf, W, bias, gates_out, zero_state, wpack=None):
    """The whole recurrence in one launch: xin [T,M,C] (or gx [T,M,4C]), hbuf / cbuf [T+1,M,C] (slot 0 = incoming state,
    slots 1.. written), W [4C,2C], gates_out [T,M,4,C] fp32 | convlstm_gates16_buffer(...) | None."""
    g16 = gates_out is not None and gates_out.dtype is torch.float16
    for t, n in ((xin, 'xin'), (hbuf, 'hbuf'), (cbuf, 'cbuf'), (W, 'W'), (bias, 'bias')):
        _ck(t, name=n)
    _ck(gates_out, torch.float16 if g16 else F32, 'gates_out')
    T = hbuf.shape[0] - 1
    C = hbuf.shape[-1]
    M = hbuf[0].numel() // C
    check(_l().leod_convlstm_seq_fwd(_p(xin), 1 if is_projection else 0, _p(hbuf), _p(cbuf), _p(W), _p(bias), _p(gates_out), _p(wpack),
                                      M, C, T, 1 if zero_state else 0, 1 if g16 else 0, _stream()), 'convlstm_seq_fwd')


def convlstm_seq_bwd(dh_seq, dc_last, gates, cbuf, W, dgates_out, dh0=None, dc0=None, zero_state=False, wpack=None) -> bool:
    """Backward through time in one launch -> dgates_out [T,M,4C] (+ dh0, dc0).  False: the weight slice does not fit the registers
    for this C / precision mode (the caller then runs the per-timestep kernels on the same saved tensors)."""
    g16 = gates.dtype is torch.float16
    for t, n in ((dh_seq, 'dh_seq'), (dc_last, 'dc_last'), (cbuf, 'cbuf'), (W, 'W'), (dh0, 'dh0'), (dc0, 'dc0')):
        _ck(t, name=n)
    _ck(gates, torch.float16 if g16 else F32, 'gates')
    _ck(dgates_out, torch.bfloat16 if g16 else F32, 'dgates_out')
    T = cbuf.shape[0] - 1
    C = cbuf.shape[-1]
    M = cbuf[0].numel() // C
    rc = _l().leod_convlstm_seq_bwd(_p(dh_seq), _p(dc_last), _p(gates), _p(cbuf), _p(W), _p(dgates_out), _p(dh0), _p(dc0), _p(wpack),
                                    M, C, T, 1 if zero_state else 0, 1 if g16 else 0, _stream())
    if rc == -3:
        return False
    check(rc, 'convlstm_seq_bwd')
    return True


def linear_dgrad(dy, W, kscale=None, aux_u=None, colsum=None, out=None, accumulate=False, split=0, out2=None, dres=None, out_bf16=False):
    """dx = (dy * kscale) @ W  with W [N,K] (+ dres: the other gradient source of a residual branch); see leod_linear_dgrad."""
    dy16 = dy.dtype is torch.bfloat16                         # bf16 gradient rows (du / dqkv of precision mode bf16)
    _ck(dy, torch.bfloat16 if dy16 else F32, 'dy')
    for t, n in ((W, 'W'), (kscale, 'kscale'), (colsum, 'colsum'), (out, 'out'), (out2, 'out2'), (dres, 'dres')):
        _ck(t, name=n)
    N, K = W.shape[0], W.shape[1] if W.dim() == 2 else W.numel() // W.shape[0]
    M = dy.numel() // N
    aux_b = 0.0 if aux_u is None else aux_u.element_size() * M * K
    out_b = (2.0 if (out_bf16 or (aux_u is not None and aux_u.dtype is torch.float16 and BF16_GRADS)) else 4.0) * M * K
    ev = _probe('linear_gemm', dy.element_size() * M * N + 4.0 * N * K + aux_b + out_b + (4.0 * M * K if (accumulate or dres is not None) else 0.0),
                2.0 * M * N * K)
    try:
        return _linear_dgrad(dy, W, kscale, aux_u, colsum, out, accumulate, split, out2, dres, dy16, N, K, M, out_bf16)
    finally:
        if ev is not None:
            ev.record()


def _linear_dgrad(dy, W, kscale, aux_u, colsum, out, accumulate, split, out2, dres, dy16, N, K, M, out_bf16=False):
    if aux_u is not None and aux_u.dtype is torch.float16:    # through GELU on the fp16 pre-activation (stages 1-2, bf16 mode)
        _ck(aux_u, torch.float16, 'aux_u')
        if split or colsum is not None or accumulate or out is not None or dres is not None:
            raise LeodHipError('linear_dgrad: unsupported option with an fp16 pre-activation')
        if dy16:
            raise LeodHipError('linear_dgrad: bf16 dy does not combine with an fp16 pre-activation')
        # the gradient of the hidden goes out as bf16: its two consumers (dgrad of fc1, fc1 weight gradient) feed bf16 MFMAs
        out = torch.empty(dy.shape[:-1] + (K,), dtype=torch.bfloat16 if BF16_GRADS else F32, device=dy.device)
        check(_l().leod_linear_dgrad_gelu16(_p(dy), _p(kscale), _p(W), _p(aux_u), _p(out), M, N, K, 1 if BF16_GRADS else 0, _stream()),
              'linear_dgrad_gelu16')
        return out
    _ck(aux_u, name='aux_u')
    if split:
        if out is None:
            out = torch.empty(dy.shape[:-1] + (split,), dtype=F32, device=dy.device)
        if out2 is None:
            out2 = torch.empty(dy.shape[:-1] + (K - split,), dtype=F32, device=dy.device)
        ld1, ld2 = split, K - split
    else:
        if out is None:
            out = torch.empty(dy.shape[:-1] + (K,), dtype=torch.bfloat16 if out_bf16 else F32, device=dy.device)
        ld1, ld2 = K, 0
    check(_l().leod_linear_dgrad(_p(dy), N, _p(kscale), _p(W), _p(out), ld1, _p(out2), ld2, split, _p(aux_u),
                                  _p(colsum), 1 if accumulate else 0, _p(dres), M, N, K, 1 if dy16 else 0, 1 if out_bf16 else 0, _stream()),
          'linear_dgrad')
    return (out, out2) if split else out


_WORKSPACES = {}     # raw stream -> uint8 tensor registered as that stream's weight-gradient workspace (kept alive here)


def _wgrad_workspace(device):
    """The partial-tile scratch of the wide weight-gradient kernel (wgrad_bf16.hpp), one per stream, from torch's allocator -- which also
    serves a stream under graph capture, where the library could not allocate for itself."""
    s = _stream()
    if s not in _WORKSPACES:
        ws = torch.empty(int(_l().leod_workspace_bytes()), dtype=torch.uint8, device=device)
        check(_l().leod_set_workspace(ws.data_ptr(), ws.numel(), s), 'set_workspace')
        _WORKSPACES[s] = ws


def _x_fmt(x, stats, gelu):
    """x_fmt of leod_linear_wgrad / leod_linear_wgrad_group."""
    if gelu:
        return 2
    if x.dtype is torch.bfloat16:
        return 3
    if x.dtype is torch.float16:
        return 4
    return 1 if stats is not None else 0


def _wgrad_work(M, N, K, dy16, x16):
    """(nbytes, flops, nbytes16) of one weight gradient for the probe: the algorithmic work of one launch -- reads dy and X once,
    read-modify-writes dW once, 2*M*N*K flops; nbytes16: the same with both operands in 16 bits."""
    return ((2.0 if dy16 else 4.0) * M * N + (2.0 if x16 else 4.0) * M * K + 4.0 * N * K, 2.0 * M * N * K,
            2.0 * M * (N + K) + 4.0 * N * K)


def linear_wgrad(dy, x, dW, dbias=None, stats=None, ln_w=None, ln_b=None, x2=None, x_gelu=None):
    """dW += dy^T X ; dbias += colsum(dy).  X = x | LN(x) | [x|x2] | gelu(x) (x the fp16 pre-activation; x_gelu as in linear_lsres_fwd)."""
    dy16 = dy.dtype is torch.bfloat16
    _ck(dy, torch.bfloat16 if dy16 else F32, 'dy')
    for t, n in ((dW, 'dW'), (dbias, 'dbias'), (stats, 'stats'), (ln_w, 'ln_w'), (ln_b, 'ln_b'), (x2, 'x2')):
        _ck(t, name=n)
    N = dW.shape[0]
    K = dW.numel() // N
    M = dy.numel() // N
    K1 = x.shape[-1]
    if M >= 8192 and _stream() not in _WORKSPACES and is_16bit():
        _wgrad_workspace(dW.device)
    gelu = x.dtype is torch.float16 and x_gelu is not False   # X = gelu(x): x is the fp16 pre-activation of the MLP hidden
    if gelu and (stats is not None or x2 is not None or dy16):
        raise LeodHipError('linear_wgrad: LayerNorm / concat / bf16-dy options do not combine with an fp16 pre-activation')
    x16 = _is16(x)                                            # 16-bit rows (the attention output: bf16, or fp16 in mode 16f)
    _ck(x, x.dtype if x16 else F32, 'x')
    nb, fl, nb16 = _wgrad_work(M, N, K, dy16, x16)
    ev = _probe('linear_wgrad', nb, fl, rows=M, nbytes16=nb16)
    check(_l().leod_linear_wgrad(_p(dy), N, _p(x), K1, _p(stats), _p(ln_w), _p(ln_b), _p(x2),
                                  (x2.shape[-1] if x2 is not None else 0), K1, _p(dW), _p(dbias), M, N, K,
                                  1 if dy16 else 0, _x_fmt(x, stats, gelu), _stream()), 'linear_wgrad')
    if ev is not None:
        ev.record()


def linear_wgrad_route(M, N, K, dy_fmt=0, x_fmt=0, K1=None, lddy=None, ldx=None, ldx2=None, has_stats=None) -> int:
    """The kernel ``linear_wgrad`` runs for this problem in the current precision mode (``leod_linear_wgrad_route``; nothing is launched):
    100 + tile LDS-DMA, 200 + combination wide kernel, 300 + configuration wgradw, 400 + 10 TN + TK wgrad16, 0 nothing to do, negative
    the error code of the call.  dy_fmt / x_fmt as in ``leod_linear_wgrad``; K1 < K: X = [x | x2] with K1 columns from x; the strides
    default to dense rows (N, K1, K - K1), has_stats to ``x_fmt == 1``."""
    K1 = K if K1 is None else K1
    x2 = K1 < K
    return int(_l().leod_linear_wgrad_route(M, N, K, N if lddy is None else lddy, K1 if ldx is None else ldx,
                                            (K - K1 if ldx2 is None else ldx2) if x2 else 0, K1, dy_fmt, x_fmt,
                                            int(x_fmt == 1 if has_stats is None else has_stats), int(x2)))


def linear_route(entry, M, N, K, lda=None, ldo=None, a16=0, out16=0, flags=0, nsplit=0) -> int:
    """The kernel Linear forward / dgrad call number ``entry`` runs for this problem in the current precision mode, or the negative error
    code it returns (``leod_linear_route`` in include/leod_hip.h lists the entries, the flags and the route codes; nothing is launched).
    The strides default to dense rows."""
    dgrad = entry >= 6
    return int(_l().leod_linear_route(entry, M, N, K, (N if dgrad else K) if lda is None else lda, (K if dgrad else N) if ldo is None else ldo,
                                      a16, out16, flags, nsplit))


def mlp_fused_route(entry, M, H, K) -> int:
    """``leod_mlp_fused_route``: 7000 + 100 (K / 16) + H / 16 where ``mlp_fwd_fused`` (entry 0) / ``mlp_bwd_dgrad_fused`` (entry 1) run, else UNSUPPORTED."""
    return int(_l().leod_mlp_fused_route(entry, M, H, K))


def linear_wgrad_group_route(M, Ns, Ks, dy_fmts, x_fmts) -> int:
    """``leod_linear_wgrad_group_route``: 100 + tile where ``linear_wgrad_group`` launches for these problems, else the call's negative code."""
    return int(_l().leod_linear_wgrad_group_route(len(Ns), M, _int_array(Ns), _int_array(Ks), _int_array(dy_fmts), _int_array(x_fmts)))


def linear_wgrad_group(problems) -> bool:
    """n <= 4 Linear weight gradients of one row count in ONE preparation / contraction / reduce launch (``leod_linear_wgrad_group``).
    problems: dicts with dy, x, dW, dbias and optionally stats + ln_w + ln_b (X = LayerNorm(x)) or gelu=True (x the fp16 pre-activation).
    False: not coverable -- nothing was launched (the caller runs them singly)."""
    if not 1 <= len(problems) <= 4:
        return False
    M = problems[0]['dy'].numel() // problems[0]['dW'].shape[0]
    Ns, Ks, dyf, xf = [], [], [], []
    for p in problems:
        dy, x, dW = p['dy'], p['x'], p['dW']
        N = dW.shape[0]
        K = dW.numel() // N
        fmt = _x_fmt(x, p.get('stats'), p.get('gelu'))
        if dy.numel() // N != M or x.numel() != M * K or x.shape[-1] != K or p.get('x2') is not None or (fmt == 2 and x.dtype is not torch.float16):
            return False
        Ns.append(N); Ks.append(K); dyf.append(int(dy.dtype is torch.bfloat16)); xf.append(fmt)
    if linear_wgrad_group_route(M, Ns, Ks, dyf, xf) == UNSUPPORTED:
        return False
    _linear_wgrad_group(problems, M, Ns, Ks, dyf, xf)
    return True


def _linear_wgrad_group(problems, M, Ns, Ks, dyf, xf):
    """the launch of ``linear_wgrad_group``, for problems ``linear_wgrad_group_route`` covers"""
    nb = fl = nb16 = 0.0
    for p, N, K, dy16, fmt in zip(problems, Ns, Ks, dyf, xf):
        _ck(p['dy'], torch.bfloat16 if dy16 else F32, 'dy')
        _ck(p['x'], p['x'].dtype, 'x')
        for t_ in (p['dW'], p.get('dbias'), p.get('stats'), p.get('ln_w'), p.get('ln_b')):
            _ck(t_, name='linear_wgrad_group')
        w = _wgrad_work(M, N, K, dy16, fmt >= 2)
        nb += w[0]; fl += w[1]; nb16 += w[2]
    if _stream() not in _WORKSPACES:
        _wgrad_workspace(problems[0]['dW'].device)
    ev = _probe('linear_wgrad', nb, fl, rows=M, nbytes16=nb16)
    check(_l().leod_linear_wgrad_group(len(problems), _ptr_array([p['dy'] for p in problems]), _int_array(dyf), _ptr_array([p['x'] for p in problems]),
                                       _int_array(xf), _ptr_array([p.get('stats') for p in problems]), _ptr_array([p.get('ln_w') for p in problems]),
                                       _ptr_array([p.get('ln_b') for p in problems]), _ptr_array([p['dW'] for p in problems]),
                                       _ptr_array([p.get('dbias') for p in problems]), M, _int_array(Ns), _int_array(Ks), _stream()),
          'linear_wgrad_group')
    if ev is not None:
        ev.record()


def attn_block_wgrads(dz, h, h_gelu, du, y, st2, n2w, n2b, dy, o, dqkv, x, st1, n1w, n1b, fc2, fc1, proj, qkv) -> bool:
    """The four weight gradients of an attention block (fc2 and proj behind LayerScale, fc1 and qkv behind LayerNorm) in one grouped launch.
    fc2 / proj = (W, b, gamma, dW, db, dgamma); fc1 / qkv = (dW, db).  False: not coverable, nothing was launched."""
    W2, b2, g2, dW2, db2, dg2 = fc2
    Wp, bp, g1, dWp, dbp, dg1 = proj
    (N2, K2), (Np, Kp) = W2.shape, Wp.shape
    st1 = st1 if n1w is not None else None
    M = dz.numel() // N2
    Ns, Ks = zip(W2.shape, fc1[0].shape, Wp.shape, qkv[0].shape)
    dyf = [int(t.dtype is torch.bfloat16) for t in (dz, du, dy, dqkv)]
    xf = [_x_fmt(h, None, h_gelu), 1, _x_fmt(o, None, False), _x_fmt(x, st1, False)]
    if linear_wgrad_group_route(M, Ns, Ks, dyf, xf) == UNSUPPORTED:
        return False
    scratch = StatArena.zeros((N2 * K2 + N2 + Np * Kp + Np,), dz.device, torch.float32)
    G2, s2 = scratch[:N2 * K2].view(N2, K2), scratch[N2 * K2:N2 * K2 + N2]
    off = N2 * K2 + N2
    Gp, sp = scratch[off:off + Np * Kp].view(Np, Kp), scratch[off + Np * Kp:]
    _linear_wgrad_group([dict(dy=dz, x=h, dW=G2, dbias=s2),
                         dict(dy=du, x=y, dW=fc1[0], dbias=fc1[1], stats=st2, ln_w=n2w, ln_b=n2b),
                         dict(dy=dy, x=o, dW=Gp, dbias=sp),
                         dict(dy=dqkv, x=x, dW=qkv[0], dbias=qkv[1], stats=st1, ln_w=n1w, ln_b=n1b)], M, Ns, Ks, dyf, xf)
    check(_l().leod_layerscale_finalize(_p(W2), _p(b2), _p(g2), _p(G2), _p(s2), _p(dW2), _p(db2), _p(dg2), N2, K2, _stream()), 'layerscale_finalize')
    check(_l().leod_layerscale_finalize(_p(Wp), _p(bp), _p(g1), _p(Gp), _p(sp), _p(dWp), _p(dbp), _p(dg1), Np, Kp, _stream()), 'layerscale_finalize')
    return True


def layernorm_fwd(x, w, b, want_stats=False, eps=1e-5):
    for t, n in ((x, 'x'), (w, 'w'), (b, 'b')):
        _ck(t, name=n)
    C = x.shape[-1]
    M = x.numel() // C
    y = _empty(x.shape, x)
    stats = _empty((M, 2), x) if want_stats else None
    check(_l().leod_layernorm_fwd(_p(x), _p(w), _p(b), _p(y), _p(stats), M, C, eps, _stream()), 'layernorm_fwd')
    return y, stats


def layernorm_bwd(dn, x, stats, w, dres, dw, db, eps=1e-5):
    for t, n in ((dn, 'dn'), (x, 'x'), (stats, 'stats'), (w, 'w'), (dres, 'dres'), (dw, 'dw'), (db, 'db')):
        _ck(t, name=n)
    C = x.shape[-1]
    M = x.numel() // C
    dx = _empty(x.shape, x)
    check(_l().leod_layernorm_bwd(_p(dn), _p(x), _p(stats), _p(w), _p(dres), _p(dx), _p(dw), _p(db), M, C, eps,
                                   _stream()), 'layernorm_bwd')
    return dx


def linear_dgrad_ln_bwd(dy, W, x, stats, ln_w, dres, dw, db, eps=1e-5):
    """dx of  x -> LayerNorm -> Linear(W)  from dy: LN-backward(dy @ W) + dres; dw / db accumulate the LayerNorm weight / bias
    gradients.  One fused launch for the stage-1 shapes, leod_linear_dgrad + leod_layernorm_bwd otherwise."""
    dy16 = dy.dtype is torch.bfloat16
    _ck(dy, torch.bfloat16 if dy16 else F32, 'dy')
    for t, n in ((W, 'W'), (x, 'x'), (stats, 'stats'), (ln_w, 'ln_w'), (dres, 'dres'), (dw, 'dw'), (db, 'db')):
        _ck(t, name=n)
    N, K = W.shape
    M = dy.numel() // N
    if linear_route(7, M, N, K, a16=int(dy16), flags=2 | (256 if dres is not None else 0)) == UNSUPPORTED:   # outside the fused kernel's coverage
        return layernorm_bwd(linear_dgrad(dy, W), x, stats, ln_w, dres, dw, db, eps)
    dx = _empty(x.shape, x)
    check(_l().leod_linear_dgrad_lnbwd(_p(dy), _p(W), _p(x), _p(stats), _p(ln_w), _p(dres), _p(dx), _p(dw), _p(db), M, N, K,
                                       1 if dy16 else 0, _stream()), 'linear_dgrad_lnbwd')
    return dx


def layerscale_bwd(dz, t, gamma, dgamma):
    for tt, n in ((dz, 'dz'), (t, 't'), (gamma, 'gamma'), (dgamma, 'dgamma')):
        _ck(tt, name=n)
    C = dz.shape[-1]
    M = dz.numel() // C
    dt = _empty(dz.shape, dz)
    check(_l().leod_layerscale_bwd(_p(dz), _p(t), _p(gamma), _p(dt), _p(dgamma), M, C, _stream()), 'layerscale_bwd')
    return dt


def layerscale_linear_wgrad(dz, h, W, b, gamma, dW, db, dgamma, h_gelu=None):
    """Weight, bias and LayerScale gradients of z = res + gamma * (h W^T + b) from dz alone: the un-scaled G = dz^T h goes
    into a scratch buffer (one wgrad launch), ``leod_layerscale_finalize`` turns it into dW, db and dgamma -- the stored
    pre-scale tensor of the forward pass and the scaled copy of dz are not needed."""
    N, K = W.shape
    scratch = StatArena.zeros((N * K + N,), dz.device, torch.float32)         # one memset per step instead of 16 fill kernels
    G, s = scratch[:N * K].view(N, K), scratch[N * K:]
    linear_wgrad(dz, h, G, s, x_gelu=h_gelu)
    check(_l().leod_layerscale_finalize(_p(W), _p(b), _p(gamma), _p(G), _p(s), _p(dW), _p(db), _p(dgamma), N, K, _stream()),
          'layerscale_finalize')


# ---------------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------------
def _out_hw(H, W, ks, stride, pad):
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def stem_conv_fwd(x_nchw, w, padded_hw, stride, pad):
    """x [B,Cin,H,W] uint8|fp32 NCHW (unpadded) -> y [B,Ho,Wo,N] NHWC."""
    if x_nchw.dtype not in (torch.uint8, F32):
        raise LeodHipError(f'stem input must be uint8 or float32, got {x_nchw.dtype}')
    _ck(x_nchw, x_nchw.dtype, 'x')
    _ck(w, name='w')
    B, Cin, H, W = x_nchw.shape
    N, ks = w.shape[0], w.shape[-1]
    Ho, Wo = _out_hw(padded_hw[0], padded_hw[1], ks, stride, pad)
    y = torch.empty((B, Ho, Wo, N), dtype=F32, device=x_nchw.device)
    check(_l().leod_stem_conv_fwd(_p(x_nchw), 1 if x_nchw.dtype == torch.uint8 else 0, _p(w), _p(y), B, Cin, H, W,
                                   padded_hw[0], padded_hw[1], N, ks, stride, pad, _stream()), 'stem_conv_fwd')
    return y


def stem_conv_wgrad(dy, x_nchw, dw, padded_hw, stride, pad):
    _ck(dy, name='dy')
    _ck(x_nchw, x_nchw.dtype, 'x')
    _ck(dw, name='dw')
    B, Cin, H, W = x_nchw.shape
    N, ks = dw.shape[0], dw.shape[-1]
    check(_l().leod_stem_conv_wgrad(_p(dy), _p(x_nchw), 1 if x_nchw.dtype == torch.uint8 else 0, _p(dw), B, Cin, H, W,
                                     padded_hw[0], padded_hw[1], N, ks, stride, pad, _stream()), 'stem_conv_wgrad')


BF16_GRADS = True          # 16-bit modes: du (and dqkv) stored as bf16
STAT_REPLICAS = 32          # most copies of the BatchNorm (sum, sumsq) accumulators a conv epilogue spreads its atomics over


def _replica_count(rows: int, per: int, cap: int) -> int:
    """Copies of a per-channel accumulator block that the producers of ``rows`` rows spread their closing atomics over: one per ``per``
    rows, a power of two in [1, cap] -- the consumer folds the copies in every workgroup, so small layers should not carry ``cap``."""
    r = 1
    while r < cap and r * per < rows:
        r *= 2
    return r


def stat_replicas(rows: int) -> int:
    """(sum, sumsq) copies for a conv with ``rows`` output pixels: one per ~1280 rows (80 wave tiles), at most 32; bn_silu_fwd folds them"""
    return _replica_count(rows, 1280, STAT_REPLICAS)


def bn_bwd_replicas(rows: int) -> int:
    """(sum du, sum du*xhat) copies for bn_silu_bwd_reduce over ``rows`` rows: one per 2560 rows, at most 16; bn_silu_bwd_apply folds them"""
    return _replica_count(rows, 2560, 16)


class PackCache:
    """Packed copies of the conv weights (K-contiguous / per-tap bf16, written by the conv calls themselves into ``wpack``), kept for
    as long as the weights they were made from are unchanged: the 20 3x3 convs of PAFPN + head each re-packed their weights on every
    forward AND dgrad call (40 pack launches per training step) although weights change once per optimiser step.

    An entry is valid for (weight tensor object, direction, geometry) while the tensor's address, its torch version counter, the
    library's precision mode and ``epoch`` are unchanged.  ``epoch`` is advanced by whatever rewrites parameters behind torch's back -- the fused AdamW
    kernel (``FlatParams.adamw_step``) -- and must be advanced (``PackCache.invalidate()``) by any other code that edits parameter
    memory through another alias (e.g. in-place ops on ``FlatParams.data``; ``FlatParams`` wraps that in ``FlatParams.touch()``)."""
    epoch = 0
    entries = {}
    next_token = 1

    @classmethod
    def get(cls, w, key, nfloats):
        # Identity of the WEIGHT TENSOR OBJECT, not of its address: a token stored on the tensor the first time it is seen.  Keyed by
        # data_ptr alone, the parameter of a NEW module that the allocator placed at the address of a dead module's parameter (same
        # geometry, same version counter, no optimiser step in between -- two evaluation models in one process) hit the dead
        # module's pack: stale weights in that conv (seen as a 25 % flake of the TTA test inside the full suite).
        tok = getattr(w, '_leod_pack_token', None)
        if tok is None:
            tok = cls.next_token
            cls.next_token += 1
            w._leod_pack_token = tok
        k = (tok,) + key
        ver = (w.data_ptr(), w._version, cls.epoch, w.numel(), get_precision())
        e = cls.entries.get(k)
        if e is not None and e[1] == ver and e[0].numel() >= nfloats:
            return e[0], 1
        buf = e[0] if (e is not None and e[0].numel() >= nfloats and e[0].device == w.device) else cls._alloc(nfloats, w.device)
        if len(cls.entries) > 4096:
            cls.entries.clear()
        cls.entries[k] = (buf, ver)
        return buf, 0

    _aux = {}

    @classmethod
    def _alloc(cls, nfloats, device):
        """A pack buffer lives as long as the cache and must never come out of a stream capture's private pool: a buffer from that pool may
        alias a temporary of the captured step, and the launch plans hoist weight packs out of their captured order (csrc/k_plan.hip).
        While the current stream is capturing, the allocation is made on a non-capturing stream (torch's allocator then serves it from the
        ordinary pool; the capture runs in relaxed mode)."""
        if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            st = cls._aux.get(device)
            if st is None:
                st = cls._aux[device] = torch.cuda.Stream(device=device)
            with torch.cuda.stream(st):
                return torch.empty(nfloats, dtype=F32, device=device)
        return torch.empty(nfloats, dtype=F32, device=device)

    @classmethod
    def ranges(cls):
        """[(address, bytes)] of every live pack buffer (what a launch plan may hoist a weight pack into)"""
        seen = {}
        for buf, _ in cls.entries.values():
            seen[buf.data_ptr()] = buf.numel() * 4
        return sorted(seen.items())

    @classmethod
    def invalidate(cls):
        cls.epoch += 1


# flags of ``conv_route``: what the call is given (include/leod_hip.h, leod_conv_route)
CF_BIAS, CF_COLSTATS, CF_BN, CF_PACK, CF_WS, CF_DBIAS, CF_ACCUMULATE, CF_U8, CF_ALIGN4 = 1, 2, 4, 8, 16, 32, 64, 128, 256
_CONV_ROUTES = {}


def conv_route(entry, B, H, W, Cin, N, ks=3, stride=1, pad=None, flags=0, padded_hw=None) -> int:
    """The kernel dense-convolution call number ``entry`` (0 conv_nhwc_fwd, 1 conv_nhwc_dgrad, 2 conv_nhwc_wgrad, 3 stem_conv_fwd,
    4 stem_conv_wgrad) runs for this problem in the current precision mode, or the negative error code it returns (``leod_conv_route`` in
    include/leod_hip.h lists the flags and the route codes; nothing is launched).  pad defaults to (ks - 1) // 2, the stem's padded frame
    to its stored one.  Answers are remembered per precision mode (``leod_conv_route`` reads nothing but its arguments and the mode): the
    conv wrappers ask on every call, and a repeated question must not cost the eager step a C call that a launch probe brackets."""
    pad = (ks - 1) // 2 if pad is None else pad
    key = (int(_l().leod_get_precision()), entry, B, H, W, Cin, N, ks, stride, pad, flags, padded_hw)
    code = _CONV_ROUTES.get(key)
    if code is None:
        if len(_CONV_ROUTES) > 4096:
            _CONV_ROUTES.clear()
        hp, wp = padded_hw if padded_hw is not None else (0, 0)
        code = _CONV_ROUTES[key] = int(_l().leod_conv_route(entry, B, H, W, Cin, N, ks, stride, pad, flags, hp, wp))
    return code


def conv_route_reads_pack(code: int) -> bool:
    """the routes that read ``wpack``: the direct 3x3 kernels (per-tap 16-bit pack) and the LDS-staged GEMM on the K-contiguous fp32 pack"""
    return code in (110, 120, 220) or (code >= 10000 and code % 10000 // 1000 == 7)


def _is_depthwise(w, cin: int) -> bool:
    """a conv weight [C,1,ks,ks] over a C-channel map (C > 1) is a depthwise convolution (nn.Conv2d(C, C, ks, groups=C))"""
    return w.dim() == 4 and w.shape[1] == 1 and cin > 1 and w.shape[0] == cin


def conv_nhwc_fwd(x, w, bias=None, stride=1, colstats=None, bn=None, bn_eps=1e-5):
    """x [B,H,W,Cin] -> y [B,Ho,Wo,N]; pad = (ks-1)//2.  bn = (weight, bias, running_mean, running_var) -> eval BN+SiLU fused.
    colstats: zero-filled float64 [2,N] or [R,2,N] (R a power of two: the epilogue's atomics are spread over the R copies)."""
    _ck(x, name='x')
    _ck(w, name='w')
    _ck(bias, name='bias')
    _ck(colstats, torch.float64, 'colstats')
    B, H, W, Cin = x.shape
    N, ks = w.shape[0], w.shape[-1]
    pad = (ks - 1) // 2
    Ho, Wo = _out_hw(H, W, ks, stride, pad)
    y = _empty((B, Ho, Wo, N), x)
    bw = bb = brm = brv = None
    if bn is not None:
        bw, bb, brm, brv = bn
        for t in bn:
            _ck(t, name='bn')
    if _is_depthwise(w, Cin):                    # groups == channels: w [C,1,ks,ks] (DWConv.dconv, conv3x3_dws of the ConvLSTM)
        rep = colstats.shape[0] if colstats is not None and colstats.dim() == 3 else 1
        check(_l().leod_dwconv_nhwc_fwd(_p(x), _p(w), _p(bias), _p(y), _p(colstats), rep, _p(bw), _p(bb), _p(brm), _p(brv), bn_eps,
                                         B, H, W, Cin, ks, stride, pad, _stream()), 'dwconv_nhwc_fwd')
        return y
    flags = (CF_PACK if ks > 1 else 0) | (CF_BIAS if bias is not None else 0) | (CF_COLSTATS if colstats is not None else 0) | (CF_BN if bn is not None else 0)
    wpack, valid = None, 0                        # a pack buffer is offered to ks > 1 only, and taken only for the routes that read one
    if conv_route_reads_pack(conv_route(0, B, H, W, Cin, N, ks, stride, pad, flags)):
        wpack, valid = PackCache.get(w, ('fwd', B, H, W, stride, bn is not None, bias is not None), N * Cin * ks * ks)
    rep = colstats.shape[0] if colstats is not None and colstats.dim() == 3 else 1
    check(_l().leod_conv_nhwc_fwd(_p(x), _p(w), _p(bias), _p(y), _p(colstats), rep, _p(bw), _p(bb), _p(brm), _p(brv), bn_eps,
                                   B, H, W, Cin, N, ks, stride, pad, _p(wpack), valid, _stream()), 'conv_nhwc_fwd')
    return y


def conv_nhwc_dgrad(dy, w, x_shape, stride=1, out=None, accumulate=False):
    _ck(dy, name='dy')
    _ck(w, name='w')
    B, H, W, Cin = x_shape
    N, ks = w.shape[0], w.shape[-1]
    pad = (ks - 1) // 2
    if out is None:
        out = _empty(tuple(x_shape), dy)
        accumulate = False
    _ck(out, name='dx')
    if _is_depthwise(w, Cin):
        check(_l().leod_dwconv_nhwc_dgrad(_p(dy), _p(w), _p(out), 1 if accumulate else 0, B, H, W, Cin, ks, stride, pad, _stream()),
              'dwconv_nhwc_dgrad')
        return out
    wpack, valid = None, 0
    if conv_route_reads_pack(conv_route(1, B, H, W, Cin, N, ks, stride, pad, CF_PACK if ks > 1 else 0)):
        wpack, valid = PackCache.get(w, ('dgrad', B, H, W, stride), N * Cin * ks * ks)
    check(_l().leod_conv_nhwc_dgrad(_p(dy), _p(w), _p(out), 1 if accumulate else 0, B, H, W, Cin, N, ks, stride, pad,
                                     _p(wpack), valid, _stream()), 'conv_nhwc_dgrad')
    return out


def _conv3x3_group_routes_to(code, entry, flags, shapes, Cin, N) -> bool:
    """1..8 stride-1 3x3 problems of one channel geometry share a launch when every member routes to ``code`` (a refused grouped call must
    not have touched the pack cache: a pack marked valid there would never have been written)"""
    return 1 <= len(shapes) <= 8 and all(conv_route(entry, sh[0], sh[1], sh[2], Cin, N, 3, 1, 1, flags) == code for sh in shapes)


def conv3x3_group_ok(xs, ws) -> bool:
    """n <= 8 dense 3x3 convs of one (Cin, Cout) geometry on fp32 NHWC maps: candidates for ``conv3x3_group_fwd`` / ``_dgrad``"""
    w0 = ws[0]
    return (1 < len(xs) <= 8 and all(w.shape == w0.shape and w.dim() == 4 and w.shape[-1] == 3 and w.shape[-2] == 3 for w in ws)
            and all(x.dim() == 4 and x.shape[-1] == w0.shape[1] and x.dtype is F32 and x.is_cuda for x in xs) and not _is_depthwise(w0, xs[0].shape[-1]))


def _replicas(t) -> int:                      # copies in a statistics block: [R,2,N] -> R, a plain [2,N] -> 1
    return t.shape[0] if t.dim() == 3 else 1


def _conv3x3_group_tables(shapes, Cin, N, ws=None, pack_key=None):
    """The tables of a grouped call that ``_conv3x3_group_routes_to`` has accepted: the members' B, H and W, behind -- for the entries that
    read packed weights (``pack_key``: the PackCache key around (B, H, W)) -- the pack addresses and their valid flags."""
    tables = [_int_array([sh[d] for sh in shapes]) for d in range(3)]
    if pack_key is not None:
        packs = [PackCache.get(w, pack_key[:1] + tuple(sh[:3]) + pack_key[1:], N * Cin * 9) for w, sh in zip(ws, shapes)]
        tables = [_ptr_array([p for p, _ in packs]), _int_array([v for _, v in packs])] + tables
    return tables


def _ck_conv3x3_group(*tensors):
    for t in tensors:
        _ck(t, name='conv3x3_group')


def conv3x3_group_fwd(xs, ws, colstats):
    """[x_k [B,H,W,Cin]], [w_k [N,Cin,3,3]], [colstats_k: zero-filled float64 [R,2,N]] -> [y_k] in ONE launch (stride 1, pad 1), or None
    where the direct kernel does not cover the geometry (run them singly)."""
    _ck_conv3x3_group(*xs, *ws)
    for c in colstats:
        _ck(c, torch.float64, 'colstats')
    N, Cin = ws[0].shape[0], ws[0].shape[1]
    shapes = [x.shape for x in xs]
    if not _conv3x3_group_routes_to(110, 0, CF_PACK | CF_COLSTATS, shapes, Cin, N):
        return None
    ys = [_empty(tuple(x.shape[:3]) + (N,), x) for x in xs]
    tables = _conv3x3_group_tables(shapes, Cin, N, ws, ('fwd', 1, False, False))
    check(_l().leod_conv3x3_group_fwd(len(xs), _ptr_array(xs), _ptr_array(ws), _ptr_array(ys), _ptr_array(colstats),
                                       _int_array([_replicas(c) for c in colstats]), *tables, Cin, N, _stream()), 'conv3x3_group_fwd')
    return ys


def conv3x3_group_dgrad(dys, ws, x_shapes, outs, accumulate) -> bool:
    """outs[k] (+)= input gradient of conv(x_k, w_k) from dys[k] in ONE launch; False where not coverable (nothing was written)."""
    _ck_conv3x3_group(*dys, *ws, *outs)
    N, Cin = ws[0].shape[0], ws[0].shape[1]
    if not _conv3x3_group_routes_to(110, 1, CF_PACK, x_shapes, Cin, N):
        return False
    tables = _conv3x3_group_tables(x_shapes, Cin, N, ws, ('dgrad', 1))
    check(_l().leod_conv3x3_group_dgrad(len(dys), _ptr_array(dys), _ptr_array(ws), _ptr_array(outs), _int_array([1 if a else 0 for a in accumulate]),
                                         *tables, Cin, N, _stream()), 'conv3x3_group_dgrad')
    return True


def conv3x3_group_wgrad(dys, xs, dws) -> bool:
    """dws[k] += weight gradient of conv(x_k, w_k) from dys[k] (stride 1) in ONE launch (+ one reduce); False where not coverable."""
    _ck_conv3x3_group(*dys, *xs, *dws)
    N, Cin = dws[0].shape[0], dws[0].shape[1]
    shapes = [x.shape for x in xs]
    if not _conv3x3_group_routes_to(500, 2, CF_WS, shapes, Cin, N):
        return False
    sizes = [int(_l().leod_conv3x3_group_wgrad_workspace_floats(x.shape[0], x.shape[1], x.shape[2], Cin, N)) for x in xs]
    parts = list(_empty((sum(sizes),), dys[0]).split(sizes))
    check(_l().leod_conv3x3_group_wgrad(len(dys), _ptr_array(dys), _ptr_array(xs), _ptr_array(dws), _ptr_array(parts),
                                         *_conv3x3_group_tables(shapes, Cin, N), Cin, N, _stream()), 'conv3x3_group_wgrad')
    return True


_CONV1X1_ROUTES = {}


def conv1x1_group_route(entry, shapes, flags=0) -> int:
    """``leod_conv1x1_group_route`` for members of (rows, contraction length, output columns) -- entry 0: (M, Cin, N) of the forward call,
    1: (M, N, Cin) of the dgrad -- in the current precision mode: the route code of the one launch, or the negative code of a refusal.
    Nothing is launched; answers are remembered per precision mode like those of ``conv_route``."""
    key = (int(_l().leod_get_precision()), entry, tuple(tuple(int(d) for d in sh) for sh in shapes), flags)
    code = _CONV1X1_ROUTES.get(key)
    if code is None:
        if len(_CONV1X1_ROUTES) > 4096:
            _CONV1X1_ROUTES.clear()
        dims = [_int_array([sh[d] for sh in key[2]]) for d in range(3)]
        code = _CONV1X1_ROUTES[key] = int(_l().leod_conv1x1_group_route(entry, len(key[2]), *dims, flags))
    return code


def is_conv1x1(w, x) -> bool:
    """a dense 1x1 conv weight [N,Cin,1,1] over an fp32 NHWC device map of Cin channels: its stride-1 form is a GEMM over the pixel rows"""
    return (w.dim() == 4 and w.shape[-1] == 1 and w.shape[-2] == 1 and x.dim() == 4 and w.shape[1] == x.shape[-1] and x.dtype is F32
            and x.is_cuda)


def conv1x1_group_ok(entry, shapes) -> bool:
    """1..4 stride-1 1x1 convs (``conv1x1_group_route``'s members) go out as ONE launch of the short-problem kernel: the one question
    ``conv1x1_group_fwd`` / ``_dgrad`` ask before they allocate or launch anything"""
    return conv1x1_group_route(entry, shapes) > 0


def conv1x1_group_fwd(xs, ws, colstats):
    """[x_k [B,H,W,Cin]], [w_k [N,Cin,1,1]], [colstats_k: zero-filled float64 [R,2,N] | None] -> [y_k [B,H,W,N]] in ONE launch, or None where
    the route refuses the group (nothing was allocated or launched: run them singly)."""
    for t in (*xs, *ws):
        _ck(t, name='conv1x1_group')
    for c in colstats:
        _ck(c, torch.float64, 'colstats')
    shapes = [(x.numel() // x.shape[-1], x.shape[-1], w.shape[0]) for x, w in zip(xs, ws)]
    if not (1 <= len(xs) <= 4) or not conv1x1_group_ok(0, shapes):
        return None
    ys = [_empty(tuple(x.shape[:-1]) + (w.shape[0],), x) for x, w in zip(xs, ws)]
    check(_l().leod_conv1x1_group_fwd(len(xs), _ptr_array(xs), _ptr_array(ws), _ptr_array(ys), _ptr_array(colstats),
                                       _int_array([1 if c is None else _replicas(c) for c in colstats]),
                                       *[_int_array([sh[d] for sh in shapes]) for d in range(3)], _stream()), 'conv1x1_group_fwd')
    return ys


def conv1x1_group_dgrad(dys, ws, outs, accumulate) -> bool:
    """outs[k] [B,H,W,Cin] (+)= dys[k] [B,H,W,N] w_k [N,Cin,1,1] in ONE launch; False where the route refuses (nothing was written)."""
    for t in (*dys, *ws, *outs):
        _ck(t, name='conv1x1_group')
    shapes = [(dy.numel() // dy.shape[-1], w.shape[1], w.shape[0]) for dy, w in zip(dys, ws)]         # (M, Cin, N)
    if not (1 <= len(dys) <= 4) or not conv1x1_group_ok(1, [(m, n, c) for m, c, n in shapes]):
        return False
    check(_l().leod_conv1x1_group_dgrad(len(dys), _ptr_array(dys), _ptr_array(ws), _ptr_array(outs), _int_array([1 if a else 0 for a in accumulate]),
                                         *[_int_array([sh[d] for sh in shapes]) for d in range(3)], _stream()), 'conv1x1_group_dgrad')
    return True


def conv_nhwc_wgrad(dy, x, dw, dbias=None, stride=1):
    for t, n in ((dy, 'dy'), (x, 'x'), (dw, 'dw'), (dbias, 'dbias')):
        _ck(t, name=n)
    B, H, W, Cin = x.shape
    N, ks = dw.shape[0], dw.shape[-1]
    pad = (ks - 1) // 2
    if _is_depthwise(dw, Cin):
        check(_l().leod_dwconv_nhwc_wgrad(_p(dy), _p(x), _p(dw), _p(dbias), B, H, W, Cin, ks, stride, pad, _stream()), 'dwconv_nhwc_wgrad')
        return
    nws = int(_l().leod_conv_nhwc_wgrad_workspace_floats(B, H, W, Cin, N, ks, stride, pad, 0 if dbias is None else 1))
    ws = _empty((nws,), dy) if nws else None
    check(_l().leod_conv_nhwc_wgrad(_p(dy), _p(x), _p(dw), _p(dbias), _p(ws), B, H, W, Cin, N, ks, stride, pad, _stream()),
          'conv_nhwc_wgrad')


def _bn_rows(zs, who):                        # -> (N, rows per layer) of the layers of one launch
    N = zs[0].shape[-1]
    if any(z.shape[-1] != N for z in zs):
        raise LeodHipError(f'{who}: one channel count per launch')
    return N, [z.numel() // N for z in zs]


def _dy_stride(dy, N, who) -> int:            # row stride of a gradient the BN backward kernels read in place (``row_stride``)
    ld = row_stride(dy, N)
    if not ld:
        raise LeodHipError(f'{who}: dy must be contiguous or a channel slice of a contiguous map')
    _ck_dtype_dev(dy, F32, 'dy')
    return ld


def _count_devs(count_devs):                  # device-side row counts (SyncBatchNorm: the global image count); NULL when no layer has one
    return None if count_devs is None or all(c is None for c in count_devs) else _ptr_array(count_devs)


def bn_silu_fwd(z, colstats, w, b, run_mean, run_var, count, eps=1e-5, momentum=0.1, count_dev=None):
    _ck(z, name='z')
    _ck(colstats, torch.float64, 'colstats')
    N = z.shape[-1]
    y, mean, rstd = _empty(z.shape, z), _empty((N,), z), _empty((N,), z)
    check(_l().leod_bn_silu_fwd(_p(z), _p(colstats), _replicas(colstats), _p(w), _p(b), _p(y), _p(mean), _p(rstd), _p(run_mean), _p(run_var),
                                 z.numel() // N, N, float(count), _p(count_dev), eps, momentum, _stream()), 'bn_silu_fwd')
    return y, mean, rstd


def bn_silu_fwd_group(zs, colstats, ws, bs, run_means, run_vars, counts, eps, momenta, count_devs=None):
    """``bn_silu_fwd`` for 1 <= n <= 8 layers of one channel count in ONE launch -> [(y, mean, rstd)].  Here as in the two calls below a
    lone layer goes to the scalar wrapper (the scalar C entry: same call table, same replayed plan, no host arrays)."""
    if len(zs) == 1:
        return [bn_silu_fwd(zs[0], colstats[0], ws[0], bs[0], run_means[0], run_vars[0], counts[0], eps=eps, momentum=momenta[0],
                            count_dev=count_devs[0] if count_devs else None)]
    N, rows = _bn_rows(zs, 'bn_silu_fwd_group')
    for z, c in zip(zs, colstats):
        _ck(z, name='z')
        _ck(c, torch.float64, 'colstats')
    ys, means, rstds = [_empty(z.shape, z) for z in zs], [_empty((N,), z) for z in zs], [_empty((N,), z) for z in zs]
    check(_l().leod_bn_silu_fwd_group(len(zs), _ptr_array(zs), _ptr_array(colstats), _int_array([_replicas(c) for c in colstats]),
                                       _ptr_array(ws), _ptr_array(bs), _ptr_array(ys), _ptr_array(means), _ptr_array(rstds),
                                       _ptr_array(run_means), _ptr_array(run_vars), _int_array(rows), N, _f64_array(counts),
                                       _count_devs(count_devs), float(eps), _f32_array(momenta), _stream()), 'bn_silu_fwd_group')
    return list(zip(ys, means, rstds))


def bn_silu_bwd_reduce_group(dys, zs, means, rstds, ws, bs, outs):
    """``bn_silu_bwd_reduce`` for 1 <= n <= 8 layers of one channel count in ONE launch, into the zero-filled ``outs``"""
    if len(zs) == 1:
        bn_silu_bwd_reduce(dys[0], zs[0], means[0], rstds[0], ws[0], bs[0], out=outs[0])
        return
    N, rows = _bn_rows(zs, 'bn_silu_bwd_reduce_group')
    lds = [_dy_stride(dy, N, 'bn_silu_bwd_reduce_group') for dy in dys]
    check(_l().leod_bn_silu_bwd_reduce_group(len(zs), _ptr_array(dys), _ptr_array(zs), _ptr_array(means), _ptr_array(rstds), _ptr_array(ws),
                                              _ptr_array(bs), _ptr_array(outs), _int_array([_replicas(o) for o in outs]), _int_array(rows), N,
                                              _int_array(lds), _stream()), 'bn_silu_bwd_reduce_group')


def bn_silu_bwd_apply_group(dys, zs, means, rstds, ws, bs, sums, dws, dbs, counts, count_devs=None):
    """``bn_silu_bwd_apply`` for 1 <= n <= 8 layers of one channel count in ONE launch -> [dz]"""
    if len(zs) == 1:
        return [bn_silu_bwd_apply(dys[0], zs[0], means[0], rstds[0], ws[0], bs[0], sums[0], dws[0], dbs[0], counts[0],
                                  count_dev=count_devs[0] if count_devs else None)]
    N, rows = _bn_rows(zs, 'bn_silu_bwd_apply_group')
    lds = [_dy_stride(dy, N, 'bn_silu_bwd_apply_group') for dy in dys]
    dzs = [_empty(z.shape, z) for z in zs]
    check(_l().leod_bn_silu_bwd_apply_group(len(zs), _ptr_array(dys), _ptr_array(zs), _ptr_array(means), _ptr_array(rstds), _ptr_array(ws),
                                             _ptr_array(bs), _ptr_array(sums), _int_array([_replicas(o) for o in sums]), _ptr_array(dzs),
                                             _ptr_array(dws), _ptr_array(dbs), _int_array(rows), N, _f64_array(counts), _count_devs(count_devs),
                                             _int_array(lds), _stream()), 'bn_silu_bwd_apply_group')
    return dzs


class StatArena:
    """Zero-initialised scratch of ONE training step: the BatchNorm statistic accumulators ((sum, sumsq) per conv in the forward pass,
    (sum du, sum du*xhat) in the backward pass: 78 tiny float64 buffers per step) and the fp32 un-scaled weight-gradient scratch of
    the 16 LayerScale layers (``layerscale_linear_wgrad``).  The engine zeroes the used part of the arena with ONE memset at the start
    of a step and the ops take slices; outside an engine step (or when the arena is exhausted) the ops fall back to ``torch.zeros``."""
    buf: Optional[torch.Tensor] = None                # uint8
    off = 0
    high = 0                                          # bytes handed out since the arena was last zeroed in full
    active = False
    SIZE = 48 << 20                                   # bytes

    @classmethod
    def begin_step(cls, device):
        if cls.buf is None or cls.buf.device != torch.device(device):
            cls.buf = torch.zeros(cls.SIZE, dtype=torch.uint8, device=device)
        elif cls.high:
            cls.buf[:cls.high].zero_()                # everything beyond the high-water mark was never handed out: still zero
        cls.off, cls.high, cls.active = 0, 0, True

    @classmethod
    def end_step(cls):
        cls.active = False

    @classmethod
    def swap(cls, buf, off=0, high=0, active=False):
        """Install another arena buffer (a captured step keeps a private one: its replays write at the offsets handed out during capture,
        behind the back of this class's high-water bookkeeping); returns the state to hand back to ``swap`` afterwards."""
        old = (cls.buf, cls.off, cls.high, cls.active)
        cls.buf, cls.off, cls.high, cls.active = buf, off, high, active
        return old

    @classmethod
    def zeros(cls, shape, device, dtype=torch.float64):
        n = 1
        for d in shape:
            n *= d
        nbytes = n * (8 if dtype is torch.float64 else 4)
        n_al = (nbytes + 15) & ~15                    # keep 16-byte alignment
        if cls.active and cls.buf is not None and cls.buf.device == torch.device(device) and cls.off + n_al <= cls.SIZE:
            t = cls.buf[cls.off:cls.off + nbytes].view(dtype).view(shape)
            cls.off += n_al
            cls.high = max(cls.high, cls.off)
            return t
        return torch.zeros(shape, dtype=dtype, device=device)


def row_stride(t: torch.Tensor, N: int) -> int:
    """Row stride (elements) of ``t`` seen as [rows, N] when its rows are evenly spaced -- a contiguous tensor (N) or the channel slice
    ``wide[..., c0:c0 + N]`` of a contiguous wider map, which is what ``torch.cat``'s backward hands out; 0: anything else."""
    if t.is_contiguous():
        return N
    if t.dim() < 2 or t.shape[-1] != N or t.stride(-1) != 1:
        return 0
    ld = t.stride(-2)
    exp = ld
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] != 1 and t.stride(d) != exp:
            return 0
        exp *= t.shape[d]
    return ld if (ld >= N and ld % 4 == 0 and t.storage_offset() % 4 == 0) else 0


def bn_silu_bwd_reduce(dy, z, mean, rstd, w, b, out=None):
    """out: zero-filled float64 [2,N] or [R,2,N] (R replicas, see ``bn_bwd_replicas``).
    dy: contiguous, or a channel slice of a wider contiguous map (see ``row_stride``) -- read in place with its row stride."""
    N = z.shape[-1]
    M = z.numel() // N
    ld = _dy_stride(dy, N, 'bn_silu_bwd_reduce')
    sums = StatArena.zeros((bn_bwd_replicas(M), 2, N), z.device) if out is None else out
    _ck(sums, torch.float64, 'sums')
    check(_l().leod_bn_silu_bwd_reduce(_p(dy), _p(z), _p(mean), _p(rstd), _p(w), _p(b), _p(sums), _replicas(sums), M, N, ld, _stream()),
          'bn_silu_bwd_reduce')
    return sums


def bn_silu_bwd_apply(dy, z, mean, rstd, w, b, sums, dw, db, count, count_dev=None):
    N = z.shape[-1]
    ld = _dy_stride(dy, N, 'bn_silu_bwd_apply')
    dz = _empty(z.shape, z)
    check(_l().leod_bn_silu_bwd_apply(_p(dy), _p(z), _p(mean), _p(rstd), _p(w), _p(b), _p(sums), _replicas(sums), _p(dz), _p(dw), _p(db),
                                       z.numel() // N, N, float(count), _p(count_dev), ld, _stream()), 'bn_silu_bwd_apply')
    return dz


# ---------------------------------------------------------------------------------------------------
# head tail
# ---------------------------------------------------------------------------------------------------
def head_pred_fwd(cls_feat, reg_feat, cls_w, cls_b, reg_w, reg_b, obj_w, obj_b, out_train, out_infer, stride, a0):
    for t in (cls_feat, reg_feat, cls_w, cls_b, reg_w, reg_b, obj_w, obj_b, out_train, out_infer):
        _ck(t, name='head_pred')
    B, h, w, Hd = cls_feat.shape
    nc = cls_w.shape[0]
    ref = out_train if out_train is not None else out_infer
    A = ref.shape[1]
    check(_l().leod_head_pred_fwd(_p(cls_feat), _p(reg_feat), _p(cls_w), _p(cls_b), _p(reg_w), _p(reg_b), _p(obj_w),
                                   _p(obj_b), _p(out_train), _p(out_infer), B, h, w, Hd, nc, stride, a0, A, _stream()),
          'head_pred_fwd')


def head_pred_bwd(d_raw, cls_feat, reg_feat, cls_w, reg_w, obj_w, d_cls_w, d_cls_b, d_reg_w, d_reg_b, d_obj_w, d_obj_b, a0,
                  gscale=None):
    B, h, w, Hd = cls_feat.shape
    nc = cls_w.shape[0]
    A = d_raw.shape[1]
    dcf = _empty(cls_feat.shape, cls_feat)
    drf = _empty(reg_feat.shape, reg_feat)
    check(_l().leod_head_pred_bwd(_p(d_raw), _p(cls_feat), _p(reg_feat), _p(cls_w), _p(reg_w), _p(obj_w), _p(dcf), _p(drf),
                                   _p(d_cls_w), _p(d_cls_b), _p(d_reg_w), _p(d_reg_b), _p(d_obj_w), _p(d_obj_b), _p(gscale),
                                   B, h, w, Hd, nc, a0, A, _stream()), 'head_pred_bwd')
    return dcf, drf


def simota_assign(outputs, labels, hws, strides, ignore_label=1024.0):
    """outputs [B,A,5+nc] decoded+logits, labels [B,Nmax,7] -> dict of device tensors (no host sync)."""
    _ck(outputs, name='outputs')
    _ck(labels, name='labels')
    B, A, nch = outputs.shape
    Nmax = labels.shape[1]
    dev = outputs.device
    ws = torch.empty(_l().leod_simota_workspace_floats(B, Nmax, A), dtype=F32, device=dev)
    r = dict(fg_mask=torch.empty((B, A), dtype=torch.uint8, device=dev),
             ignore_mask=torch.empty((B, A), dtype=torch.uint8, device=dev),
             matched_row=torch.empty((B, A), dtype=torch.int32, device=dev),
             matched_valid_idx=torch.empty((B, A), dtype=torch.int32, device=dev),
             pred_iou=torch.empty((B, A), dtype=F32, device=dev),
             num_fg_img=torch.empty((B,), dtype=torch.int32, device=dev),
             totals=StatArena.zeros((3,), dev, torch.int32))
    check(_l().leod_simota_assign(_p(outputs), _p(labels), _p(ws), _p(r['fg_mask']), _p(r['ignore_mask']),
                                   _p(r['matched_row']), _p(r['matched_valid_idx']), _p(r['pred_iou']), _p(r['num_fg_img']),
                                   _p(r['totals']), B, Nmax, nch - 5, len(hws), _int_array([h for h, _ in hws]),
                                   _int_array([w for _, w in hws]), _int_array(strides), float(ignore_label), _stream()),
          'simota_assign')
    return r


def bg_topk_ignore(outputs, labels, assign, k, ignore_label=1024.0):
    """``ignore_bg_k`` of the YOLOX head (yolo_head.py:335-356): marks the top ``k`` fraction of each image's background objectness logits
    in ``assign['ignore_mask']`` (in place), unless the batch holds an ignore box."""
    B, A, nch = outputs.shape
    check(_l().leod_bg_topk_ignore(_p(outputs), _p(labels), _p(assign['fg_mask']), _p(assign['ignore_mask']), B, labels.shape[1], A,
                                    nch - 5, float(k), float(ignore_label), _stream()), 'bg_topk_ignore')


def yolox_loss(outputs, labels, assign, hws, strides, want_grad=True, focal=False, reg_weight=5.0, obj_weight=1.0,
               cls_weight=1.0, grad_scale=1.0, label_w=None):
    """label_w [B, Nmax] (``bbox_loss_weighting``): per-label weights of the IoU / class terms, normalised on the device to mean 1 over
    the batch's foreground anchors."""
    B, A, nch = outputs.shape
    dev = outputs.device
    sums = StatArena.zeros((3,), dev, torch.float64)
    losses = torch.empty((6,), dtype=F32, device=dev)
    d_raw = torch.empty_like(outputs) if want_grad else None
    if label_w is not None:
        _ck(label_w, name='label_w')
        if tuple(label_w.shape) != tuple(labels.shape[:2]):
            raise ValueError('yolox_loss: one weight per label row')
        wsum = StatArena.zeros((1,), dev, torch.float64)
        check(_l().leod_yolox_loss_weighted(_p(outputs), _p(labels), _p(assign['fg_mask']), _p(assign['ignore_mask']),
                                             _p(assign['matched_row']), _p(assign['pred_iou']), _p(assign['totals']), _p(label_w),
                                             _p(wsum), _p(sums), _p(losses), _p(d_raw), B, labels.shape[1], nch - 5, len(hws),
                                             _int_array([h for h, _ in hws]), _int_array([w for _, w in hws]), _int_array(strides),
                                             1 if focal else 0, reg_weight, obj_weight, cls_weight, grad_scale, _stream()),
              'yolox_loss_weighted')
        return losses, d_raw
    check(_l().leod_yolox_loss(_p(outputs), _p(labels), _p(assign['fg_mask']), _p(assign['ignore_mask']),
                                _p(assign['matched_row']), _p(assign['pred_iou']), _p(assign['totals']), _p(sums), _p(losses),
                                _p(d_raw), B, labels.shape[1], nch - 5, len(hws), _int_array([h for h, _ in hws]),
                                _int_array([w for _, w in hws]), _int_array(strides), 1 if focal else 0, reg_weight, obj_weight,
                                cls_weight, grad_scale, _stream()), 'yolox_loss')
    return losses, d_raw


def postprocess_nms(pred, num_classes, conf_thre, nms_thre, class_agnostic=False, max_det=None, vanilla_limit=20000):
    """pred [B,A,5+nc] (mutated in place to xyxy) or, with num_classes=0, [B,A,7] xyxy rows.
    -> det [B,max_det,7], cnt [B] (device tensors, no sync)."""
    _ck(pred, name='pred')
    B, A, _ = pred.shape
    max_det = A if max_det is None else max_det
    det = torch.empty((B, max_det, 7), dtype=F32, device=pred.device)
    cnt = torch.empty((B,), dtype=torch.int32, device=pred.device)
    nws = int(_l().leod_postprocess_nms_workspace_bytes(B, A))
    ws = torch.empty(nws, dtype=torch.uint8, device=pred.device) if nws else None
    check(_l().leod_postprocess_nms(_p(pred), _p(det), _p(cnt), _p(ws), B, A, num_classes, float(conf_thre), float(nms_thre),
                                     1 if class_agnostic else 0, max_det, vanilla_limit, _stream()), 'postprocess_nms')
    return det, cnt


def host_counts(cnt, what='postprocess_nms'):
    """Per-image counts on the host (one sync).  A negative count can only come from calling the C ABI without the NMS
    workspace (``ops.postprocess_nms`` always passes it)."""
    counts = cnt.tolist()
    if counts and min(counts) < 0:
        raise LeodHipError(f'{what}: image {counts.index(min(counts))} overflowed the LDS candidate arrays and no workspace was given')
    return counts


_THRESHOLDS = {}


def _threshold_tensor(thr, device):
    """Per-class thresholds as a device tensor, uploaded once per distinct value (a fresh pageable upload per call made every
    pseudo-label chunk wait for the device at this point)."""
    key = ((float(thr),) if isinstance(thr, (float, int)) else tuple(float(t) for t in thr), str(device))
    t = _THRESHOLDS.get(key)
    if t is None:
        if len(_THRESHOLDS) > 64:
            _THRESHOLDS.clear()
        t = _THRESHOLDS[key] = torch.tensor(key[0], dtype=F32, device=device)
    return t


def pseudo_filter(det, cnt, obj_thr, cls_thr, filter_boxes, frame_hw):
    _ck(det, name='det')
    _ck(cnt, torch.int32, 'cnt')
    B, max_det, _ = det.shape
    ot, ct = _threshold_tensor(obj_thr, det.device), _threshold_tensor(cls_thr, det.device)
    if ot.numel() != ct.numel():
        raise LeodHipError('obj_thresh and cls_thresh must both be floats or per-class lists of equal length')
    lab = torch.empty((B, max_det, 8), dtype=F32, device=det.device)
    lcnt = torch.empty((B,), dtype=torch.int32, device=det.device)
    check(_l().leod_pseudo_filter(_p(det), _p(cnt), _p(lab), _p(lcnt), B, max_det, _p(ot), _p(ct), ot.numel(),
                                   1 if filter_boxes else 0, float(frame_hw[1]), float(frame_hw[0]), _stream()),
          'pseudo_filter')
    return lab, lcnt


# ---------------------------------------------------------------------------------------------------
def adamw_clip_step(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_value=0.0, grad_scale=1.0,
                    hp_dev=None):
    for t in (p, g, m, v):
        _ck(t, name='adamw buffer')
    check(_l().leod_adamw_clip_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay,
                                     int(step), float(clip_value), float(grad_scale), _p(hp_dev), _stream()), 'adamw_clip_step')


def adamw_clip_step_guarded(p, g, m, v, lr, nonfinite_total, state, scratch, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                            clip_value=0.0, grad_scale=1.0):
    """``adamw_clip_step`` that is not taken when ``nonfinite_total`` (device int32[1], from ``grad_stats`` over ``g``) is non-zero: p, g, m, v
    stay as they are and ``state`` (device int32[2] = applied, skipped) counts the step as skipped; otherwise the applied count advances and
    gives the bias corrections.  ``scratch``: device float32[8] of the caller.  Decided on the device: no read-back."""
    for t in (p, g, m, v):
        _ck(t, name='adamw buffer')
    _ck(nonfinite_total, torch.int32, 'nonfinite_total')
    _ck(state, torch.int32, 'state')
    _ck(scratch, name='scratch')
    if nonfinite_total.numel() < 1 or state.numel() < 2 or scratch.numel() < 8:
        raise ValueError('adamw_clip_step_guarded: nonfinite_total int32[1], state int32[2], scratch float32[8]')
    check(_l().leod_adamw_clip_step_guarded(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay,
                                             float(clip_value), float(grad_scale), _p(nonfinite_total), _p(state), _p(scratch), _stream()),
          'adamw_clip_step_guarded')


def _grad_stats_query(nchunk: int = 0):
    cf, ws = (ctypes.c_int * 1)(), (ctypes.c_long * 1)()
    check(_l().leod_grad_stats_query(int(nchunk), cf, ws), 'grad_stats_query')
    return int(cf[0]), int(ws[0])


def __getattr__(name):                                       # ops.GRAD_STATS_CHUNK: the library's own constant, asked once
    if name == 'GRAD_STATS_CHUNK':
        globals()[name] = _grad_stats_query()[0]
        return globals()[name]
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def grad_stats_tables(offsets: Sequence[int], lengths: Sequence[int], chunk: Optional[int] = None):
    """Host tables of ``grad_stats`` for segments (offset, length) in floats: seg int64 [nseg, 3] = (offset, length, first chunk) and
    chunk int32 [nchunk, 2] = (segment, chunk index within the segment); a segment of length L owns ceil(L / chunk) consecutive chunks,
    so no chunk straddles two segments.  Nothing is validated here: the library entry refuses a bad table."""
    chunk = int(chunk if chunk is not None else __getattr__('GRAD_STATS_CHUNK'))
    seg, cm = [], []
    for s, (o, n) in enumerate(zip(offsets, lengths)):
        seg.append((int(o), int(n), len(cm)))
        cm.extend((s, k) for k in range(max(0, -(-int(n) // chunk))))
    return (torch.tensor(seg, dtype=torch.int64).reshape(-1, 3), torch.tensor(cm, dtype=torch.int32).reshape(-1, 2))


class GradStatsPlan:
    """Everything ``grad_stats`` needs for one segment layout, made once: the tables on the host and on the device, the caller-owned
    scratch and the outputs (``stats`` float64 [nseg, 3] = sum |g|, sum g^2, max |g| over finite elements; ``nonfinite`` int32 [nseg];
    ``total`` int32 [1]) -- nothing is allocated during a step."""

    def __init__(self, offsets: Sequence[int], lengths: Sequence[int], device):
        self.seg_host, chunk_host = grad_stats_tables(offsets, lengths)
        self.nseg, self.nchunk = int(self.seg_host.shape[0]), int(chunk_host.shape[0])
        dev = torch.device(device)
        self.seg_dev, self.chunk_dev = self.seg_host.to(dev), chunk_host.to(dev)
        self.ws = torch.empty(max(1, _grad_stats_query(self.nchunk)[1] // 8), dtype=torch.float64, device=dev)
        self.stats = torch.zeros((self.nseg, 3), dtype=torch.float64, device=dev)
        self.nonfinite = torch.zeros((self.nseg,), dtype=torch.int32, device=dev)
        self.total = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.lengths = torch.tensor([int(n) for n in lengths], dtype=torch.float64)


def grad_stats(g: torch.Tensor, plan: GradStatsPlan):
    """One segmented pass over the fp32 buffer ``g`` (two launches, no read-back) -> (plan.stats, plan.nonfinite, plan.total)."""
    _ck(g, name='g')
    for t, dt, n in ((plan.seg_dev, torch.int64, 'segment table'), (plan.chunk_dev, torch.int32, 'chunk table'), (plan.ws, torch.float64, 'workspace'),
                     (plan.stats, torch.float64, 'stats'), (plan.nonfinite, torch.int32, 'nonfinite'), (plan.total, torch.int32, 'total')):
        _ck(t, dt, n)
    check(_l().leod_grad_stats(_p(g), g.numel(), _p(plan.seg_host), _p(plan.seg_dev), plan.nseg, _p(plan.chunk_dev), plan.nchunk,
                                _p(plan.ws), _p(plan.stats), _p(plan.nonfinite), _p(plan.total), _stream()), 'grad_stats')
    return plan.stats, plan.nonfinite, plan.total


def rows_index_add(dst: torch.Tensor, src: torch.Tensor, idx: torch.Tensor) -> None:
    """dst[idx[j]] += src[j] on dim 0 (fp32, contiguous, UNIQUE int64 indices on the device): one launch, no atomics."""
    _ck(dst, name='dst')
    _ck(src, name='src')
    _ck(idx, torch.int64, 'idx')
    if dst.shape[1:] != src.shape[1:] or src.shape[0] != idx.numel():
        raise ValueError('rows_index_add: src rows must match idx and the row shape of dst')
    row = dst[0].numel()
    check(_l().leod_rows_index_add(_p(dst), _p(src), _p(idx), int(idx.numel()), row, int(dst.shape[0]), _stream()), 'rows_index_add')


def cat2_up_fwd(a: torch.Tensor, b: torch.Tensor, up: bool = False) -> torch.Tensor:
    """out [B,H,W,Ca+Cb] = cat(a (nearest x2 upsampled if ``up``), b) on the channel axis of NHWC maps, one launch."""
    _ck(a, name='a')
    _ck(b, name='b')
    B, H, W, Cb = b.shape
    Ca = a.shape[-1]
    if tuple(a.shape[:3]) != ((B, H // 2, W // 2) if up else (B, H, W)):
        raise ValueError(f'cat2_up: a {tuple(a.shape)} does not match b {tuple(b.shape)} (up={up})')
    out = _empty((B, H, W, Ca + Cb), b)
    check(_l().leod_cat2_up_fwd(_p(a), _p(b), _p(out), B, H, W, Ca, Cb, 1 if up else 0, _stream()), 'cat2_up_fwd')
    return out


def cat2_up_bwd(dout: torch.Tensor, Ca: int, up: bool = False):
    """-> (da [B,H>>up,W>>up,Ca], db [B,H,W,C-Ca]) of ``cat2_up_fwd``."""
    _ck(dout, name='dout')
    B, H, W, C = dout.shape
    Cb = C - Ca
    da = _empty((B, H // 2, W // 2, Ca) if up else (B, H, W, Ca), dout)
    db = _empty((B, H, W, Cb), dout)
    check(_l().leod_cat2_up_bwd(_p(dout), _p(da), _p(db), B, H, W, Ca, Cb, 1 if up else 0, _stream()), 'cat2_up_bwd')
    return da, db


def set_weight_shadow(base: torch.Tensor, shadow: Optional[torch.Tensor]) -> None:
    """Register ``shadow`` (bf16, same length) as the 16-bit copy of the flat fp32 parameter buffer ``base`` (None: withdraw it)."""
    _ck(base, name='weight buffer')
    if shadow is not None and (shadow.dtype != torch.bfloat16 or shadow.numel() != base.numel() or shadow.device != base.device):
        raise ValueError('weight shadow: bf16 tensor of the length and device of the parameter buffer')
    check(_l().leod_set_weight_shadow(_p(base), base.numel(), _p(shadow)), 'set_weight_shadow')


def set_weight_shadow_f16(base: torch.Tensor, shadow_f16: Optional[torch.Tensor]) -> None:
    """Attach ``shadow_f16`` (fp16, same length) to the registration of ``base``: the copy the forward GEMMs of precision mode 16f read."""
    _ck(base, name='weight buffer')
    if shadow_f16 is not None and (shadow_f16.dtype != torch.float16 or shadow_f16.numel() != base.numel() or shadow_f16.device != base.device):
        raise ValueError('weight shadow: fp16 tensor of the length and device of the parameter buffer')
    check(_l().leod_set_weight_shadow_f16(_p(base), _p(shadow_f16)), 'set_weight_shadow_f16')


def unset_weight_shadow_ptr(base_ptr: int) -> None:
    """Withdraw the registration of the buffer that lived at ``base_ptr`` (finaliser of its owner; the tensor may be gone)."""
    try:
        _l().leod_set_weight_shadow(DevPtr(base_ptr, 'f32'), 0, None)
    except Exception:                                      # noqa: BLE001 -- interpreter shutdown
        pass


def weight_shadow_refresh(force: bool = False) -> int:
    """Round the registered parameter buffers whose shadow is stale into their shadows (``force``: all of them, freshness untouched --
    for launches that are being recorded, see ``weight_shadow_pin``).  Returns the number of launches."""
    if not torch.cuda.is_available():
        return 0
    rc = _l().leod_weight_shadow_refresh(1 if force else 0, _stream())
    if rc < 0:
        check(rc, 'weight_shadow_refresh')
    return rc


def weight_shadow_invalidate() -> None:
    check(_l().leod_weight_shadow_invalidate(), 'weight_shadow_invalidate')


def weight_shadow_pin(on: bool) -> None:
    """While a step is being recorded behind a forced refresh, the GEMM launchers read the shadows whatever their freshness flags say."""
    check(_l().leod_weight_shadow_pin(1 if on else 0), 'weight_shadow_pin')


def _ptr_array(ts):
    """host array of device addresses; None entries become NULL"""
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _long_array(v):
    return (ctypes.c_long * len(v))(*[int(x) for x in v])


def _int_array(v):
    return (ctypes.c_int * len(v))(*[int(a) for a in v])


def _f64_array(v):
    return (ctypes.c_double * len(v))(*[float(a) for a in v])


def _f32_array(v):
    return (ctypes.c_float * len(v))(*[float(a) for a in v])


def multi_ok(ts) -> bool:
    """Operands the multi-buffer plumbing kernels take: dense device tensors, 16-byte aligned, a multiple of 16 bytes per row."""
    def dense(t):      # rows (dim 0) back to back, each row dense: plain contiguous, or NCHW-shaped views of NHWC memory
        return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))
    return 0 < len(ts) <= 16 and all(t.is_cuda and dense(t) and t.data_ptr() % 16 == 0 and t.numel() > 0 and
                                     (t[0].numel() * t.element_size()) % 16 == 0 for t in ts)


ACTIVATIONS = {'gelu': 0, 'silu': 1, 'swish': 1, 'relu': 2, 'sigmoid': 3, 'tanh': 4, 'relu6': 5, 'leaky_relu': 6, 'elu': 7, 'hard_sigmoid': 8,
               'hardsigmoid': 8, 'hard_swish': 9, 'hardswish': 9, 'mish': 10, 'selu': 11, 'celu': 12, 'hard_mish': 13}


def act_glu_fwd(p, act: str, gated: bool):
    """h = a * act(g) with (a | g) the two halves of p's last dim (gated), or h = act(p): the MLP activation options of the attention block."""
    _ck(p, name='p')
    I = p.shape[-1] // 2 if gated else p.shape[-1]
    M = p.numel() // p.shape[-1]
    h = _empty(p.shape[:-1] + (I,), p)
    check(_l().leod_act_glu_fwd(_p(p), _p(h), M, I, ACTIVATIONS[act], 1 if gated else 0, _stream()), 'act_glu_fwd')
    return h


def act_glu_bwd(p, dh, act: str, gated: bool):
    _ck(p, name='p')
    _ck(dh, name='dh')
    I = dh.shape[-1]
    M = dh.numel() // I
    dp = _empty(p.shape, p)
    check(_l().leod_act_glu_bwd(_p(p), _p(dh), _p(dp), M, I, ACTIVATIONS[act], 1 if gated else 0, _stream()), 'act_glu_bwd')
    return dp


def token_mask_fwd_(x, mask, token):
    """x[mask] = token in place: x [.., C] contiguous rows, mask bool with one entry per row, token [C] (maxvit_rnn.py:190-192)."""
    _ck(x, name='x')
    _ck(token, name='token')
    C = x.shape[-1]
    if mask.dtype is not torch.bool or not mask.is_contiguous() or mask.device != x.device or mask.numel() * C != x.numel():
        raise LeodHipError('token_mask: one contiguous bool per row on the device of x')
    check(_l().leod_token_mask_fwd(_p(x), _p(mask), _p(token), mask.numel(), C, _stream()), 'token_mask_fwd')
    return x


def token_mask_bwd_(dx, mask, dtoken):
    """dtoken += sum of the masked rows of dx; those rows of dx are zeroed (in place)."""
    _ck(dx, name='dx')
    _ck(dtoken, name='dtoken')
    check(_l().leod_token_mask_bwd(_p(dx), _p(mask), _p(dtoken), mask.numel(), dx.shape[-1], _stream()), 'token_mask_bwd')
    return dx


def rows_masked_zero(tensors, mask):
    """t[b] = 0 where mask[b], for every t in ``tensors`` ([B, ...] each), in one launch (RNNStates.reset)."""
    if mask.dtype is not torch.bool or not mask.is_cuda or not mask.is_contiguous() or not multi_ok(tensors):
        raise LeodHipError('rows_masked_zero: contiguous device tensors with 16-byte rows and a bool device mask')
    B = mask.numel()
    if any(t.shape[0] != B for t in tensors):
        raise LeodHipError('rows_masked_zero: every tensor needs one row per mask entry')
    check(_l().leod_rows_masked_zero(_ptr_array(tensors), _long_array([t[0].numel() * t.element_size() for t in tensors]), len(tensors),
                                      _p(mask), B, _stream()), 'rows_masked_zero')


def copy_multi(dsts, srcs):
    """dst_k[:] = src_k[:] for all k in one launch (same dtype and element count per pair)."""
    if len(dsts) != len(srcs) or not multi_ok(dsts) or not multi_ok(srcs) or \
            any(d.dtype is not s_.dtype or d.shape != s_.shape or d.stride() != s_.stride() or (d.numel() * d.element_size()) % 16
                for d, s_ in zip(dsts, srcs)):
        raise LeodHipError('copy_multi: pairs of dense, 16-byte aligned device tensors of equal dtype, shape and strides')
    check(_l().leod_copy_multi(_ptr_array(dsts), _ptr_array(srcs), _long_array([d.numel() * d.element_size() for d in dsts]), len(dsts),
                                _stream()), 'copy_multi')


def onehot_scale(g: torch.Tensor, n: int, idx: int) -> torch.Tensor:
    """[0, .., g, .., 0] (n entries, g a device scalar at position idx) in one launch."""
    _ck(g.reshape(1), name='g')
    out = torch.empty((n,), dtype=F32, device=g.device)
    check(_l().leod_onehot_scale(_p(g), _p(out), int(n), int(idx), _stream()), 'onehot_scale')
    return out


def set_scalars4(dst, a, b, c, d):
    _ck(dst, name='dst')
    check(_l().leod_set_scalars4(_p(dst), float(a), float(b), float(c), float(d), _stream()), 'set_scalars4')


def stack_hflip_u8(frames) -> torch.Tensor:
    """T frame tensors [B, ...spatial..., W] (uint8 / bool / int8, same shape, contiguous) -> [T, 2B, ..., W]: the frames and, behind them on
    the batch axis, their horizontally flipped copies (torch.cat([torch.stack(frames), torch.stack(frames).flip(-1)], 1)) in one pass."""
    f0 = frames[0]
    if f0.element_size() != 1 or any(f.shape != f0.shape or f.dtype is not f0.dtype or not f.is_cuda or not f.is_contiguous() for f in frames):
        raise LeodHipError('stack_hflip_u8: contiguous one-byte device tensors of one shape expected')
    B, W = f0.shape[0], f0.shape[-1]
    out = torch.empty((len(frames), 2 * B) + tuple(f0.shape[1:]), dtype=f0.dtype, device=f0.device)
    check(_l().leod_stack_hflip_u8(_ptr_array(frames), len(frames), ctypes.c_void_p(out.data_ptr()), B, f0.numel() // (B * W), W, _stream()),
          'stack_hflip_u8')
    return out


def voxelize_u8(x, y, pol, t, bins, height, width, count_cutoff=None, fastmode=True):
    for a in (x, y, pol, t):
        _ck(a, torch.int64, 'events')
    dev = x.device
    ws = torch.empty((2 * bins * height * width,), dtype=torch.int32, device=dev)
    out = torch.empty((2 * bins, height, width), dtype=torch.uint8, device=dev)
    check(_l().leod_voxelize_u8(_p(x), _p(y), _p(pol), _p(t), x.numel(), _p(ws), _p(out), bins, height, width,
                                 0 if count_cutoff is None else int(count_cutoff), 1 if fastmode else 0, _stream()),
          'voxelize_u8')
    return out


# int32 count workspace of one chunk of windows (voxelize_dat_windows): 32 Gen1 windows = 187 MB, the fastest of the sweep in DESIGN.md section 4
# (the chunk's counts are cleared, counted into and read back while they still sit in the 256 MB Infinity Cache; 64 windows no longer do)
INGEST_WS_BYTES = 32 * 2 * 10 * 240 * 304 * 4


def ingest_ws_windows(bins, height, width, ds2=False) -> int:
    """Default number of windows per chunk of ``voxelize_dat_windows``: as many as fit ``INGEST_WS_BYTES`` of int32 counts."""
    per_win = 2 * bins * (height // 2 if ds2 else height) * (width // 2 if ds2 else width) * 4
    return max(1, INGEST_WS_BYTES // per_win)


def voxelize_dat_windows(records_u8, win_off, bins, height, width, ds2=False, count_cutoff=None, fastmode=True, ws_windows=None):
    """Raw Prophesee .dat records on the device (uint8 [n_events * 8] or [n_events, 8], as they lie in the file, time sorted) ->
    (out uint8 [n_win, 2*bins, Ho, Wo], dropped int64 [1]).  Window w holds events win_off[w] .. win_off[w+1]-1 (int64 [n_win + 1],
    ascending, first >= 0, last <= n_events; a host tensor / array is checked and uploaded, a device tensor is taken as it is) and equals
    ``voxelize_u8`` on those events; ``ds2`` keeps full[.., 1::2, 1::2].  ``dropped`` counts the events outside [0,W) x [0,H), which are
    skipped.  3 * ceil(n_win / ws_windows) enqueues (``ws_windows`` None: ``ingest_ws_windows``)."""
    _ck(records_u8, torch.uint8, 'records')
    if records_u8.numel() % 8:
        raise LeodHipError(f'records: {records_u8.numel()} bytes are no whole number of 8-byte events')
    if ds2 and (height % 2 or width % 2):
        raise LeodHipError(f'ds2 needs an even height and width, got {height} x {width}')
    dev = records_u8.device
    n_events = records_u8.numel() // 8
    if not (isinstance(win_off, torch.Tensor) and win_off.is_cuda):
        off = torch.as_tensor(win_off, dtype=torch.int64).reshape(-1)
        if off.numel() < 1 or int(off[0]) < 0 or int(off[-1]) > n_events or bool((off[1:] < off[:-1]).any()):
            raise LeodHipError('win_off: ascending offsets within [0, n_events] expected')
        win_off = off.to(dev)
    _ck(win_off, torch.int64, 'win_off')
    n_win = win_off.numel() - 1
    Ho, Wo = (height // 2, width // 2) if ds2 else (height, width)
    ws_windows = ingest_ws_windows(bins, height, width, ds2) if ws_windows is None else int(ws_windows)
    ws_windows = max(1, min(ws_windows, max(n_win, 1)))
    ws = torch.empty((ws_windows * 2 * bins * Ho * Wo,), dtype=torch.int32, device=dev)
    out = torch.empty((n_win, 2 * bins, Ho, Wo), dtype=torch.uint8, device=dev)
    dropped = torch.zeros((1,), dtype=torch.int64, device=dev)
    check(_l().leod_voxelize_dat_windows(_p(records_u8), n_events, _p(win_off), n_win, _p(ws), ws_windows, _p(out), bins, height, width,
                                          1 if ds2 else 0, 0 if count_cutoff is None else int(count_cutoff), 1 if fastmode else 0,
                                          _p(dropped), _stream()), 'voxelize_dat_windows')
    return out, dropped


EVT_FORMATS = {'evt2': 2, 'evt3': 3, 2: 2, 3: 3}
EVT_WORD_BYTES = {2: 4, 3: 2}
EVT_STATE_LONGS = 16
_EVT_COUNTERS = dict(events=8, early_events=9, ignored_words=10, unknown_words=11, overflow=12, wraps=2)


def evt_query(n_words: int = 0):
    """(words per tile, tile summaries per pass of the scan workgroup, workspace bytes for a chunk of ``n_words`` words): the decoder's own
    constants (csrc/k_evt.hip)."""
    tw, tp, ws = (ctypes.c_int * 1)(), (ctypes.c_int * 1)(), (ctypes.c_long * 1)()
    check(_l().leod_evt_query(int(n_words), tw, tp, ws), 'evt_query')
    return int(tw[0]), int(tp[0]), int(ws[0])


def decode_evt(words_u8, fmt, state=None, out=None):
    """A chunk of a Metavision RAW payload on the device (uint8, as it lies in the file: EVT2 u32 words or EVT3 u16 words, whole words)
    -> (records uint8 [n, 8], state).  The records are those of a .dat file (``voxelize_dat_windows`` reads them), in stream order.
    ``state`` (int64 [16] on the device, layout in include/leod_hip.h) carries the decoder from chunk to chunk: None starts a recording;
    the given tensor is not modified, the returned one is new.  ``out``: a contiguous device uint8 buffer to store the records in; it must
    hold them all (its first n * 8 bytes are returned as the view [n, 8], nothing behind them is written).  Three launches and one
    read-back (the chunk's event count)."""
    if fmt not in EVT_FORMATS or isinstance(fmt, bool):
        raise LeodHipError(f'encoding {fmt!r}: evt2 or evt3 expected')
    fmt = EVT_FORMATS[fmt]
    _ck(words_u8, torch.uint8, 'words')
    if words_u8.numel() % EVT_WORD_BYTES[fmt]:
        raise LeodHipError(f'words: {words_u8.numel()} bytes are no whole number of {EVT_WORD_BYTES[fmt]}-byte words')
    dev = words_u8.device
    if words_u8.data_ptr() % 16:
        words_u8 = words_u8.clone()                              # the kernels load 16 bytes at a time; a fresh allocation is aligned
    n_words = words_u8.numel() // EVT_WORD_BYTES[fmt]
    if state is None:
        state = torch.zeros((EVT_STATE_LONGS,), dtype=torch.int64, device=dev)
    _ck(state, torch.int64, 'state')
    if state.numel() != EVT_STATE_LONGS:
        raise LeodHipError(f'state: {EVT_STATE_LONGS} int64 expected, got {tuple(state.shape)}')
    ws_bytes = evt_query(n_words)[2]
    ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.int64, device=dev)
    new = torch.empty_like(state)
    check(_l().leod_evt_scan(_p(words_u8), n_words, fmt, _p(state), _p(new), _p(ws), ws_bytes, _stream()), 'decode_evt (scan)')
    n = int(new[14].item())
    buf = _records_out(out, n, dev, 'records of the chunk')
    check(_l().leod_evt_emit(_p(words_u8), n_words, fmt, _p(ws), ws_bytes, _p(buf), n, _p(new), _stream()), 'decode_evt (emit)')
    return buf, new


def _records_out(out, n, dev, what):
    """Where an op stores its ``n`` records: a fresh [n, 8], or the first n * 8 bytes of the caller's ``out`` as the view [n, 8]."""
    if out is None:
        return torch.empty((n, 8), dtype=torch.uint8, device=dev)
    _ck(out, torch.uint8, 'out')
    if out.numel() < n * 8:
        raise LeodHipError(f'out: {out.numel()} bytes do not hold the {n} {what}')
    if out.data_ptr() % 8:
        raise LeodHipError('out: an 8-byte aligned buffer expected')
    return out.reshape(-1)[:n * 8].view(n, 8)


def _state_counters(state, table, head=None, noun=None):
    """The counters ``table`` (name -> index) of a state block, one read-back of its first ``head`` words (None: all of it)."""
    _ck(state, torch.int64, 'state')
    if head is not None and state.numel() < head:
        raise LeodHipError(f'state: {noun} state expected, got {tuple(state.shape)}')
    host = state[:head].cpu().tolist()
    return {k: int(host[i]) for k, i in table.items()}


def evt_state_counters(state):
    """The counters of a decoder state (one read-back): events, early_events, ignored_words, unknown_words, overflow, wraps."""
    return _state_counters(state, _EVT_COUNTERS)


EVT_ENC_STATE_LONGS = 32
EVT_ENC_HOLD = 12                # the most events a state holds back: one group of a vector stream
EVT_ENC_FIRST_HIGH_LIMIT = {2: 1 << 27, 3: 4096}
EVT_ENC_PERIOD_LIMIT = 1 << 30
_EVT_ENC_COUNTERS = dict(events=5, words=6, groups=4, vector_groups=7, held=8)


def evt_encode_query(n_events: int = 0, fmt='evt3'):
    """(events per tile, workspace bytes for a chunk of ``n_events`` events, an upper bound of the words ``n_events`` events take in one
    call): the encoder's own constants (csrc/k_evtenc.hip)."""
    if fmt not in EVT_FORMATS or isinstance(fmt, bool):
        raise LeodHipError(f'encoding {fmt!r}: evt2 or evt3 expected')
    te, ws, mw = (ctypes.c_int * 1)(), (ctypes.c_long * 1)(), (ctypes.c_long * 1)()
    check(_l().leod_evtenc_query(int(n_events), EVT_FORMATS[fmt], te, ws, mw), 'evt_encode_query')
    return int(te[0]), int(ws[0]), int(mw[0])


def encode_evt(records_u8, fmt, state=None, final=False, vectors=False, high_period=64, first_time_high=0, out=None):
    """A chunk of .dat records on the device (uint8 [n * 8] or [n, 8], stream order, t non-decreasing) -> (words uint8 [n_words *
    word bytes], state): the next words of the Metavision RAW payload (EVT2 u32 words or EVT3 u16 words, as they lie in a file) that
    ``raw_events.encode_evt2`` / ``encode_evt3`` write for ALL the events of the recording at once, however it is cut into chunks
    (DESIGN.md section 1).  ``state`` (int64 [32] on the device, layout in include/leod_hip.h) carries the encoder from chunk to chunk:
    None starts a recording -- that call writes the opening TIME_HIGH = ``first_time_high`` whatever its events are; the given tensor is
    not modified, the returned one is new.  ``vectors`` (evt3 only), ``high_period`` and ``first_time_high`` must be the same in every
    call of a recording.  With ``vectors`` the last group of a chunk (at most 12 records) is held back in the state until a later event
    closes it; ``final=True`` writes it out (an empty chunk with ``final`` flushes).  ``out``: a contiguous device uint8 buffer to store
    the words in; it must hold them all (its first bytes are returned as a view, nothing behind them is written).  A record with
    x >= 2048 or y >= 2048, which no EVT word holds, raises ``LeodHipError`` naming its position; a chunk whose times decrease --
    against the chunk before, too -- raises ``EventOrderError``.  One memset, two to four launches, one read-back (the new state), one
    launch to emit."""
    if fmt not in EVT_FORMATS or isinstance(fmt, bool):
        raise LeodHipError(f'encoding {fmt!r}: evt2 or evt3 expected')
    fmt = EVT_FORMATS[fmt]
    if vectors not in (False, True) or final not in (False, True):
        raise LeodHipError(f'vectors={vectors!r}, final={final!r}: True or False expected')
    if vectors and fmt != 3:
        raise LeodHipError('vectors: only EVT3 has vector words')
    if isinstance(high_period, bool) or not isinstance(high_period, int) or not 1 <= high_period <= EVT_ENC_PERIOD_LIMIT:
        raise LeodHipError(f'high_period={high_period!r}: an integer in [1, 2^30] expected')
    if isinstance(first_time_high, bool) or not isinstance(first_time_high, int) or not 0 <= first_time_high < EVT_ENC_FIRST_HIGH_LIMIT[fmt]:
        raise LeodHipError(f'first_time_high={first_time_high!r}: an integer in [0, {EVT_ENC_FIRST_HIGH_LIMIT[fmt]}) expected for EVT{fmt}')
    records_u8, n = _ck_records(records_u8)
    dev = records_u8.device
    if state is None:
        state = torch.zeros((EVT_ENC_STATE_LONGS,), dtype=torch.int64, device=dev)
    _ck(state, torch.int64, 'state')
    if state.numel() != EVT_ENC_STATE_LONGS:
        raise LeodHipError(f'state: {EVT_ENC_STATE_LONGS} int64 expected, got {tuple(state.shape)}')
    ws_bytes = evt_encode_query(n, fmt)[1]
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    new = torch.empty_like(state)
    args = (_p(records_u8), n, fmt, int(vectors), int(final), high_period, first_time_high, _p(state))
    check(_l().leod_evtenc_scan(*args, _p(new), _p(ws), ws_bytes, _stream()), 'encode_evt (scan)')
    host = new.cpu().tolist()
    if host[13] >= 0:
        raise EventOrderError(host[13], host[14], host[15])
    if host[11]:
        r = records_u8.reshape(-1, 8)[host[12]].view(torch.int32)[1].item()
        raise LeodHipError(f'records: event {host[12]} of the chunk (event {host[5] - n + host[12]} of the recording) lies at x = {r & 16383}, '
                           f'y = {(r >> 14) & 16383}; an EVT{fmt} word holds 11 bits of each ({host[11]} such records in the chunk)')
    n_words, wb = host[10], EVT_WORD_BYTES[fmt]
    if out is None:
        buf = torch.empty((n_words * wb,), dtype=torch.uint8, device=dev)
    else:
        _ck(out, torch.uint8, 'out')
        if out.numel() < n_words * wb:
            raise LeodHipError(f'out: {out.numel()} bytes do not hold the {n_words} words of the chunk')
        if out.data_ptr() % 4:
            raise LeodHipError('out: a 4-byte aligned buffer expected')
        buf = out.reshape(-1)[:n_words * wb]
    check(_l().leod_evtenc_emit(*args, _p(ws), ws_bytes, _p(buf), n_words, _stream()), 'encode_evt (emit)')
    return buf, new


def evt_encode_counters(state):
    """The counters of an encoder state (one read-back): events taken, words and groups written, vector_groups among them, events held."""
    return _state_counters(state, _EVT_ENC_COUNTERS, EVT_ENC_STATE_LONGS, 'an encoder')


# scratch of one piece of a chunk of ``filter_events`` (the (slot, pixel) table of csrc/k_filter.hip): 64 MiB takes 2^21 records in one
# piece.  Sweep in DESIGN.md section 4 (profiles/r11_a_kbench_filter.txt, SYNTHETIC recording): 1 MiB is 5x slower, 16 MiB 13 %, 32 MiB 5 %;
# 64 MiB is within 4 % of the fastest bound (256 MiB, a whole 64 MiB chunk of records in one piece) at a quarter of its memory
FILTER_WS_BYTES = 64 << 20
FILTER_WS_MIN_BYTES = 8192       # the smallest table that still takes a whole tile of records per piece
FILTER_STATE_HEAD = 8
FILTER_TAU_LIMIT = 1 << 31
_FILTER_COUNTERS = dict(seen=0, kept=1, outside=2, masked=3, unsupported=4)
_LONG_MAX = (1 << 63) - 1


class EventOrderError(LeodHipError):
    """A chunk of records whose times decrease: ``position`` of the first event that is earlier than the one before it (0: earlier than
    the last event of the chunk before), and the two times."""

    def __init__(self, position: int, t_before: int, t_at: int):
        super().__init__(f'records: timestamps decrease at event {position} ({t_before} -> {t_at}); a recording must be sorted in time')
        self.position, self.t_before, self.t_at = position, t_before, t_at


def event_filter_query(n_events: int = 0):
    """(records per tile, tile counts per pass of the scan workgroup, table bytes that take ``n_events`` records in one piece, bytes of
    marks for a chunk of ``n_events``): the filter's own constants (csrc/k_filter.hip)."""
    te, tp, tb, mb = (ctypes.c_int * 1)(), (ctypes.c_int * 1)(), (ctypes.c_long * 1)(), (ctypes.c_long * 1)()
    check(_l().leod_event_filter_query(int(n_events), te, tp, tb, mb), 'event_filter_query')
    return int(te[0]), int(tp[0]), int(tb[0]), int(mb[0])


def _ck_records(records_u8):
    _ck(records_u8, torch.uint8, 'records')
    if records_u8.numel() % 8:
        raise LeodHipError(f'records: {records_u8.numel()} bytes are no whole number of 8-byte events')
    if records_u8.data_ptr() % 8:
        records_u8 = records_u8.clone()                          # the kernels load a record at a time; a fresh allocation is aligned
    n = records_u8.numel() // 8
    if n >= 1 << 31:
        raise LeodHipError(f'records: {n} events in one chunk; at most 2^31 - 1')
    return records_u8, n


def _ck_sensor(height, width):
    for name, v in (('height', height), ('width', width)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 16384:
            raise LeodHipError(f'{name}={v!r}: an integer in [1, 16384] expected')


def _ck_pixel_mask(pixel_mask, height, width):
    if pixel_mask is None:
        return
    if not isinstance(pixel_mask, torch.Tensor) or pixel_mask.dtype not in (torch.uint8, torch.bool):
        raise LeodHipError(f'pixel_mask: a uint8 or bool tensor expected, got {getattr(pixel_mask, "dtype", type(pixel_mask))}')
    _ck(pixel_mask, pixel_mask.dtype, 'pixel_mask')
    if tuple(pixel_mask.shape) != (height, width):
        raise LeodHipError(f'pixel_mask: shape {tuple(pixel_mask.shape)}, the sensor is {(height, width)}')


def _filter_state(state, n_state, height, width):
    """A checked copy of the state block a filter call was given (None: the caller starts a recording with its initial block)."""
    if state is None:
        return None
    _ck(state, torch.int64, 'state')
    if state.numel() != n_state:
        raise LeodHipError(f'state: {n_state} int64 expected for a {height} x {width} sensor, got {tuple(state.shape)}')
    return state.clone()


def _scan_and_emit(name, scan, records_u8, n, marks, marks_bytes, out, emit=None):
    """What both filters do around their scan entry point: the io block (csrc/filter_common.hpp: records emitted, first bad position,
    the two times around it), ``scan(io)``, ONE read-back -- the kept count, or ``EventOrderError`` -- and the emit of the kept records
    (``emit(buf, m)``: an emit entry point of the caller's own; None: ``leod_event_filter_emit``, which copies them unchanged)."""
    io = torch.tensor([0, _LONG_MAX, 0, 0], dtype=torch.int64).to(records_u8.device)
    check(scan(_p(io)), f'{name} (scan)')
    m, bad, t_before, t_at = io.cpu().tolist()
    if bad != _LONG_MAX:
        raise EventOrderError(bad, t_before, t_at)
    buf = _records_out(out, m, records_u8.device, 'records the filter keeps')
    if emit is None:
        check(_l().leod_event_filter_emit(_p(records_u8), n, _p(marks), marks_bytes, _p(buf), m, _stream()), f'{name} (emit)')
    else:
        check(emit(_p(buf), m), f'{name} (emit)')
    return buf


def filter_events(records_u8, height, width, tau_us, state=None, pixel_mask=None, out=None, ws_bytes=None):
    """A chunk of .dat records on the device (uint8 [n * 8] or [n, 8], stream order, t non-decreasing) -> (kept records uint8 [m, 8],
    state) by the rule of DESIGN.md section 1: events outside [0, W) x [0, H) and events on a pixel where ``pixel_mask`` (uint8 or bool
    [H, W] on the device) is non-zero are removed; any other is kept iff an earlier such event lies on one of its 8 neighbours at most
    ``tau_us`` before it (0 <= tau_us < 2^31; None: this third rule is off).  Kept records come out unchanged and in order.
    ``state`` (int64 [8 + H * W] on the device, layout in include/leod_hip.h: five counters, the last time seen, the last time per pixel)
    carries the filter from chunk to chunk: None starts a recording; the given tensor is not modified, the returned one is new.  ``out``:
    a contiguous device uint8 buffer to store the records in; it must hold them all (its first m * 8 bytes are returned as the view
    [m, 8], nothing behind them is written).  A chunk whose times decrease -- against the chunk before, too -- raises
    ``EventOrderError``.  ``ws_bytes`` (None: ``FILTER_WS_BYTES``) bounds the table: a chunk that needs more is cut into pieces that fit,
    which changes nothing but the launches.  One memset and four launches per piece, one launch to emit, one read-back (the kept count)."""
    _ck_sensor(height, width)
    if tau_us is not None and (isinstance(tau_us, bool) or not isinstance(tau_us, int) or not 0 <= tau_us < FILTER_TAU_LIMIT):
        raise LeodHipError(f'tau_us={tau_us!r}: an integer in [0, 2^31) expected (None: bounds and mask only)')
    records_u8, n = _ck_records(records_u8)
    dev = records_u8.device
    _ck_pixel_mask(pixel_mask, height, width)
    n_state = FILTER_STATE_HEAD + height * width
    new = _filter_state(state, n_state, height, width)
    if new is None:
        new = torch.full((n_state,), -1, dtype=torch.int64, device=dev)
        new[:FILTER_STATE_HEAD] = torch.tensor([0, 0, 0, 0, 0, -1, 0, 0], dtype=torch.int64)
    ws_bytes = FILTER_WS_BYTES if ws_bytes is None else int(ws_bytes)
    if ws_bytes < FILTER_WS_MIN_BYTES:
        raise LeodHipError(f'ws_bytes={ws_bytes}: at least {FILTER_WS_MIN_BYTES} expected')
    _, _, table_bytes, marks_bytes = event_filter_query(n)
    table_bytes = min(table_bytes, ws_bytes)
    table = torch.empty((max(table_bytes, 16) // 8,), dtype=torch.int64, device=dev)
    marks = torch.empty((max(marks_bytes, 8) // 8,), dtype=torch.int64, device=dev)
    scan = lambda io: _l().leod_event_filter_scan(_p(records_u8), n, height, width, -1 if tau_us is None else tau_us, _p(pixel_mask),      # noqa: E731
                                                  _p(new), _p(table), table_bytes, _p(marks), marks_bytes, io, _stream())
    return _scan_and_emit('filter_events', scan, records_u8, n, marks, marks_bytes, out), new


def event_filter_counters(state):
    """The counters of a filter state (one read-back): seen, kept, outside, masked, unsupported."""
    return _state_counters(state, _FILTER_COUNTERS, FILTER_STATE_HEAD, 'a filter')


# scratch of one piece of a chunk of ``pixel_filter_events`` (keys and indices of the sort of csrc/k_pixfilter.hip, twice, and its digit
# counts: 16.5 bytes a record): 16 MiB takes a million records in one piece.  Sweep in DESIGN.md section 4
# (profiles/r12_a_kbench_pixfilter.txt, SYNTHETIC recording): the fastest of 4, 16, 64 and 256 MiB, which lie within 18 % of each other
PIXFILTER_WS_BYTES = 16 << 20
PIXFILTER_STATE_HEAD = 8
PIXFILTER_PIXEL_LONGS = 4
PIXFILTER_KEEP = dict(first=0, second=1, from_second=2)
_PIXFILTER_COUNTERS = dict(seen=0, kept=1, outside=2, masked=3, flicker=4, burst=5)


def pixel_filter_query(n_events: int, height: int, width: int):
    """(records per tile, tile counts per pass of the scan workgroup, key bits per pass of the sort, workspace bytes that take ``n_events``
    records in one piece, bytes of marks for a chunk of ``n_events``): the per-pixel filter's own constants (csrc/k_pixfilter.hip)."""
    _ck_sensor(height, width)
    te, tp, db = (ctypes.c_int * 1)(), (ctypes.c_int * 1)(), (ctypes.c_int * 1)()
    wb, mb = (ctypes.c_long * 1)(), (ctypes.c_long * 1)()
    check(_l().leod_pixel_filter_query(int(n_events), height, width, te, tp, db, wb, mb), 'pixel_filter_query')
    return int(te[0]), int(tp[0]), int(db[0]), int(wb[0]), int(mb[0])


def _ck_flicker(flicker):
    """None or (p_min_us, p_max_us, lock) -> (p_min, p_max, lock) for the C side (lock 0: off)."""
    if flicker is None:
        return 0, 0, 0
    if not isinstance(flicker, (tuple, list)) or len(flicker) != 3 or \
            any(isinstance(v, bool) or not isinstance(v, int) for v in flicker):
        raise LeodHipError(f'flicker={flicker!r}: None or three integers (p_min_us, p_max_us, lock) expected')
    p_min, p_max, lock = flicker
    if not 1 <= p_min <= p_max < FILTER_TAU_LIMIT:
        raise LeodHipError(f'flicker={flicker!r}: 1 <= p_min_us <= p_max_us < 2^31 expected')
    if not 1 <= lock <= 255:
        raise LeodHipError(f'flicker={flicker!r}: 1 <= lock <= 255 expected')
    return p_min, p_max, lock


def pixel_filter_events(records_u8, height, width, burst_us=None, burst_keep='first', flicker=None, state=None, pixel_mask=None, out=None,
                        ws_bytes=None):
    """A chunk of .dat records on the device (uint8 [n * 8] or [n, 8], stream order, t non-decreasing) -> (kept records uint8 [m, 8],
    state) by the per-pixel rule of DESIGN.md section 1: events outside [0, W) x [0, H) and events on a pixel where ``pixel_mask`` (uint8
    or bool [H, W] on the device) is non-zero are removed and touch no state; any other is a candidate.  ``burst_us`` (0 <= burst_us <
    2^31; None: off): a candidate of the polarity of the candidate before it on its pixel, at most ``burst_us`` behind it, continues that
    one's burst; ``burst_keep`` keeps the 'first' of every burst (trail filter), the 'second' alone, or all 'from_second' on (STC).
    ``flicker`` (None: off; (p_min_us, p_max_us, lock) with 1 <= p_min_us <= p_max_us < 2^31, 1 <= lock <= 255): after ``lock``
    consecutive periods between rising edges of a pixel inside the band, every event of the pixel is removed until a period misses the
    band or an event comes later than p_max_us behind the last edge.  Kept records come out unchanged and in order.
    ``state`` (int64 [8 + 4 * H * W] on the device, layout in include/leod_hip.h: six counters, the last time seen, four words per pixel)
    carries the filter from chunk to chunk: None starts a recording; the given tensor is not modified, the returned one is new.  ``out``:
    a contiguous device uint8 buffer to store the records in; it must hold them all (its first m * 8 bytes are returned as the view
    [m, 8], nothing behind them is written).  A chunk whose times decrease -- against the chunk before, too -- raises
    ``EventOrderError``.  ``ws_bytes`` (None: ``PIXFILTER_WS_BYTES``) bounds the workspace: a chunk that needs more is cut into pieces
    that fit, which changes nothing but the launches.  Per piece four launches and three per pass of the sort, one launch to emit, one
    read-back (the kept count and the order verdict)."""
    _ck_sensor(height, width)
    if burst_us is not None and (isinstance(burst_us, bool) or not isinstance(burst_us, int) or not 0 <= burst_us < FILTER_TAU_LIMIT):
        raise LeodHipError(f'burst_us={burst_us!r}: an integer in [0, 2^31) expected (None: no burst rule)')
    if not isinstance(burst_keep, str) or burst_keep not in PIXFILTER_KEEP:
        raise LeodHipError(f"burst_keep={burst_keep!r}: 'first', 'second' or 'from_second' expected")
    p_min, p_max, lock = _ck_flicker(flicker)
    records_u8, n = _ck_records(records_u8)
    dev = records_u8.device
    _ck_pixel_mask(pixel_mask, height, width)
    new = _filter_state(state, PIXFILTER_STATE_HEAD + PIXFILTER_PIXEL_LONGS * height * width, height, width)
    if new is None:
        new = torch.tensor([-1, -1, 0, 0], dtype=torch.int64, device=dev).repeat(height * width + 2)
        new[:PIXFILTER_STATE_HEAD] = torch.tensor([0, 0, 0, 0, 0, 0, -1, 0], dtype=torch.int64)
    _, _, _, need, marks_bytes = pixel_filter_query(n, height, width)
    least = pixel_filter_query(1, height, width)[3]
    ws_bytes = PIXFILTER_WS_BYTES if ws_bytes is None else int(ws_bytes)
    if ws_bytes < least:
        raise LeodHipError(f'ws_bytes={ws_bytes}: at least {least} (one tile of records) expected')
    ws_bytes = min(need, ws_bytes)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    marks = torch.empty((max(marks_bytes, 8) // 8,), dtype=torch.int64, device=dev)
    scan = lambda io: _l().leod_pixel_filter_scan(_p(records_u8), n, height, width, -1 if burst_us is None else burst_us,                  # noqa: E731
                                                  PIXFILTER_KEEP[burst_keep], p_min, p_max, lock, _p(pixel_mask), _p(new), _p(ws), ws_bytes,
                                                  _p(marks), marks_bytes, io, _stream())
    return _scan_and_emit('pixel_filter_events', scan, records_u8, n, marks, marks_bytes, out), new


def pixel_filter_counters(state):
    """The counters of a per-pixel filter state (one read-back): seen, kept, outside, masked, flicker, burst."""
    return _state_counters(state, _PIXFILTER_COUNTERS, PIXFILTER_STATE_HEAD, 'a per-pixel filter')


# scratch of one piece of a chunk of ``fit_events`` with reduce 'fire': the sort of csrc/pixel_sort.hpp, as for ``pixel_filter_events``
FIT_WS_BYTES = PIXFILTER_WS_BYTES
FIT_STATE_HEAD = 8
FIT_REDUCE = dict(pick=0, sum=1, fire=2)
FIT_MAX_SCALE = 64
FIT_MAX_OFFSET = 16384
FIT_MAX_THRESHOLD = 32767
_FIT_COUNTERS = dict(seen=0, kept=1, outside=2, cropped=3, skipped=4, merged=5)


def _ck_hw(hw, name):
    if not isinstance(hw, (tuple, list)) or len(hw) != 2 or \
            any(isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 16384 for v in hw):
        raise LeodHipError(f'{name}={hw!r}: (height, width), two integers in [1, 16384], expected')
    return int(hw[0]), int(hw[1])


def _ck_reduce(reduce):
    if not isinstance(reduce, str) or reduce not in FIT_REDUCE:
        raise LeodHipError(f"reduce={reduce!r}: 'pick', 'sum' or 'fire' expected")
    return FIT_REDUCE[reduce]


def fit_query(n_events: int, dst_hw, reduce: str = 'fire'):
    """(records per tile, tile counts per pass of the scan workgroup, key bits per pass of the sort, workspace bytes that take ``n_events``
    records in one piece -- 0 for 'pick' and 'sum', which sort nothing -- bytes of marks for a chunk of ``n_events``): the sensor fit's own
    constants (csrc/k_fit.hip)."""
    hd, wd = _ck_hw(dst_hw, 'dst_hw')
    te, tp, db = (ctypes.c_int * 1)(), (ctypes.c_int * 1)(), (ctypes.c_int * 1)()
    wb, mb = (ctypes.c_long * 1)(), (ctypes.c_long * 1)()
    check(_l().leod_event_fit_query(int(n_events), hd, wd, _ck_reduce(reduce), te, tp, db, wb, mb), 'fit_query')
    return int(te[0]), int(tp[0]), int(db[0]), int(wb[0]), int(mb[0])


def fit_events(records_u8, src_hw, dst_hw, orient=0, mirror=False, scale=1, offset=(0, 0), reduce='pick', threshold=None, state=None,
               out=None, ws_bytes=None):
    """A chunk of .dat records on the device (uint8 [n * 8] or [n, 8], stream order, t non-decreasing) of a sensor ``src_hw`` = (Hs, Ws)
    -> (kept records uint8 [m, 8] at the frame geometry ``dst_hw`` = (Hd, Wd), state) by the fit rule of DESIGN.md section 1: events
    outside the source sensor are removed; any other is mirrored (``mirror``), turned by ``orient`` (0, 90, 180 or 270 degrees clockwise),
    scaled by the integer ``scale`` = k (1 <= k <= 64; the cell of (x', y') is (x' // k, y' // k), incomplete edge cells are cropped) and
    placed at ``offset`` = (ox, oy) (|ox|, |oy| <= 16384); events that leave the frame are cropped.  ``reduce``: 'pick' keeps the events
    of the centre pixel of a cell (x' % k == k // 2 and y' % k == k // 2; the others are skipped), 'sum' keeps every event, 'fire'
    integrates and fires per destination pixel: +1 for ON, -1 for OFF, in stream order; the event that brings the accumulator to
    +-``threshold`` (1 <= threshold <= 32767; None: k * k; only with 'fire') is kept and resets it, any other is merged.  A kept record
    keeps t and bits 28-31 and takes (xd, yd); kept records stay in stream order.
    ``state`` (int64 [8 + Hd * Wd] on the device, layout in include/leod_hip.h: six counters, the last time seen, the accumulators)
    carries the fit from chunk to chunk: None starts a recording; the given tensor is not modified, the returned one is new.  ``out``:
    a contiguous device uint8 buffer to store the records in; it must hold them all (its first m * 8 bytes are returned as the view
    [m, 8], nothing behind them is written).  A chunk whose times decrease -- against the chunk before, too -- raises
    ``EventOrderError``.  ``ws_bytes`` (None: ``FIT_WS_BYTES``; only 'fire' has a workspace) bounds it: a chunk that needs more is cut into
    pieces that fit, which changes nothing but the launches.  'pick' / 'sum': two launches; 'fire': per piece four launches and three per
    pass of the sort; one launch to emit, one read-back (the kept count and the order verdict)."""
    hs, ws_ = _ck_hw(src_hw, 'src_hw')
    hd, wd = _ck_hw(dst_hw, 'dst_hw')
    if isinstance(orient, bool) or orient not in (0, 90, 180, 270):
        raise LeodHipError(f'orient={orient!r}: 0, 90, 180 or 270 (degrees clockwise) expected')
    if not isinstance(mirror, bool):
        raise LeodHipError(f'mirror={mirror!r}: True or False expected')
    if isinstance(scale, bool) or not isinstance(scale, int) or not 1 <= scale <= FIT_MAX_SCALE:
        raise LeodHipError(f'scale={scale!r}: an integer in [1, {FIT_MAX_SCALE}] expected')
    if not isinstance(offset, (tuple, list)) or len(offset) != 2 or \
            any(isinstance(v, bool) or not isinstance(v, int) or abs(v) > FIT_MAX_OFFSET for v in offset):
        raise LeodHipError(f'offset={offset!r}: (ox, oy), two integers in [-{FIT_MAX_OFFSET}, {FIT_MAX_OFFSET}], expected')
    red = _ck_reduce(reduce)
    if threshold is not None and reduce != 'fire':
        raise LeodHipError(f"threshold={threshold!r}: only reduce='fire' has a threshold")
    if threshold is None:
        threshold = scale * scale
    if isinstance(threshold, bool) or not isinstance(threshold, int) or not 1 <= threshold <= FIT_MAX_THRESHOLD:
        raise LeodHipError(f'threshold={threshold!r}: an integer in [1, {FIT_MAX_THRESHOLD}] expected')
    records_u8, n = _ck_records(records_u8)
    dev = records_u8.device
    n_state = FIT_STATE_HEAD + hd * wd
    new = _filter_state(state, n_state, hd, wd)
    if new is None:
        new = torch.zeros((n_state,), dtype=torch.int64, device=dev)
        new[6] = -1
    _, _, _, need, marks_bytes = fit_query(n, (hd, wd), reduce)
    ws = None
    if reduce == 'fire':
        least = fit_query(1, (hd, wd), reduce)[3]
        ws_bytes = FIT_WS_BYTES if ws_bytes is None else int(ws_bytes)
        if ws_bytes < least:
            raise LeodHipError(f'ws_bytes={ws_bytes}: at least {least} (one tile of records) expected')
        ws_bytes = min(need, ws_bytes)
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    else:
        ws_bytes = 0
    marks = torch.empty((max(marks_bytes, 8) // 8,), dtype=torch.int64, device=dev)
    geo = (hs, ws_, hd, wd, orient, int(mirror), scale, offset[0], offset[1], red)
    scan = lambda io: _l().leod_event_fit_scan(_p(records_u8), n, *geo, threshold, _p(new), _p(ws), ws_bytes, _p(marks), marks_bytes, io,    # noqa: E731
                                               _stream())
    emit = lambda buf, m: _l().leod_event_fit_emit(_p(records_u8), n, *geo, _p(marks), marks_bytes, buf, m, _stream())                      # noqa: E731
    return _scan_and_emit('fit_events', scan, records_u8, n, marks, marks_bytes, out, emit), new


def fit_counters(state):
    """The counters of a fit state (one read-back): seen, kept, outside, cropped, skipped, merged."""
    return _state_counters(state, _FIT_COUNTERS, FIT_STATE_HEAD, 'a fit')


# the video-to-events simulator (csrc/k_simulate.hip; the rule: DESIGN.md section 1)
SIM_STATE_HEAD = 8
SIM_MAX_FRAMES = 65536           # per call
SIM_LUT_LIMIT = 1 << 24
SIM_MAX_CANDIDATES = 4096        # (max lut - min lut) // min theta: candidates per pixel and interval
SIM_T_LIMIT = 1 << 32            # the .dat clock
SIM_MAX_EVENTS = (1 << 31) - 1   # per piece of a call: the sort's positions
_SIM_COUNTERS = dict(frames=0, kept=1, on=2, off=3, dropped=4, t_last=5)


def simulate_query(n_events: int, height: int, width: int):
    """(pixels per tile -- a lane takes a pixel --, key bits per pass of the sort, int64 words of the state block, int64 words of the count
    block before its per-frame counts, workspace bytes of a call that keeps ``n_events`` events): the simulator's own constants
    (csrc/k_simulate.hip)."""
    tp, db = (ctypes.c_int * 1)(), (ctypes.c_int * 1)()
    sl, cl, wb = (ctypes.c_long * 1)(), (ctypes.c_long * 1)(), (ctypes.c_long * 1)()
    check(_l().leod_simulate_query(int(n_events), int(height), int(width), tp, db, sl, cl, wb), 'simulate_query')
    return int(tp[0]), int(db[0]), int(sl[0]), int(cl[0]), int(wb[0])


def simulate_check(height, width, times_us, lut, theta_on, theta_off, refractory_us=0, t_last=-1):
    """Every limit of the simulator's rule, on the HOST (no device is touched): ``ValueError``, else (times int64
    [n], lut int32 [256], theta_on int32 [H, W], theta_off int32 [H, W]) as numpy arrays.  H, W in [1, 16384] with H * W < 2^30; ``lut``
    256 integers in [0, 2^24); thresholds (an integer, or an integer array [H, W]) >= 1; (max lut - min lut) // the least threshold <=
    4096; ``refractory_us`` in [0, 2^32); ``times_us`` integers in [0, 2^32), strictly increasing and above ``t_last``."""
    import numpy as np
    for name, v in (('height', height), ('width', width)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= 16384:
            raise ValueError(f'{name}={v!r}: an integer in [1, 16384] expected')
    height, width = int(height), int(width)
    if height * width >= 1 << 30:
        raise ValueError(f'{height} x {width} pixels: fewer than 2^30 expected (pixel * 2 + polarity is a 32-bit value of the sort)')

    def ints(v, name, shape):
        if isinstance(v, torch.Tensor):
            if v.is_cuda:
                raise ValueError(f'{name}: host data expected (it is checked here, then uploaded), got a tensor on {v.device}')
            v = v.numpy()
        a = np.asarray(v)
        if a.size == 0 and shape is None:
            a = a.astype(np.int64)                               # an empty list has no type of its own
        if a.dtype == np.bool_ or a.dtype.kind not in 'iu':
            raise ValueError(f'{name}: integers expected, got {a.dtype}')
        if shape is not None and a.ndim == 0:
            a = np.full(shape, a)
        if shape is not None and a.shape != shape:
            raise ValueError(f'{name}: shape {a.shape}, expected {shape}')
        return a.astype(np.int64)
    lut = ints(lut, 'lut', None).reshape(-1)
    if lut.shape != (256,) or lut.min() < 0 or lut.max() >= SIM_LUT_LIMIT:
        raise ValueError('lut: 256 integers in [0, 2^24) expected')
    th = []
    for name, v in (('theta_on', theta_on), ('theta_off', theta_off)):
        a = ints(v, name, (height, width))
        if a.min() < 1 or a.max() >= 1 << 31:
            raise ValueError(f'{name}: thresholds in [1, 2^31) expected, got [{int(a.min())}, {int(a.max())}]')
        th.append(a)
    least = int(min(th[0].min(), th[1].min()))
    span = int(lut.max() - lut.min())
    if span // least > SIM_MAX_CANDIDATES:
        raise ValueError(f'the table spans {span} and the least threshold is {least}: {span // least} candidates per pixel and interval, '
                         f'at most {SIM_MAX_CANDIDATES}')
    if isinstance(refractory_us, bool) or not isinstance(refractory_us, (int, np.integer)) or not 0 <= refractory_us < SIM_T_LIMIT:
        raise ValueError(f'refractory_us={refractory_us!r}: an integer in [0, 2^32) expected')
    times = ints(times_us, 'times_us', None)
    if times.ndim != 1:
        raise ValueError(f'times_us: a list of integers expected, got shape {times.shape}')
    if len(times):
        if times.min() < 0 or times.max() >= SIM_T_LIMIT:
            raise ValueError('times_us: times in [0, 2^32) expected (the .dat clock)')
        if times[0] <= t_last:
            raise ValueError(f'times_us: the first frame, at {int(times[0])}, is not later than the last frame of the state, at {int(t_last)}')
        step = np.diff(times)
        if len(step) and step.min() <= 0:
            k = int(np.argmax(step <= 0))
            raise ValueError(f'times_us: {int(times[k])} is followed by {int(times[k + 1])}; strictly increasing times expected')
    return times, lut.astype(np.int32), th[0].astype(np.int32), th[1].astype(np.int32)


def simulate_events(frames_u8, times_us, lut, theta_on, theta_off, refractory_us=0, state=None, ws_bytes=None):
    """Luma frames on the device (uint8 [n, H, W]) with their times -> (records uint8 [m, 8], state) by the simulator's rule of DESIGN.md
    section 1: per pixel a reference level m; between two frames the table value ``lut[v]`` moves linearly, and every multiple of the
    pixel's threshold it passes on its way from m is an ON (rising) or OFF (falling) event at the integer time the line reaches it; an
    event less than ``refractory_us`` behind the pixel's last kept one is dropped.  The records are .dat records ordered by time, then
    pixel, then the event's number.  ``times_us``, ``lut``, ``theta_on``, ``theta_off`` are HOST data (lists / numpy / CPU tensors; a
    threshold may be one integer): checked here by ``simulate_check`` (``ValueError``), then uploaded.
    ``state`` (int64 on the device, layout in include/leod_hip.h: the counters, the time of the last frame, {m, t_keep} per pixel, the
    last frame) carries a recording from call to call, with the same table and thresholds: None starts one, whose first frame emits
    nothing; the given tensor is not modified, the returned one is new.  One launch counts, ONE read-back (the kept events per frame, with
    the head of the state) sizes the output and the workspace exactly, then the emit launches.  ``ws_bytes`` (None: no bound) bounds the
    workspace: a call that needs more takes the longest prefix of its frames that fits, then goes on with the rest, which changes nothing
    but the launches; a single frame whose events do not fit raises ``LeodHipError`` naming the bytes it needs."""
    _ck(frames_u8, torch.uint8, 'frames')
    if frames_u8.dim() != 3:
        raise LeodHipError(f'frames: uint8 [n, H, W] expected, got {tuple(frames_u8.shape)}')
    n_frames, height, width = (int(v) for v in frames_u8.shape)
    times, lut, th_on, th_off = simulate_check(height, width, times_us, lut, theta_on, theta_off, refractory_us)
    if len(times) != n_frames:
        raise ValueError(f'times_us: {len(times)} times for {n_frames} frames')
    if n_frames > SIM_MAX_FRAMES:
        raise ValueError(f'{n_frames} frames in one call; at most {SIM_MAX_FRAMES}')
    dev = frames_u8.device
    _, _, n_state, n_count, _ = simulate_query(0, height, width)
    new = _filter_state(state, n_state, height, width)
    if new is None:
        new = torch.zeros((n_state,), dtype=torch.int64, device=dev)
        new[5] = -1
        new[SIM_STATE_HEAD + 1:SIM_STATE_HEAD + 2 * height * width:2] = -1
    if n_frames == 0:
        return torch.empty((0, 8), dtype=torch.uint8, device=dev), new
    d_times, d_lut = torch.from_numpy(times).to(dev), torch.from_numpy(lut).to(dev)
    d_on, d_off = torch.from_numpy(th_on).to(dev), torch.from_numpy(th_off).to(dev)
    counts = torch.empty((n_count + n_frames,), dtype=torch.int64, device=dev)
    refr = int(refractory_us)

    def count(a, b):
        check(_l().leod_simulate_count(_p(frames_u8[a:b]), b - a, height, width, _p(d_times[a:b]), _p(d_lut), _p(d_on), _p(d_off), refr,
                                       _p(new), _p(counts), _stream()), 'simulate_events (count)')
    count(0, n_frames)
    host = torch.cat((new[:SIM_STATE_HEAD], counts[n_count:])).cpu().tolist()                    # the one read-back
    seen, t_last, per = host[0], host[5], host[SIM_STATE_HEAD:]
    if seen > 0 and int(times[0]) <= t_last:
        raise ValueError(f'times_us: the first frame, at {int(times[0])}, is not later than the last frame of the state, at {t_last}')
    limit = None if ws_bytes is None else int(ws_bytes)
    need = lambda n: simulate_query(n, height, width)[4]                                         # noqa: E731
    total = sum(per)
    if total <= SIM_MAX_EVENTS and (limit is None or need(total) <= limit):
        pieces = [(0, n_frames, total)]
    else:
        pieces, a, acc = [], 0, 0
        for k, c in enumerate(per):
            if c > SIM_MAX_EVENTS:
                raise LeodHipError(f'simulate_events: frame {k} alone brings {c} events; at most {SIM_MAX_EVENTS} per interval')
            if limit is not None and need(c) > limit:
                raise LeodHipError(f'simulate_events: ws_bytes={limit}, and the {c} events of frame {k} alone need {need(c)} bytes')
            if k > a and (acc + c > SIM_MAX_EVENTS or (limit is not None and need(acc + c) > limit)):
                pieces.append((a, k, acc))
                a, acc = k, 0
            acc += c
        pieces.append((a, n_frames, acc))
    out = torch.empty((total, 8), dtype=torch.uint8, device=dev)
    at = 0
    for a, b, n in pieces:
        if len(pieces) > 1:
            count(a, b)                                          # the counts of the piece's own frames, from the state as it is now
        t_base = int(times[a - 1]) if a > 0 else (t_last if seen > 0 else int(times[0]))
        nbytes = need(n) if n else 0
        ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev) if n else None
        check(_l().leod_simulate_emit(_p(frames_u8[a:b]), b - a, height, width, _p(d_times[a:b]), _p(d_lut), _p(d_on), _p(d_off), refr,
                                      _p(new), _p(counts), t_base, int(times[b - 1]), n, _p(ws), nbytes, _p(out[at:at + n]) if n else None,
                                      n, _stream()), 'simulate_events (emit)')
        at += n
    return out, new


def simulate_counters(state):
    """The counters of a simulator state (one read-back): frames, kept, on, off, dropped, t_last."""
    return _state_counters(state, _SIM_COUNTERS, SIM_STATE_HEAD, 'a simulator')


# scratch of one piece of a chunk of ``survey_events``: the sort of csrc/pixel_sort.hpp, as for ``pixel_filter_events``
SURVEY_WS_BYTES = PIXFILTER_WS_BYTES
SURVEY_STATE_HEAD = 8
SURVEY_PIXEL_LONGS = 4
SURVEY_MAX_EDGES = 64
SURVEY_RUN_BINS = 256
_SURVEY_HEAD = dict(seen=0, candidates=1, outside=2, masked=3, t_first=4, t_last=5)


def _ck_edges(edges_us):
    """A strictly increasing list of 1 to 64 integers in [0, 2^31) -> the list."""
    try:
        edges = list(edges_us)
    except TypeError:
        raise LeodHipError(f'edges_us={edges_us!r}: a list of integers expected') from None
    if not 1 <= len(edges) <= SURVEY_MAX_EDGES:
        raise LeodHipError(f'edges_us: {len(edges)} edges; 1 to {SURVEY_MAX_EDGES} expected')
    for e in edges:
        if isinstance(e, bool) or not isinstance(e, int) or not 0 <= e < FILTER_TAU_LIMIT:
            raise LeodHipError(f'edges_us: {e!r}; integers in [0, 2^31) expected')
    for a, b in zip(edges[:-1], edges[1:]):
        if not a < b:
            raise LeodHipError(f'edges_us: {a} is followed by {b}; a strictly increasing list expected')
    return edges


def survey_query(n_events: int, height: int, width: int, n_edges: int):
    """(records per tile of the sort, key bits per pass of the sort, workspace bytes that take ``n_events`` records in one piece, int64
    words of the state block): the survey's own constants (csrc/k_survey.hip)."""
    _ck_sensor(height, width)
    te, db, wb, sl = (ctypes.c_int * 1)(), (ctypes.c_int * 1)(), (ctypes.c_long * 1)(), (ctypes.c_long * 1)()
    check(_l().leod_survey_query(int(n_events), height, width, int(n_edges), te, db, wb, sl), 'survey_query')
    return int(te[0]), int(db[0]), int(wb[0]), int(sl[0])


def survey_events(records_u8, height, width, edges_us, flicker=None, state=None, pixel_mask=None, ws_bytes=None):
    """A chunk of .dat records on the device (uint8 [n * 8] or [n, 8], stream order, t non-decreasing) -> the survey state with the chunk
    added: nothing is filtered; the interval each filter's rule looks at is binned by ``edges_us`` (1 to 64 strictly
    increasing integers in [0, 2^31); bin(d) = the number of edges < d) into integer histograms, from which ``survey_counters`` and
    ``data.utils.event_filter.survey_responses`` give the exact count each filter would remove at every edge.  Events outside
    [0, W) x [0, H) and events on a pixel where ``pixel_mask`` (uint8 or bool [H, W] on the device) is non-zero are counted and touch
    nothing else.  ``flicker`` (None: the histogram ``run`` stays empty; (p_min_us, p_max_us) as ``event_filter.flicker_band`` makes it,
    1 <= p_min_us <= p_max_us < 2^31): the band of the anti-flicker rule.
    ``state`` (int64 on the device, layout in include/leod_hip.h: the head, the histograms, four words per pixel) carries the survey from
    chunk to chunk, with the same edges and band: None starts a recording; the given tensor is not modified, the returned one is new.  A
    chunk whose times decrease -- against the chunk before, too -- raises ``EventOrderError``.  ``ws_bytes`` (None:
    ``SURVEY_WS_BYTES``) bounds the workspace: a chunk that needs more is cut into pieces that fit, which changes nothing but the
    launches.  Per piece four launches and three per pass of the sort; one read-back (the order verdict)."""
    _ck_sensor(height, width)
    edges = _ck_edges(edges_us)
    if flicker is None:
        p_min = p_max = 0
    else:
        if not isinstance(flicker, (tuple, list)) or len(flicker) != 2:
            raise LeodHipError(f'flicker={flicker!r}: None or two integers (p_min_us, p_max_us) expected')
        p_min, p_max, _ = _ck_flicker((flicker[0], flicker[1], 1))
    records_u8, n = _ck_records(records_u8)
    dev = records_u8.device
    _ck_pixel_mask(pixel_mask, height, width)
    K = len(edges)
    _, _, need, n_state = survey_query(n, height, width, K)
    new = _filter_state(state, n_state, height, width)
    if new is None:
        n_hist = n_state - SURVEY_STATE_HEAD - SURVEY_PIXEL_LONGS * height * width
        new = torch.cat([torch.tensor([0, 0, 0, 0, -1, -1, 0, 0], dtype=torch.int64), torch.zeros(n_hist, dtype=torch.int64),
                         torch.tensor([-1, -1, 510, 0], dtype=torch.int64).repeat(height * width)]).to(dev)
    least = survey_query(1, height, width, K)[2]
    ws_bytes = SURVEY_WS_BYTES if ws_bytes is None else int(ws_bytes)
    if ws_bytes < least:
        raise LeodHipError(f'ws_bytes={ws_bytes}: at least {least} (one tile of records) expected')
    ws_bytes = min(need, ws_bytes)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    io = torch.tensor([0, _LONG_MAX, 0, 0], dtype=torch.int64).to(dev)
    check(_l().leod_survey_events(_p(records_u8), n, height, width, _long_array(edges), K, p_min, p_max, _p(pixel_mask), _p(new), _p(ws),
                                  ws_bytes, _p(io), _stream()), 'survey_events')
    _, bad, t_before, t_at = io.cpu().tolist()
    if bad != _LONG_MAX:
        raise EventOrderError(bad, t_before, t_at)
    return new


def survey_counters(state, n_edges):
    """The head and the histograms of a survey state taken with ``n_edges`` edges (one read-back): the integers seen, candidates, outside,
    masked, t_first, t_last, and numpy int64 arrays nb [K + 2], same, sec_on, sec_off, period [K + 1], run [256]."""
    if isinstance(n_edges, bool) or not isinstance(n_edges, int) or not 1 <= n_edges <= SURVEY_MAX_EDGES:
        raise LeodHipError(f'n_edges={n_edges!r}: an integer in [1, {SURVEY_MAX_EDGES}] expected')
    K = n_edges
    sizes = (('nb', K + 2), ('same', K + 1), ('sec_on', K + 1), ('sec_off', K + 1), ('period', K + 1), ('run', SURVEY_RUN_BINS))
    head = SURVEY_STATE_HEAD + sum(s for _, s in sizes)
    _ck(state, torch.int64, 'state')
    if state.numel() < head or (state.numel() - head) % SURVEY_PIXEL_LONGS:
        raise LeodHipError(f'state: a survey state of {n_edges} edges expected, got {tuple(state.shape)}')
    host = state[:head].cpu().numpy()
    out = {k: int(host[i]) for k, i in _SURVEY_HEAD.items()}
    at = SURVEY_STATE_HEAD
    for k, s in sizes:
        out[k] = host[at:at + s].copy()
        at += s
    return out


def event_pixel_counts(records_u8, height, width, counts=None):
    """Events per pixel of a chunk of .dat records on the device, added into ``counts`` (int64 [H, W] on the device; None: a new one of
    zeros) -> (counts, outside): ``outside`` (int64 [1] on the device) is the number of events with x >= W or y >= H, which are skipped.
    One launch, no read-back."""
    _ck_sensor(height, width)
    records_u8, n = _ck_records(records_u8)
    dev = records_u8.device
    if counts is None:
        counts = torch.zeros((height, width), dtype=torch.int64, device=dev)
    _ck(counts, torch.int64, 'counts')
    if tuple(counts.shape) != (height, width):
        raise LeodHipError(f'counts: shape {tuple(counts.shape)}, the sensor is {(height, width)}')
    outside = torch.zeros((1,), dtype=torch.int64, device=dev)
    check(_l().leod_event_pixel_counts(_p(records_u8), n, height, width, _p(counts), _p(outside), _stream()), 'event_pixel_counts')
    return counts, outside


def unpack_frames(blob_u8, slot_off, slot_flags, C, H, W, out=None):
    """Packed event frames (``data/utils/packed.py``) -> dense uint8 [n_slots, C, H, W] in one launch.  ``blob_u8``: device uint8 buffer of
    validated frame blobs; ``slot_off`` device int64 [n_slots]: byte offset (multiple of 16) of the blob each output frame decodes, < 0 for a
    frame of zeros; ``slot_flags`` device int32 [n_slots] or None: bit 0 = channel planes reversed (the time-flipped view).  ``out``: any
    contiguous device uint8 tensor of n_slots*C*H*W elements (e.g. [L, B, C, H, W]); every byte of it is written."""
    _ck(blob_u8, torch.uint8, 'blob')
    _ck(slot_off, torch.int64, 'slot_off')
    _ck(slot_flags, torch.int32, 'slot_flags')
    n_slots = slot_off.numel()
    if slot_flags is not None and slot_flags.numel() != n_slots:
        raise LeodHipError(f'slot_flags: {slot_flags.numel()} entries for {n_slots} slots')
    if min(C, H, W) < 1:
        raise LeodHipError(f'frame shape {(C, H, W)}')
    if out is None:
        out = torch.empty((n_slots, C, H, W), dtype=torch.uint8, device=blob_u8.device)
    else:
        _ck(out, torch.uint8, 'out')
        if out.numel() != n_slots * C * H * W:
            raise LeodHipError(f'out: {tuple(out.shape)} does not hold {n_slots} frames of {(C, H, W)}')
    check(_l().leod_unpack_frames_u8(_p(blob_u8), blob_u8.numel(), _p(slot_off), _p(slot_flags), n_slots, _p(out), C, H, W, _stream()),
          'unpack_frames')
    return out


def pack_frames(frames_u8):
    """Dense uint8 frames [n, C, H, W] on the device -> (blob uint8 [total] on the device, offsets int64 [n + 1] on the host): frame k is
    blob[offsets[k]:offsets[k + 1]], byte for byte what ``packed.encode_frames`` gives.  Count, scan and write passes into a workspace of
    worst-case blobs, ONE read-back (the n sizes), then the compaction."""
    _ck(frames_u8, torch.uint8, 'frames')
    if frames_u8.dim() < 2:
        raise LeodHipError(f'frames: [n, ...] expected, got {tuple(frames_u8.shape)}')
    n = frames_u8.shape[0]
    E = frames_u8.numel() // max(n, 1)
    dev = frames_u8.device
    if n == 0 or E == 0:
        return torch.empty((0,), dtype=torch.uint8, device=dev), torch.zeros((n + 1,), dtype=torch.int64)
    stride = int(_l().leod_pack_frame_stride(E))
    ws = torch.empty((n * stride,), dtype=torch.uint8, device=dev)
    sizes = torch.empty((n,), dtype=torch.int64, device=dev)
    check(_l().leod_pack_frames_u8(_p(frames_u8), n, E, _p(ws), stride, _p(sizes), _stream()), 'pack_frames')
    offsets = torch.zeros((n + 1,), dtype=torch.int64)
    torch.cumsum(sizes.cpu(), 0, out=offsets[1:])
    total = int(offsets[-1])
    blob = torch.empty((total,), dtype=torch.uint8, device=dev)
    check(_l().leod_pack_compact_u8(_p(ws), stride, _p(offsets.to(dev)), n, _p(blob), total, _stream()), 'pack_frames (compaction)')
    return blob, offsets


def mixed_density_i8(x, y, pol, t, bins, height, width, count_cutoff=None):
    """MixedDensityEventStack.construct (data/utils/representations.py:132-221): int64 events sorted in time -> int8 [bins, H, W]."""
    for a in (x, y, pol, t):
        _ck(a, torch.int64, 'events')
    if count_cutoff is not None and not 0 <= int(count_cutoff) <= 127:
        raise ValueError('count_cutoff must lie in [0, 127]')
    dev = x.device
    ws = torch.empty((bins * height * width,), dtype=torch.int32, device=dev)
    out = torch.empty((bins, height, width), dtype=torch.int8, device=dev)
    check(_l().leod_mixed_density_i8(_p(x), _p(y), _p(pol), _p(t), x.numel(), _p(ws), _p(out), bins, height, width,
                                     -1 if count_cutoff is None else int(count_cutoff), _stream()), 'mixed_density_i8')
    return out


# ---------------------------------------------------------------------------------------------------
# prediction-video frames (csrc/k_render.hip)
# ---------------------------------------------------------------------------------------------------
RENDER_RECT, RENDER_TEXT = 0, 1
RENDER_MAX_SCALE = 65536                                     # text scale / rectangle thickness: the limit include/leod_hip.h states (beyond it the kernel draws nothing)


def render_font():
    """The renderer's 5 x 7 font as the library holds it: uint8 numpy array [95, 7], glyphs of ASCII 0x20-0x7E, rows from the top, bit 4 =
    leftmost column."""
    import numpy as np
    buf = (ctypes.c_ubyte * (95 * 7))()
    check(_l().leod_render_font(buf), 'render_font')
    return np.frombuffer(bytes(buf), dtype=np.uint8).reshape(95, 7).copy()


def _render_items(L, frame_off, items, text):
    """Host-side check of the overlay arrays of ``render_frames`` -> (frame_off int32 [L+1], items int32 [n,8], text uint8 [m]) as numpy
    arrays, or (None, None, None) without items.  ValueError on anything the kernel would have to index blindly."""
    import numpy as np
    if items is None or len(items) == 0:
        if frame_off is not None:
            fo = np.asarray(frame_off, dtype=np.int64).reshape(-1)
            if fo.size and (fo[0] != 0 or fo[-1] != 0 or (np.diff(fo) < 0).any()):
                raise ValueError('render_frames: frame_off names items, but there are none')
        return None, None, None
    it = np.asarray(items.cpu() if isinstance(items, torch.Tensor) else items, dtype=np.int64)
    if it.ndim != 2 or it.shape[1] != 8:
        raise ValueError(f'render_frames: items must be [n_items, 8], got {it.shape}')
    if frame_off is None:
        raise ValueError('render_frames: items without frame_off')
    fo = np.asarray(frame_off.cpu() if isinstance(frame_off, torch.Tensor) else frame_off, dtype=np.int64).reshape(-1)
    if fo.size != L + 1:
        raise ValueError(f'render_frames: frame_off must have L + 1 = {L + 1} entries, got {fo.size}')
    if fo[0] != 0:
        raise ValueError(f'render_frames: frame_off[0] must be 0, got {fo[0]}')
    if (np.diff(fo) < 0).any():
        raise ValueError('render_frames: frame_off must be ascending')
    if fo[-1] != len(it):
        raise ValueError(f'render_frames: frame_off[-1] = {fo[-1]} but there are {len(it)} items')
    if np.abs(it).max() >= 2 ** 31:
        raise ValueError('render_frames: an item field does not fit int32')
    if text is None:
        tx = np.zeros((0,), dtype=np.uint8)
    elif isinstance(text, (bytes, bytearray)):
        tx = np.frombuffer(bytes(text), dtype=np.uint8)
    else:
        tx = np.asarray(text.cpu() if isinstance(text, torch.Tensor) else text, dtype=np.uint8).reshape(-1)
    kind = it[:, 1]
    if ((kind != RENDER_RECT) & (kind != RENDER_TEXT)).any():
        raise ValueError('render_frames: item kind must be 0 (rectangle) or 1 (text)')
    rect, txt = it[kind == RENDER_RECT], it[kind == RENDER_TEXT]
    if len(rect) and (rect[:, 6].min() < 1 or rect[:, 6].max() > RENDER_MAX_SCALE):
        raise ValueError(f'render_frames: rectangle thickness must lie in [1, {RENDER_MAX_SCALE}]')
    if len(txt):
        if txt[:, 4].min() < 1 or txt[:, 4].max() > RENDER_MAX_SCALE:
            raise ValueError(f'render_frames: text scale must lie in [1, {RENDER_MAX_SCALE}]')
        if txt[:, 5].min() < 0 or txt[:, 6].min() < 0 or (txt[:, 5] + txt[:, 6]).max() > tx.size:
            raise ValueError(f'render_frames: a text range lies outside the text buffer of {tx.size} bytes')
    return fo.astype(np.int32), np.ascontiguousarray(it.astype(np.int32)), tx


def render_frames(ev, frame_off=None, items=None, text=None, upsample=2, out=None):
    """Event representation [L, 2*bins, H, W] (uint8 or fp32 device tensor) -> RGB frames [L, up*H, up*W, 3] uint8 on the device: pixels
    with events dark on white, bilinear x ``upsample`` (1 or 2), and the overlay ``items`` [n, 8] = {frame, kind, x, y, a, b, c, rgb} of
    ``leod_render_frames_u8`` drawn in the same pass (``frame_off`` [L+1]: each frame's item range, ``text``: the bytes the text items index).
    The overlay arrays are HOST data (lists / numpy / CPU tensors; ``text`` also bytes): checked here (ValueError), then uploaded."""
    import numpy as np
    if ev.dim() != 4:
        raise ValueError(f'render_frames: ev must be [L, 2*bins, H, W], got {tuple(ev.shape)}')
    if upsample not in (1, 2):
        raise ValueError(f'render_frames: upsample must be 1 or 2, got {upsample}')
    L, C2, H, W = ev.shape
    fo, it, tx = _render_items(L, frame_off, items, text)
    if ev.dtype not in (torch.uint8, torch.float32):
        raise LeodHipError(f'render_frames: expected uint8 or float32 events, got {ev.dtype}')
    _ck(ev, ev.dtype, 'ev')
    shape = (L, upsample * H, upsample * W, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=ev.device)
    else:
        _ck(out, torch.uint8, 'out')
        if tuple(out.shape) != shape:
            raise LeodHipError(f'render_frames: out must be {shape}, got {tuple(out.shape)}')
    ws = torch.empty((L * H * W,), dtype=torch.uint8, device=ev.device)
    d_fo = d_it = d_tx = None
    if it is not None:                                          # the three overlay arrays in ONE host -> device copy: frame_off | items | text
        blob = np.concatenate([fo.view(np.uint8), it.reshape(-1).view(np.uint8), tx])
        d_blob = torch.from_numpy(blob).to(ev.device)
        n_fo, n_it = fo.nbytes, it.nbytes
        d_fo, d_it = d_blob[:n_fo].view(torch.int32), d_blob[n_fo:n_fo + n_it].view(torch.int32)
        d_tx = d_blob[n_fo + n_it:] if tx.size else None
    check(_l().leod_render_frames_u8(_p(ev), 1 if ev.dtype is torch.float32 else 0, _p(out), L, C2, H, W, int(upsample), _p(d_fo), _p(d_it),
                                      0 if it is None else len(it), _p(d_tx), 0 if d_tx is None else d_tx.numel(), _p(ws), _stream()),
          'render_frames')
    return out


# ---------------------------------------------------------------------------------------------------
# baseline JPEG of rendered frames (csrc/k_jpeg.hip)
# ---------------------------------------------------------------------------------------------------
JPEG_WS_BYTES = 16 << 20                                     # default workspace bound of encode_jpeg, as in the ingestion ops


def jpeg_query(n: int, height: int, width: int):
    """(workspace bytes for ``n`` frames of height x width, the most bytes their files can take, bytes of a file's header): the
    encoder's own constants (csrc/k_jpeg.hip)."""
    ws, bound, hdr = (ctypes.c_long * 1)(), (ctypes.c_long * 1)(), (ctypes.c_int * 1)()
    check(_l().leod_jpeg_query(int(n), int(height), int(width), ws, bound, hdr), 'jpeg_query')
    return int(ws[0]), int(bound[0]), int(hdr[0])


def encode_jpeg(frames, quality=90, out=None, ws_bytes=None):
    """RGB frames uint8 [N, H, W, 3] on the device (what ``render_frames`` returns; H, W up to 65535) -> (blob, offsets): N complete
    baseline JFIF files back to back in one device uint8 buffer, and int64 [N + 1] on the device with file i at
    blob[offsets[i]:offsets[i + 1]].  The stream is fixed: 4:4:4, IJG tables of ``quality`` 1 .. 100, the standard's
    example Huffman tables, one restart interval per row of blocks.  ``out``: a contiguous device uint8 buffer to store the files in;
    its first offsets[N] bytes are returned as the blob, nothing behind them is written, and a buffer that does not hold them all raises
    ``LeodHipError`` (nothing behind ITS end is written either).  ``ws_bytes`` (None: ``JPEG_WS_BYTES``) bounds the workspace: frames that
    need more are encoded in sub-chunks, each with one read-back (its byte count)."""
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise LeodHipError(f'encode_jpeg: quality must be an integer in 1 .. 100, got {quality!r}')
    quality = int(quality)
    _ck(frames, torch.uint8, 'frames')
    if frames.dim() != 4 or frames.shape[3] != 3 or min(frames.shape) < 1 or max(frames.shape[1:3]) > 65535:
        raise LeodHipError(f'encode_jpeg: frames must be [N, H, W, 3] with N, H, W >= 1 and H, W <= 65535, got {tuple(frames.shape)}')
    N, H, W = (int(s) for s in frames.shape[:3])
    dev = frames.device
    if out is not None:
        _ck(out, torch.uint8, 'out')
        out = out.reshape(-1)
    per_frame = jpeg_query(1, H, W)[0]
    ws_bytes = JPEG_WS_BYTES if ws_bytes is None else int(ws_bytes)
    if ws_bytes < per_frame:
        raise LeodHipError(f'ws_bytes={ws_bytes}: at least {per_frame} (one frame of {H} x {W}) expected')
    step = min(N, ws_bytes // per_frame)
    ws_need = jpeg_query(step, H, W)[0]
    ws = torch.empty((ws_need // 8,), dtype=torch.int64, device=dev)
    offsets = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
    pieces, base = [], 0
    for f0 in range(0, N, step):
        n = min(step, N - f0)
        check(_l().leod_jpeg_scan(_p(frames[f0:f0 + n]), n, H, W, quality, _p(ws), ws_need, _p(offsets[f0:]), base, _stream()),
              'encode_jpeg (scan)')
        end = int(offsets[f0 + n].item())
        if out is None:
            piece = torch.empty((end - base,), dtype=torch.uint8, device=dev)
            pieces.append(piece)
            room = piece
        else:
            if end > out.numel():
                raise LeodHipError(f'out: {out.numel()} bytes do not hold the {end} bytes of the first {f0 + n} files')
            room = out[base:]
        check(_l().leod_jpeg_emit(_p(ws), ws_need, n, H, W, quality, _p(room), room.numel(), base, _stream()), 'encode_jpeg (emit)')
        base = end
    if out is not None:
        return out[:base], offsets
    return (pieces[0] if len(pieces) == 1 else torch.cat(pieces)), offsets


# ---------------------------------------------------------------------------------------------------
# launch plans: a captured hipGraph replayed as plain stream launches (csrc/k_plan.hip)
# ---------------------------------------------------------------------------------------------------
class LaunchPlan:
    """``LaunchPlan(torch.cuda.CUDAGraph(keep_graph=True) after capture)``: ``launch()`` enqueues every kernel / memset / copy of
    the captured work on torch's current stream (lane 0) and on the plan's own side streams (parallel branches of the capture), in one
    C loop.  The CUDAGraph object (it owns the hipGraph whose argument blocks the plan borrows, and the memory pool) is kept alive here."""

    def __init__(self, graph: 'torch.cuda.CUDAGraph', max_lanes: int = 8):
        self.graph = graph
        raw = graph.raw_cuda_graph()
        # weight-pack kernels may leave their captured position only when they write a persistent pack buffer (PackCache)
        rg = PackCache.ranges()
        check(_l().leod_plan_set_hoist_ranges(_long_array([a for a, _ in rg]), _long_array([b for _, b in rg]), len(rg)), 'plan_set_hoist_ranges')
        h = int(_l().leod_plan_create(ctypes.c_void_p(int(raw)), int(max_lanes)))
        if h <= 0:
            raise LeodHipError(f'leod_plan_create: {_l().leod_plan_last_error().decode()} (rc {h})')
        self.handle = h
        info = (ctypes.c_int * 9)()
        check(_l().leod_plan_info(h, info), 'plan_info')
        self.info = dict(zip(('kernels', 'memsets', 'memcpys', 'empty', 'lanes', 'events', 'waits', 'ops', 'collectives'), list(info)))

    def launch(self, join: bool = True):
        """``join=False``: the current stream does not wait for the plan's side lanes (call ``join()`` before the next launch of this plan
        and before anything reads what they wrote)."""
        if join:
            check(_l().leod_plan_launch(self.handle, _stream()), 'plan_launch')
        else:
            check(_l().leod_plan_launch_nojoin(self.handle, _stream()), 'plan_launch_nojoin')

    def join(self):
        check(_l().leod_plan_join(self.handle, _stream()), 'plan_join')

    def rebase_input(self, captured: torch.Tensor, new: torch.Tensor) -> int:
        """Re-point the plan's input-reading kernels (the stem convolution and its weight gradient) from the buffer they were captured with
        to ``new`` (same shape / dtype / layout).  -> number of kernels re-pointed (0: none here)."""
        n = int(_l().leod_plan_rebase_input(self.handle, ctypes.c_void_p(captured.data_ptr()), captured.numel() * captured.element_size(),
                                             ctypes.c_void_p(new.data_ptr())))
        if n < 0:
            raise LeodHipError(f'leod_plan_rebase_input: rc {n}')
        return n

    def dump(self, path: str):
        check(_l().leod_plan_dump(self.handle, path.encode()), 'plan_dump')

    # A plan must not be torn down while a stream capture is open: leod_plan_destroy destroys streams and events, and dropping the CUDAGraph
    # destroys a hipGraph and releases its memory pool -- inside a capture the graph's destructor aborts the process.  close() is also the
    # finaliser, and the cyclic garbage collector runs whenever it likes: in the middle of the capture of a LATER step it finalises the plans
    # of a module that an earlier step dropped.  Such plans are parked here and released when the last open capture has ended.
    _captures_open = 0
    _parked: list = []

    @staticmethod
    def _stream_capturing() -> bool:
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    @classmethod
    def capture_opened(cls):
        cls._captures_open += 1

    @classmethod
    def capture_closed(cls):
        cls._captures_open = max(0, cls._captures_open - 1)
        cls.release_parked()

    @classmethod
    def release_parked(cls):
        if cls._captures_open or not cls._parked or cls._stream_capturing():
            return
        parked, cls._parked = cls._parked, []
        for handle, graph in parked:
            if handle:
                _l().leod_plan_destroy(handle)
            del graph

    def close(self):
        cls = type(self)
        handle, graph = getattr(self, 'handle', 0), getattr(self, 'graph', None)
        self.handle, self.graph = 0, None
        if not handle and graph is None:
            return
        if cls._captures_open or cls._stream_capturing():
            cls._parked.append((handle, graph))
            return
        if handle:
            _l().leod_plan_destroy(handle)
        del graph
        cls.release_parked()

    def __del__(self):
        try:
            self.close()
        except Exception:                                     # interpreter shutdown
            pass

# ---------------------------------------------------------------------------------------------------
# live kernel timing for bench.py's roofline object
# ---------------------------------------------------------------------------------------------------
_PROBE = None


class KernelProbe:
    """Brackets every launch of the probed kernel FAMILIES with HIP events on the launch stream (torch's current stream is
    the stream every leod_* call is enqueued on) and tallies their algorithmic bytes / flops:
    achieved GB/s = sum(bytes) / sum(event time).  Families: ``linear_wgrad`` (the weight-gradient GEMM of the Linear layers -- ``wgrad_wide_bf16_kernel`` and its reduce kernel in precision mode
    bf16, ``wgradw_kernel`` in f32 mode -- the largest
    single kernel family of the training step) and ``linear_gemm`` (forward / dgrad GEMMs of the Linear layers: row-streaming,
    LDS-staged and wide-tile kernels).  With ``families=True`` every C entry point is bracketed as well (``family_ms``): the
    benchmark line then carries its own per-family time table."""

    def __init__(self, targets=('linear_wgrad', 'linear_gemm'), kernel_names=None, families=True):
        global _PROBE, _LIB
        self.targets = tuple(targets)
        self.kernel_names = kernel_names or {'linear_wgrad': 'wgrad_wide_bf16_kernel + wgrad_wide_reduce_kernel (bf16 mode) / wgradw_kernel<.., XRows> (f32 mode)',
                                             'linear_gemm': 'rowstream* / gemm_lds_kernel / gemm_wide_bf16_kernel (Linear forward + dgrad)'}
        self.step = 0                      # index of the probe step being recorded (mark_step() closes one)
        self.events = {t: [] for t in self.targets}     # target -> [(step, e0, e1, bytes, flops, bytes16, rows)]
        self.fam_events = {}               # C entry point -> [(step, e0, e1)]
        self.calls = []                    # (C entry point, small integer arguments, start event, end event, step) in launch order
        self.real_lib = _l()
        if families:
            _LIB = _ProbedLib(self.real_lib, self)
        _PROBE = self

    def mark_step(self):
        """Closes one probe step: figures are medians over the steps recorded (a host stall inside one bracket -- first use of a code
        object, a page fault of the launch thread -- lands in one step's sum and the median drops it)."""
        self.step += 1

    @property
    def steps(self):
        return max(self.step, 1)

    def begin(self, target, nbytes, flops=0.0, rows=None, nbytes16=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.events[target].append((self.step, e0, e1, nbytes, flops, nbytes if nbytes16 is None else nbytes16, rows))
        return e1

    def amend(self, target, nbytes, flops, nbytes16=None):
        """Sets the work of the bracket ``begin`` opened last for ``target`` (the byte count was not known when it was opened)."""
        st, e0, e1, _, _, _, rows = self.events[target][-1]
        self.events[target][-1] = (st, e0, e1, nbytes, flops, nbytes if nbytes16 is None else nbytes16, rows)

    def close(self):
        global _PROBE, _LIB
        _PROBE = None
        _LIB = self.real_lib
        torch.cuda.synchronize()

    @staticmethod
    def _median(v):
        v = sorted(v)
        n = len(v)
        return 0.0 if not n else (v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2]))

    def family_ms(self, steps=None, top=8):
        """{C entry point: ms per step}, largest first: per probe step the sum of the entry point's event brackets, then the MEDIAN over
        the recorded steps (single-stream probe steps)."""
        tot = {}
        for k, v in self.fam_events.items():
            per = [0.0] * self.steps
            for st, a, b in v:
                per[min(st, self.steps - 1)] += a.elapsed_time(b)
            tot[k] = self._median(per)
        return {k: round(v, 3) for k, v in sorted(tot.items(), key=lambda kv: -kv[1])[:top]}

    def call_table(self, step=0):
        """[(C entry point, small integer arguments (shapes / flags), us)] of every bracketed launch of one probe step, in launch order."""
        return [(n, ints, round(1e3 * a.elapsed_time(b), 1)) for n, ints, a, b, st in self.calls if st == step]

    def finish(self, peak_gbs, peak_tflops=157.3, target=None):
        """Roofline object of one probed family.  The bound is chosen by the family's arithmetic intensity
        (sum flops / sum algorithmic bytes) against the ridge peak_tflops / peak_gbs; ``achieved`` is in the unit of that
        bound, the other roof is reported alongside.  Times: the family's summed event brackets of the MEDIAN probe step.
        ``achieved`` / ``frac`` are denominated in SURVEY 8(d)'s bytes (activation and gradient operands once at 2 bytes, parameter
        gradients at 4: ``algorithmic_bytes_16bit_per_launch``); the figure with every operand at its stored width is kept beside it."""
        if _PROBE is self:
            self.close()
        target = target or self.targets[0]
        ev = self.events[target]
        if not ev:
            return None
        per = [0.0] * self.steps
        for e in ev:
            per[min(e[0], self.steps - 1)] += e[1].elapsed_time(e[2])
        ms = self._median(per)                                   # one step's worth of launches
        pick = min(range(self.steps), key=lambda i: (abs(per[i] - ms), i))
        one = [e for e in ev if min(e[0], self.steps - 1) == pick]
        n = len(one)
        stored, flops, nbytes = sum(e[3] for e in one), sum(e[4] for e in one), sum(e[5] for e in one)
        gbs = nbytes / (ms * 1e-3) / 1e9
        tfl = flops / (ms * 1e-3) / 1e12
        ridge = peak_tflops * 1e12 / (peak_gbs * 1e9)
        intensity = flops / max(nbytes, 1.0)
        out = {'kernel': self.kernel_names.get(target, target), 'launches': n, 'probe_steps': self.steps,
               'family_ms_per_probe_step': [round(v, 3) for v in per], 'avg_us': round(1e3 * ms / n, 3),
               'algorithmic_bytes_16bit_per_launch': round(nbytes / n, 1), 'algorithmic_bytes_stored_width_per_launch': round(stored / n, 1),
               'algorithmic_flops_per_launch': round(flops / n, 1),
               'flop_per_byte': round(intensity, 2), 'ridge_flop_per_byte': round(ridge, 2),
               'hbm_achieved_GBs': round(gbs, 2), 'hbm_frac': round(gbs / peak_gbs, 5),
               'hbm_frac_stored_width': round(stored / (ms * 1e-3) / 1e9 / peak_gbs, 5),
               'mfma_achieved_TFLOPs': round(tfl, 2), 'mfma_frac': round(tfl / peak_tflops, 5), 'traffic': None}
        # the same family split by the row count of the launch (= the stage of the backbone): the long row ranges of stages 1-2 are
        # the HBM-bound launches, the short ones of stages 3-4 carry the same flops on 1/4 - 1/16 of the bytes
        rows = sorted({e[6] for e in one if e[6] is not None}, reverse=True)
        if rows:
            split = []
            for r in rows:
                evs = [e for e in one if e[6] == r]
                t = sum(e[1].elapsed_time(e[2]) for e in evs) * 1e-3
                by, fl = sum(e[5] for e in evs), sum(e[4] for e in evs)
                split.append({'rows': int(r), 'launches': len(evs), 'avg_us': round(1e6 * t / len(evs), 1), 'hbm_GBs': round(by / t / 1e9, 1),
                              'hbm_frac': round(by / t / 1e9 / peak_gbs, 4), 'mfma_TFLOPs': round(fl / t / 1e12, 1)})
            out['by_rows'] = split
        if intensity >= ridge:
            out.update(bound='mfma', achieved=round(tfl, 2), peak=peak_tflops, unit='TFLOP/s', frac=round(tfl / peak_tflops, 5))
        else:
            out.update(bound='hbm', achieved=round(gbs, 2), peak=peak_gbs, unit='GB/s', frac=round(gbs / peak_gbs, 5))
        return out


class _ProbedLib:
    """Stand-in for the CDLL while a KernelProbe with ``families=True`` is active: every leod_* launch is bracketed with events."""

    def __init__(self, lib, probe):
        self._lib, self._probe, self._cache = lib, probe, {}

    def __getattr__(self, name):
        fn = self._cache.get(name)
        if fn is None:
            real = getattr(self._lib, name)
            if not name.startswith('leod_') or name.endswith(('_ok', '_mode', '_bytes', '_floats', '_route', 'get_precision', 'set_precision')):
                fn = real
            else:
                probe = self._probe

                def fn(*a, _real=real, _name=name):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rc = _real(*a)
                    e1.record()
                    probe.fam_events.setdefault(_name, []).append((probe.step, e0, e1))
                    probe.calls.append((_name, [x for x in a if isinstance(x, int) and not isinstance(x, bool) and 0 < x < (1 << 24)], e0, e1, probe.step))
                    return rc
            self._cache[name] = fn
        return fn


def _probe(name, nbytes, flops=0.0, rows=None, nbytes16=None):
    """``nbytes``: algorithmic bytes of the launch with every operand at its STORED width; ``nbytes16``: the SURVEY 8(d) figure -- every
    activation / gradient operand once at 2 bytes (the reference's autocast class), parameters and their gradients at 4."""
    if _PROBE is not None and name in _PROBE.targets:
        return _PROBE.begin(name, nbytes, flops, rows, nbytes16)
    return None
