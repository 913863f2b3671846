"""Operands on which the five dense-convolution entry points (csrc/conv_route.hpp: conv_route / launch_conv -- conv_nhwc_fwd, _dgrad, _wgrad,
stem_conv_fwd, _wgrad) have NO rounding error, in any precision mode and any summation order, and the float64 reference of each entry -- so
that tests/test_conv_exact_gpu.py compares for equality.  One missing product, a wrong border tap at one pixel, the halo of image b + 1 read
into the last row of image b, one dropped or doubled pixel row of a weight gradient: each moves an element by at least 1.

* operands: NHWC / NCHW fp32 maps in +-{1,2,3,4}, weights in +-{1,2}, bias integers in [-3, 3], dy in +-{1,2,3}: at most 3 significant
  bits, never zero (a zero operand would hide a dropped contribution).  uint8 stem frames hold integers 0..15, most entries 0, like event
  histograms: 4 bits.  bf16 keeps 8 significant bits and fp16 11, so bf16 / fp16 storage (weight packs, LDS halos, the stem's patch) and
  the rounding of an operand to 16 bits are the identity (``representable``, asserted on every generated operand); every product and partial
  sum is an integer far below 2^24, so fp32 accumulation is exact in every order.
* ``tier`` shrinks the value sets -- first W to +-1, then the map to +-1 as well -- wherever a bound below would otherwise fail.  It only
  chooses (a sum of K independent zero-mean products has standard deviation sqrt(K E[a^2] E[w^2]); ``problem`` steps further down if the
  reference it then computes still misses a bound).  The check is the bounds themselves, asserted by the CPU test and again by the GPU test
  on every row (``bounds``), each < 2^24 = ``LIMIT``:
    fwd, dgrad      K max|a| max|w| (+ 3 for the bias): the worst case of any partial sum of one output element
    dgrad_acc       start value (5) + two calls of it
    wgrad, dbias    start value (5) + two calls of M_out max|dy| max|x|, M_out the pixel rows the gradient contracts over
    stat_sum        rows * max|y_ref|: the column sum of the BatchNorm statistics, and every partial sum of it
    stat_sq         max(y_ref^2) * STAT_ROWS: the fp32 part of the column sum of squares; y_ref^2 < 2^24 is itself exactly representable
  STAT_ROWS = 48 is the largest number of rows any forward kernel adds in fp32 before the sum goes to double: conv3s1_kernel (k_conv3.hip
  line 225, ``cs[n] += v; cq[n] += v * v`` over TW <= 3 row tiles of 4 rows per lane, then quad16_sum over the 4 row groups, line 264:
  3 * 16 rows; TW is set in conv3s1_group_launch, line 806); the GEMM epilogues (gemm16.hpp EpStore::run line 570 and run_rows / stats_tail
  lines 629 - 643) add 4 rows per lane and 4 row groups: 16 rows.  Beyond that the sums are double atomics: exact up to 2^53, whatever the
  order and the number of replicas.  The statistics are therefore compared in float64 (no weaker than a comparison of fp32 casts).
* accumulating outputs (dx with ``accumulate``, dw, dbias) start from non-zero integer patterns (``start_values`` / ``start_vector``).
* the stem reads an NCHW frame stored H x W inside a padded Hp x Wp (the padding exists only as geometry: the kernels must produce its
  zeros themselves).  The ABI takes a bare pointer, so the frame may lie inside a larger buffer: ``frame_buffer`` puts it at an address
  that is or is not a multiple of 4 and fills everything before the first and after the last image with a non-zero sentinel (77 as uint8,
  64.0 as fp32).  One byte of it read as data moves a sum by at least 1.
* references: ``F.conv2d`` and its autograd in float64 on the CPU.  ``conv_taps`` is a second, independent definition -- an explicit loop
  over the taps with shifted slices, forward and both gradients -- which tests/test_conv_exact_cpu.py requires to equal the first for every
  (ks, stride, pad) in use.
* eval-mode BatchNorm + SiLU rows: bn weight in +-{0.5,1,2}, bn bias and running mean integers, running variance in {0.25, 1, 4}; the
  reference is the true float64 formula silu((y - mean) w / sqrt(var + eps) + b) with the eps passed.  fast_exp / fast_rcp and rsqrtf make
  this inexact: it is compared at the fp32 bound of ``close`` in EVERY precision mode (``linear_exact.close_fp32``: rtol 2e-5, floor 2e-6 +
  5e-6 max|ref|) -- the exact convolution underneath is what makes the 16-bit tolerance unnecessary.
* ``problem`` / ``stem_problem`` are cached per shape and shared by the three modes: the precision mode changes formats, never values.

tests/test_conv_exact_cpu.py checks these claims on the generated values themselves."""
import functools

import torch
import torch.nn.functional as F

from linear_exact import _gen, _ints, _pick, _signed, representable, start_values, start_vector  # noqa: F401  (re-exported)

BIAS, COLSTATS, BN, PACK, WS, DBIAS, ACCUMULATE, U8, ALIGN4 = 1, 2, 4, 8, 16, 32, 64, 128, 256       # the flags of leod_conv_route
LIMIT = float(2 ** 24)
STAT_ROWS = 48
MAP, WEIGHT, DY = (1., 2., 3., 4.), (1., 2.), (1., 2., 3.)
U8_MAX, U8_DENSITY = 15, 0.3
SENTINEL_U8, SENTINEL_F32, FRAME_TAIL = 77, 64.0, 64
BN_EPS = 1e-5
START_MAX, START_VEC_MAX, BIAS_MAX = 5.0, 3.0, 3.0


def out_hw(H, W, ks, stride, pad):
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _mean_sq(values):
    return sum(v * v for v in values) / len(values)


def tier(K, rows):
    """how far the value sets shrink: 0 = full sets, 1 = W in +-1, 2 = the map in +-1 as well -- the first at which 6 standard deviations
    of an output element (plus the bias) keep stat_sum and stat_sq below LIMIT.  This only chooses; ``bounds`` on the reference is the check."""
    for t, (a2, w2) in enumerate(((_mean_sq(MAP), _mean_sq(WEIGHT)), (_mean_sq(MAP), 1.0), (1.0, 1.0))):
        y = 6.0 * (K * a2 * w2) ** 0.5 + BIAS_MAX
        if y * y * STAT_ROWS < LIMIT and rows * y < LIMIT:
            return t
    return 2


# ---- the bounds: the worst case of any partial sum, each to stay below LIMIT -----------------------------------------------------------------
def fwd_bound(K, a_max, w_max, bias=False):
    return K * a_max * w_max + (BIAS_MAX if bias else 0.0)


def dgrad_acc_bound(K, dy_max, w_max):
    return START_MAX + 2 * fwd_bound(K, dy_max, w_max)


def wgrad_bound(m_out, dy_max, x_max):
    return START_MAX + 2 * m_out * dy_max * x_max


def stat_sum_bound(rows, y_max):
    return rows * y_max


def stat_sq_bound(y_max):
    return y_max * y_max * STAT_ROWS


def bounds(p):
    """every bound of one problem (conv or stem) as {name: worst case}; each must be < LIMIT"""
    ks2 = p['ks'] * p['ks']
    m_out = p['ref']['y'].numel() // p['N']
    b = dict(fwd=fwd_bound(ks2 * p['Cin'], p['x_max'], p['w_max'], p.get('bias') is not None),
             wgrad=wgrad_bound(m_out, p['dy_max'], p['x_max']))
    if p.get('bias') is not None:
        b['dbias'] = wgrad_bound(m_out, p['dy_max'], p['x_max'])
    if not p['stem']:
        y_max = float(p['ref']['y'].abs().max())
        b.update(dgrad=fwd_bound(ks2 * p['N'], p['dy_max'], p['w_max']), dgrad_acc=dgrad_acc_bound(ks2 * p['N'], p['dy_max'], p['w_max']),
                 stat_sum=stat_sum_bound(m_out, y_max), stat_sq=stat_sq_bound(y_max), y_sq=y_max * y_max)
    return b


# ---- references --------------------------------------------------------------------------------------------------------------------------
def conv_ref(x, w, bias, dy, stride, pad):
    """float64 F.conv2d and its autograd.  x [B,C,H,W], w [N,C,ks,ks], dy [B,N,Ho,Wo] or None -> y, dx, dw, dbias (NCHW, float64)"""
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    bd = bias.double().requires_grad_(True) if bias is not None else None
    y = F.conv2d(xd, wd, bd, stride=stride, padding=pad)
    if dy is None:
        return y.detach(), None, None, None
    y.backward(dy.double())
    return y.detach(), xd.grad, wd.grad, (bd.grad if bd is not None else None)


def conv_taps(x, w, bias, dy, stride, pad):
    """the same four tensors from the definition itself: y[b,n,oy,ox] = bias[n] + sum over taps (ky, kx) and channels c of
    xp[b,c,s oy + ky,s ox + kx] w[n,c,ky,kx] on the zero-padded xp -- one shifted, strided slice per tap; the gradients tap by tap as well"""
    x, w = x.double(), w.double()
    B, C, H, W = x.shape
    N, _, ks, _ = w.shape
    Ho, Wo = out_hw(H, W, ks, stride, pad)
    xp = torch.zeros((B, C, H + 2 * pad, W + 2 * pad), dtype=torch.float64)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    y = torch.zeros((B, N, Ho, Wo), dtype=torch.float64)
    dxp, dw = torch.zeros_like(xp), torch.zeros_like(w)
    for ky in range(ks):
        for kx in range(ks):
            rows, cols = slice(ky, ky + stride * (Ho - 1) + 1, stride), slice(kx, kx + stride * (Wo - 1) + 1, stride)
            y += torch.einsum('bchw,nc->bnhw', xp[:, :, rows, cols], w[:, :, ky, kx])
            if dy is not None:
                dw[:, :, ky, kx] = torch.einsum('bnhw,bchw->nc', dy.double(), xp[:, :, rows, cols])
                dxp[:, :, rows, cols] += torch.einsum('bnhw,nc->bchw', dy.double(), w[:, :, ky, kx])
    if bias is not None:
        y += bias.double().view(1, N, 1, 1)
    if dy is None:
        return y, None, None, None
    return y, dxp[:, :, pad:pad + H, pad:pad + W], dw, (dy.double().sum((0, 2, 3)) if bias is not None else None)


def _accumulated(start, grad):
    """what an accumulating output holds after one and after two calls"""
    return [(start.double() + n * grad).float() for n in (1, 2)]


def _within(p):
    return all(v < LIMIT for v in bounds(p).values())


def _conv_problem(B, H, W, Cin, N, ks, stride, bias, t):
    pad = (ks - 1) // 2
    g = _gen(B * 1000003 + H * 7919 + W * 131 + Cin * 17 + N * 5 + ks * 3 + stride + (11 if bias else 0))
    x = _signed(list(MAP) if t < 2 else [1.], (B, Cin, H, W), g)
    w = _signed(list(WEIGHT) if t == 0 else [1.], (N, Cin, ks, ks), g)
    b = _ints(-3, 3, (N,), g) if bias else None
    Ho, Wo = out_hw(H, W, ks, stride, pad)
    dy = _signed(list(DY), (B, N, Ho, Wo), g)
    y, dx, dw, db = conv_ref(x, w, b, dy, stride, pad)
    yn = nhwc(y)
    rows = yn.reshape(-1, N)
    dx0, dw0, db0 = start_values(B * H * W, Cin, 2).view(B, H, W, Cin), start_values(N, Cin * ks * ks, 1).view(N, Cin, ks, ks), start_vector(N, 3)
    ref = dict(y=yn.float(), s1=rows.sum(0), s2=(rows * rows).sum(0), dx=nhwc(dx).float(), dx_acc=_accumulated(dx0, nhwc(dx)),
               dw=_accumulated(dw0, dw), db=_accumulated(db0, db) if bias else None)
    return dict(stem=False, B=B, H=H, W=W, Cin=Cin, N=N, ks=ks, stride=stride, pad=pad, tier=t, x=nhwc(x), w=w, bias=b, dy=nhwc(dy),
                dx0=dx0, dw0=dw0, db0=db0, x_max=float(MAP[-1] if t < 2 else 1), w_max=float(WEIGHT[-1] if t == 0 else 1), dy_max=float(DY[-1]),
                ref=ref, y64=yn)


@functools.lru_cache(maxsize=6)
def problem(B, H, W, Cin, N, ks, stride, bias=False):
    """CPU operands (fp32, NHWC maps, w [N,Cin,ks,ks]) and the float64 reference of one dense convolution, pad = (ks - 1) // 2.  Computed
    once per shape, shared by the precision modes, never modified.  ``ref``: y, s1 / s2 (float64 column sum and sum of squares of y), dx,
    dx_acc / dw / db (lists: after one and after two accumulating calls from dx0 / dw0 / db0)."""
    pad = (ks - 1) // 2
    Ho, Wo = out_hw(H, W, ks, stride, pad)
    for t in range(tier(ks * ks * Cin, B * Ho * Wo), 3):
        p = _conv_problem(B, H, W, Cin, N, ks, stride, bias, t)
        if _within(p):
            return p
    raise ValueError(f'no value set keeps {(B, H, W, Cin, N, ks, stride)} inside its bounds: {bounds(p)}')


@functools.lru_cache(maxsize=4)
def stem_problem(B, H, W, Cin, N, ks, stride, pad, u8, padded):
    """the stem: x [B,Cin,H,W] NCHW (uint8 0..15 mostly zero, or fp32 +-{1..4}) stored H x W inside the zero frame Hp x Wp = ``padded``
    (None: H x W); ``ref``: y [B,Ho,Wo,N], dw (list: after one and two calls from dw0)"""
    Hp, Wp = padded if padded is not None else (H, W)
    g = _gen(B * 1000003 + H * 7919 + W * 131 + Cin * 17 + N * 5 + ks * 3 + stride + (23 if u8 else 0) + Hp * 29 + Wp * 31)
    if u8:
        x = (torch.randint(1, U8_MAX + 1, (B, Cin, H, W), generator=g) * (torch.rand((B, Cin, H, W), generator=g) < U8_DENSITY)).to(torch.uint8)
    else:
        x = _signed(list(MAP), (B, Cin, H, W), g)
    w = _signed(list(WEIGHT), (N, Cin, ks, ks), g)
    Ho, Wo = out_hw(Hp, Wp, ks, stride, pad)
    dy = _signed(list(DY), (B, N, Ho, Wo), g)
    xp = torch.zeros((B, Cin, Hp, Wp), dtype=torch.float64)
    xp[:, :, :H, :W] = x.double()
    y, _, dw, _ = conv_ref(xp, w, None, dy, stride, pad)
    dw0 = start_values(N, Cin * ks * ks, 4).view(N, Cin, ks, ks)
    return dict(stem=True, B=B, H=H, W=W, Cin=Cin, N=N, ks=ks, stride=stride, pad=pad, padded=(Hp, Wp), x=x, xp=xp, w=w, dy=nhwc(dy), dw0=dw0,
                x_max=float(U8_MAX if u8 else MAP[-1]), w_max=float(WEIGHT[-1]), dy_max=float(DY[-1]),
                ref=dict(y=nhwc(y).float(), dw=_accumulated(dw0, dw)), y64=nhwc(y))


def frame_buffer(x, aligned, device):
    """-> (buffer of bytes, view of it holding x): x copied to an address that is a multiple of 16 (aligned) or of 16 plus 1 (not aligned;
    uint8 frames only), inside a larger buffer whose every other byte belongs to the sentinel"""
    nbytes = x.numel() * x.element_size()
    buf = torch.empty(nbytes + 16 + FRAME_TAIL - nbytes % 4, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 4 == 0 and (aligned or x.dtype is torch.uint8)
    if x.dtype is torch.uint8:
        buf.fill_(SENTINEL_U8)
    else:
        buf.view(torch.float32).fill_(SENTINEL_F32)
    off = (-buf.data_ptr()) % 16 + (0 if aligned else 1)
    view = buf[off:off + nbytes].view(x.dtype).view(x.shape)
    view.copy_(x)
    return buf, view


# ---- eval-mode BatchNorm + SiLU ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def bn_problem(B, H, W, Cin, N, ks, stride):
    """the bias-free ``problem`` of the shape plus folded-BatchNorm parameters and the true float64 value of silu(bn(conv))"""
    p = problem(B, H, W, Cin, N, ks, stride, False)
    g = _gen(N * 977 + Cin * 13 + ks)
    bw, bb, rm, rv = _signed([0.5, 1., 2.], (N,), g), _ints(-3, 3, (N,), g), _ints(-3, 3, (N,), g), _pick([0.25, 1., 4.], (N,), g)
    v = (p['y64'] - rm.double()) * (bw.double() / torch.sqrt(rv.double() + BN_EPS)) + bb.double()
    return dict(p=p, bn=(bw, bb, rm, rv), ref=v * torch.sigmoid(v))
