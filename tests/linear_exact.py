"""Operands on which the nine Linear forward / input-gradient entry points (csrc/linear_common.hpp: linear_route / launch_linear) have NO
rounding error, in any precision mode and any summation order, and the float64 reference of each entry -- so that the tests of
tests/test_linear_fwd_routes_gpu.py compare for equality.  One misplaced row or column, a slab offset by one, a padding column read as data:
each moves an element by at least 0.5.

* plain rows: A (x, a, dy) in +-{1,2,3,4} / +-{1,2,3}, W in +-{1,2}, bias and res small integers, gamma and kscale in +-{0.5,1,2}.  At most
  3 significant bits per operand: bf16 / fp16 storage and the rounding of an operand (dy kscale included) to 16 bits are the identity;
  every product and partial sum is an integer or half-integer far below 2^24, so fp32 accumulation is exact in every order, and so is
  ``res + gamma (t + bias)``.
* 16-bit stored outputs (u16 of entry 2, out16 of entry 3, bf16 dx of entries 6 / 8): the value sets shrink with the contraction length
  (``tier``) until the reference is representable -- bf16 holds integers up to 256 and half-integers up to 128, fp16 integers up to 2048.
  ``representable`` is asserted on every such reference, by the CPU test and again by the GPU test.
* LayerNorm on load (entries 0, 2, 3): the kernels derive (mean, rstd) themselves.  Row values are m +- c with an integer mean m in [-2, 2],
  c in {0.5, 1, 2} and exactly K / 2 of each sign: variance c^2, rstd = 1 / sqrt(c^2 + eps).  ln_w in {+-1, +-2}, ln_b in {-1, 0, 1, 2}; a
  column where one sign would give +-ln_w + ln_b == 0 carries the other sign in every row.  In the 16-bit modes the normalised operand is
  rounded to bf16 / fp16 before the MFMA: the few ulp of mean and rstd and the 1e-5 of eps lie far below half an ulp of a 3-bit value, so the
  operand IS the integer +-ln_w + ln_b and the outputs are compared for equality.  In mode f32 nothing absorbs that error: the float64
  reference of the true LayerNorm (``ln_true``) and the fp32 bound of tests/test_kernels_gpu.py (``close_fp32``).
* GELU written by the kernel (out_act of entry 0): the bias lifts every pre-activation to an integer >= 8, where common.hpp's normal_cdf
  returns exactly 1.0f: gelu(out) == out bit for bit.
* GELU / GELU' on load (entries 5, 8, aux_u of entry 6): u in {8,10,12,14,16}: gelu(u) == u, gelu'(u) == 1.0f.  The masked variant draws u
  from +-{8..16}: for u <= -8 both functions are below 1e-12 in magnitude but not zero, so the result is the reference (which takes them as 0)
  up to 1e-9 -- and a wrong aux index moves it by >= 0.5.  Entry 5 feeds gelu(u) to the MFMA as an operand: only fp16 rounds gelu(u <= -8) to
  an exact zero, so its masked rows are rows of mode 16f (in entries 6 and 8 gelu' multiplies the finished sum: every mode).
* reductions over M (colsum of entry 6, dgamma / dbeta of entry 7): dy, W in +-1; ``reduction_bound`` is the worst case of every partial sum
  in units of its smallest step and must stay below 2^24.  Accumulating outputs start from non-zero integers.
* entry 7 divides by K in its epilogue and cannot be exact; dn = dy W is.  The statistics are the caller's: integer mean, rstd in {0.5,1,2},
  x - mean = +-0.5 (|xhat| <= 1).  Compared at the fp32 bounds of test_linear_dgrad_ln_bwd in every mode.

tests/test_linear_exact_cpu.py checks these claims on the generated values themselves."""
import functools

import numpy as np
import torch

LN, STATS, KSCALE, AUX, TOUT, DX2, COLSUM, ACCUMULATE, DRES = 1, 2, 4, 8, 16, 32, 64, 128, 256   # the flags of leod_linear_route
MASKED = 1024                   # test-only bit of a row's flags: the GELU / GELU' operand u takes both signs; not passed to the library
ABI_FLAGS = 511
PAD_VALUE = 64.0                # padding columns of strided buffers: representable in every format, and one read as data moves a sum by >= 64
EPS = 1e-5
U_VALUES = (8., 10., 12., 14., 16.)
MASK_TOL = 1e-9                 # |gelu(u)|, |gelu'(u)| < 1e-12 for u <= -8, times an exact result below 1e3
BF16_INT, BF16_HALF, F16_INT = 256.0, 128.0, 2048.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pick(values, shape, g):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g).float() * 2 - 1


def _signed(mags, shape, g):
    return _pick(mags, shape, g) * _signs(shape, g)


def _ints(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def start_values(M, C, salt=0):
    """accumulating outputs never start at zero: a non-zero integer pattern in [-5, 5]"""
    m, c = torch.arange(M).view(M, 1), torch.arange(C).view(1, C)
    return ((m * 7 + c * 3 + salt) % 11 - 5).float()


def start_vector(C, salt=0):
    return ((torch.arange(C) * 5 + salt) % 7 - 3).float()


def padded(t, pad):
    """[M, C] -> ([M, C + pad] buffer whose extra columns hold PAD_VALUE, its row stride)"""
    if pad == 0:
        return t.contiguous(), t.shape[1]
    buf = torch.full((t.shape[0], t.shape[1] + pad), PAD_VALUE, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf, t.shape[1] + pad


def representable(t, dtype):
    return torch.equal(t.to(dtype).float(), t.float())


def close_fp32(a, b, rtol=2e-5, atol=2e-6, what=''):
    """the fp32 branch of ``close`` of tests/test_kernels_gpu.py, whatever the precision mode: |a - b| <= atol + 5e-6 max|b| + rtol |b|"""
    a, b = np.asarray(a.detach().double().cpu()), np.asarray(b.detach().double().cpu())
    scale = float(np.abs(b).max()) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol + 5e-6 * scale if atol > 0 else 0, err_msg=what)


def tier(kc, limit, a_sq, w_sq, extra_sq=1.0):
    """how far the value sets shrink for a 16-bit stored output: 0 = full sets, 1 = W in +-1, 2 = A in +-1 as well.  A sum of kc independent
    zero-mean products has standard deviation sqrt(kc E[a^2] E[w^2]); 10 of them (plus the bias) must stay inside ``limit``.  This only
    chooses; ``representable`` on the reference is the check."""
    for t, (a2, w2) in enumerate(((a_sq, w_sq), (a_sq, 1.0), (1.0, 1.0))):
        if 10.0 * (kc * a2 * w2 * extra_sq) ** 0.5 + 4 <= limit:
            return t
    raise ValueError(f'no value set keeps a contraction of {kc} inside {limit}')


def ln_rows(M, K, g):
    """-> x [M,K], ln_w, ln_b, mean [M,1], c [M,1], Xn [M,K] = the exact normalised operand sign * ln_w + ln_b (never 0)"""
    assert K % 2 == 0
    ln_w, ln_b = _pick([1., 2., -1., -2.], (K,), g), _pick([-1., 0., 1., 2.], (K,), g)
    # forced[k] = the sign every row carries in column k because the other one would give a zero operand; 0 = free
    forced = torch.where(ln_w + ln_b == 0, -1.0, 0.0) + torch.where(ln_b - ln_w == 0, 1.0, 0.0)
    for s in (1.0, -1.0):                       # more than K / 2 columns forced to one sign: free the surplus with ln_b = 0
        idx = (forced == s).nonzero().flatten()
        for k in idx[K // 2:].tolist():
            ln_b[k], forced[k] = 0.0, 0.0
    free = (forced == 0).nonzero().flatten()
    n_plus = K // 2 - int((forced == 1).sum())
    assert 0 <= n_plus <= len(free)
    sign = forced.repeat(M, 1)
    order = torch.rand((M, len(free)), generator=g).argsort(1)          # per row: which free columns are +
    sign[:, free] = torch.where(order < n_plus, 1.0, -1.0)
    mean, c = _ints(-2, 2, (M, 1), g), _pick([0.5, 1., 2.], (M, 1), g)
    return sign * c + mean, ln_w, ln_b, mean, c, sign * ln_w + ln_b


def ln_true(x, ln_w, ln_b):
    """float64 LayerNorm as the kernels define it: two-pass mean / variance, rstd = 1 / sqrt(var + eps)"""
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return (xd - mean) * rstd * ln_w.double() + ln_b.double(), mean, rstd


def u_rows(M, C, g, masked):
    u = _pick(list(U_VALUES), (M, C), g)
    return u * _signs((M, C), g) if masked else u


def out16_kind(entry, out16):
    """what a 16-bit stored output of the entry holds: 'f16', 'act16' (bf16, fp16 in mode 16f), 'bf16' or None (fp32)"""
    return 'f16' if entry == 2 else 'act16' if entry == 3 else 'bf16' if out16 else None


@functools.lru_cache(maxsize=4)
def problem(entry, M, N, K, a16=0, out16=0, flags=0, nsplit=0):
    """CPU operands (as the values they hold, fp32; the test stores them in the row's formats) and the float64 reference of one row.  The
    precision mode changes formats only, never values.  Computed once per shape, shared, never modified.
    -> dict: operands by the name of the C parameter; ``ref``: {output name: fp32 tensor, exact}; ``true``: the same from the true LayerNorm
    (mode f32 of LN rows); ``calls``: how often the test calls (2 for accumulating outputs: ref holds a list per call)."""
    g = _gen(entry * 1000003 + M * 7 + N * 131 + K * 17 + a16 + 2 * out16 + flags * 5 + nsplit)
    p = dict(entry=entry, M=M, N=N, K=K, flags=flags, calls=1)
    masked = bool(flags & MASKED)
    kind16 = out16_kind(entry, out16)
    if entry in (0, 2, 3):
        ln = bool(flags & LN)
        limit = {None: None, 'f16': F16_INT, 'act16': BF16_INT}[kind16]
        t = 0 if limit is None else tier(K, limit, 5.5 if ln else 7.5, 2.5)
        W = _signed([1., 2.] if t == 0 else [1.], (N, K), g)
        if ln:
            x, ln_w, ln_b, mean, c, X = ln_rows(M, K, g)
            p.update(ln_w=ln_w, ln_b=ln_b, mean=mean, c=c)
        else:
            x = X = _signed([1., 2., 3., 4.] if t < 2 else [1.], (M, K), g)
        acc = X.double() @ W.double().t()
        if flags & AUX:                         # out_act: every pre-activation an integer >= 8
            bias = (8.0 - acc.min(0).values).float() + (torch.arange(N) % 5).float()
        else:
            bias = _ints(-3, 3, (N,), g)
        out = (acc + bias.double()).float()
        p.update(x=x, X=X, W=W, bias=bias, ref=dict(out=out))
        if flags & AUX:
            p['ref']['out_act'] = out
        if ln:
            tn, tmean, trstd = ln_true(x, ln_w, ln_b)
            tout = tn @ W.double().t() + bias.double()
            p['true'] = dict(out=tout, out_act=tout, mean=tmean.flatten(), rstd=trstd.flatten())
        return p
    if entry in (1, 4, 5):
        W, bias = _signed([1., 2.], (N, K), g), _ints(-3, 3, (N,), g)
        gamma, res = _signed([0.5, 1., 2.], (N,), g), _ints(-3, 3, (M, N), g)
        a = u_rows(M, K, g, masked) if entry == 5 else _signed([1., 2., 3., 4.], (M, K), g)
        A = torch.where(a > 0, a, torch.zeros(())) if entry == 5 else a           # gelu(u): u above 8, 0 below -8
        tt = A.double() @ W.double().t() + bias.double()
        p.update(a=a, A=A, W=W, bias=bias, gamma=gamma, res=res, ref=dict(out=(res.double() + gamma.double() * tt).float()))
        if flags & TOUT:
            p['ref']['tout'] = tt.float()
        return p
    # ---- the dgrads: W [N, K], contraction over N ------------------------------------------------------------------------------------------
    reduces = bool(flags & (COLSUM | ACCUMULATE)) or entry == 7
    ks = _signed([0.5, 1., 2.], (N,), g) if flags & KSCALE else None
    t = 0
    if kind16 is not None:
        t = tier(N, BF16_HALF if ks is not None else BF16_INT, 14.0 / 3, 2.5, 1.75 if ks is not None else 1.0)
    if reduces:
        t = 2
    dy = _signed([1., 2., 3.] if t < 2 else [1.], (M, N), g)
    W = _signed([1., 2.] if t == 0 else [1.], (N, K), g)
    p.update(dy=dy, W=W, kscale=ks, dy_max=3.0 if t < 2 else 1.0, w_max=2.0 if t == 0 else 1.0)
    grad = (dy.double() * (ks.double() if ks is not None else 1.0)) @ W.double()
    if entry == 7:
        d, mean, rstd = _signed([0.5], (M, K), g), _ints(-2, 2, (M, 1), g), _pick([0.5, 1., 2.], (M, 1), g)
        ln_w = _pick([1., 2., -1., -2.], (K,), g)
        dres = _ints(-3, 3, (M, K), g) if flags & DRES else None
        xhat = (d * rstd).double()
        gw = grad * ln_w.double()
        dx = rstd.double() * (gw - gw.mean(1, keepdim=True) - xhat * (gw * xhat).mean(1, keepdim=True))
        if dres is not None:
            dx = dx + dres.double()
        g0, b0 = start_vector(K, 1), start_vector(K, 4)
        p.update(x=d + mean, stats=torch.cat([mean, rstd], 1).contiguous(), ln_w=ln_w, dres=dres, dgamma0=g0, dbeta0=b0, xhat_max=1.0,
                 ref=dict(dn=grad.float()), true=dict(dx=dx, dgamma=g0.double() + (grad * xhat).sum(0), dbeta=b0.double() + grad.sum(0)))
        return p
    if flags & AUX:                             # times gelu'(u): 1 above 8, 0 below -8
        u = u_rows(M, K, g, masked)
        grad = grad * (u > 0).double()
        p['aux_u'] = u
    if flags & DRES:
        p['dres'] = _ints(-3, 3, (M, K), g)
        grad = grad + p['dres'].double()
    if flags & ACCUMULATE:
        p['dx0'], p['calls'] = start_values(M, K), 2
        stored = [p['dx0'].double() + n * grad for n in (1, 2)]
    else:
        stored = [grad]
    if flags & COLSUM:
        p['colsum0'], p['calls'] = start_vector(K, 2), 2
        stored = stored if len(stored) == 2 else stored * 2
        c1 = p['colsum0'].double() + stored[0].sum(0)
        p['ref_colsum'] = [c1.float(), (c1 + stored[1].sum(0)).float()]
    p['ref'] = dict(dx=[s.float() for s in stored])
    return p


def reduction_bound(entry, M, N, K, flags, dy_max=1.0, w_max=1.0):
    """worst case of any partial sum of the row's reductions over M: must be < 2^24.  Where equality is asserted it is counted in units of
    the smallest step (0.5 with kscale) -- dx: N dy W kscale, accumulating: start (5) + 2 calls of it; + dres (3); colsum: start (3) + 2
    calls M max|dx|.
    Entry 7 is compared at a tolerance: M max|dn| max|xhat| + start (3) as it stands (dn <= N, |xhat| <= 1), which keeps the rounding of the
    fp32 sums themselves far inside that tolerance."""
    ks_max, step = (2.0, 0.5) if flags & KSCALE else (1.0, 1.0)
    dn = N * dy_max * w_max * ks_max
    if entry == 7:
        return 3 + M * dn * 1.0
    dx = (5 + 2 * dn if flags & ACCUMULATE else dn) + (3 if flags & DRES else 0)
    return (3 + 2 * M * dx) / step if flags & COLSUM else dx / step
