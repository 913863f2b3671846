"""Operands on which the LayerNorm / LayerScale row kernels of csrc/k_norm.hip (``ln_fwd_kernel``, ``ln_bwd_kernel``, ``ls_bwd_kernel``,
``ls_finalize_kernel``) have no rounding error wherever their arithmetic allows it, and the float64 reference of each -- so that
tests/test_rownorm_exact_gpu.py compares for equality and a row of the second grid-stride pass, a column group of another CJ instantiation
or a row of the ragged last group that goes wrong moves an element by at least 0.5.  These kernels are fp32 in every precision mode.
Built on tests/linear_exact.py.

* rows are ``ln_rows``: integer mean m, values m +- c, c in {0.5, 1, 2}, C / 2 of each sign.  dn, dz, t in +-{1, 2, 3}; w and gamma in
  +-{0.5, 1, 2}; dres small integers; accumulating outputs start from ``start_vector`` / ``start_values``.
* layernorm_bwd with the caller's statistics (integer mean, rstd = 1 / c): xhat = (x - mean) rstd = +-1 exactly.
  dw = dw0 + sum_m dn xhat and db = db0 + sum_m dn are sums of integers of magnitude <= 3 M + 3 < 2^24: exact in every order, equality.
  dx = rstd (g - mean(g) - xhat mean(g xhat)) + dres with g = dn w a multiple of 0.5: the row sums are exact; the kernel divides them by
  (float) C.  C a power of two (256, 512): the means are multiples of 2^-10 below 8 and every later value a multiple of 2^-11 below 2^6 --
  exact; ``dx_fp32`` evaluates the kernel's operation order in fp32 and ``ln_bwd_problem`` records in ``dx_exact`` whether it equals the
  float64 reference (tests/test_rownorm_exact_cpu.py asserts that it does for 256 and 512).  Other C (96, 192, 320, 448): the quotient is
  rounded, ``close_fp32``.
* layernorm_bwd with ``stats = None``: the kernel recomputes (mean, rstd) with eps, xhat is +-1 only up to 1e-5: ``close_fp32`` for dx, dw
  and db against the float64 evaluation with the true statistics.
* layerscale_bwd: dt = gamma dz is one exact product; dgamma = dgamma0 + sum_m dz t, integers of magnitude <= 9 M + 3 < 2^24: equality.
* layernorm_fwd: y and stats are not exact (rsqrt, eps): ``close_fp32`` against ``ln_true``.  The normalised rows are +-ln_w + ln_b up to
  2e-4, never zero, and neighbouring rows differ in mean and c: a wrong row or column is an error of >= 0.5.
* layerscale_finalize: dW = dW0 + gamma G, db = db0 + gamma s, dgamma = dgamma0 + sum_k W G + b s with W, G in +-{1, 2}, b, s small
  integers: multiples of 0.5 below 2^14, equality.

Shapes.  The backward kernels run at most 512 workgroups of 16 rows, the forward 2048: a second grid-stride pass starts at M > 8192 and
M > 32768.  8211 = 512 * 16 + 19: one workgroup and a quarter of the next take a second pass, the last row group holds 3 of 4 rows.
16391: every workgroup takes two or three passes.  32851 = 2048 * 16 + 83 for the forward.  C = 96, 192, 256, 320, 448, 512 instantiate
CJ = 2, 3, 4, 6 (320: 5 -> 6, the last column group entirely out of range), 8 (448: 7 -> 8) and 8; C = 32 is CJ = 1."""
import functools

import torch

from linear_exact import (_ints, _pick, _signed, close_fp32, ln_rows, ln_true, representable, start_values, start_vector)  # noqa: F401

LN_BWD_SHAPES = ((8211, 96), (8211, 192), (8211, 320), (16391, 448), (16391, 256), (3, 256), (20, 512))
LN_FWD_SHAPES = ((32851, 32), (8211, 96), (70, 192), (33, 320), (20, 448))
FINALIZE_SHAPES = ((48, 192), (192, 48), (96, 384), (6, 1536), (5, 260))
HALVES = [0.5, 1., 2.]
DISPATCHED_CJ = (1, 2, 3, 4, 6, 8)


def cj_of(C):
    """the instantiation DISPATCH_CJ picks: column groups of 64, rounded up to 1, 2, 3, 4, 6, 8"""
    n = (C + 63) // 64
    return next(c for c in DISPATCHED_CJ if n <= c)


def passes(M, cap):
    """(fewest, most) grid-stride passes of a wave: at most `cap` workgroups of 4 waves, a wave takes 4 rows per pass"""
    grid = min(cap, max(1, (M + 15) // 16))
    counts = [len(range(4 * v, M, 16 * grid)) for v in range(4 * grid)]
    return min(counts), max(counts)


def _gen(*key):
    seed = 0
    for v in key:
        seed = seed * 1000003 + int(v) + 11
    return torch.Generator().manual_seed(seed % (2 ** 62))


def dx_fp32(p):
    """dx of ln_bwd_kernel with the caller's statistics, in its operation order, fp32 throughout (row sums are exact in any order)"""
    f = torch.float32
    C = p['C']
    mean, rstd = p['stats'][:, :1], p['stats'][:, 1:]
    xh = (p['x'] - mean) * rstd
    g = p['dn'] * p['w']
    cf = torch.tensor(float(C), dtype=f)
    s1 = g.sum(1, keepdim=True, dtype=torch.float64).to(f) / cf
    s2 = (g * xh).sum(1, keepdim=True, dtype=torch.float64).to(f) / cf
    r = ((g - s1) - xh * s2) * rstd
    return r + p['dres'] if p['dres'] is not None else r


@functools.lru_cache(maxsize=None)
def ln_bwd_problem(M, C, with_dres):
    g = _gen(1, M, C, with_dres)
    x, _, _, mean, c, _ = ln_rows(M, C, g)
    w = _signed(HALVES, (C,), g)
    dn = _signed([1., 2., 3.], (M, C), g)
    dres = _ints(-3, 3, (M, C), g) if with_dres else None
    stats = torch.cat([mean, 1.0 / c], 1).contiguous()
    p = dict(M=M, C=C, x=x, w=w, dn=dn, dres=dres, stats=stats, dw0=start_vector(C, 2), db0=start_vector(C, 5))
    d = torch.float64

    def model(mean_, rstd_):
        xh = (x.to(d) - mean_) * rstd_
        gw = dn.to(d) * w.to(d)
        dx = rstd_ * (gw - gw.mean(1, keepdim=True) - xh * (gw * xh).mean(1, keepdim=True))
        if dres is not None:
            dx = dx + dres.to(d)
        return dict(dx=dx, dw=p['dw0'].to(d) + (dn.to(d) * xh).sum(0), db=p['db0'].to(d) + dn.to(d).sum(0))
    p['ref'] = model(mean.to(d), (1.0 / c).to(d))                 # the caller's statistics: exact
    _, tmean, trstd = ln_true(x, torch.ones(C), torch.zeros(C))
    p['true'] = model(tmean, trstd)                               # stats = None: the kernel's own, with eps
    p['reduction_bound'] = 3.0 + float(dn.abs().sum(0).max())
    p['dx_exact'] = bool(C & (C - 1) == 0 and torch.equal(dx_fp32(p).double(), p['ref']['dx']))
    return p


@functools.lru_cache(maxsize=None)
def ls_bwd_problem(M, C):
    g = _gen(2, M, C)
    dz, t, gamma = _signed([1., 2., 3.], (M, C), g), _signed([1., 2., 3.], (M, C), g), _signed(HALVES, (C,), g)
    p = dict(M=M, C=C, dz=dz, t=t, gamma=gamma, dgamma0=start_vector(C, 3))
    p['ref'] = dict(dt=(dz.double() * gamma.double()).float(), dgamma=p['dgamma0'].double() + (dz.double() * t.double()).sum(0))
    p['reduction_bound'] = 3.0 + float((dz * t).abs().sum(0).max())
    return p


@functools.lru_cache(maxsize=None)
def ln_fwd_problem(M, C):
    x, ln_w, ln_b, mean, c, Xn = ln_rows(M, C, _gen(3, M, C))
    y, tmean, trstd = ln_true(x, ln_w, ln_b)
    return dict(M=M, C=C, x=x, w=ln_w, b=ln_b, Xn=Xn, mean=mean, c=c, ref=dict(y=y, stats=torch.cat([tmean, trstd], 1)))


@functools.lru_cache(maxsize=None)
def finalize_problem(N, K):
    g = _gen(4, N, K)
    W, G = _signed([1., 2.], (N, K), g), _signed([1., 2.], (N, K), g)
    b, s, gamma = _ints(-3, 3, (N,), g), _ints(-3, 3, (N,), g), _signed(HALVES, (N,), g)
    p = dict(N=N, K=K, W=W, G=G, b=b, s=s, gamma=gamma, dW0=start_values(N, K, 1), db0=start_vector(N, 2), dgamma0=start_vector(N, 6))
    d = torch.float64
    dot = (W.to(d) * G.to(d)).sum(1)
    p['ref'] = dict(dW=p['dW0'].to(d) + gamma.to(d).view(N, 1) * G.to(d), db=p['db0'].to(d) + gamma.to(d) * s.to(d),
                    dgamma=p['dgamma0'].to(d) + dot + b.to(d) * s.to(d), dgamma_nob=p['dgamma0'].to(d) + dot)
    return p
