"""The LayerNorm / LayerScale row kernels of csrc/k_norm.hip on the operands of tests/rownorm_exact.py: ``layernorm_bwd``, ``layerscale_bwd``
and ``leod_layerscale_finalize`` compared for EQUALITY with the float64 reference wherever their arithmetic is exact, ``layernorm_fwd`` (and
everything behind recomputed statistics) within ``close_fp32``.  The argument is the docstring of tests/rownorm_exact.py;
tests/test_rownorm_exact_cpu.py checks it without a GPU.  The kernels are fp32 in every precision mode: mode f32.

* layernorm_bwd, (M, C) with a second grid-stride pass for some (8211) or all (16391) workgroups, a ragged last row group, and every CJ
  instantiation but 1 (96, 192, 256, 320 -> 6, 448 -> 8, 512), ``dres`` given and None.  Caller's statistics: dw, db equal; dx equal where
  C is a power of two, ``close_fp32`` otherwise (the division by C rounds).  ``stats = None``: ``close_fp32`` for all three;
* layerscale_bwd, same shapes: dt and dgamma equal;
* layernorm_fwd, (32851, 32) for the second pass of its 2048 workgroups: y and stats within ``close_fp32`` of the float64 LayerNorm;
* leod_layerscale_finalize, called as ``ops.layerscale_linear_wgrad`` calls it, on G and s of the test's own: dW, db, dgamma equal, each
  started non-zero; ``b = None`` and ``db = None``.

Outputs that ``ops`` allocates with ``torch.empty`` are preceded by a NaN-filled tensor of the same size, created and freed on the same
stream (``mlp_exact.poison``): best effort against a row never written that the allocator's reuse would hide.
``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_kernels_gpu as tk  # noqa: E402
from test_kernels_gpu import ops  # noqa: E402,F401  (fixture)
import rownorm_exact as rx  # noqa: E402
from mlp_exact import poison  # noqa: E402

F32 = torch.float32


def _dev(t):
    return None if t is None else t.to(tk.DEV)


def _equal(got, want, what):
    got, want = got.detach().cpu().double(), want.double()
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    idx = tuple(bad[0].tolist())
    rows = sorted(set(bad[:, 0].tolist()))[:8] if got.dim() == 2 else '-'
    raise AssertionError(f'{what}: {len(bad)} of {got.numel()} elements differ, first at {idx}: got {float(got[idx])}, want {float(want[idx])}; '
                         f'rows affected {rows}')


@pytest.mark.parametrize('with_dres', [True, False], ids=['dres', 'nodres'])
@pytest.mark.parametrize('M,C', rx.LN_BWD_SHAPES)
def test_layernorm_bwd_exact(ops, M, C, with_dres):
    assert ops.get_precision() == 'f32'
    p = rx.ln_bwd_problem(M, C, with_dres)
    dn, x, w, dres, stats = (_dev(p[k]) for k in ('dn', 'x', 'w', 'dres', 'stats'))
    dw, db = _dev(p['dw0'].clone()), _dev(p['db0'].clone())
    poison(tk.DEV, ((M, C), F32))
    dx = ops.layernorm_bwd(dn, x, stats, w, dres, dw, db)
    r = p['ref']
    _equal(dw, r['dw'], 'dw')
    _equal(db, r['db'], 'db')
    if p['dx_exact']:
        _equal(dx, r['dx'], 'dx')
    else:
        rx.close_fp32(dx, r['dx'], what='dx (C no power of two: the row means are rounded)')
    del dx
    dw, db = _dev(p['dw0'].clone()), _dev(p['db0'].clone())
    poison(tk.DEV, ((M, C), F32))
    dx = ops.layernorm_bwd(dn, x, None, w, dres, dw, db)
    t = p['true']
    rx.close_fp32(dx, t['dx'], what='dx, statistics recomputed')
    rx.close_fp32(dw, t['dw'], what='dw, statistics recomputed')
    rx.close_fp32(db, t['db'], what='db, statistics recomputed')


@pytest.mark.parametrize('M,C', rx.LN_BWD_SHAPES)
def test_layerscale_bwd_exact(ops, M, C):
    p = rx.ls_bwd_problem(M, C)
    dg = _dev(p['dgamma0'].clone())
    poison(tk.DEV, ((M, C), F32))
    dt = ops.layerscale_bwd(_dev(p['dz']), _dev(p['t']), _dev(p['gamma']), dg)
    _equal(dt, p['ref']['dt'], 'dt')
    _equal(dg, p['ref']['dgamma'], 'dgamma')


@pytest.mark.parametrize('want_stats', [True, False], ids=['stats', 'nostats'])
@pytest.mark.parametrize('M,C', rx.LN_FWD_SHAPES)
def test_layernorm_fwd_rows(ops, M, C, want_stats):
    p = rx.ln_fwd_problem(M, C)
    poison(tk.DEV, ((M, C), F32), ((M, 2), F32))
    y, st = ops.layernorm_fwd(_dev(p['x']), _dev(p['w']), _dev(p['b']), want_stats=want_stats)
    rx.close_fp32(y, p['ref']['y'], what='y')
    assert float((y.cpu().double() - p['Xn'].double()).abs().max()) < 0.01, 'a wrong row or column is off by >= 0.5'
    if want_stats:
        assert tuple(st.shape) == (M, 2)
        rx.close_fp32(st, p['ref']['stats'], what='stats')
    else:
        assert st is None


@pytest.mark.parametrize('variant', ['all', 'no_b', 'no_db'])
@pytest.mark.parametrize('N,K', rx.FINALIZE_SHAPES)
def test_layerscale_finalize_exact(ops, N, K, variant):
    p = rx.finalize_problem(N, K)
    W, G, s, gamma = (_dev(p[k]) for k in ('W', 'G', 's', 'gamma'))
    b = None if variant == 'no_b' else _dev(p['b'])
    dW, dg = _dev(p['dW0'].clone()), _dev(p['dgamma0'].clone())
    db = None if variant == 'no_db' else _dev(p['db0'].clone())
    P = ops._p
    ops.check(ops._l().leod_layerscale_finalize(P(W), P(b), P(gamma), P(G), P(s), P(dW), P(db), P(dg), N, K, ops._stream()), 'layerscale_finalize')
    r = p['ref']
    _equal(dW, r['dW'], 'dW')
    _equal(dg, r['dgamma_nob' if variant == 'no_b' else 'dgamma'], 'dgamma')
    if db is not None:
        _equal(db, r['db'], 'db')
