"""The depthwise convolution kernels of csrc/k_dwconv.hip on the operands of tests/dwconv_exact.py: forward (with and without bias), the fold
of the statistics copies for stat_rep 1, 4 and 32, dgrad (plain, and accumulating twice), dw and dbias (accumulating twice) compared for
EQUALITY with the float64 reference; the eval-BatchNorm + SiLU epilogue within ``close_fp32``.  The argument is the docstring of
tests/dwconv_exact.py; tests/test_dwconv_exact_cpu.py checks it without a GPU.  The kernels ignore the precision mode.

Shapes with the padding of the wrappers go through ``ops.conv_nhwc_fwd`` / ``_dgrad`` / ``_wgrad``; an explicit ``pad`` and the refused
arguments go to the raw entries.  Outputs are NaN-filled before the call wherever the caller provides them; dw and dbias lie at the front of
buffers that reach to the end of the last 256-channel tile and whose tail must stay as it was.
``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_kernels_gpu as tk  # noqa: E402
from test_kernels_gpu import ops  # noqa: E402,F401  (fixture)
import dwconv_exact as de  # noqa: E402
from mlp_exact import poison  # noqa: E402

F32, F64 = torch.float32, torch.float64
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _ids(shape):
    return 'x'.join(str(v) for v in shape)


def _dev(t):
    return None if t is None else t.to(tk.DEV)


def same(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.double()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: {len(bad)} of {ref.numel()} elements differ, first at {first}: got {got[first].item()}, exact {ref[first].item()}')


def bounded(p):
    b = de.bounds(p)
    assert all(v < de.LIMIT for v in b.values()), b


def _geom(p):
    return tuple(p[k] for k in ('B', 'H', 'W', 'C', 'ks', 'stride', 'pad'))


def _wrapped(shape):
    return shape[6] is None


def _fwd(ops, shape, p, x, w, bias, colstats=None, bn=None):
    if _wrapped(shape):
        poison(tk.DEV, ((p['B'], p['Ho'], p['Wo'], p['C']), F32))
        return ops.conv_nhwc_fwd(x, w, bias, stride=p['stride'], colstats=colstats, bn=bn, bn_eps=de.BN_EPS)
    P = ops._p
    y = torch.full((p['B'], p['Ho'], p['Wo'], p['C']), float('nan'), device=tk.DEV)
    bn = bn or (None,) * 4
    rep = colstats.shape[0] if colstats is not None else 1
    assert ops._l().leod_dwconv_nhwc_fwd(P(x), P(w), P(bias), P(y), P(colstats), rep, P(bn[0]), P(bn[1]), P(bn[2]), P(bn[3]), de.BN_EPS, *_geom(p),
                                         ops._stream()) == 0
    return y


def _dgrad(ops, shape, p, dy, w, out, accumulate):
    if _wrapped(shape):
        return ops.conv_nhwc_dgrad(dy, w, (p['B'], p['H'], p['W'], p['C']), stride=p['stride'], out=out, accumulate=accumulate)
    P = ops._p
    assert ops._l().leod_dwconv_nhwc_dgrad(P(dy), P(w), P(out), 1 if accumulate else 0, *_geom(p), ops._stream()) == 0
    return out


def _wgrad(ops, shape, p, dy, x, dw, dbias):
    if _wrapped(shape):
        return ops.conv_nhwc_wgrad(dy, x, dw, dbias, stride=p['stride'])
    P = ops._p
    assert ops._l().leod_dwconv_nhwc_wgrad(P(dy), P(x), P(dw), P(dbias), *_geom(p), ops._stream()) == 0


@pytest.mark.parametrize('shape', de.SHAPES, ids=_ids)
def test_dwconv_forward_exact(ops, shape):
    assert ops.get_precision() == 'f32'
    p = de.problem(*shape)
    bounded(p)
    r = p['ref']
    x, w, bias = _dev(p['x']), _dev(p['w']), _dev(p['bias'])
    same(_fwd(ops, shape, p, x, w, bias), r['y'], 'forward')
    same(_fwd(ops, shape, p, x, w, None), r['y_nobias'], 'forward without bias')
    grid = de.flat_grid(de.fwd_items(p))
    for rep in de.STAT_REPS:
        cs = torch.zeros((rep, 2, p['C']), dtype=F64, device=tk.DEV)
        same(_fwd(ops, shape, p, x, w, bias, colstats=cs), r['y'], f'forward with statistics, {rep} copies')
        cs = cs.cpu()
        same(cs.sum(0), r['stats'], f'(sum, sumsq), the fold of {rep} copies')
        live = cs.abs().sum((1, 2)) > 0
        assert bool(live[:min(rep, grid)].all()) and not bool(live[min(rep, grid):].any()), f'copies written: {live.tolist()}, workgroups {grid}'
    cs = torch.zeros((2, p['C']), dtype=F64, device=tk.DEV)                      # a plain [2, C] block is one copy
    _fwd(ops, shape, p, x, w, bias, colstats=cs.view(1, 2, -1) if not _wrapped(shape) else cs)
    same(cs, r['stats'], '(sum, sumsq), one plain block')
    y = _fwd(ops, shape, p, x, w, bias, bn=tuple(_dev(t) for t in p['bn']))
    de.close_fp32(y, r['bn'], what='silu(bn(depthwise conv)), eval mode')


@pytest.mark.parametrize('shape', de.SHAPES, ids=_ids)
def test_dwconv_dgrad_exact(ops, shape):
    p = de.problem(*shape)
    bounded(p)
    dy, w = _dev(p['dy']), _dev(p['w'])
    out = torch.full(tuple(p['x'].shape), float('nan'), device=tk.DEV)
    dx = _dgrad(ops, shape, p, dy, w, out, False)
    same(dx, p['ref']['dx'], 'dx')
    rows, cols = de.unread(p)
    if rows:
        assert bool((dx[:, p['H'] - rows:] == 0).all()), 'input rows that no output reads must be written as zeros'
    if cols:
        assert bool((dx[:, :, p['W'] - cols:] == 0).all()), 'input columns that no output reads must be written as zeros'
    acc = _dev(p['dx0'].clone())
    for calls in (1, 2):
        _dgrad(ops, shape, p, dy, w, acc, True)
        same(acc, de.accumulated(p, 'dx0', 'dx', calls), f'dx accumulated, call {calls}')


@pytest.mark.parametrize('with_dbias', [True, False], ids=['dbias', 'nodbias'])
@pytest.mark.parametrize('shape', de.SHAPES, ids=_ids)
def test_dwconv_wgrad_exact(ops, shape, with_dbias):
    p = de.problem(*shape)
    bounded(p)
    C, ks2 = p['C'], p['ks'] ** 2
    dy, x = _dev(p['dy']), _dev(p['x'])
    dw_buf, db_buf = _dev(de.guarded(p, 'dw0', ks2)), _dev(de.guarded(p, 'db0', 1))
    dw, db = dw_buf[:C * ks2].view(C, 1, p['ks'], p['ks']), db_buf[:C]
    for calls in (1, 2):
        _wgrad(ops, shape, p, dy, x, dw, db if with_dbias else None)
        same(dw, de.accumulated(p, 'dw0', 'dw', calls), f'dw, call {calls}')
        same(db, de.accumulated(p, 'db0', 'dbias', calls) if with_dbias else p['db0'], f'dbias, call {calls}')
    same(dw_buf[C * ks2:], de.guarded(p, 'dw0', ks2)[C * ks2:], 'the buffer behind dw')
    same(db_buf[C:], de.guarded(p, 'db0', 1)[C:], 'the buffer behind dbias')


def test_dwconv_refused_arguments_write_nothing(ops):
    lib, P, st = ops._l(), ops._p, ops._stream()

    def bufs(B, H, W, C, ks, stride, pad):
        """sentinel-filled operands of the geometry, every extent at least 1 and C rounded up to 4: a call that were launched after all
        would stay inside them"""
        Ho, Wo = max((H + 2 * pad - ks) // stride + 1, 1), max((W + 2 * pad - ks) // stride + 1, 1)
        Cb = (C + 3) // 4 * 4
        f = lambda *s: torch.full(s, de.SENTINEL, device=tk.DEV)                                    # noqa: E731
        return dict(x=f(B, H, W, Cb), w=f(Cb, ks * ks), bias=f(Cb), y=f(B, Ho, Wo, Cb), dy=f(B, Ho, Wo, Cb), dx=f(B, H, W, Cb), dw=f(Cb, ks * ks),
                    db=f(Cb), cs=torch.full((4, 2, Cb), de.SENTINEL, dtype=F64, device=tk.DEV), bn=f(4, Cb))

    def fwd(t, g, rep=1, stats=False, bn=False):
        b = [P(t['bn'][k]) if bn else None for k in range(4)]
        return lib.leod_dwconv_nhwc_fwd(P(t['x']), P(t['w']), P(t['bias']), P(t['y']), P(t['cs']) if stats else None, rep, *b, de.BN_EPS, *g, st)

    def all_three(g, want):
        t = bufs(*g)
        assert fwd(t, g) == want, ('fwd', g)
        assert fwd(t, g, 4, stats=True) == want, ('fwd with statistics', g)
        assert lib.leod_dwconv_nhwc_dgrad(P(t['dy']), P(t['w']), P(t['dx']), 0, *g, st) == want, ('dgrad', g)
        assert lib.leod_dwconv_nhwc_wgrad(P(t['dy']), P(t['x']), P(t['dw']), P(t['db']), *g, st) == want, ('wgrad', g)
        return t
    kept = [all_three((1, 6, 6, 6, 3, 1, 1), ERR_ARG),                 # C % 4 != 0
            all_three((1, 20, 20, 8, 16, 1, 8), ERR_ARG),              # ks = 16
            all_three((1, 3, 3, 8, 5, 1, 0), ERR_ARG),                 # ks larger than the padded map
            all_three((1, 3, 3, 8, 4, 2, 0), ERR_ARG),                 # ... by less than the stride: (3 - 4) / 2 truncates to 0
            all_three((1, 3, 9, 8, 5, 2, 0), ERR_ARG)]                 # ... in one direction only
    g = (1, 6, 6, 8, 3, 1, 1)
    t = bufs(*g)
    assert fwd(t, g, 4, stats=True, bn=True) == ERR_ARG                # bn_w together with colstats
    assert fwd(t, g, 3, stats=True) == ERR_ARG                         # stat_rep no power of two
    kept.append(t)
    g = (1, 3, 3, 20484, 3, 1, 1)
    t = bufs(*g)
    assert fwd(t, g, 4, stats=True) == ERR_UNSUPPORTED                 # the statistics partials of 20484 channels do not fit the LDS
    kept.append(t)
    torch.cuda.synchronize()
    for t in kept:
        for name in ('y', 'dx', 'dw', 'db', 'cs'):
            assert bool((t[name] == de.SENTINEL).all()), f'refused call: {name} was written'
    # in range, the same buffers are taken
    g = (1, 6, 6, 8, 3, 1, 1)
    t = bufs(*g)
    assert fwd(t, g, 4, stats=True) == 0 and fwd(t, g, 1, bn=True) == 0
    torch.cuda.synchronize()
