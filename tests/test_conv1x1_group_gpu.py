"""The grouped 1x1 / stride-1 convolutions (csrc/conv1x1_short.hpp: conv1x1_short_kernel behind leod_conv1x1_group_fwd / _dgrad) on the
exact operands of tests/conv_exact.py: small integers, so that every summation order and every 16-bit operand format gives the same fp32
value -- forward outputs, BatchNorm column statistics and input gradients are compared for EQUALITY with a float64 torch convolution, in
modes bf16 and 16f.

Rows 1, 15, 31, 32, 33: below, at and one past the 32-row tile; 2560 (80 tiles of 32 rows, the short maps of the step) and 8200 (64-row
tiles, a ragged last one).  Contraction lengths 16 (one MFMA step), 48, 192, 384 (bodies with a compile-time K) and 80 (the run-time-K body);
output columns 16, 48, 80 (a partial 48-column tile), 384.  The dgrad of a (Cin -> N) member contracts over N and writes Cin columns, so both
lists are walked in both roles.  Groups: one member, two on one map, three of different rows and K (the head stems), four, accumulation on a
pre-filled buffer, two sharers of one map in two rounds.  One random-data case per direction against the single-call entries at the tolerance
tests/test_kernels_gpu.py applies to them in that mode -- and, stronger, for EQUALITY with them: a group computes bit for bit what its members
compute alone (same operand rounding, same order of the fp32 sums, the four-wave K split of the short maps' single calls included); a refused
group launches nothing; ConvBNFn grouped against ungrouped.
``pytest -m gpu``."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_exact as ce  # noqa: E402
import test_kernels_gpu as tk  # noqa: E402
from test_bf16_gpu import bf16_ops  # noqa: E402,F401  (fixture: both 16-bit modes, with the tolerance of tk.close set to the mode's)

DEV = 'cuda'
MODES_16 = ('bf16', '16f')
MAPS = {1: (1, 1, 1), 15: (1, 3, 5), 31: (1, 1, 31), 32: (2, 4, 4), 33: (1, 3, 11), 2560: (32, 8, 10), 8200: (1, 82, 100)}
KS, NS = (16, 48, 80, 192, 384), (16, 48, 80, 384)
REPLICAS = (1, 8, 32)


@pytest.fixture
def ops16():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops
    prev = ops.get_precision()
    yield ops
    ops.set_precision(prev)


def _problem(rows, cin, n):
    p = ce.problem(*MAPS[rows], cin, n, 1, 1)
    assert all(v < ce.LIMIT for v in ce.bounds(p).values())
    return p


def _gemm_shapes(ps, entry):
    return [(p['B'] * p['H'] * p['W'], p['Cin'], p['N']) if entry == 0 else (p['B'] * p['H'] * p['W'], p['N'], p['Cin']) for p in ps]


def _fwd_equal(ops, ps, reps, xs=None, refs=None):
    """one grouped forward launch of the members -> outputs and statistics equal the float64 reference"""
    xs = xs if xs is not None else [p['x'].to(DEV) for p in ps]
    stats = [torch.zeros((r, 2, p['N']), dtype=torch.float64, device=DEV) for p, r in zip(ps, reps)]
    ys = ops.conv1x1_group_fwd(xs, [p['w'].to(DEV) for p in ps], stats)
    assert ys is not None
    for k, (p, y, st) in enumerate(zip(ps, ys, stats)):
        y64 = refs[k] if refs is not None else p['y64']
        rows = y64.reshape(-1, p['N'])
        assert torch.equal(y.cpu(), y64.float()), f'forward member {k}'
        assert torch.equal(st.sum(0)[0].cpu(), rows.sum(0)) and torch.equal(st.sum(0)[1].cpu(), (rows * rows).sum(0)), f'statistics member {k}'


def _dgrad_equal(ops, ps):
    """written, then accumulated twice onto the non-zero start pattern"""
    dys, ws = [p['dy'].to(DEV) for p in ps], [p['w'].to(DEV) for p in ps]
    outs = [torch.full(tuple(p['x'].shape), 7.0, device=DEV) for p in ps]
    assert ops.conv1x1_group_dgrad(dys, ws, outs, [False] * len(ps))
    for k, (p, dx) in enumerate(zip(ps, outs)):
        assert torch.equal(dx.cpu(), p['ref']['dx']), f'dgrad member {k}'
    outs = [p['dx0'].to(DEV).clone() for p in ps]
    for call in (0, 1):
        assert ops.conv1x1_group_dgrad(dys, ws, outs, [True] * len(ps))
        for k, (p, dx) in enumerate(zip(ps, outs)):
            assert torch.equal(dx.cpu(), p['ref']['dx_acc'][call]), f'dgrad accumulate {call + 1} member {k}'


def _single_member(ops, rows, cin, n, rep, want=None):
    """want: (forward code, dgrad code).  Both entries refuse a lone long map (nothing is written): its tiles are then reached next to a
    short companion."""
    p = _problem(rows, cin, n)
    for mode in MODES_16:
        ops.set_precision(mode)
        ps = [p]
        if ops.conv1x1_group_route(0, _gemm_shapes(ps, 0)) < 0:
            assert rows >= 8192 and ops.conv1x1_group_route(1, _gemm_shapes(ps, 1)) < 0
            dx = torch.full(tuple(p['x'].shape), 7.0, device=DEV)
            assert not ops.conv1x1_group_dgrad([p['dy'].to(DEV)], [p['w'].to(DEV)], [dx], [False]) and bool((dx == 7.0).all())
            assert ops.conv1x1_group_fwd([p['x'].to(DEV)], [p['w'].to(DEV)], [None]) is None
            ps = [p, _problem(15, 48, 16)]
        for entry in (0, 1):
            code = ops.conv1x1_group_route(entry, _gemm_shapes(ps, entry))
            assert code > 0 and (want is None or code == want[entry]), (mode, entry, code)
        _fwd_equal(ops, ps, [rep, 1][:len(ps)])
        _dgrad_equal(ops, ps)


@pytest.mark.parametrize('cin', KS)
@pytest.mark.parametrize('rows', (1, 15, 31, 32, 33))
def test_exact_one_member_short_rows(ops16, rows, cin):
    for j, n in enumerate(NS):
        _single_member(ops16, rows, cin, n, REPLICAS[(j + rows) % 3], want=(12, 12))


@pytest.mark.parametrize('rows,cin,n,want', [(2560, 384, 384, (12, 12)), (2560, 192, 48, (12, 12)), (2560, 48, 80, (12, 12)),
                                             (2560, 16, 16, (12, 12)), (2560, 80, 192, (12, 12)), (8200, 48, 48, (142, 142)),
                                             (8200, 192, 96, (142, 142)), (8200, 96, 80, (142, 122)), (8200, 384, 96, (122, 142)),
                                             (2560, 256, 48, (12, 12)), (2560, 48, 144, (12, 12)), (8200, 192, 48, (122, 142))])
def test_exact_one_member_long_rows(ops16, rows, cin, n, want):
    _single_member(ops16, rows, cin, n, REPLICAS[(cin + n) // 16 % 3], want=want)


def test_exact_two_members_on_one_map(ops16):
    """conv1 | conv2 of a CSP layer: both read the first member's map"""
    ps = [_problem(2560, 192, 96), _problem(2560, 192, 48)]
    x = ps[0]['x']
    x_nchw = x.permute(0, 3, 1, 2).contiguous()
    refs = [ce.nhwc(ce.conv_ref(x_nchw, p['w'], None, None, 1, 0)[0]) for p in ps]
    assert torch.equal(refs[0], ps[0]['y64']) and float(refs[1].abs().max()) ** 2 * ce.STAT_ROWS < ce.LIMIT
    for mode in MODES_16:
        ops16.set_precision(mode)
        xd = x.to(DEV)
        _fwd_equal(ops16, ps, [2, 2], xs=[xd, xd], refs=refs)


def test_exact_two_sharers_in_two_rounds(ops16):
    """the input gradients of two readers of one map: round 0 writes the shared buffer, round 1 adds to it"""
    ps = [_problem(33, 48, 80), _problem(33, 48, 16)]
    want = (ps[0]['ref']['dx'].double() + ps[1]['ref']['dx'].double()).float()
    for mode in MODES_16:
        ops16.set_precision(mode)
        dx = torch.full(tuple(ps[0]['x'].shape), -3.0, device=DEV)
        for rnd, p in enumerate(ps):
            assert ops16.conv1x1_group_dgrad([p['dy'].to(DEV)], [p['w'].to(DEV)], [dx], [rnd > 0])
        assert torch.equal(dx.cpu(), want)


STEMS = ((8, 5, 8, 96, 96), (8, 2, 5, 192, 96), (8, 1, 2, 384, 96))           # the head stems at 40 / 10 / 2 pixels x 8 images


def test_exact_three_members_of_different_rows_and_k(ops16):
    ps = [ce.problem(*s, 1, 1) for s in STEMS]
    for mode in MODES_16:
        ops16.set_precision(mode)
        assert ops16.conv1x1_group_route(0, _gemm_shapes(ps, 0)) == 1222 and ops16.conv1x1_group_route(1, _gemm_shapes(ps, 1)) == 1222
        _fwd_equal(ops16, ps, [1, 2, 4])
        _dgrad_equal(ops16, ps)


def test_exact_four_members(ops16):
    """32- and 64-row tiles, compile-time and run-time contraction lengths, a partial column tile and a one-row member in one launch"""
    ps = [_problem(8200, 48, 48), _problem(33, 80, 80), _problem(2560, 192, 48), _problem(1, 16, 384)]
    for mode in MODES_16:
        ops16.set_precision(mode)
        assert ops16.conv1x1_group_route(0, _gemm_shapes(ps, 0)) == 14222 and ops16.conv1x1_group_route(1, _gemm_shapes(ps, 1)) == 14222
        _fwd_equal(ops16, ps, [8, 1, 2, 1])
        _dgrad_equal(ops16, ps)


@pytest.mark.parametrize('sizes', [[(8, 16, 20, 192, 96)], [(32, 32, 40, 96, 96), (32, 16, 20, 192, 96), (32, 8, 10, 384, 96)],
                                   [(32, 8, 10, 384, 192), (32, 8, 10, 384, 384), (32, 8, 10, 192, 192), (8, 16, 20, 256, 144)]])
def test_random_data_against_the_single_calls(bf16_ops, sizes):
    ops = bf16_ops
    xs = [tk.rnd((B, H, W, c), 10 + k).to(DEV) for k, (B, H, W, c, n) in enumerate(sizes)]
    ws = [tk.rnd((n, c, 1, 1), 30 + k, 0.1).to(DEV) for k, (B, H, W, c, n) in enumerate(sizes)]
    dys = [tk.rnd((B, H, W, n), 50 + k).to(DEV) for k, (B, H, W, c, n) in enumerate(sizes)]
    reps = [ops.stat_replicas(x.numel() // x.shape[-1]) for x in xs]
    cs_g = [torch.zeros((r, 2, w.shape[0]), dtype=torch.float64, device=DEV) for r, w in zip(reps, ws)]
    cs_s = [torch.zeros((r, 2, w.shape[0]), dtype=torch.float64, device=DEV) for r, w in zip(reps, ws)]
    ys = ops.conv1x1_group_fwd(xs, ws, cs_g)
    assert ys is not None
    for k in range(len(sizes)):
        y1 = ops.conv_nhwc_fwd(xs[k], ws[k], None, colstats=cs_s[k])
        tk.close(ys[k], y1, rtol=5e-5, atol=1e-5, what=f'forward {k}', fwd=True)
        assert torch.equal(ys[k], y1), f'forward {k}: not the bits of the single call'
        assert torch.allclose(cs_g[k].sum(0), cs_s[k].sum(0), rtol=1e-12, atol=1e-9), f'statistics {k}: not the partial sums of the single call'
        tk.close(cs_g[k].sum(0)[0], cs_s[k].sum(0)[0], rtol=1e-5, atol=1e-4, what=f'column sums {k}', fwd=True)
        tk.close(cs_g[k].sum(0)[1], cs_s[k].sum(0)[1], rtol=1e-5, atol=1e-4, what=f'column sums of squares {k}', fwd=True)
    outs = [torch.empty_like(x) for x in xs]
    assert ops.conv1x1_group_dgrad(dys, ws, outs, [False] * len(sizes))
    singles = [ops.conv_nhwc_dgrad(dys[k], ws[k], tuple(xs[k].shape)) for k in range(len(sizes))]
    for k in range(len(sizes)):
        tk.close(outs[k], singles[k], rtol=1e-4, atol=1e-5, what=f'dgrad {k}')
        assert torch.equal(outs[k], singles[k]), f'dgrad {k}: not the bits of the single call'
    assert ops.conv1x1_group_dgrad(dys, ws, outs, [True] * len(sizes))
    for k in range(len(sizes)):
        tk.close(outs[k], 2 * singles[k], rtol=1e-4, atol=1e-5, what=f'dgrad accumulate {k}')


def test_refused_group_launches_nothing(ops16):
    from leod_amd import _lib
    ops = ops16
    lib, p, st = _lib.lib(), ops._p, ops._stream()
    ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731

    def call_fwd(n, M, cin, N):
        x, w = torch.ones((M, cin), device=DEV), torch.ones((N, cin), device=DEV)
        y, cs = torch.full((M, N), 5.0, device=DEV), torch.zeros((1, 2, N), dtype=torch.float64, device=DEV)
        rc = lib.leod_conv1x1_group_fwd(n, ops._ptr_array([x] * n), ops._ptr_array([w] * n), ops._ptr_array([y] * n), ops._ptr_array([cs] * n),
                                        ints([1] * n), ints([M] * n), ints([cin] * n), ints([N] * n), st)
        dx = torch.full((M, cin), 5.0, device=DEV)
        rd = lib.leod_conv1x1_group_dgrad(1, ops._ptr_array([y]), ops._ptr_array([w]), ops._ptr_array([dx]), ints([0]), ints([M]), ints([cin]),
                                          ints([N]), st) if n == 1 else rc
        torch.cuda.synchronize()
        untouched = bool((y == 5.0).all()) and not bool(cs.any()) and bool((dx == 5.0).all())
        return rc, rd, untouched

    ops.set_precision('f32')
    assert call_fwd(1, 64, 32, 32) == (-3, -3, True)                 # 16-bit modes only
    assert ops.conv1x1_group_fwd([torch.ones((1, 8, 8, 32), device=DEV)], [torch.ones((32, 32, 1, 1), device=DEV)], [None]) is None
    ops.set_precision('16f')
    assert call_fwd(5, 64, 32, 32) == (-1, -1, True)                 # five members
    assert call_fwd(1, 64, 400, 32) == (-3, -3, True)                # K = 400 forward; the dgrad then writes 400 columns
    assert call_fwd(1, 64, 32, 400) == (-3, -3, True)                # N = 400 forward = K = 400 of the dgrad
    assert call_fwd(1, 64, 32, 32)[:2] == (0, 0)                     # ... and the same call inside the coverage launches


def _conv_bn_run(ops, Fn, specs, maps_of, grouped, monkeypatch):
    """BaseConv layers (cin, n) on the maps maps_of[k] as ONE ConvBNFn node; grouped = False: ops.conv1x1_group_ok answers no"""
    from leod_amd.models.detection.yolox.models.network_blocks import BaseConv
    calls = {'fwd': 0, 'dgrad': 0}
    fwd, dgrad = ops.conv1x1_group_fwd, ops.conv1x1_group_dgrad
    with monkeypatch.context() as mp:
        def counted(name, fn):                                 # launches: the calls the route accepted
            def call(*a):
                got = fn(*a)
                calls[name] += 1 if got else 0
                return got
            return call
        mp.setattr(ops, 'conv1x1_group_fwd', counted('fwd', fwd))
        mp.setattr(ops, 'conv1x1_group_dgrad', counted('dgrad', dgrad))
        if not grouped:
            mp.setattr(ops, 'conv1x1_group_ok', lambda entry, shapes: False)
        mods = []
        for k, (cin, n) in enumerate(specs):
            m = BaseConv(cin, n, 1, 1)
            with torch.no_grad():
                m.conv.weight.copy_(tk.rnd(m.conv.weight.shape, 30 + k, 0.1))
                m.bn.weight.copy_(1 + 0.2 * tk.rnd((n,), 40 + k))
                m.bn.bias.copy_(tk.rnd((n,), 50 + k, 0.1))
            mods.append(m.to(DEV).train())
        maps = [tk.rnd(s, 60 + j).to(DEV).requires_grad_(True) for j, s in enumerate(maps_of['shapes'])]
        xs = [maps[j] for j in maps_of['reads']]
        ys = Fn.base_conv_group(mods, xs)
        sum((y * tk.rnd(y.shape, 70 + k, 0.1).to(DEV)).sum() for k, y in enumerate(ys)).backward()
        torch.cuda.synchronize()
    out = {f'y{k}': y.detach().clone() for k, y in enumerate(ys)}
    for k, m in enumerate(mods):
        out.update({f'b.{k}.mean': m.bn.running_mean.clone(), f'b.{k}.var': m.bn.running_var.clone()})
        out.update({f'g.{k}.{n}': p.grad.clone() for n, p in m.named_parameters()})
    out.update({f'gx{j}': x.grad.clone() for j, x in enumerate(maps)})
    return out, copy.copy(calls)


@pytest.mark.parametrize('specs,maps_of,launches', [
    # conv1 | conv2 of a CSP layer: one map, one forward launch, input gradients in two rounds of one member
    (((96, 48), (96, 48)), dict(shapes=[(4, 16, 20, 96)], reads=(0, 0)), (1, 2)),
    # the three head stems
    (((96, 96), (192, 96), (384, 96)), dict(shapes=[(2, 32, 40, 96), (2, 16, 20, 192), (2, 8, 10, 384)], reads=(0, 1, 2)), (1, 1)),
], ids=['csp_pair', 'three_stems'])
def test_conv_bn_fn_grouped_against_ungrouped(bf16_ops, monkeypatch, specs, maps_of, launches):
    from leod_amd import functions as Fn
    ref, ref_calls = _conv_bn_run(bf16_ops, Fn, specs, maps_of, False, monkeypatch)
    got, got_calls = _conv_bn_run(bf16_ops, Fn, specs, maps_of, True, monkeypatch)
    assert ref_calls == {'fwd': 0, 'dgrad': 0} and got_calls == {'fwd': launches[0], 'dgrad': launches[1]}
    assert got.keys() == ref.keys()
    for k in ref:
        tk.close(got[k], ref[k], rtol=1e-4, atol=1e-5, what=k, fwd=k.startswith(('y', 'b')))


def test_conv_bn_fn_in_mode_f32_is_what_it_was(ops16, monkeypatch):
    """the route refuses mode f32 before anything is allocated or registered: the node runs today's single calls, bit for bit"""
    from leod_amd import functions as Fn
    ops16.set_precision('f32')
    args = (((96, 48), (96, 48)), dict(shapes=[(2, 8, 10, 96)], reads=(0, 0)))
    ref, _ = _conv_bn_run(ops16, Fn, *args, False, monkeypatch)
    got, calls = _conv_bn_run(ops16, Fn, *args, True, monkeypatch)
    assert calls == {'fwd': 0, 'dgrad': 0}
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
