"""Without a GPU: (1) the operand recipes of tests/conv_exact.py do what their docstring says, checked on the generated values; (2) the
float64 reference is pinned by a second definition; (3) every row of tests/test_conv_exact_gpu.py still routes to the kernel it is there
for, in its mode; (4) that table is complete: every (entry, code) pair that launches in the literal route table of
tests/test_conv_routes_cpu.py has an exact row per mode class, and every forward code has an eval-BatchNorm row."""
import pytest
import torch

import conv_exact as ce
import test_conv_exact_gpu as T
import test_conv_routes_cpu as R

BF16, F16 = torch.bfloat16, torch.float16
CLASSES = (('f32', ('f32',)), ('16', ('bf16', '16f')))


def _roundtrips(t):
    return ce.representable(t, BF16) and ce.representable(t, F16)


def _integers(t):
    return torch.equal(t, t.round())


def _conv_shapes():
    return sorted({r[:8] for k in T.CONV_ROWS for r in T.CONV_ROWS[k]} | {r[:7] + (False,) for k in T.BN_ROWS for r in T.BN_ROWS[k]})


def _stem_shapes():
    return sorted({r[:9] + (r[10],) for k in T.STEM_ROWS for r in T.STEM_ROWS[k]}, key=str)


# ---- (1) the claims on the generated values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', _conv_shapes(), ids=lambda s: 'x'.join(map(str, s)))
def test_conv_operands_bounds_and_references(shape):
    B, H, W, Cin, N, ks, stride, bias = shape
    p = ce.problem(*shape)
    sets = dict(x=ce.MAP, w=ce.WEIGHT, dy=ce.DY)
    for k in ('x', 'w', 'dy'):
        t = p[k]
        assert t.dtype is torch.float32 and _roundtrips(t) and bool((t != 0).all()), f'{k}: a zero operand would hide a dropped contribution'
        assert set(t.abs().unique().tolist()) <= set(sets[k]) and float(t.abs().max()) <= p[k + '_max']
    assert p['tier'] == 0 or float(p['w'].abs().max()) == 1 and (p['tier'] == 1 or float(p['x'].abs().max()) == 1)
    if bias:
        assert _roundtrips(p['bias']) and _integers(p['bias']) and float(p['bias'].abs().max()) <= ce.BIAS_MAX
    for k in ('dx0', 'dw0', 'db0'):
        assert _integers(p[k]) and bool((p[k] != 0).any()) and float(p[k].abs().max()) <= ce.START_MAX
    b = ce.bounds(p)
    assert set(b) >= {'fwd', 'dgrad', 'dgrad_acc', 'wgrad', 'stat_sum', 'stat_sq', 'y_sq'} and ('dbias' in b) == bias
    assert all(v < ce.LIMIT for v in b.values()), b
    ref = p['ref']
    outs = [ref['y'], ref['dx']] + ref['dx_acc'] + ref['dw'] + (ref['db'] if bias else [])
    for t in outs:                                     # integers that fp32 holds: the cast of the float64 reference lost nothing
        assert t.dtype is torch.float32 and _integers(t) and float(t.abs().max()) < ce.LIMIT
    assert torch.equal(ref['y'].double(), p['y64']) and float(ref['y'].abs().max()) <= b['fwd'] and float(ref['dx'].abs().max()) <= b['dgrad']
    assert float(ref['dx_acc'][1].abs().max()) <= b['dgrad_acc'] and float(ref['dw'][1].abs().max()) <= b['wgrad']
    y2 = p['y64'] * p['y64']
    assert torch.equal(y2.float().double(), y2), 'y^2 itself must be an fp32 number'
    for s in (ref['s1'], ref['s2']):
        assert s.dtype is torch.float64 and _integers(s) and float(s.abs().max()) < 2.0 ** 53
    assert float(ref['s1'].abs().max()) <= b['stat_sum']
    # accumulating outputs: start + n * gradient, the gradient being what the written dgrad holds
    assert torch.equal(ref['dx_acc'][0] - p['dx0'], ref['dx']) and torch.equal(ref['dx_acc'][1] - ref['dx_acc'][0], ref['dx'])
    assert torch.equal(ref['dw'][1] - ref['dw'][0], ref['dw'][0] - p['dw0'])
    assert ce.problem(*shape) is p                     # cached: the three modes share one reference


@pytest.mark.parametrize('shape', _stem_shapes(), ids=lambda s: 'x'.join(map(str, s)))
def test_stem_operands_bounds_and_references(shape):
    B, H, W, Cin, N, ks, stride, pad, u8, padded = shape
    p = ce.stem_problem(*shape)
    x = p['x']
    if u8:
        assert x.dtype is torch.uint8 and int(x.max()) == ce.U8_MAX and 0.5 < float((x == 0).float().mean()) < 0.9
    else:
        assert x.dtype is torch.float32 and bool((x != 0).all()) and set(x.abs().unique().tolist()) <= set(ce.MAP)
    assert _roundtrips(x.float()) and _roundtrips(p['w']) and _roundtrips(p['dy']) and bool((p['w'] != 0).all()) and bool((p['dy'] != 0).all())
    Hp, Wp = p['padded']
    assert (Hp, Wp) == (padded or (H, W)) and Hp >= H and Wp >= W
    assert torch.equal(p['xp'][:, :, :H, :W], x.double()) and not p['xp'][:, :, H:].any() and not p['xp'][:, :, :, W:].any()
    b = ce.bounds(p)
    assert all(v < ce.LIMIT for v in b.values()), b
    for t in [p['ref']['y']] + p['ref']['dw']:
        assert _integers(t) and float(t.abs().max()) < ce.LIMIT
    assert float(p['ref']['y'].abs().max()) <= b['fwd'] and float(p['ref']['dw'][1].abs().max()) <= b['wgrad']
    assert _integers(p['dw0']) and bool((p['dw0'] != 0).any())


def test_frame_buffer_surrounds_the_frame_with_sentinels():
    for u8, aligned in ((True, True), (True, False), (False, True)):
        p = ce.stem_problem(2, 13, 11, 4, 16, 5, 4, 2, u8, (16, 12))
        buf, view = ce.frame_buffer(p['x'], aligned, 'cpu')
        assert torch.equal(view, p['x']) and (view.data_ptr() % 4 == 0) == aligned and view.data_ptr() % 16 == (0 if aligned else 1)
        off, nbytes = view.data_ptr() - buf.data_ptr(), p['x'].numel() * p['x'].element_size()
        assert len(buf) - off - nbytes >= ce.FRAME_TAIL - 16 - 4 and (off > 0 or aligned)
        if u8:
            assert bool((buf[:off] == ce.SENTINEL_U8).all()) and bool((buf[off + nbytes:] == ce.SENTINEL_U8).all())
        else:
            rest = torch.cat([buf[:off], buf[off + nbytes:]]).clone().view(torch.float32)
            assert bool((rest == ce.SENTINEL_F32).all())
    assert ce.SENTINEL_U8 != 0 and ce.SENTINEL_F32 != 0 and _roundtrips(torch.tensor([ce.SENTINEL_F32]))


def test_tier_shrinks_where_a_bound_would_fail():
    assert ce.tier(9 * 16, 1000) == 0 and ce.tier(9 * 192, 1000) > 0 and ce.tier(96, 70000) > 0 and ce.tier(9 * 512, 70000) == 2
    assert ce.problem(17, 64, 64, 96, 96, 1, 1, False)['tier'] > 0                # 69632 rows: stat_sum
    assert ce.problem(1, 4, 4, 16, 32, 3, 1, True)['tier'] == 0
    assert ce.stat_sq_bound(591.0) < ce.LIMIT < ce.stat_sq_bound(592.0) and ce.STAT_ROWS == 48


def test_eval_bn_parameters_and_reference():
    q = ce.bn_problem(2, 9, 12, 48, 96, 3, 1)
    bw, bb, rm, rv = q['bn']
    assert set(bw.abs().tolist()) <= {0.5, 1., 2.} and _integers(bb) and _integers(rm) and set(rv.tolist()) <= {0.25, 1., 4.}
    assert q['p'] is ce.problem(2, 9, 12, 48, 96, 3, 1, False)
    v = (q['p']['y64'] - rm.double()) / torch.sqrt(rv.double() + ce.BN_EPS) * bw.double() + bb.double()
    assert torch.allclose(q['ref'], torch.nn.functional.silu(v), rtol=1e-12, atol=1e-12)
    assert not _integers(q['ref'])


# ---- (2) the reference itself ------------------------------------------------------------------------------------------------------------
def test_every_geometry_in_use_is_pinned():
    used = {(r[5], r[6], (r[5] - 1) // 2) for k in T.CONV_ROWS for r in T.CONV_ROWS[k]} | {(r[5], r[6], r[7]) for k in T.STEM_ROWS for r in T.STEM_ROWS[k]}
    assert used == set(PINNED), sorted(used ^ set(PINNED))


PINNED = ((1, 1, 0), (3, 1, 1), (3, 2, 1), (5, 4, 2), (7, 4, 3))


@pytest.mark.parametrize('ks,stride,pad', PINNED)
@pytest.mark.parametrize('H,W', [(7, 9), (8, 12)])
def test_conv2d_equals_the_tap_loop(ks, stride, pad, H, W):
    g = ce._gen(ks * 100 + stride * 10 + H)
    B, C, N = 2, 5, 6
    H, W = H * stride, W * stride + (1 if stride == 4 else 0)
    x, w, b = ce._signed(list(ce.MAP), (B, C, H, W), g), ce._signed(list(ce.WEIGHT), (N, C, ks, ks), g), ce._ints(-3, 3, (N,), g)
    Ho, Wo = ce.out_hw(H, W, ks, stride, pad)
    dy = ce._signed(list(ce.DY), (B, N, Ho, Wo), g)
    for a, c in zip(ce.conv_ref(x, w, b, dy, stride, pad), ce.conv_taps(x, w, b, dy, stride, pad)):
        assert a.dtype is torch.float64 and a.shape == c.shape and torch.equal(a, c) and bool(a.any())


def test_the_problem_reference_is_the_tap_loop_on_a_padded_stem_frame():
    p = ce.stem_problem(2, 13, 11, 4, 16, 5, 4, 2, True, (16, 12))
    y, _, dw, _ = ce.conv_taps(p['xp'], p['w'], None, p['dy'].permute(0, 3, 1, 2), 4, 2)
    assert torch.equal(ce.nhwc(y), p['y64']) and torch.equal((p['dw0'].double() + 2 * dw).float(), p['ref']['dw'][1])
    q = ce.problem(2, 5, 7, 8, 12, 3, 2, True)
    y, dx, dw, db = ce.conv_taps(q['x'].permute(0, 3, 1, 2), q['w'], q['bias'], q['dy'].permute(0, 3, 1, 2), 2, 1)
    assert torch.equal(ce.nhwc(y), q['y64']) and torch.equal(ce.nhwc(dx).float(), q['ref']['dx'])
    assert torch.equal((q['dw0'].double() + dw).float(), q['ref']['dw'][0]) and torch.equal((q['db0'].double() + 2 * db).float(), q['ref']['db'][1])


# ---- (3) the routes ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ops():
    import __graft_entry__ as g
    g.build()
    from leod_amd import ops
    prev = ops.get_precision()
    yield ops
    ops.set_precision(prev)


@pytest.mark.parametrize('mode', R.MODES)
def test_every_gpu_row_routes_where_it_says(ops, mode):
    ops.set_precision(mode)
    k = T.klass(mode)
    bad = [(r, got) for r in T.CONV_ROWS[k] for got in [T.conv_routes_of(ops, r)] if got != tuple(r[-1])]
    bad += [(r, got) for r in T.STEM_ROWS[k] for got in [T.stem_routes_of(ops, r)] if got != tuple(r[-1])]
    bad += [(r, got) for r in T.BN_ROWS[k] for got in [T.bn_route_of(ops, r)] if got != r[-1]]
    assert not bad, f'{len(bad)} rows route elsewhere (row, got): {bad[:10]}'


def test_rows_are_well_formed():
    for k in T.CONV_ROWS:
        rows = T.CONV_ROWS[k]
        assert len(set(rows)) == len(rows) and all(len(r) == 10 and all(c > 0 for c in r[-1]) for r in rows)
        assert len(set(T.STEM_ROWS[k])) == len(T.STEM_ROWS[k]) and all(len(r) == 12 and all(c > 0 for c in r[-1]) for r in T.STEM_ROWS[k])
        assert {T.STAT_REPLICAS[i % 3] for i in range(len(rows))} == {1, 8, 32}
        assert any(not r[8] for r in rows) and any(r[7] for r in rows)                  # the raw C ABI without a pack; a bias
    assert len(T.conv_cases()) + len(T.stem_cases()) + len(T.bn_cases()) < 400


# ---- (4) completeness ----------------------------------------------------------------------------------------------------------------------
def _pairs(k):
    return ({(e, c) for r in T.CONV_ROWS[k] for e, c in enumerate(r[-1])} | {(3 + e, c) for r in T.STEM_ROWS[k] for e, c in enumerate(r[-1])})


@pytest.mark.parametrize('k,modes', CLASSES)
def test_every_launching_pair_of_the_route_table_has_an_exact_row(k, modes):
    """the set test_conv_routes_cpu.test_gpu_cases_cover_every_launching_pair computes"""
    need = {(r[0], r[-1]) for r in R.ROWS if r[1] in modes and r[-1] > 0}
    assert len(need) > 40 and need <= _pairs(k), sorted(need - _pairs(k))


# forward codes that no shape of the row lists reaches when the router is asked with CF_BN, no statistics and no bias (with and without a pack)
NO_EVAL_BN = {'f32': set(), '16': set()}


@pytest.mark.parametrize('k,modes', CLASSES)
def test_every_forward_code_has_an_eval_bn_row(ops, k, modes):
    codes = {r[-1][0] for r in T.CONV_ROWS[k]}
    have = {r[-1] for r in T.BN_ROWS[k]}
    reachable = set()
    for mode in modes:
        ops.set_precision(mode)
        reachable |= {T.bn_route_of(ops, r[:7] + (pack,)) for r in T.CONV_ROWS[k] for pack in (True, False)}
    assert codes - reachable == NO_EVAL_BN[k]
    assert codes - NO_EVAL_BN[k] <= have, sorted(codes - NO_EVAL_BN[k] - have)


def test_geometry_rows_show_what_they_are_there_for():
    g16, gf = T.GEOM_16, T.GEOM_F32
    lds = lambda c: c // 1000 in (17, 18, 27, 28)                                        # noqa: E731
    reg = lambda c: c // 1000 in (19, 29)                                                # noqa: E731
    for rows in (g16, gf):
        # a 16- / 64-row tile that spans two images and a ragged last tile, on both implicit-GEMM families
        assert any(reg(r[-1][0]) and r[0] >= 2 and (r[1] * r[2]) % 16 and (r[0] * r[1] * r[2]) % 16 for r in rows if r[6] == 1)
        assert any(lds(r[-1][0]) and r[0] >= 2 and (r[1] * r[2]) % 64 and (r[0] * r[1] * r[2]) % 64 for r in rows if r[6] == 1)
        assert any(r[:3] == (1, 7, 9) and r[6] == 2 for r in rows) and any(lds(r[-1][0]) and r[6] == 2 and r[1] % 2 and r[2] % 2 for r in rows)
        assert any(r[3:5] == (36, 100) and reg(r[-1][0]) for r in rows) and any(r[3:5] == (36, 100) and lds(r[-1][0]) for r in rows)
        q = [r[0] * (r[1] // 2) * (r[2] // 2) for r in rows if r[-1][1] // 1000 == 29]
        assert q and all(v % 16 == 0 and v % 128 for v in q) and any(r[0] >= 2 for r in rows if r[-1][1] // 1000 == 29)
    assert any(r[-1][1] // 1000 == 27 and (r[0] * (r[1] // 2) * (r[2] // 2)) % 128 == 0 for k in T.CONV_ROWS for r in T.CONV_ROWS[k])
    direct = [r for r in g16 if r[-1][0] in (110, 120)]
    assert all(r[0] >= 2 or r[2] == 160 for r in direct) and {5, 9} <= {r[1] for r in direct} and {7, 12, 20, 160} <= {r[2] for r in direct}
    assert any(r[2] == 160 and r[3] == 128 for r in direct) and any(r[3:5] == (96, 192) for r in direct) and any(r[1:5] == (16, 20, 192, 384) for r in direct)
    assert any(r[:3] == (70, 8, 12) for r in direct) and {r[6] for r in direct if r[3:5] == (192, 192)} == {1, 2}
    assert {c for r in g16 for c in r[-1]} >= {110, 120, 220, 500}
    assert {301, 302, 303, 304, 305} <= {r[-1][2] for r in T.CONV_ROWS['16']}
    assert any(r[-1][2] == 305 and r[0] * r[1] * r[2] > 65536 for r in T.CONV_ROWS['16'])
    for k in T.STEM_ROWS:
        rows = T.STEM_ROWS[k]
        pf = lambda r: r[10] or (r[1], r[2])                                             # noqa: E731
        assert any(r[1] < pf(r)[0] and r[2] == pf(r)[1] for r in rows) and any(r[1] == pf(r)[0] and r[2] < pf(r)[1] for r in rows)
        assert any(r[1] < pf(r)[0] and r[2] < pf(r)[1] for r in rows) and any(r[1:3] == (60, 90) and r[8] for r in rows)
        assert any(not r[9] for r in rows) and any(r[5] == 5 for r in rows) and any(not r[8] for r in rows) and {16, 32, 48, 64} <= {r[4] for r in rows}
    assert any(r[3] == 24 for r in T.STEM_ROWS['16'])
