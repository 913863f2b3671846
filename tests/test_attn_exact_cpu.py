"""Without a GPU: (1) the operands of tests/attn_exact.py do what their docstring says (``bounds`` on every row of
tests/test_attn_exact_gpu.py, the Hadamard codes, the group sizes); (2) the explicit float64 formulas of the reference equal float64
autograd of the attention of tests/test_kernels_gpu.py, window and grid; (3) the model of the kernels (``simulate``) reproduces the
reference exactly on O and stays within HALF of every backward bound in every mode and family -- the margin for the error of exp in D,
which the model does not carry -- and every mutation of it is seen: O moves by at least 2^-6 somewhere and the backward leaves its bound by
at least 4x; (4) every row still routes to the kernels it is there for, in its mode; (5) the table is complete: every (entry, code) pair
that launches in the attention tables of tests/test_attn_lstm_routes_cpu.py has a row per mode class, and the geometry rows show what they
are there for."""
import numpy as np
import pytest
import torch

import attn_exact as ae
import test_attn_exact_gpu as T
import test_attn_lstm_routes_cpu as R

CLASSES = (('f32', ('f32',)), ('16', ('bf16', '16f')))


def _shapes():
    """(part, d, heads, B, grid) of every row, with the (mode, family) pairs that run on it"""
    out = {}
    for k, modes in CLASSES:
        for part, d, t16, want, heads, B, grid in T.ROWS[k]:
            out.setdefault((tuple(part), d, heads, B, tuple(grid)), set()).update((m, ae.family_of(want[0])) for m in modes)
    return sorted(out.items())


SHAPES = _shapes()


def _sid(s):
    (part, d, heads, B, grid), _ = s
    return f'{part[0]}x{part[1]}-d{d}-h{heads}-b{B}-{grid[0]}x{grid[1]}'


# ---- (1) the claims on the generated values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', (12, 20, 24, 32))
def test_hadamard_rows_are_orthogonal(d):
    H = ae.hadamard(d)
    assert H.shape == (d, d) and set(np.unique(H)) == {-1.0, 1.0}
    assert np.array_equal(H @ H.T, d * np.eye(d)) and (H[0] == 1).all() and (H[:, 0] == 1).all()
    assert (H[1:].sum(1) == 0).all()                            # every code is orthogonal to the vector of ones


def test_group_sizes():
    assert ae.group_sizes(16, 7, 4) == [8, 4, 2, 1, 1]
    for n, gmax in ((15, 7), (16, 7), (30, 15), (35, 15), (80, 7), (121, 19), (225, 15), (240, 15), (240, 19)):
        s = ae.group_sizes(n, gmax)
        assert sum(s) == n and len(s) <= gmax and all(v & (v - 1) == 0 and v <= 16 for v in s) and 2 * len(s) <= n
    assert min(ae.group_sizes(15, 7)) == 1 and 2 in ae.group_sizes(30, 15) and 4 in ae.group_sizes(240, 19)
    with pytest.raises(ValueError):
        ae.group_sizes(240, 14)


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_bounds_and_the_clean_model(shape):
    (part, d, heads, B, grid), runs = shape
    p = ae.problem(part, d, heads, B, True, 0, grid)
    b = ae.bounds(p)
    assert len(b) >= 14 and all(ok for ok, _ in b.values()), {k: v for k, v in b.items() if not v[0]}
    assert ae.problem(part, d, heads, B, True, 0, grid) is p                     # cached: the three modes share one reference
    n, ref = part[0] * part[1], p['ref']
    assert p['qkv'].shape == (B, grid[0] * part[0], grid[1] * part[1], 3 * heads * d) and p['qkv'].dtype is torch.float32
    assert set(p['q'].unique().tolist()) <= {ae.GAMMA - ae.A, ae.GAMMA + ae.A} and float(p['k'].abs().min()) >= 2 and float(p['k'].abs().max()) <= 10
    assert set(p['v'].abs().unique().tolist()) <= {1.0, 2.0} and set(p['do'].abs().unique().tolist()) <= {1.0, 2.0, 3.0}
    for pi in range(p['NP']):
        for h in range(heads):
            keys = p['k'][pi, h]
            assert len({tuple(r.tolist()) for r in keys}) == n, 'two tokens share a key'
            for g in p['group'][pi, h].unique():                                 # a key coordinate keeps its sign inside a group
                kg = keys[p['group'][pi, h] == g]
                assert bool(((kg > 0).all(0) | (kg < 0).all(0)).all())
    assert bool((p['tie'] == 1).any()) == (min(min(s) for row in p['sizes'] for s in row) == 1)
    assert float(ref['dq'].abs().max()) > 0.05 and float(ref['dk'].abs().max()) > 0.05 and float(ref['dv'].abs().max()) > 0.5
    # window and grid addressing hold the same partition-space values at other rows of the image
    g = ae.problem(part, d, heads, B, False, 0, grid)
    assert g['ref'] is p['ref'] and torch.equal(ae.from_image(g['qkv'], g['rows'], heads), ae.from_image(p['qkv'], p['rows'], heads))
    assert (grid == (1, 1)) == np.array_equal(g['rows'], p['rows'])
    for t in ('O', 'dqkv'):
        assert torch.equal(ae.from_image(p[t], p['rows'], heads), ae.from_image(g[t], g['rows'], heads))
    # the model of the kernels, unmutated: O exactly, the backward within half of every bound
    for mode, fam in sorted(runs):
        s = ae.simulate(p, mode, fam)
        assert torch.equal(s['O'].float(), ref['O'].float()), (mode, fam)
        if s['O16'] is not None:
            assert torch.equal(s['O16'].float(), ref['O'].float()), (mode, fam)
        assert float((s['lse'] - ref['lse']).abs().max()) < 1e-6
        tol = ae.tolerance(p, mode, fam)
        for t in ('dq', 'dk', 'dv'):
            ratio, where = ae.worst(s[t], ref[t], tol[t], p)
            assert ratio <= 0.5, f'mode {mode}, family {fam}, {t}: the clean model is at {ratio:.3f} of the bound at {where}'


def test_tolerance_is_the_documented_one():
    p = ae.problem((5, 6), 32)
    r = p['ref']
    floor = {t: 2e-6 + 5e-6 * float(r[t].abs().max()) + 2e-5 * r[t].abs() for t in ('dq', 'dk', 'dv')}
    for mode, fam in (('f32', 1), ('f32', 2), ('f32', 3), ('bf16', 1), ('16f', 1)):
        tol = ae.tolerance(p, mode, fam)
        assert all(torch.equal(tol[t], floor[t]) for t in floor), (mode, fam)
    for mode in ('bf16', '16f'):
        t2, t3 = ae.tolerance(p, mode, 2), ae.tolerance(p, mode, 3)
        assert torch.allclose(t2['dq'], floor['dq'] + ae.U * (r['dS'].abs() @ p['k'].abs()), rtol=1e-14, atol=0)
        assert torch.allclose(t2['dk'], floor['dk'] + ae.U * (r['dS'].abs().transpose(-1, -2) @ p['q'].abs()), rtol=1e-14, atol=0)
        assert torch.equal(t2['dv'], floor['dv'])
        assert all(torch.allclose(t3[t], t2[t] + ae.U * r[t].abs(), rtol=1e-14, atol=0) for t in floor)
    assert ae.U == 2.0 ** -8 and (ae.RTOL, ae.ATOL, ae.ATOL_SCALE) == (2e-5, 2e-6, 5e-6)
    # the floor is linear_exact.close_fp32's: a value on the bound passes it, one 1 % beyond does not
    import linear_exact as le
    le.close_fp32(r['dv'] + 0.999 * floor['dv'], r['dv'])
    with pytest.raises(AssertionError):
        le.close_fp32(r['dv'] + 1.01 * floor['dv'], r['dv'])


# ---- (2) the reference itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('part,d,heads,B,grid', [((3, 5), 12, 3, 2, (2, 2)), ((4, 8), 32, 2, 1, (2, 2)), ((5, 7), 24, 1, 2, (1, 2))])
@pytest.mark.parametrize('window', (True, False))
def test_explicit_formulas_equal_autograd(part, d, heads, B, grid, window):
    import test_kernels_gpu as tk
    p = ae.problem(part, d, heads, B, window, 0, grid)
    qkv = p['qkv'].double().requires_grad_(True)
    out = tk._attn_ref(qkv, heads, part, window)
    out.backward(p['dO'].double())
    M = qkv.shape[0] * qkv.shape[1] * qkv.shape[2]
    r = p['ref']
    ref_O = ae.to_image(r['O'], p['rows'], M).view(out.shape)
    ref_g = ae.to_image(torch.cat([r['dq'], r['dk'], r['dv']], -1), p['rows'], M).view(qkv.shape)
    assert torch.allclose(out.detach(), ref_O, rtol=1e-12, atol=1e-13) and torch.allclose(qkv.grad, ref_g, rtol=1e-10, atol=1e-12)
    assert torch.equal(ref_O.float(), p['O']) and torch.equal(ref_g.float(), p['dqkv'])
    # the pieces: P is a softmax, D = rowsum(P dP), dS = P (dP - D) scale sums to zero over the keys
    assert torch.allclose(r['P'].sum(-1), torch.ones((), dtype=torch.float64), rtol=1e-13, atol=0)
    assert torch.allclose(r['D'], (r['O'] * p['do']).sum(-1), rtol=1e-12, atol=1e-12) and float(r['dS'].sum(-1).abs().max()) < 1e-13
    assert torch.allclose(r['lse'], torch.log(p['tie'].double()), rtol=0, atol=1e-12)


# ---- (3) the mutations are seen --------------------------------------------------------------------------------------------------------------
MUTATION_SHAPES = [(part, d) for d, parts in ((12, ((3, 5), (4, 4), (8, 10))), (20, ((5, 7), (15, 15))), (24, ((3, 5), (7, 8), (8, 10), (12, 20))),
                                              (32, ((5, 6), (8, 8), (7, 11), (15, 15)))) for part in parts]
CHANGES_P = ('pad_key', 'drop_key', 'mask24')                   # these move the probabilities, hence all of dq, dk, dv


@pytest.mark.parametrize('part,d', MUTATION_SHAPES, ids=lambda v: str(v).replace(' ', ''))
def test_every_mutation_is_seen(part, d):
    p = ae.problem(part, d)
    ref = p['ref']
    runs = (('f32', 1), ('bf16', 1)) if d in (12, 20) else (('f32', 2), ('bf16', 2), ('bf16', 3), ('16f', 3))
    for mode, fam in runs:
        tol = ae.tolerance(p, mode, fam)
        for m in ae.MUTATIONS:
            if m == 'mask24' and not (d == 24 and fam == 3):
                continue
            s = ae.simulate(p, mode, fam, m)
            assert float((s['O'] - ref['O']).abs().max()) >= 2.0 ** -6, (mode, fam, m)
            assert not torch.equal(s['O'].float(), ref['O'].float())
            ratios = {t: ae.worst(s[t], ref[t], tol[t], p)[0] for t in ('dq', 'dk', 'dv')}
            assert max(ratios.values()) >= 4, (mode, fam, m, ratios)
            if m in CHANGES_P:
                assert min(ratios.values()) >= 4, (mode, fam, m, ratios)
            else:                                               # dv = P^T dO does not read v
                assert min(ratios['dq'], ratios['dk']) >= 4, (mode, fam, m, ratios)


# ---- (4) the routes ------------------------------------------------------------------------------------------------------------------------
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
    rows = T.ROWS[T.klass(mode)]
    bad = [(r, fl, got) for r in rows for fl in T.flag_sets(r[2]) for got in [T.routes_of(ops, r, fl)] if got != tuple(r[3])]
    assert not bad, f'{len(bad)} rows route elsewhere (row, flags, got): {bad[:10]}'
    assert all(ae.family_of(r[3][0]) == ae.family_of(r[3][1]) for r in rows)


def test_rows_are_well_formed():
    for k in T.ROWS:
        rows = T.ROWS[k]
        assert len(set(rows)) == len(rows) and all(len(r) == 7 and all(c > 0 for c in r[3]) for r in rows)
        assert all(r[2] == (ae.family_of(r[3][0]) == 3) for r in rows)           # 16-bit tensors exactly on the 16-bit-tile family
    assert not any(r[2] for r in T.ROWS['f32'])
    assert len(T.cases()) == len(T.ROWS['f32']) + 2 * len(T.ROWS['16']) < 400
    assert all(r[5] * r[6][0] * r[6][1] * r[0][0] * r[0][1] <= 4 * 240 for k in T.ROWS for r in T.ROWS[k])                # at most 4 x 240 tokens


# ---- (5) completeness ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,modes', CLASSES)
def test_every_launching_pair_of_the_route_tables_has_an_exact_row(k, modes):
    table = list(R.attn_rows()) + list(R.ATTN_EXTRA)
    have = {(e, c) for r in T.ROWS[k] for e, c in enumerate(r[3])}
    for mode in modes:
        need = {(r[1], r[-1]) for r in table if r[0] == mode and r[-1] > 0}
        assert len(need) >= 56 and need <= have, (mode, sorted(need - have))


def test_geometry_rows_show_what_they_are_there_for():
    for k in T.ROWS:
        rows = T.ROWS[k]
        fams = {ae.family_of(r[3][0]) for r in rows}
        assert fams == ({1, 2} if k == 'f32' else {1, 2, 3})
        for fam in fams:
            mine = [r for r in rows if ae.family_of(r[3][0]) == fam]
            assert any(r[5] == 2 for r in mine), 'two images'
            assert any(r[4] == 1 for r in mine) and any(r[4] == 3 for r in mine), 'one head; an odd head offset'
            assert any(r[6] == (1, 1) for r in mine), 'one partition per image'
            assert any((r[0][0] * r[0][1]) % 16 for r in mine) and any((r[0][0] * r[0][1]) % 16 == 0 for r in mine), 'padded and full partitions'
        assert {r[1] for r in rows} == {12, 20, 24, 32}
    # the one-key ties of test_exp_of_zero_is_one sit in a FULL partition, two per (partition, head), each the target of two queries or more
    assert T.ONE_KEY_ROWS['16'][-1] == (24, True) and (T.ONE_KEY_PART[0] * T.ONE_KEY_PART[1]) % 16 == 0
    for d in (12, 24):
        p = ae.problem(T.ONE_KEY_PART, d, 2, 1, True, 0, (2, 2), T.ONE_KEY_SPLITS)
        assert all(ok for ok, _ in ae.bounds(p).values()) and all(sorted(s.tolist()) == [1, 1, 2, 4, 8] for row in p['sizes'] for s in row)
        assert bool(((p['tie'] == 1).sum(-1) >= 4).all())
        s = ae.simulate(p, 'bf16', 3 if d == 24 else 1)
        assert torch.equal(s['O'].float(), p['ref']['O'].float()) and bool((s['lse'][p['tie'] == 1] == 0).all())
