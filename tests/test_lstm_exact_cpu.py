"""Without a GPU: the operands of tests/lstm_exact.py do what its docstring says, on every shape that tests/test_lstm_exact_gpu.py runs --
(1) forward: the margin rule on every pre-activation, |c| <= 6, every operand representable in bf16 and fp16, the share of gates decided by
h (>= 20 %) and by the bias (>= 5 %) at every timestep after the first, every gate taking both values at every timestep, and the step
functions of the reference being float64 sigmoid / tanh; (2) backward: every modelled intermediate exact in fp32 and the span of the partial
sums, every dgates gate column nonzero in >= 10 % of its elements at every timestep, the G16 forward inputs reproducing the constructed gates;
(3) every mutation changes the reference's discrete output; (4) every row still routes where it says, and every (entry, code) pair that
launches in the ConvLSTM tables of tests/test_attn_lstm_routes_cpu.py has a row, in every mode.  The shares are conditions that keep the
tests from going vacuous, not measurements."""
import math

import pytest
import torch

import linear_exact as le
import lstm_exact as lx
import test_attn_lstm_routes_cpu as R
import test_lstm_exact_gpu as T

CLASSES = (('f32', ('f32',)), ('16', ('bf16', '16f')))
SHAPES = sorted({c[1:2] + c[3:] for c in T.cases()} | {(C, 35, 3, s) for C in T.PER_STEP_C for s in (True, False)})       # (C, M, T, state)
BWD_SHAPES = sorted({c[1:2] + c[3:5] for c in T.cases()} | {(C, 35, 3) for C in T.PER_STEP_C})


def _sid(s):
    return '-'.join(str(v) for v in s)


# ---- (1) forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_forward_operands(shape):
    C, M, Tn, state = shape
    p = lx.forward_problem(*shape)
    assert lx.forward_problem(*shape) is p                                            # cached: the three modes share one reference
    ref, pre, need = p['ref'], p['pre'], p['need']
    assert p['x'].shape == (Tn, M, C) and p['W'].shape == (4 * C, 2 * C) and p['gx'].shape == (Tn, M, 4 * C)
    # the margin: 128 + what rounding can move, at most 128 + 6 and a little
    assert bool((pre.abs() >= need).all()) and float(need.min()) == lx.S and float(need.max()) <= lx.S + 6 + 1e-3
    assert float(pre.abs().min()) >= lx.S
    x_decides = p['decided'] == 0
    assert float(pre.abs()[x_decides].min()) >= lx.WX_MAG - 3 * lx.WH_MAG - 256 if bool(x_decides.any()) else True
    # the step functions of the model are float64 sigmoid / tanh there
    assert float((torch.sigmoid(pre[:, :, :3]) - ref['gates'][:, :, :3]).abs().max()) < 1e-50
    assert float((torch.tanh(pre[:, :, 3]) - ref['gates'][:, :, 3]).abs().max()) == 0
    assert set(ref['gates'][:, :, :3].unique().tolist()) == {0.0, 1.0} and set(ref['gates'][:, :, 3].unique().tolist()) == {-1.0, 1.0}
    # c: small integers; h = o tanh(c)
    assert float(ref['c'].abs().max()) <= lx.C_CAP and torch.equal(ref['c'], ref['c'].round())
    assert torch.equal(ref['h'][1:], ref['gates'][:, :, 2] * torch.tanh(ref['c'][1:]))
    # every operand is the same number in bf16 and fp16
    for n in ('x', 'W', 'b', 'h0', 'c0'):
        assert le.representable(p[n], torch.bfloat16) and le.representable(p[n], torch.float16), n
    W, b = p['W'].double(), p['b'].double()
    assert set(W[:, :C].abs().unique().tolist()) == {0.0, lx.WX_MAG} and bool(((W[:, :C] != 0).sum(1) == 1).all())
    assert set(W[:, C:].abs().unique().tolist()) == {0.0, lx.WH_MAG} and bool(((W[:, C:] != 0).sum(1) == 3).all())
    assert set(b.abs().unique().tolist()) == {128.0, 256.0} and set(p['x'].abs().unique().tolist()) <= {0.0, 1.0, 2.0}
    col = lx.xcol(C)
    assert sorted(col.tolist()) == list(range(C)) and bool((col != torch.arange(C)).all())
    assert bool((W[:, :C][torch.arange(4 * C), col.repeat(4)] != 0).all())
    # gx is the projection, exactly
    assert torch.equal(p['gx'].double(), torch.einsum('tmc,nc->tmn', p['x'].double(), W[:, :C]) + b) and float(p['gx'].abs().max()) < 2 ** 14
    if state:
        assert set(p['h0'].abs().unique().tolist()) <= {0.0, 0.75, 1.0} and set(p['c0'].abs().unique().tolist()) <= {0.0, 1.0, 2.0}
        assert bool((p['h0'] != 0).any()) and bool((p['c0'] != 0).any())
    else:
        assert not bool(p['h0'].any()) and not bool(p['c0'].any())
    for t in range(Tn):
        d, g = p['decided'][t], ref['gates'][t]
        if t > 0:
            assert float((d == 1).double().mean()) >= 0.20 and float((d == 2).double().mean()) >= 0.05, (t, 'shares of h and of the bias')
        if t > 0:
            assert bool((d == 1).any()) and bool((d == 2).any())
        for k in range(4):
            assert len(g[:, k].unique()) == 2, (t, lx.GATE_NAMES[k], 'takes one value only')
            assert 0.2 <= float((g[:, k] > 0).double().mean()) <= 0.8


def test_the_h_bound_is_the_derived_one():
    per_c = {c: lx.tanh_error_bound(c) / 2.0 ** -24 for c in range(-lx.C_CAP, lx.C_CAP + 1)}
    assert lx.H_BOUND == max(per_c.values()) * 2.0 ** -24 and max(per_c, key=per_c.get) == 1
    assert 7.0 < per_c[1] < 7.1 and per_c[0] == 4.5 and max(v for c, v in per_c.items() if c < 0) < 2.5       # "a few 2^-24"
    assert math.tanh(6) - math.tanh(5) > 150 * lx.H_BOUND                             # the smallest effect of a discrete error on h
    # ... and what the margin rule assumes about the perturbation: three terms of 512 |h| 2^-8 with |h| <= 1
    assert 3 * lx.WH_MAG * lx.U16 == 6


# ---- (2) backward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', BWD_SHAPES, ids=_sid)
def test_backward_operands(shape):
    C, M, Tn = shape
    key = T.bwd_key(*shape)
    p = lx.backward_problem(*key)
    g = p['gates']
    assert set(g[:, :, :3].unique().tolist()) == {0.0, 0.5, 1.0} and set(g[:, :, 3].unique().tolist()) == {-1.0, 0.0, 1.0}
    assert set(p['cbuf'].unique().tolist()) == {-32.0, 0.0, 32.0} and set(p['dh_seq'].abs().unique().tolist()) == {0.0, 1.0, 2.0}
    assert set(p['dc_last'].abs().unique().tolist()) <= {0.0, 1.0, 2.0}
    W = p['W']
    assert bool((W[:, :C] == 3.0).all()) and set(W[:, C:].abs().unique().tolist()) == {0.0, 0.5, 1.0} and bool(((W[:, C:] != 0).sum(1) == 2).all())
    for n in ('gates', 'cbuf', 'dh_seq', 'dc_last', 'W'):
        assert le.representable(p[n], torch.bfloat16) and le.representable(p[n], torch.float16), n
    # the G16 forward inputs: W_h = 0, one W_x entry per row, pre-activations that are multiples of S and give exactly the constructed gates
    q = p['g16']
    Wf = q['W'].double()
    assert not bool(Wf[:, C:].any()) and bool(((Wf[:, :C] != 0).sum(1) == 1).all())
    pre = torch.einsum('tmc,nc->tmn', q['x'].double(), Wf[:, :C]) + q['b'].double()
    assert torch.equal(pre.float(), q['gx']) and torch.equal(pre, (pre / lx.S).round() * lx.S)
    assert float(pre[pre != 0].abs().min()) == lx.S and torch.equal(lx.act3(pre.view(Tn, M, 4, C)).float(), g)
    for n in ('x', 'W', 'b'):
        assert le.representable(q[n], torch.bfloat16) and le.representable(q[n], torch.float16), n
    for mode16 in (False, True):
        for kw in ({}, {'zero_state': True}, {'dh_seq': False}, {'dc_last': False}):
            ex = lx.backward_exactness(key, mode16, **kw)
            assert len(ex) == 7 * Tn and all(ok for ok, _ in ex.values()), {k: v for k, v in ex.items() if not v[0]}
        r = lx.backward_model(key, mode16)
        for n in ('dgates', 'dgates16', 'dh0', 'dc0'):
            assert torch.equal(r[n].float().double(), r[n]), n
        assert le.representable(r['dgates16'], torch.bfloat16)
        if mode16 and C >= 192 and Tn == 3:
            assert not torch.equal(r['dgates'], r['dgates16']), 'the bf16 rounding of the tile never rounds anything'
        for t in range(Tn):
            d = r['dgates'][t].view(M, 4, C)
            for k in range(4):
                assert float((d[:, k] != 0).double().mean()) >= 0.10, (mode16, t, lx.GATE_NAMES[k])
        assert float((r['dh0'] != 0).double().mean()) >= 0.10 and float((r['dc0'] != 0).double().mean()) >= 0.10


def test_bf16_rounding_is_to_nearest_even():
    v = torch.tensor([257.0, 259.0, 258.0, -257.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=torch.float64)
    assert lx.round_bf16(v).tolist() == [256.0, 260.0, 258.0, -256.0, 1.0, 1 + 2.0 ** -6]
    with pytest.raises(AssertionError):
        lx.round_bf16(torch.tensor([1 + 2.0 ** -30], dtype=torch.float64))
    assert lx.lowbit(torch.tensor([0.0, 6.0, -0.75, 40.0], dtype=torch.float64)) == 0.25


# ---- (3) the mutations are seen ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('state', (True, False))
@pytest.mark.parametrize('C', sorted({r[0] for k in T.ROWS for r in T.ROWS[k]}))
def test_every_forward_mutation_is_seen(C, state):
    p = lx.forward_problem(C, 35, 3, state)
    assert not lx.discrete_differs(lx.forward_model(p), p['ref'])
    for m in lx.FWD_MUTATIONS:
        s = lx.forward_model(p, m)
        assert lx.discrete_differs(s, p['ref']), m
        n = int((s['gates'] != p['ref']['gates']).sum()) + int((s['c'] != p['ref']['c']).sum())
        assert n >= 4, (m, n)


@pytest.mark.parametrize('C', sorted({r[0] for k in T.ROWS for r in T.ROWS[k]}))
def test_every_backward_mutation_is_seen(C):
    key = T.bwd_key(C, 35, 3)
    for mode16 in (False, True):
        for m in lx.BWD_MUTATIONS:
            zs = m == 'slot0_read'
            a, b = lx.backward_model(key, mode16, None, zero_state=zs), lx.backward_model(key, mode16, m, zero_state=zs)
            assert not torch.equal(a['dgates'], b['dgates']) and not torch.equal(a['dgates16'], b['dgates16']), (mode16, m)
            assert not torch.equal(a['dh0'], b['dh0']), (mode16, m)
    assert set(lx.MUTATIONS) == set(lx.FWD_MUTATIONS) | set(lx.BWD_MUTATIONS) and len(lx.MUTATIONS) == 9


# ---- (4) the routes and the completeness of the case list --------------------------------------------------------------------------------------
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
    for C, want in T.ROWS[T.klass(mode)]:
        for g16 in ((False, True) if mode != 'f32' else (False,)):
            assert T.routes_of(ops, C, want, g16) == tuple(want), (mode, C, g16)
    for C, code in T.PROBE_C[T.klass(mode)]:
        assert ops.convlstm_seq_route(T.FWD, C, T.flags_of((code, 0), False)[0]) == code
    for C, code in T.PROBE_BWD_C[T.klass(mode)]:
        assert ops.convlstm_seq_route(T.BWD, C, T.PACK if code // 1000 == 3 else 0) == code


@pytest.mark.parametrize('k,modes', CLASSES)
def test_every_launching_pair_of_the_route_tables_has_an_exact_row(k, modes):
    table = list(R.lstm_rows()) + list(R.LSTM_EXTRA)
    for mode in modes:
        have = {(e, c) for case in T.cases() if case[0] == mode for e, c in enumerate(case[2])}
        need = {(r[1], r[-1]) for r in table if r[0] == mode and r[-1] > 0}
        assert len(need) >= 10 and need == have, (mode, sorted(need - have), sorted(have - need))
        # ... under exactly the flags the row's calls carry, with fp32 gates and (16-bit modes) with the fp16 gate buffer
        codes = {r[:-1]: r[-1] for r in table}
        for case in T.cases():
            if case[0] == mode:
                for g16 in ((False, True) if mode != 'f32' else (False,)):
                    fl = T.flags_of(case[2], g16)
                    assert (codes[(mode, T.FWD, case[1], fl[0])], codes[(mode, T.BWD, case[1], fl[1])]) == case[2]


def test_case_list_is_well_formed():
    cases = T.cases()
    assert len(set(cases)) == len(cases) and len(cases) == 2 * 5 + 4 * 2 + 2 * (2 * 9 + 4 * 3)
    for k, _ in CLASSES:
        fams = {c[2][0] // 1000 for c in cases if T.klass(c[0]) == k and (c[3], c[4]) != (35, 3)}
        assert fams == ({1, 2} if k == 'f32' else {1, 2, 3}), 'the M and T edges run at one C per forward family'
        bfams = {c[2][1] // 1000 for c in cases if T.klass(c[0]) == k and (c[3], c[4]) != (35, 3)}
        assert bfams == ({4} if k == 'f32' else {3, 4}), '... and per backward family'
    assert {(c[3], c[4]) for c in cases} == {(35, 3), (1, 3), (16, 3), (35, 1), (35, 2)}
    assert all(c[3] <= 35 and c[1] <= 512 and c[4] <= 3 for c in cases)
    assert {c[5] for c in cases if (c[3], c[4]) == (35, 3) and c[1] == 512} == {True, False}
