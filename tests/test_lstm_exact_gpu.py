"""Every route of the ConvLSTM sequence kernels (csrc/lstm_route.hpp: lstm_seq_route / launch_lstm_seq in csrc/k_lstm.hip) and the per-timestep
cell kernels on the saturated-gate operands of tests/lstm_exact.py, in the three precision modes.  Forward: the gates and the whole c
history are EXACT (``torch.equal`` against ONE float64 recurrence), h lies within lstm_exact.H_BOUND = 7.05 * 2^-24 (derived there, absolute).
Backward: dgates (fp32 rows and the bf16 rows of the G16 path), dh0 and dc0 are exact against the float64 model, which rounds the dgates tile to
bf16 where the 16-bit kernels do.

Rows: every C of test_kernels_gpu.LSTM_SEQ_ROUTE_CASES_F32 in mode f32 and of test_bf16_gpu.LSTM_SEQ_ROUTE_CASES_16 in modes bf16 and 16f, at
M = 35 (two full 16-row tiles and a ragged one), T = 3 (both LDS buffers, the prefetch of t + 1 and of t + 2), with and without incoming
state; at one C per family (``EDGE_C``: fused, hoisted, streamed forward; resident and streamed backward) also M = 1, M = 16, T = 1 and
T = 2 (the ``T > 1`` and ``t + 2 < T`` loads are edges).  Every test first asserts that the router still sends the row where it says;
tests/test_lstm_exact_cpu.py asserts the same without a GPU, and that every (entry, code) pair that launches in the ConvLSTM tables of
tests/test_attn_lstm_routes_cpu.py has a row here, in every mode.

Forward, per row: (1) with fp32 ``gates_out``: gates and slots 1..T of cbuf equal, slots 1..T of hbuf within the bound; (2) with
``gates_out = None``: h and slot T of cbuf as before, slots 1..T-1 of cbuf still hold their sentinel.  Without incoming state (``zero_state``)
slot 0 of hbuf and cbuf is NaN before the call, and still after it.  Backward, per row: fp32 gates and, in the 16-bit modes, the fp16 gate
buffer of the G16 path; run twice with identical bits (no atomics); without incoming state slot 0 of cbuf is NaN under ``zero_state``; at the
``EDGE_C`` rows repeated with ``dh_seq = None``, ``dc_last = None`` and ``dh0 = dc0 = None``.  The G16 gate buffer is opaque and only a forward
launch can write it: the forward runs on lstm_exact's ``g16`` inputs (W_h = 0, three-valued pre-activations), whose fp32-gates instantiation
is first shown to equal the constructed gates.  The cbuf handed to the backward is always the CONSTRUCTED one, never that forward's.
Every output is a view into a larger buffer with one guard slab behind the last timestep (for [M, C] outputs: behind the last row), checked
untouched afterwards; a store to row M of slab t lands in row 0 of slab t + 1, which is compared (and in the guard for the last slab).

The per-timestep schedule (what runs in mode f32 at C >= 192): ``ops.convlstm_fwd`` chained T times on the forward problem at C = 32, 192, 384,
compared the same way, and ``ops.convlstm_gates_bwd`` on the last timestep of the backward problem, equal.

``test_device_takes_saturated_activations_exactly`` observes the assumptions on the device, per mode and family, with T = 1 and W = 0:
sigmoid(>= 128) == 1, sigmoid(<= -128) == 0, sigmoid(0) == 0.5, tanh(0) == 0, tanh(+-32 and beyond) == +-1 in the forward (tanhf in mode f32
and in the per-timestep kernels, the fast formula elsewhere), and a backward with known answer (c_t = +-32: dc == 0 exactly only if tanh is
exactly +-1).  If an equality fails elsewhere while it passes, the arithmetic holds on the device and the defect is in indexing.
A failure names timestep, row, channel and gate, and what decided that gate in the reference (x, h or the bias).
``pytest -m gpu``; ``-s`` prints the largest h error of every case as a fraction of the bound.

Observed on an MI355X (first run; 186 cases, 3.6 s in all): everything passes; every assumption of the probe test holds in the three modes --
no operand had to move.  Largest h error as a fraction of the bound: mode f32 0.069 (tanhf), mode bf16 0.236, mode 16f 0.236 (the fast
formula; 1.66 * 2^-24 against the derived 7.05 * 2^-24); the per-timestep kernels (tanhf) 0.069 in every mode.  With the streamed backward
as it stood before it took ``zero_state`` (it read slot 0 of cbuf at t = 0 whatever the flag said) the NaN-slot rows of routes 3192 .. 3512
fail, as the kernel's text says they must: run against that kernel, the twelve zero_state cases of test_backward_exact on those routes
(six shapes, modes bf16 and 16f) failed and the other 66 passed.

What the equality buys, measured once on an MI355X with ONE source mutation in a build that was never committed -- lstm_pack_kernel packing
the forward copy ``wpf`` with chunks kc = 0 and kc = 1 exchanged at C = 192 (wrong values only, every address in range): 12 of the 186 cases
here fail, namely every test_forward_exact case of route 3192 (six shapes, modes bf16 and 16f), e.g. "439 of 2304 gate values differ, first
got 0.0, exact 1.0 at timestep 0, row 0, channel 1, gate f: the reference has pre = 640.0, decided by h"; the backward cases pass (``wpb`` is
untouched).  test_convlstm_seq_every_route_16bit at its current bound notices this one too: its eight cases of route 3192 fail (h off by
0.85 .. 1.3 against 0.03 * 0.93; four test_convlstm_sequence_bf16 cases at C = 192 as well) -- 64 exchanged columns of dense Gaussian weights
are a gross error.  What the tolerance tests cannot do is say where: they report one number for T steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import lstm_exact as lx  # noqa: E402
import test_bf16_gpu as tb  # noqa: E402
import test_kernels_gpu as tk  # noqa: E402

DEV = 'cuda'
MODES = ('f32', 'bf16', '16f')
FWD, BWD = 0, 1
PROJ, GATES16, PACK = 1, 2, 4
NAN = float('nan')

ROWS = {'f32': [tuple(r) for r in tk.LSTM_SEQ_ROUTE_CASES_F32], '16': [tuple(r) for r in tb.LSTM_SEQ_ROUTE_CASES_16]}
# one C per family -- forward fused, hoisted, streamed; backward resident (the first two), streamed
EDGE_C = {'f32': (32, 64), '16': (32, 128, 192)}
MAIN = ((35, 3, True), (35, 3, False))                    # (M, T, incoming state)
EDGES = ((1, 3, True), (16, 3, False), (35, 1, True), (35, 2, False))
# seed of the backward problem per (C, M, T) where 0 does not clear the floors of tests/test_lstm_exact_cpu.py (32 elements per gate column)
BWD_SEED = {(32, 1, 3): 6, (64, 1, 3): 1}
PER_STEP_C = (32, 192, 384)
PROBE_C = {'f32': ((32, 1032), (64, 2064)), '16': ((32, 1032), (128, 2128), (192, 3192))}
PROBE_BWD_C = {'f32': ((32, 4032),), '16': ((32, 4032), (192, 3192))}


def klass(mode):
    return 'f32' if mode == 'f32' else '16'


def cases():
    """(mode, C, (forward code, backward code), M, T, state): the modes of one shape side by side, so that its cached reference is computed once"""
    out = []
    for mode in MODES:
        for C, want in ROWS[klass(mode)]:
            for M, T, state in MAIN + (EDGES if C in EDGE_C[klass(mode)] else ()):
                out.append((mode, C, tuple(want), M, T, state))
    return sorted(out, key=lambda c: (c[1], c[3], c[4], c[5], MODES.index(c[0])))


def _id(c):
    mode, C, want, M, T, state = c
    return f'{mode}-{want[0]}-{want[1]}-M{M}-T{T}-{"state" if state else "zero"}'


def flags_of(want, g16):
    """(forward flags, backward flags) of the calls a row makes"""
    fl = (PROJ if want[0] >= 2000 else 0) | (PACK if want[0] >= 3000 else 0) | (GATES16 if g16 else 0)
    return fl, fl & ~PROJ


def routes_of(ops, C, want, g16):
    fl = flags_of(want, g16)
    return ops.convlstm_seq_route(FWD, C, fl[0]), ops.convlstm_seq_route(BWD, C, fl[1])


def bwd_key(C, M, T):
    return (C, M, T, BWD_SEED.get((C, M, T), 0))


@pytest.fixture
def ops_in():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops
    prev = ops.get_precision()

    def enter(mode):
        ops.set_precision(mode)
        return ops
    yield enter
    ops.set_precision(prev)


def guarded(slots, slab, dtype=torch.float32):
    """-> (buffer of slots + 1 slabs full of the sentinel, the view of the first ``slots`` that a call is given)"""
    big = torch.full((slots + 1,) + tuple(slab), lx.SENTINEL, dtype=dtype, device=DEV)
    return big, big[:slots]


def untouched(big, what):
    assert bool((big[-1] == lx.SENTINEL).all()), f'{what}: the guard behind the output was written'


def first_bad(got, ref):
    bad = (got != ref).nonzero()
    return len(bad), bad[0].tolist()


def same_gates(got, p, what):
    got, ref = got.float().cpu(), p['ref']['gates'].float()
    if torch.equal(got, ref):
        return
    n, (t, m, g, ch) = first_bad(got, ref)
    raise AssertionError(f'{what}: {n} of {ref.numel()} gate values differ, first got {got[t, m, g, ch].item()!r}, exact {ref[t, m, g, ch].item()!r} at '
                         f'{lx.explain_forward(p, t, m, g, ch)}.  (If the probe test passes in this mode, the saturated arithmetic holds on the device.)')


def same_c(got, p, slots, what):
    """got [len(slots), M, C] equals the reference's c at those slots"""
    got, ref = got.float().cpu(), p['ref']['c'][list(slots)].float()
    if torch.equal(got, ref):
        return
    n, (k, m, ch) = first_bad(got, ref)
    t = slots[k] - 1
    raise AssertionError(f'{what}: {n} of {ref.numel()} c values differ, first c_{slots[k]} got {got[k, m, ch].item()!r}, exact {ref[k, m, ch].item()!r}; its gates: '
                         + '; '.join(lx.explain_forward(p, t, m, g, ch) for g in range(4)))


WORST_H = {}


def h_within_bound(got, p, mode, what):
    err = (got.double().cpu() - p['ref']['h'][1:]).abs()
    worst = float(err.max()) / lx.H_BOUND
    WORST_H[mode] = max(WORST_H.get(mode, 0.0), worst)
    print(f'LSTM_EXACT {mode} {what}: worst h error {worst:.4f} of the bound (largest so far in this mode {WORST_H[mode]:.4f})')
    if worst > 1.0:
        t, m, ch = (err == err.max()).nonzero()[0].tolist()
        raise AssertionError(f'{what}: h_{t + 1} is {worst:.3f} of its bound off at row {m}, channel {ch}: got {got[t, m, ch].item()!r}, reference '
                             f'{p["ref"]["h"][t + 1, m, ch].item()!r} = o tanh({p["ref"]["c"][t + 1, m, ch].item()!r}); '
                             + lx.explain_forward(p, t, m, 2, ch))


def seq_forward(ops, xin, proj, W, b, wpack, M, C, T, h0, c0, gates_out):
    """one forward launch on guarded state buffers; h0 / c0 None: zero_state with NaN in slot 0 -> (hbuf, cbuf) views, after the guard checks"""
    hbig, hb = guarded(T + 1, (M, C))
    cbig, cb = guarded(T + 1, (M, C))
    hb[0], cb[0] = (NAN, NAN) if h0 is None else (h0, c0)
    ops.convlstm_seq_fwd(xin, proj, hb, cb, W, b, gates_out, h0 is None, wpack)
    torch.cuda.synchronize()
    untouched(hbig, 'hbuf'); untouched(cbig, 'cbuf')
    if h0 is None:
        assert bool(hb[0].isnan().all()) and bool(cb[0].isnan().all()), 'slot 0 was written under zero_state'
    else:
        assert torch.equal(hb[0], h0) and torch.equal(cb[0], c0), 'the incoming state was overwritten'
    return hb, cb


@pytest.mark.parametrize('case', cases(), ids=_id)
def test_forward_exact(ops_in, case):
    mode, C, want, M, T, state = case
    ops = ops_in(mode)
    for g16 in ((False, True) if mode != 'f32' else (False,)):
        assert routes_of(ops, C, want, g16) == want, 'the channel count no longer reaches the routes this row is here for'
    p = lx.forward_problem(C, M, T, state)
    proj = want[0] >= 2000
    W, b, xin = p['W'].to(DEV), p['b'].to(DEV), (p['gx'] if proj else p['x']).to(DEV)
    wpack = ops.convlstm_seq_pack(W, C) if want[0] >= 3000 else None
    assert (wpack is not None) == (want[0] >= 3000)
    h0, c0 = (p['h0'].to(DEV), p['c0'].to(DEV)) if state else (None, None)
    tag = f'route {want[0]}, M = {M}, T = {T}, {"incoming state" if state else "zero_state, NaN in slot 0"}'
    # (1) fp32 gates_out: the gates and the whole c history
    gbig, go = guarded(T, (M, 4, C))
    hb, cb = seq_forward(ops, xin, proj, W, b, wpack, M, C, T, h0, c0, go)
    untouched(gbig, 'gates_out')
    same_gates(go, p, f'gates, {tag}')
    same_c(cb[1:], p, tuple(range(1, T + 1)), f'c history, {tag}')
    h_within_bound(hb[1:], p, mode, f'with gates_out, {tag}')
    # (2) no gates_out: h, the last c, and nothing else of cbuf
    hb, cb = seq_forward(ops, xin, proj, W, b, wpack, M, C, T, h0, c0, None)
    same_c(cb[T:], p, (T,), f'final c without gates_out, {tag}')
    h_within_bound(hb[1:], p, mode, f'without gates_out, {tag}')
    assert bool((cb[1:T] == lx.SENTINEL).all()), f'slots 1..T-1 of cbuf were written without gates_out, {tag}'


def same_grad(got, ref, what, C, per_gate):
    got, ref = got.float().cpu(), ref.float()
    if torch.equal(got, ref):
        return
    n, idx = first_bad(got, ref)
    where = (f'timestep {idx[0]}, row {idx[1]}, gate {lx.GATE_NAMES[idx[2] // C]}, channel {idx[2] % C}' if per_gate
             else f'row {idx[0]}, channel {idx[1]}')
    raise AssertionError(f'{what}: {n} of {ref.numel()} elements differ, first at {where}: got {got[tuple(idx)].item()!r}, exact {ref[tuple(idx)].item()!r}')


def g16_gates(ops, p, want, tag):
    """the G16 gate buffer of the constructed gates: a forward launch on the g16 inputs (W_h = 0), after its fp32-gates instantiation has
    been shown to produce exactly the constructed tensor"""
    C, M, T, q = p['C'], p['M'], p['T'], p['g16']
    proj = want[0] >= 2000
    W, b, xin = q['W'].to(DEV), q['b'].to(DEV), (q['gx'] if proj else q['x']).to(DEV)
    wpack = ops.convlstm_seq_pack(W, C) if want[0] >= 3000 else None
    gbig, go = guarded(T, (M, 4, C))
    seq_forward(ops, xin, proj, W, b, wpack, M, C, T, None, None, go)
    untouched(gbig, 'gates_out')
    got, ref = go.cpu(), p['gates']
    if not torch.equal(got, ref):
        n, (t, m, g, ch) = first_bad(got, ref)
        raise AssertionError(f'{tag}: the fp32 gates of the three-valued forward differ from the constructed ones in {n} elements, first at timestep {t}, '
                             f'row {m}, gate {lx.GATE_NAMES[g]}, channel {ch}: got {got[t, m, g, ch].item()!r}, constructed {ref[t, m, g, ch].item()!r}')
    big = ops.convlstm_gates16_buffer(T + 1, M, C, DEV)
    big.fill_(lx.SENTINEL)
    seq_forward(ops, xin, proj, W, b, wpack, M, C, T, None, None, big[:T])
    untouched(big, 'the fp16 gate buffer')
    return big[:T]


def seq_backward(ops, p, want, mode, gates, zero_state, dh_seq=True, dc_last=True, state_grads=True, tag=''):
    """one backward configuration, launched twice: equal to the model, identical bits, guards untouched"""
    C, M, T = p['C'], p['M'], p['T']
    key = (C, M, T, p['seed'])
    g16 = gates.dtype is torch.float16
    r = lx.backward_model(key, mode != 'f32', None, dh_seq, dc_last, zero_state)
    W = p['W'].to(DEV)
    wpack = ops.convlstm_seq_pack(W, C) if want[1] // 1000 == 3 else None
    cbuf = p['cbuf'].to(DEV)
    if zero_state:
        cbuf[0] = NAN
    dh, dcl = (p['dh_seq'].to(DEV) if dh_seq else None), (p['dc_last'].to(DEV) if dc_last else None)
    runs = []
    for _ in range(2):
        dbig, dg = guarded(T, (M, 4 * C), torch.bfloat16 if g16 else torch.float32)
        hbig, cbig = guarded(1, (M + 1, C)), guarded(1, (M + 1, C))                    # [M, C] outputs: one guard row behind the last row
        hbuf, cbuf0 = hbig[0][0], cbig[0][0]
        dh0, dc0 = (hbuf[:M], cbuf0[:M]) if state_grads else (None, None)
        assert ops.convlstm_seq_bwd(dh, dcl, gates, cbuf, W, dg, dh0, dc0, zero_state, wpack) is True
        torch.cuda.synchronize()
        untouched(dbig, 'dgates_out')
        for b_ in (hbuf, cbuf0):
            assert bool((b_[M:] == lx.SENTINEL).all()), f'{tag}: row M of dh0 / dc0 was written'
        if not state_grads:
            assert bool((hbuf == lx.SENTINEL).all()) and bool((cbuf0 == lx.SENTINEL).all())
        runs.append((dg, dh0, dc0))
    assert torch.equal(runs[0][0], runs[1][0]), f'{tag}: two runs of the backward differ in dgates'
    same_grad(runs[0][0], r['dgates16' if g16 else 'dgates'], f'{tag}: dgates ({"bf16 rows" if g16 else "fp32"})', C, True)
    if state_grads:
        assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2]), f'{tag}: two runs of the backward differ in dh0 / dc0'
        same_grad(runs[0][1], r['dh0'], f'{tag}: dh0', C, False)
        same_grad(runs[0][2], r['dc0'], f'{tag}: dc0', C, False)


@pytest.mark.parametrize('case', cases(), ids=_id)
def test_backward_exact(ops_in, case):
    mode, C, want, M, T, state = case
    ops = ops_in(mode)
    p = lx.backward_problem(*bwd_key(C, M, T))
    zero_state = not state
    edge_row = C in EDGE_C[klass(mode)] and (M, T) == (35, 3)
    for g16 in ((False, True) if mode != 'f32' else (False,)):
        assert routes_of(ops, C, want, g16) == want, 'the channel count no longer reaches the routes this row is here for'
        tag = f'route {want[1]}, M = {M}, T = {T}, {"fp16 gates" if g16 else "fp32 gates"}, {"zero_state, NaN in slot 0 of cbuf" if zero_state else "c_0 read"}'
        gates = g16_gates(ops, p, want, tag) if g16 else p['gates'].to(DEV)
        seq_backward(ops, p, want, mode, gates, zero_state, tag=tag)
        if edge_row:
            seq_backward(ops, p, want, mode, gates, zero_state, dh_seq=False, tag=tag + ', dh_seq = None')
            seq_backward(ops, p, want, mode, gates, zero_state, dc_last=False, tag=tag + ', dc_last = None')
            seq_backward(ops, p, want, mode, gates, zero_state, state_grads=False, tag=tag + ', dh0 = dc0 = None')


# ---- the per-timestep schedule on the same operands ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('state', (True, False), ids=('state', 'zero'))
@pytest.mark.parametrize('C', PER_STEP_C)
@pytest.mark.parametrize('mode', MODES)
def test_per_timestep_forward_exact(ops_in, mode, C, state):
    ops = ops_in(mode)
    p = lx.forward_problem(C, 35, 3, state)
    M, T = p['M'], p['T']
    W, b, x = p['W'].to(DEV), p['b'].to(DEV), p['x'].to(DEV)
    h, c = (p['h0'].to(DEV), p['c0'].to(DEV)) if state else (None, None)
    gs, cs, hs = [], [], []
    for t in range(T):
        hbig, cbig, gbig = guarded(1, (M, C)), guarded(1, (M, C)), guarded(1, (M, 4, C))
        h, c, g = ops.convlstm_fwd(x[t], h, c, W, b, h_out=hbig[1][0], c_out=cbig[1][0], gates_out=gbig[1][0])
        torch.cuda.synchronize()
        for big in (hbig, cbig, gbig):
            untouched(big[0], 'convlstm_fwd')
        gs.append(g); cs.append(c); hs.append(h)
    tag = f'per-timestep cell, C = {C}, {"incoming state" if state else "no state"}'
    same_gates(torch.stack(gs), p, f'gates, {tag}')
    same_c(torch.stack(cs), p, tuple(range(1, T + 1)), f'c history, {tag}')
    h_within_bound(torch.stack(hs), p, mode, tag)


@pytest.mark.parametrize('C', PER_STEP_C)
@pytest.mark.parametrize('mode', MODES)
def test_per_timestep_gate_backward_exact(ops_in, mode, C):
    """the pointwise gate backward on the last timestep of the backward problem (dh2 = None: nothing flows in from t + 1 there)"""
    ops = ops_in(mode)
    key = bwd_key(C, 35, 3)
    p, r = lx.backward_problem(*key), lx.backward_model(key, False)
    M, T = p['M'], p['T']
    s = r['steps'][T - 1]
    dbig, dg = guarded(1, (M, 4 * C))
    for c_prev in (p['cbuf'][T - 1].to(DEV), None):
        d, dcp = ops.convlstm_gates_bwd(p['dh_seq'][T - 1].to(DEV), p['dc_last'].to(DEV), p['gates'][T - 1].to(DEV), c_prev, p['cbuf'][T].to(DEV), dgates_out=dg[0])
        torch.cuda.synchronize()
        untouched(dbig, 'dgates')
        ref = s['d'].clone()
        if c_prev is None:
            ref[:, :C] = 0
        same_grad(d.view(1, M, 4 * C), ref.view(1, M, 4 * C), f'per-timestep gate backward, C = {C}, c_prev {"given" if c_prev is not None else "None"}', C, True)
        same_grad(dcp, s['dcn'], f'per-timestep dc_prev, C = {C}', C, False)


# ---- the assumptions, observed ------------------------------------------------------------------------------------------------------------
PROBE_VALUES = (128., -128., 136., -136., 1024., -1024., 30000., -30000., 0., 32., -32., 64., -64., 256., -256., 0.)


def probe_expectation(C):
    """channel ch holds PROBE_VALUES[ch % 16] in all four gate rows -> (v [C], sigmoid(v) or NaN where not claimed, tanh(v))"""
    v = torch.tensor(PROBE_VALUES, dtype=torch.float32).repeat(C // 16)
    sig = torch.where(v >= 128, 1.0, torch.where(v <= -128, 0.0, torch.where(v == 0, 0.5, NAN)))
    return v, sig, torch.sign(v)


@pytest.mark.parametrize('mode', MODES)
def test_device_takes_saturated_activations_exactly(ops_in, mode):
    ops = ops_in(mode)
    M = 16
    # forward, T = 1, W = 0: the pre-activation is the bias (fused) or gx (hoisted, streamed)
    for C, code in PROBE_C[klass(mode)]:
        assert ops.convlstm_seq_route(FWD, C, flags_of((code, 0), False)[0]) == code
        v, sig, th = probe_expectation(C)
        proj = code >= 2000
        W = torch.zeros((4 * C, 2 * C), device=DEV)
        wpack = ops.convlstm_seq_pack(W, C) if code >= 3000 else None
        b = torch.zeros(4 * C, device=DEV) if proj else v.repeat(4).to(DEV)
        xin = v.repeat(4).expand(1, M, 4 * C).contiguous().to(DEV) if proj else torch.zeros((1, M, C), device=DEV)
        gbig, go = guarded(1, (M, 4, C))
        hb, cb = seq_forward(ops, xin, proj, W, b, wpack, M, C, 1, None, None, go)
        got = go[0].cpu()
        tag = f'mode {mode}, route {code}'
        for g in range(3):
            bad = ((got[:, g] != sig) & ~sig.isnan()).nonzero()
            assert len(bad) == 0, f'{tag}: sigmoid({v[bad[0, 1]].item()}) is {got[bad[0, 0], g, bad[0, 1]].item()!r}, not {sig[bad[0, 1]].item()}'
        bad = (got[:, 3] != th).nonzero()
        assert len(bad) == 0, f'{tag}: tanh({v[bad[0, 1]].item()}) is {got[bad[0, 0], 3, bad[0, 1]].item()!r}, not {th[bad[0, 1]].item()}'
        known = ~sig.isnan()
        c_ref = (sig * th)[known].double()                                                # c_1 = i g from a zero state
        assert torch.equal(cb[1].cpu()[:, known].double(), c_ref.expand(M, -1)), f'{tag}: c_1 != i g'
        h_ref = sig[known].double() * torch.tanh(c_ref)
        worst = float((hb[1].cpu()[:, known].double() - h_ref).abs().max()) / lx.H_BOUND
        assert worst <= 1.0, f'{tag}: h_1 = o tanh(c_1) is {worst:.3f} of its bound off'
        assert bool((hb[1].cpu()[:, v == 0] == 0).all()), f'{tag}: o tanh(0) != 0 at c = 0'
    # backward with known answer: o = 1/2, i = f = 1, g = 0, c_0 = 0, dh = 1, dc_last = 0, W = 0; c_1 = +-32 -> th = +-1: dc == 0 exactly, d_o = +-1/4;
    # c_1 = 0 -> th = 0: dc = 1/2 = d_g = dc0, d_o = 0
    for C, code in PROBE_BWD_C[klass(mode)] + ((32, 0),):                                 # code 0: the per-timestep kernel (tanhf in every mode)
        ct = torch.tensor([32., -32., 0., 64.], dtype=torch.float32).repeat(C // 4).expand(M, C).contiguous()
        th = torch.sign(ct)
        gates = torch.zeros((1, M, 4, C))
        gates[:, :, 0], gates[:, :, 1], gates[:, :, 2] = 1.0, 1.0, 0.5
        cbuf = torch.stack([torch.zeros(M, C), ct])
        dh = torch.ones((1, M, C))
        want_d = torch.zeros((M, 4, C))
        want_d[:, 2], want_d[:, 3] = th * 0.25, (1 - th * th) * 0.5
        if code:
            assert ops.convlstm_seq_route(BWD, C, PACK if code // 1000 == 3 else 0) == code
            W = torch.zeros((4 * C, 2 * C), device=DEV)
            wpack = ops.convlstm_seq_pack(W, C) if code // 1000 == 3 else None
            dg, dh0, dc0 = (torch.full(s, lx.SENTINEL, device=DEV) for s in ((1, M, 4 * C), (M, C), (M, C)))
            assert ops.convlstm_seq_bwd(dh.to(DEV), None, gates.to(DEV), cbuf.to(DEV), W, dg, dh0, dc0, False, wpack) is True
            assert bool((dh0 == 0).all())
            d, dcp = dg[0], dc0
        else:
            d, dcp = ops.convlstm_gates_bwd(dh[0].to(DEV), None, gates[0].to(DEV), cbuf[0].to(DEV), cbuf[1].to(DEV))
        tag = f'mode {mode}, backward {code if code else "per-timestep"}'
        assert torch.equal(d.cpu().view(M, 4, C), want_d), f'{tag}: tanh(+-32), tanh(+-64) or tanh(0) is not exactly +-1 / 0 in the gate backward'
        assert torch.equal(dcp.cpu(), want_d[:, 3]), f'{tag}: dc0'
