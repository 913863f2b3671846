"""The corner behaviour of the launch-plan cache (modules/step_plan.py), checked without a GPU: ``BackbonePlan.capture`` / ``HeadPlan.capture``
are replaced by stubs that succeed (recorders with ``close()`` and ``info()``) or raise, the plans themselves live on CPU tensors.  What a
step launches is the GPU tests' business; this file pins what only matters when something goes wrong -- second sight, failed and evicted
captures, the pruning of markers, the head LRU, the counters' report, the refusal of a backward whose activations are gone, and what the
capture harness leaves behind when a recorded pass raises."""
import warnings

import pytest
import torch

from leod_amd import ops
from leod_amd._lib import LeodHipError
from leod_amd.modules import step_plan
from leod_amd.modules.step_plan import BackbonePlan, HeadPlan, TrainStepPlans, SEEN, EAGER, CAPTURE

INFO_KEYS = ('kernels', 'memsets', 'memcpys', 'lanes', 'waits', 'segments', 'callbacks', 'collectives')
COUNTER_KEYS = {'captures', 'head_captures', 'head_plans', 'planned_steps', 'replays', 'eager_steps', 'plan_hit_rate'}
KERNEL_KEYS = {'backbone_forward_kernels', 'head_forward_kernels', 'head_backward_kernels', 'backbone_backward_kernels'}


class _Rec:
    """stands for a PlanRecorder: counts its ``close()`` calls, reports ``info()``"""

    def __init__(self, log=None, name='', **info):
        self.closed, self.log, self.name = 0, log, name
        self._info = dict(zip(INFO_KEYS, (0,) * len(INFO_KEYS)), **info)

    def info(self):
        return dict(self._info)

    def join(self):
        self.log.append(self.name + '.join')

    def close(self):
        self.closed += 1


@pytest.fixture
def stubs(monkeypatch):
    """small arenas; captures that succeed unless the module handed over is an exception to raise"""
    monkeypatch.setattr(ops.StatArena, 'SIZE', 64)

    def capture(self, module, wgrad_side, max_lanes):
        if isinstance(module, BaseException):
            raise module
        self.fwd, self.bwd = _Rec(), _Rec()
        return self
    monkeypatch.setattr(BackbonePlan, 'capture', capture)
    monkeypatch.setattr(HeadPlan, 'capture', capture)


def _ev(n=1):
    return torch.zeros(2, n, 1, 2, 2, dtype=torch.uint8)


_LIKE = [(torch.zeros(1), torch.zeros(1))]


def _build(plans, key, module=None):
    return plans.build(key, module, _ev(), _LIKE, True)


def _backbone():
    return BackbonePlan('k', None, _ev(), _LIKE)


# ---- TrainStepPlans.lookup / build ---------------------------------------------------------------------------------------------

def test_lookup_first_sight_second_sight_held_plan_and_eager(stubs):
    plans = TrainStepPlans()
    assert plans.lookup('a') is None and plans.entries['a'] is SEEN
    assert plans.lookup('a') is CAPTURE and plans.lookup('a') is CAPTURE          # until somebody builds it
    a = _build(plans, 'a')
    assert plans.lookup('b') is None and plans.lookup('b') is CAPTURE
    b = _build(plans, 'b')
    assert list(plans.entries) == ['a', 'b']
    assert plans.lookup('a') is a and list(plans.entries) == ['b', 'a']              # a held plan becomes most recently used
    assert plans.lookup('b') is b and list(plans.entries) == ['a', 'b']
    plans.entries['c'] = EAGER
    assert plans.lookup('c') is None and plans.lookup('c') is None and plans.entries['c'] is EAGER


def test_build_success_counts_and_holds_the_plan(stubs):
    plans = TrainStepPlans()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        a = _build(plans, 'a')
    assert isinstance(a, BackbonePlan) and plans.entries['a'] is a and plans.captures == 1 and a.fwd.closed == 0


@pytest.mark.parametrize('exc', [LeodHipError('no such node'), RuntimeError('capture broke')])
def test_build_failure_warns_closes_and_marks_eager(stubs, monkeypatch, exc):
    plans = TrainStepPlans()
    closed = []
    monkeypatch.setattr(BackbonePlan, 'close', lambda self: closed.append(self))
    plans.lookup('a')
    with pytest.warns(UserWarning, match=r'leod_amd: the backbone of geometry a could not be turned into a launch plan '
                                         rf'\({exc}\); its steps stay eager'):
        assert _build(plans, 'a', exc) is None
    assert len(closed) == 1 and isinstance(closed[0], BackbonePlan)
    assert plans.entries['a'] is EAGER and plans.captures == 0
    assert plans.lookup('a') is None and plans.entries['a'] is EAGER


def test_build_does_not_swallow_other_exceptions(stubs):
    plans = TrainStepPlans()
    with pytest.raises(KeyError):
        _build(plans, 'a', KeyError('x'))


def test_build_evicts_the_least_recently_used_plan_for_good(stubs):
    plans = TrainStepPlans(max_plans=2)
    a, b = _build(plans, 'a'), _build(plans, 'b')
    assert plans.lookup('a') is a                                                    # b is now the least recently used
    b_recs = (b.fwd, b.bwd)
    c = _build(plans, 'c')
    assert [r.closed for r in b_recs] == [1, 1] and b.fwd is None and a.fwd.closed == 0
    assert plans.entries['b'] is EAGER and plans.entries['a'] is a and plans.entries['c'] is c and plans.captures == 3
    assert plans.lookup('b') is None and plans.lookup('b') is None and plans.entries['b'] is EAGER      # never recaptured
    assert len([v for v in plans.entries.values() if isinstance(v, BackbonePlan)]) == 2


def test_lookup_prunes_seen_markers_beyond_64_entries_and_eager_markers_beyond_256(stubs):
    plans = TrainStepPlans()
    a = _build(plans, 'plan')
    for k in range(64):
        assert plans.lookup(('s', k)) is None
    assert len(plans.entries) == 65                                                   # nothing is pruned up to 64 entries + the new one
    assert plans.lookup('new') is None
    assert list(plans.entries) == ['plan', 'new'] and plans.entries['new'] is SEEN and plans.entries['plan'] is a
    for k in range(300):
        plans.entries[('e', k)] = EAGER
    assert plans.lookup('newer') is None
    assert list(plans.entries) == ['plan'] + [('e', k) for k in range(44, 300)] + ['newer']        # the oldest eager markers go
    assert plans.lookup(('e', 43)) is None and plans.entries[('e', 43)] is SEEN                    # a forgotten geometry starts over


# ---- head plans -----------------------------------------------------------------------------------------------------------------

def test_head_key_of_pads_the_label_width():
    P = step_plan.NMAX_PAD
    assert P == 8
    for nmax, want in ((0, P), (1, P), (P - 1, P), (P, P), (P + 1, 2 * P), (2 * P, 2 * P), (5 * P + 3, 6 * P)):
        assert TrainStepPlans.head_key_of(3, nmax) == ((3, want), want)


def test_heads_are_kept_most_recently_used_last_and_evicted_at_max_heads(stubs):
    plans = TrainStepPlans()
    bb = _backbone()
    bb.max_heads = 2
    assert bb.head('h1') is None
    h1 = plans.build_head(bb, 'h1', None, 3, 8, True)
    h2 = plans.build_head(bb, 'h2', None, 4, 8, True)
    assert isinstance(h1, HeadPlan) and h1.labels.shape == (3, 8, 7) and plans.head_captures == 2 and list(bb.heads) == ['h1', 'h2']
    assert bb.head('h1') is h1 and list(bb.heads) == ['h2', 'h1']
    h2_recs = (h2.fwd, h2.bwd)
    h3 = plans.build_head(bb, 'h3', None, 5, 8, True)
    assert list(bb.heads) == ['h1', 'h3'] and [r.closed for r in h2_recs] == [1, 1] and h2.fwd is None and h1.fwd.closed == 0
    assert bb.head('h2') is None and bb.head('h3') is h3 and plans.head_captures == 3
    bb.fwd, bb.bwd = _Rec(), _Rec()
    recs = [r for h in (h1, h3) for r in (h.fwd, h.bwd)] + [bb.fwd, bb.bwd]
    bb.close()
    assert [r.closed for r in recs] == [1] * 6 and not bb.heads and bb.fwd is None


def test_failed_head_capture_is_remembered_as_eager(stubs, monkeypatch):
    plans = TrainStepPlans()
    bb = _backbone()
    bb.max_heads = 2
    closed = []
    monkeypatch.setattr(HeadPlan, 'close', lambda self: closed.append(self))
    with pytest.warns(UserWarning, match=r'leod_amd: the head pass for 3 labelled frames could not be turned into a launch plan '
                                         r'\(no\); such steps stay eager'):
        assert plans.build_head(bb, 'h1', LeodHipError('no'), 3, 8, True) is None
    assert len(closed) == 1 and plans.head_captures == 0
    assert bb.heads['h1'] is EAGER and bb.head('h1') is EAGER                        # not None: the caller does not capture it again
    plans.build_head(bb, 'h2', None, 4, 8, True)
    plans.build_head(bb, 'h3', None, 5, 8, True)                                     # evicting a marker closes nothing
    assert list(bb.heads) == ['h2', 'h3'] and len(closed) == 1
    bb.add_head('h4', EAGER)
    bb.close()                                                                       # ... and neither does closing over one


# ---- counters and info() --------------------------------------------------------------------------------------------------------

def test_hit_rate():
    plans = TrainStepPlans()
    assert plans.hit_rate() == 0.0
    plans.steps, plans.eager_steps, plans.replays = 6, 2, 5
    assert plans.hit_rate() == 5 / 8


def _info_plans(stubs_bb_info, stubs_bw_info):
    plans = TrainStepPlans()
    _build(plans, 'old')
    bb = _build(plans, 'a')
    bb.fwd, bb.bwd = _Rec(**stubs_bb_info), _Rec(**stubs_bw_info)
    plans.steps, plans.replays, plans.eager_steps, plans.head_captures = 7, 5, 2, 9
    return plans, bb


BF = dict(kernels=100, memsets=1, memcpys=2, lanes=2, waits=10, segments=1, callbacks=0, collectives=0)
BW = dict(kernels=200, memsets=3, memcpys=0, lanes=3, waits=20, segments=2, callbacks=1, collectives=1)
HF = dict(kernels=30, memsets=4, memcpys=1, lanes=1, waits=5, segments=3, callbacks=2, collectives=2)
HW = dict(kernels=40, memsets=0, memcpys=5, lanes=4, waits=6, segments=4, callbacks=3, collectives=3)


def test_info_without_a_plan(stubs):
    plans = TrainStepPlans()
    assert plans.info() is None
    plans.lookup('a')
    plans.entries['b'] = EAGER
    assert plans.info() is None
    bb = _build(plans, 'a')
    bb.fwd = None                                                                     # a closed backbone plan and no head plan
    assert plans.info() is None


@pytest.mark.parametrize('marker', [False, True])
def test_info_planned_backbone_eager_head(stubs, marker):
    plans, bb = _info_plans(BF, BW)
    if marker:
        bb.add_head('h', EAGER)
    info = plans.info()
    assert set(info) == {'forward', 'backward', 'head'} | KERNEL_KEYS | COUNTER_KEYS
    assert info['forward'] == BF and info['backward'] == BW and info['head'] == 'eager'
    assert tuple(info['forward']) == INFO_KEYS
    assert (info['backbone_forward_kernels'], info['head_forward_kernels'], info['head_backward_kernels'], info['backbone_backward_kernels']) \
        == (100, None, None, 200)
    assert {k: info[k] for k in COUNTER_KEYS} == dict(captures=2, head_captures=0, head_plans=0, planned_steps=7, replays=5, eager_steps=2,
                                                      plan_hit_rate=round(5 / 9, 4))


def test_info_backbone_and_head(stubs):
    plans, bb = _info_plans(BF, BW)
    plans.build_head(bb, 'h0', None, 2, 8, True)
    bb.add_head('he', EAGER)
    hd = plans.build_head(bb, 'h1', None, 3, 8, True)                                # the most recently used head is reported
    hd.fwd, hd.bwd = _Rec(**HF), _Rec(**HW)
    info = plans.info()
    assert set(info) == {'forward', 'backward'} | KERNEL_KEYS | COUNTER_KEYS          # no 'head' entry
    assert info['forward'] == dict(kernels=130, memsets=5, memcpys=3, lanes=2, waits=15, segments=4, callbacks=2, collectives=2)
    assert info['backward'] == dict(kernels=240, memsets=3, memcpys=5, lanes=4, waits=26, segments=6, callbacks=4, collectives=4)
    assert (info['backbone_forward_kernels'], info['head_forward_kernels'], info['head_backward_kernels'], info['backbone_backward_kernels']) \
        == (100, 30, 40, 200)
    assert {k: info[k] for k in COUNTER_KEYS} == dict(captures=2, head_captures=11, head_plans=2, planned_steps=7, replays=5, eager_steps=2,
                                                      plan_hit_rate=round(5 / 9, 4))


class _LP:
    def __init__(self, **info):
        self.info = info


def test_recorder_info_sums_its_segments_and_takes_the_widest_lane_count():
    rec = step_plan.PlanRecorder(2, pool=object())
    assert rec.info() == dict(zip(INFO_KEYS, (0,) * 8))
    rec.segments = [(_LP(kernels=5, memsets=1, memcpys=2, lanes=2, waits=3, collectives=1), print), (None, print),
                    (_LP(kernels=7, memsets=0, memcpys=1, lanes=3, waits=4), None)]                  # an old plan without 'collectives'
    info = rec.info()
    assert tuple(info) == INFO_KEYS
    assert info == dict(kernels=12, memsets=1, memcpys=3, lanes=3, waits=7, segments=3, callbacks=2, collectives=1)


# ---- the refusal: a planned step's backward needs the activations of ITS forward ---------------------------------------------------

REFUSAL = 'backward\\(\\) of a planned training step whose activations are gone'


def _planned_pair(log):
    bb = _backbone()
    bb.fwd, bb.bwd = _Rec(log, 'bb.fwd'), _Rec(log, 'bb.bwd')
    bb.run_backward = lambda: log.append('bb.run_backward')
    hd = HeadPlan(bb, 2, 8)
    hd.fwd, hd.bwd = _Rec(log, 'hd.fwd'), _Rec(log, 'hd.bwd')
    hd.run_backward = lambda g: log.append(('hd.run_backward', float(g)))
    return bb, hd


def _loss_step(bb, hd, anchor):
    bb.uses += 1                                                                     # BackbonePlan.run_forward
    return step_plan.PlanLossFn.apply(bb, hd, anchor, torch.tensor(1.5))


def _gate_step(bb, anchor, stages=(2, 3)):
    bb.uses += 1
    return step_plan.EagerHeadGate.apply(bb, anchor, torch.tensor([0, 2]), *stages)


@pytest.fixture
def gate_bb(monkeypatch):
    def copy_multi(dst, src):
        for d, s in zip(dst, src):
            d.copy_(s)
    monkeypatch.setattr(ops, 'copy_multi', copy_multi)
    monkeypatch.setattr(ops.StatArena, 'SIZE', 64)
    log = []
    bb, _ = _planned_pair(log)
    bb.x_out = {k: torch.arange(8.).view(4, 2) * k for k in (2, 3)}
    bb.gsel = {k: torch.full((4, 2), 7.) for k in (2, 3)}
    return bb, log


def test_plan_loss_backward_claims_the_activations_and_launches_head_then_backbone(stubs):
    log = []
    bb, hd = _planned_pair(log)
    anchor = torch.zeros(1, requires_grad=True)
    loss = _loss_step(bb, hd, anchor)
    assert float(loss.detach()) == 1.5 and loss.requires_grad and bb.consumed == -1
    (loss * 2).backward()
    assert log == [('hd.run_backward', 2.0), 'bb.run_backward', 'hd.bwd.join'] and bb.consumed == bb.uses == 1
    loss = _loss_step(bb, hd, anchor)                                                # the next step of the same plan is fine
    loss.backward()
    assert log[3:] == [('hd.run_backward', 1.0), 'bb.run_backward', 'hd.bwd.join'] and bb.consumed == 2


def test_plan_loss_backward_is_refused_when_the_activations_are_gone(stubs):
    log = []
    bb, hd = _planned_pair(log)
    anchor = torch.zeros(1, requires_grad=True)
    first = _loss_step(bb, hd, anchor)
    second = _loss_step(bb, hd, anchor)
    with pytest.raises(RuntimeError, match=REFUSAL):                                 # another forward of the same plan ran in between
        first.backward()
    assert log == [] and bb.consumed == -1
    second.backward(retain_graph=True)
    assert len(log) == 3 and bb.consumed == 2
    with pytest.raises(RuntimeError, match=REFUSAL):                                 # backward twice
        second.backward()
    third = _loss_step(bb, hd, anchor)
    hd.close()                                                                       # the head plan was evicted
    with pytest.raises(RuntimeError, match=REFUSAL):
        third.backward()
    hd2 = HeadPlan(bb, 2, 8)
    hd2.fwd, hd2.bwd, hd2.run_backward = _Rec(log), _Rec(log), (lambda g: None)
    fourth = _loss_step(bb, hd2, anchor)
    bb.close()                                                                       # the backbone plan was evicted
    with pytest.raises(RuntimeError, match=REFUSAL):
        fourth.backward()
    assert len(log) == 3 and bb.consumed == 2


def test_eager_head_gate_backward_claims_fills_the_slots_and_launches_the_backbone(gate_bb):
    bb, log = gate_bb
    anchor = torch.zeros(1, requires_grad=True)
    s2, s3 = _gate_step(bb, anchor)
    assert torch.equal(s2, bb.x_out[2][[0, 2]]) and torch.equal(s3, bb.x_out[3][[0, 2]]) and s2.requires_grad
    (s2 * 3).sum().backward()                                                        # no gradient reaches stage 3: its slots are zeroed
    assert log == ['bb.run_backward'] and bb.consumed == bb.uses == 1
    assert torch.equal(bb.gsel[2], torch.tensor([[3., 3.], [3., 3.], [7., 7.], [7., 7.]]))
    assert torch.equal(bb.gsel[3], torch.tensor([[0., 0.], [0., 0.], [7., 7.], [7., 7.]]))


def test_eager_head_gate_backward_is_refused_when_the_activations_are_gone(gate_bb):
    bb, log = gate_bb
    anchor = torch.zeros(1, requires_grad=True)
    first = _gate_step(bb, anchor)[0].sum()
    second = _gate_step(bb, anchor)[0].sum()
    with pytest.raises(RuntimeError, match=REFUSAL):
        first.backward()
    second.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match=REFUSAL):
        second.backward()
    third = _gate_step(bb, anchor)[0].sum()
    bb.close()
    with pytest.raises(RuntimeError, match=REFUSAL):
        third.backward()
    assert log == ['bb.run_backward'] and bb.consumed == 2


# ---- the capture harness restores what it touched ----------------------------------------------------------------------------------

def test_failed_capture_leaves_nothing_behind(monkeypatch):
    """``HeadPlan.capture`` through the real ``step_capture`` on a machine without a device: torch's stream / graph entry points are stubs,
    the head's forward pass counts a BatchNorm call, flips the process-wide switches the way a recorded step does, and raises."""
    import contextlib
    from types import SimpleNamespace
    from leod_amd import functions as Fn
    from leod_amd.parallel import GradBuckets
    events = []

    class Stream:
        def __init__(self, device=None):
            pass

        def wait_stream(self, other):
            events.append('wait_stream')

    class Graph:
        def __init__(self, keep_graph=True):
            pass

        def capture_begin(self, pool=None, capture_error_mode=None):
            events.append(('capture_begin', ops.LaunchPlan._captures_open))

        def capture_end(self):
            events.append('capture_end')
    monkeypatch.setattr(torch.cuda, 'Stream', Stream)
    monkeypatch.setattr(torch.cuda, 'stream', lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: Stream())
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a: events.append('synchronize'))
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', Graph)
    monkeypatch.setattr(ops.StatArena, 'SIZE', 64)
    arena, buckets = torch.zeros(8, dtype=torch.uint8), object()
    monkeypatch.setattr(ops.StatArena, 'buf', arena)
    monkeypatch.setattr(ops.StatArena, 'off', 3)
    monkeypatch.setattr(ops.StatArena, 'high', 5)
    monkeypatch.setattr(ops.StatArena, 'active', True)
    monkeypatch.setattr(GradBuckets, 'current', buckets)
    monkeypatch.setattr(Fn.WgradSide, 'active', True)
    bn = torch.nn.Module()
    bn.bn_calls_pending = 4

    def forward_detect(backbone_features, targets):
        assert step_plan.PlanRecorder.current is not None and step_plan.PlanRecorder.current.capturing
        assert ops.StatArena.buf is bb.head_arena and ops.StatArena.active and torch.is_grad_enabled()
        bn.bn_calls_pending += 1
        GradBuckets.current, Fn.WgradSide.active = None, False
        raise LeodHipError('a node the plan cannot hold')
    mdl = SimpleNamespace(fpn=SimpleNamespace(in_features=(2,)), modules=lambda: [bn], forward_detect=forward_detect)
    bb = _backbone()
    bb.head_pool = object()
    bb.x_out = {2: torch.zeros(4, 1, 1, 2)}
    bb.rows[:2] = torch.tensor([0, 3])
    hd = HeadPlan(bb, 2, 8)
    epoch = ops.PackCache.epoch
    with torch.no_grad():
        with pytest.raises(LeodHipError, match='cannot hold'):
            hd.capture(SimpleNamespace(mdl=mdl), True, 2)
        assert not torch.is_grad_enabled()
    assert events == ['wait_stream', 'synchronize', ('capture_begin', 1), 'capture_end', 'wait_stream']
    assert step_plan.PlanRecorder.current is None and ops.LaunchPlan._captures_open == 0 and not ops.LaunchPlan._parked
    assert (ops.StatArena.buf, ops.StatArena.off, ops.StatArena.high, ops.StatArena.active) == (arena, 3, 5, True)
    assert GradBuckets.current is buckets and Fn.WgradSide.active is True
    assert bn.bn_calls_pending == 4 and hd.bn_incs == [(bn, 1)]
    assert hd.fwd is None and hd.bwd is None and ops.PackCache.epoch == epoch + 2
