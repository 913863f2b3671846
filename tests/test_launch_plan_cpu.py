"""ops.LaunchPlan is never torn down while a stream capture is open: close() -- which is also the finaliser the garbage collector calls at a
moment of its own choosing -- parks the plan, and the end of the last open capture releases it.  Checked without a GPU on a plan that owns no
native handle."""
import gc


class _Graph:
    """stands for the CUDAGraph a plan keeps alive; ``flag[0]`` turns False when it is destroyed (a weak reference would not do: the
    collector clears those before it runs the finaliser that parks the graph)"""

    def __init__(self, flag):
        self.flag = flag

    def __del__(self):
        self.flag[0] = False


def _plan(ops):
    flag = [True]
    p = ops.LaunchPlan.__new__(ops.LaunchPlan)
    p.handle, p.graph = 0, _Graph(flag)
    return p, lambda: flag[0] or None


def test_close_outside_a_capture_releases_at_once():
    from leod_amd import ops
    p, alive = _plan(ops)
    p.close()
    assert alive() is None and p.graph is None and not ops.LaunchPlan._parked
    p.close()                                                # idempotent


def test_close_inside_a_capture_is_deferred_to_its_end():
    from leod_amd import ops
    LP = ops.LaunchPlan
    assert LP._captures_open == 0 and not LP._parked
    LP.capture_opened()
    LP.capture_opened()                                      # nested: forward recorder still open while another begins
    try:
        p, alive = _plan(ops)
        p.close()
        assert alive() is not None and len(LP._parked) == 1 and p.graph is None
        q, _ = _plan(ops)
        graph_q = id(q.graph)
        ring = [q]
        ring.append(ring)                                    # a plan that only the cyclic collector frees
        del q, ring
        gc.collect()                                         # the collector finalises the plan: its graph is parked, not dropped
        assert len(LP._parked) == 2 and id(LP._parked[1][1]) == graph_q
        LP.capture_closed()
        assert alive() is not None and len(LP._parked) == 2  # one capture is still open
    finally:
        while LP._captures_open:
            LP.capture_closed()
    assert alive() is None and not LP._parked


def test_recorder_counts_its_capture_even_when_it_fails(monkeypatch):
    import torch
    from leod_amd import ops
    from leod_amd.modules import step_plan

    class Graph:
        def __init__(self, keep_graph=True):
            pass

        def capture_begin(self, pool=None, capture_error_mode=None):
            assert ops.LaunchPlan._captures_open == 1

        def capture_end(self):
            raise RuntimeError('capture failed')
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', Graph)
    rec = step_plan.PlanRecorder(2, pool=object())
    rec.begin()
    assert rec.capturing and ops.LaunchPlan._captures_open == 1
    try:
        rec._capture_end()
    except RuntimeError:
        pass
    assert not rec.capturing and ops.LaunchPlan._captures_open == 0


def test_engine_capture_tells_the_plans_about_its_capture(monkeypatch):
    import contextlib
    import pytest
    import torch
    from leod_amd import ops
    from leod_amd.engine import TrainEngine
    LP = ops.LaunchPlan
    seen = []

    @contextlib.contextmanager
    def graph(g):
        seen.append(('begin', LP._captures_open))
        yield
        seen.append(('end', LP._captures_open))
    monkeypatch.setattr(torch.cuda, 'graph', graph)
    monkeypatch.setattr(ops, 'weight_shadow_pin', lambda on: seen.append(('pin', on)))
    eng = TrainEngine.__new__(TrainEngine)
    eng._graph = object()

    def body(fail):
        seen.append(('body', LP._captures_open))
        if fail:
            raise RuntimeError('body failed')
        return 'losses'
    assert LP._captures_open == 0
    eng._graph_body = lambda: body(False)
    eng._capture_graph()
    assert seen == [('pin', True), ('begin', 1), ('body', 1), ('end', 1), ('pin', False)] and LP._captures_open == 0
    assert eng._g_losses == 'losses'
    del seen[:]
    eng._graph_body = lambda: body(True)
    with pytest.raises(RuntimeError, match='body failed'):
        eng._capture_graph()
    assert seen == [('pin', True), ('begin', 1), ('body', 1), ('pin', False)] and LP._captures_open == 0
