"""The video-to-events simulator on the host: the rule on the tests' restatement (tests/simulate_ref.py) -- the
worked example, the ramp, the invariant, cuts, the order -- the refractory rule, every limit on the restatement and on
``ops.simulate_check``, the response tables and thresholds of ``data/simulate.py``, the box array, and the three symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simulate_ref as sr  # noqa: E402
from leod_amd.data import simulate  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
LIN100 = [100 * v for v in range(256)]


def unpack(rec):
    return rec[:, 0].astype(np.int64), rec[:, 1] & 16383, (rec[:, 1] >> 14) & 16383, (rec[:, 1] >> 28) & 1


def one_pixel(values):
    return np.array(values, dtype=np.uint8).reshape(-1, 1, 1)


def full(h, w, v):
    return np.full((h, w), v, dtype=np.int32)


def random_case(seed, n=6, h=5, w=7):
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, 256, (n, h, w)).astype(np.uint8)
    times = np.cumsum(rng.randint(1, 3000, n)) + 17
    lut = np.sort(rng.randint(0, 60000, 256))
    th_on, th_off = rng.randint(200, 4000, (h, w)), rng.randint(200, 4000, (h, w))
    return frames, times, lut, th_on, th_off


def test_the_worked_example():
    s = sr.Sim(1, 1, LIN100, full(1, 1, 250), full(1, 1, 250))
    rec = s.feed(one_pixel([0, 10, 7, 9]), [0, 1000, 2000, 3000])
    t, x, y, p = unpack(rec)
    assert t.tolist() == [250, 500, 750, 1000, 1833] and p.tolist() == [1, 1, 1, 1, 0] and not x.any() and not y.any()
    assert s.m == [750] and s.t_keep == [1833] and s.invariant
    assert s.counters() == dict(frames=4, kept=5, on=4, off=1, dropped=0, t_last=3000)
    assert s.state().tolist() == [4, 5, 4, 1, 0, 3000, 0, 0, 750, 1833, 9]


@pytest.mark.parametrize('theta', [7, 13, 250, 999, 25200, 30000])
def test_a_monotone_ramp_gives_the_quotient(theta):
    values = [3, 3, 10, 11, 60, 200, 255]
    s = sr.Sim(1, 1, LIN100, full(1, 1, theta), full(1, 1, theta + 1))
    rec = s.feed(one_pixel(values), np.arange(len(values)) * 40000)
    assert len(rec) == (LIN100[255] - LIN100[3]) // theta and np.all(unpack(rec)[3] == 1)
    down = sr.Sim(1, 1, LIN100, full(1, 1, theta + 1), full(1, 1, theta))
    rec = down.feed(one_pixel(values[::-1]), np.arange(len(values)) * 40000)
    assert len(rec) == (LIN100[255] - LIN100[3]) // theta and np.all(unpack(rec)[3] == 0)


@pytest.mark.parametrize('seed', range(4))
def test_invariant_order_and_interval_on_random_input(seed):
    frames, times, lut, th_on, th_off = random_case(seed, n=8)
    s = sr.Sim(5, 7, lut, th_on, th_off, refractory_us=(0, 40)[seed % 2])
    rec = s.feed(frames, times)
    assert s.invariant and len(rec) > 100
    t, x, y, p = unpack(rec)
    assert np.all(np.diff(t) >= 0)
    assert len(s.intervals) == 7 and sum(len(ev) for _, _, ev in s.intervals) == len(rec)
    for t0, t1, ev in s.intervals:
        assert all(t0 < e[0] <= t1 for e in ev)
    keys = list(zip(t.tolist(), (y * 7 + x).tolist()))             # time, then pixel
    assert keys == sorted(keys)
    assert s.kept == s.on + s.off == len(rec) and int(p.sum()) == s.on


def test_cutting_the_frame_list_anywhere_changes_nothing():
    frames, times, lut, th_on, th_off = random_case(11, n=6, h=3, w=4)
    whole = sr.Sim(3, 4, lut, th_on, th_off, refractory_us=25)
    want = whole.feed(frames, times)
    assert whole.dropped > 0 and len(want) > 30
    for cut in range(len(frames) + 1):
        s = sr.Sim(3, 4, lut, th_on, th_off, refractory_us=25)
        got = np.concatenate([s.feed(frames[:cut], times[:cut]), s.feed(frames[cut:], times[cut:])])
        assert np.array_equal(got, want) and np.array_equal(s.state(), whole.state()), cut
    s = sr.Sim(3, 4, lut, th_on, th_off, refractory_us=25)
    got = np.concatenate([s.feed(frames[i:i + 1], times[i:i + 1]) for i in range(len(frames))])
    assert np.array_equal(got, want) and np.array_equal(s.state(), whole.state())


def test_a_time_the_division_leaves_at_the_earlier_frame_moves_one_microsecond():
    # the level 1 lies 1 / 25500 of the way: 1000 * 1 // 25500 = 0, and an interval is open at its start
    s = sr.Sim(1, 1, LIN100, full(1, 1, 7), full(1, 1, 7))
    rec = s.feed(one_pixel([0, 255]), [5000, 6000])
    assert rec[:3, 0].tolist() == [5001, 5001, 5001] and np.all(rec[:, 0] > 5000) and rec[-1, 0] == 5999     # 7, 14, 21: 0.27, 0.55, 0.82 us
    with pytest.raises(ValueError):
        sr.Sim(1, 1, LIN100, full(1, 1, 6), full(1, 1, 6))        # 25500 // 6 = 4250 candidates
    s = sr.Sim(1, 1, LIN100, full(1, 1, 7), full(1, 1, 7))
    rec = s.feed(one_pixel([0, 255]), [5000, 5001])               # an interval of 1 us: every event at its end
    assert len(rec) == 25500 // 7 and np.all(rec[:, 0] == 5001)


def test_the_refractory_rule_drops_counts_and_still_moves_m():
    free = sr.Sim(1, 1, LIN100, full(1, 1, 250), full(1, 1, 250))
    free.feed(one_pixel([0, 10, 7, 9]), [0, 1000, 2000, 3000])
    s = sr.Sim(1, 1, LIN100, full(1, 1, 250), full(1, 1, 250), refractory_us=300)
    rec = s.feed(one_pixel([0, 10, 7, 9]), [0, 1000, 2000, 3000])
    # 250 kept; 500 (250 behind) dropped; 750 kept; 1000 dropped; 1833 (1083 behind 750) kept
    assert unpack(rec)[0].tolist() == [250, 750, 1833] and unpack(rec)[3].tolist() == [1, 1, 0]
    assert s.dropped == 2 and s.kept == 3 and s.m == free.m == [750] and s.t_keep == [1833]
    exact = sr.Sim(1, 1, LIN100, full(1, 1, 250), full(1, 1, 250), refractory_us=250)      # t - t_keep < R: 250 behind is kept
    assert len(exact.feed(one_pixel([0, 10]), [0, 1000])) == 4 and exact.dropped == 0


def _limit_cases():
    ok = dict(height=4, width=5, times_us=[0, 10, 20], lut=LIN100, theta_on=full(4, 5, 250), theta_off=full(4, 5, 250), refractory_us=0)
    lut_hi, lut_neg = list(LIN100), list(LIN100)
    lut_hi[255], lut_neg[0] = 1 << 24, -1
    zero = full(4, 5, 250)
    zero[3, 4] = 0
    bad = [dict(height=0), dict(width=0), dict(height=16385, theta_on=250, theta_off=250), dict(width=16385, theta_on=250, theta_off=250),
           dict(height=True), dict(width=4.0), dict(lut=lut_hi), dict(lut=lut_neg), dict(lut=LIN100[:255]), dict(lut=[0.5] * 256),
           dict(theta_on=zero), dict(theta_off=zero), dict(theta_on=full(4, 4, 250)), dict(theta_off=full(5, 4, 250)),
           dict(theta_on=full(4, 5, 6)), dict(theta_off=full(4, 5, 6)),                  # 25500 // 6 = 4250 candidates
           dict(theta_on=np.full((4, 5), 250.0)), dict(refractory_us=-1), dict(refractory_us=1 << 32), dict(refractory_us=1.5),
           dict(times_us=[0, 10, 10]), dict(times_us=[0, 20, 10]), dict(times_us=[-1, 0, 1]), dict(times_us=[0, 1, 1 << 32]),
           dict(times_us=[0.0, 1.0, 2.0]), dict(times_us=[5, 6, 7], t_last=5), dict(times_us=[5, 6, 7], t_last=9)]
    return ok, bad


def test_every_limit_raises_value_error():
    from leod_amd import ops
    ok, bad = _limit_cases()
    times, lut, th_on, th_off = ops.simulate_check(**ok)
    assert (times.dtype, lut.dtype, th_on.dtype, th_off.shape) == (np.int64, np.int32, np.int32, (4, 5))
    assert ops.simulate_check(**{**ok, 'theta_on': 7, 'theta_off': 25500, 'times_us': [5, 6], 't_last': 4})[2].tolist() == full(4, 5, 7).tolist()
    assert ops.simulate_check(**{**ok, 'refractory_us': (1 << 32) - 1, 'times_us': [(1 << 32) - 1]})[0].tolist() == [(1 << 32) - 1]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.simulate_check(**{**ok, **kw})
    assert 16384 * 16384 < 1 << 30                               # sides inside their limit cannot reach 2^30 pixels: that limit is implied
    # the restatement refuses the same
    for kw in bad:
        a = {**ok, **kw}
        a['theta_on'] = a['theta_on'] if isinstance(a['theta_on'], np.ndarray) else full(4, 5, 250)
        with pytest.raises(ValueError):
            s = sr.Sim(a['height'], a['width'], a['lut'], a['theta_on'], a['theta_off'], a['refractory_us'])
            s.t_last = a.get('t_last', -1)
            s.frames = 1 if 't_last' in a else 0
            s.feed(np.zeros((3, 4, 5), np.uint8), a['times_us'])


@pytest.mark.parametrize('kind', simulate.LUTS)
def test_the_tables_are_monotone_and_inside_the_limits(kind):
    from leod_amd import ops
    lut = simulate.response_table(kind)
    assert lut.dtype == np.int32 and lut.shape == (256,) and lut[0] == 0 and np.all(np.diff(lut) >= 0) and lut[255] > lut[0]
    assert 0 <= lut.min() and lut.max() < 1 << 24
    th_on, th_off = simulate.thresholds(lut, 6, 8, 0.2, 0.2)
    assert np.all(th_on == 13107) and np.all(th_off == 13107) and th_on.dtype == np.int32     # round(0.2 * 65536)
    ops.simulate_check(6, 8, [0, 1], lut, th_on, th_off)
    # a sigma far above the contrast: the draw is clamped at the least threshold the table takes, and the op's check accepts it
    th_on, th_off = simulate.thresholds(lut, 6, 8, 0.2, 0.1, sigma=5.0, seed=3)
    least = simulate.least_threshold(lut)
    assert th_on.min() == least and th_off.min() == least and (int(lut.max()) - int(lut.min())) // least <= 4096
    assert least == 1 or (int(lut.max()) - int(lut.min())) // (least - 1) > 4096
    assert not np.array_equal(th_on, th_off) and len(np.unique(th_on)) > 10
    ops.simulate_check(6, 8, [0, 1], lut, th_on, th_off)
    again = simulate.thresholds(lut, 6, 8, 0.2, 0.1, sigma=5.0, seed=3)
    assert np.array_equal(again[0], th_on) and np.array_equal(again[1], th_off)
    with pytest.raises(ValueError):
        simulate.thresholds(lut, 6, 8, 0.0, 0.2)
    with pytest.raises(ValueError):
        simulate.thresholds(lut, 6, 8, 0.2, 0.2, sigma=-1.0)


def test_linlog_meets_the_logarithm_at_the_knee():
    lut = simulate.response_table('linlog')
    assert lut[20] == round(np.log(20) * 65536) and lut[255] == round(np.log(255) * 65536) and lut[10] == round(np.log(20) / 2 * 65536)
    assert simulate.response_table('linear')[255] == 65536 and simulate.response_table('log')[255] == round(np.log(256) * 65536)
    with pytest.raises(ValueError):
        simulate.response_table('gamma')


def test_luma_and_frame_times():
    rgb = np.array([[[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]]], dtype=np.uint8)
    assert simulate.luma(rgb).tolist() == [[[255, 0, 77, 149, 29, (770 + 3000 + 870 + 128) >> 8]]]
    grey = np.arange(12, dtype=np.uint8).reshape(1, 3, 4)
    assert np.array_equal(simulate.luma(grey), grey)
    for bad in (grey.astype(np.int32), grey[0], np.zeros((1, 2, 2, 4), np.uint8)):
        with pytest.raises(ValueError):
            simulate.luma(bad)
    assert simulate.frame_times(4, fps=30).tolist() == [0, 33333, 66667, 100000]
    assert simulate.frame_times(3, times=[5, 6, 9]).tolist() == [5, 6, 9]
    for kw in (dict(), dict(fps=30, times=[0, 1, 2]), dict(fps=0), dict(times=[0, 1]), dict(times=[0.0, 1.0, 2.0])):
        with pytest.raises(ValueError):
            simulate.frame_times(3, **kw)


def test_boxes_from_frames_is_the_array_the_labels_read():
    from leod_amd.data import ingest
    from leod_amd.data.genx_utils import labels
    times = simulate.frame_times(6, fps=20)
    boxes = simulate.boxes_from_frames([4, 1, 4, 2], [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [0.5, 1.5, 2.5, 3.5]], [0, 1, 1, 0], times)
    assert boxes.dtype == labels.BBOX_DTYPE == ingest.LABEL_DTYPE and boxes.dtype.itemsize == 40
    assert boxes['t'].tolist() == [50000, 100000, 200000, 200000] and boxes['x'].tolist() == [5, 0.5, 1, 9]
    assert boxes['class_id'].tolist() == [1, 0, 0, 1] and np.all(boxes['objectness'] == 1) and np.all(boxes['class_confidence'] == 1)
    lab, starts, repr_idx = ingest.convert_labels(boxes, 10, 50000)
    assert len(lab) == 4 and repr_idx.tolist() == [0, 1, 3] and starts.tolist() == [0, 1, 2]
    assert len(simulate.boxes_from_frames(np.zeros(0, np.int64), np.zeros((0, 4)), np.zeros(0, np.int64), times)) == 0
    for bad in (dict(frame_idx=[6]), dict(frame_idx=[-1]), dict(class_id=[-1]), dict(xywh=[[1, 2, 3]])):
        a = dict(frame_idx=[0], xywh=[[1, 2, 3, 4]], class_id=[0])
        a.update(bad)
        with pytest.raises(ValueError):
            simulate.boxes_from_frames(a['frame_idx'], a['xywh'], a['class_id'], times)


def test_options_are_checked_before_a_file_is_written(tmp_path):
    src = str(tmp_path / 'clip.npy')
    np.save(src, np.zeros((3, 4, 5), np.uint8))
    dst = str(tmp_path / 'out')
    for kw in (dict(), dict(fps=30, times=[0, 1, 2]), dict(fps=30, lut='gamma'), dict(fps=30, contrast=0.0), dict(fps=30, refractory_us=-1),
               dict(fps=30, write_events='evt4'), dict(fps=30, evt3_vectors=True), dict(times=[0, 2, 1]), dict(fps=30, batch_frames=0),
               dict(fps=30, contrast=1e-6), dict(fps=30, boxes=np.zeros(3))):
        with pytest.raises(ValueError):
            simulate.simulate_video(src, dst, **kw)
    assert not os.path.exists(dst)
    np.save(src, np.zeros((3, 4, 5), np.float32))
    with pytest.raises(ValueError):
        simulate.simulate_video(src, dst, fps=30)
    for argv in ([src, dst], [src, dst, '--fps', '30', '--times', 'x.npy'], [src, dst, '--fps', '30', '--lut', 'gamma']):
        with pytest.raises(SystemExit):
            simulate.main(argv)


def test_the_three_symbols_are_in_the_header_and_in_the_library():
    import __graft_entry__ as g
    g.build()
    from leod_amd import _lib, ops
    names = ('leod_simulate_query', 'leod_simulate_count', 'leod_simulate_emit')
    protos = _lib.parse_header()
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH], text=True)
    exported = set(re.findall(r'\bT (leod_\w+)', out))
    for name in names:
        assert name in protos and name in exported
    assert [a.__name__ for a in protos['leod_simulate_count'][1]][:1] == ['Ptr_unsigned_char']
    assert 'k_simulate.hip' in open(os.path.join(ROOT, 'leod_amd', 'csrc', 'Makefile')).read()
    # the query is host code: the state block of the rule, the sort's workspace
    tile, digit, n_state, n_count, ws = ops.simulate_query(1000, 5, 7)
    assert (tile, digit, n_state) == (256, 8, 8 + 2 * 35 + 5) and n_count == 1 + 18 and ws == 4 * (16 * 256) + 1024
    assert ops.simulate_query(0, 240, 304)[2] == 8 + 2 * 72960 + 9120
    for bad in ((-1, 5, 7), (1 << 31, 5, 7), (10, 0, 7), (10, 5, 16385)):
        with pytest.raises(_lib.LeodHipError):
            ops.simulate_query(*bad)
