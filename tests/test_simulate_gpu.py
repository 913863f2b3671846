"""``ops.simulate_events`` (csrc/k_simulate.hip) against the sequential restatement of tests/simulate_ref.py, byte for byte in the records
and in the state block, and ``data/simulate.py`` end to end into the ingestion."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simulate_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GEOMETRIES = [(5, 7), (16, 17), (33, 67)]         # one partial tile of pixels; just over one; 2 211 pixels: several tiles, and of events many sort tiles
CASES = ('random', 'together', 'swing', 'identical', 'one_us', 'three_passes', 'refractory')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as _ops
    return _ops


def _err():
    from leod_amd._lib import LeodHipError
    return LeodHipError


@functools.lru_cache(maxsize=None)
def case(name, h, w):
    """-> dict(frames, times, lut, th_on, th_off, refr) of a case at a geometry; the same arrays every time."""
    rng = np.random.RandomState(h * 1000 + w + 17 * CASES.index(name))
    P = h * w
    lut = np.sort(rng.randint(0, 60000, 256)).astype(np.int64)
    th_on, th_off = rng.randint(200, 4000, (h, w)), rng.randint(200, 4000, (h, w))       # non-uniform maps, theta_on != theta_off
    frames = rng.randint(0, 256, (5, h, w)).astype(np.uint8)
    times = np.cumsum(rng.randint(1, 3000, 5)) + 40                                      # a span below 2^16: two passes of the sort
    refr = 0
    if name == 'together':                                       # every pixel steps with every other: all events of an interval tie in time
        frames = np.broadcast_to(np.array([10, 200, 50, 50, 255, 0], dtype=np.uint8)[:, None, None], (6, h, w)).copy()
        th_on, th_off = np.full((h, w), 1500), np.full((h, w), 1500)
        times = np.array([0, 700, 1400, 2100, 2800, 3500])
    elif name == 'swing':                                        # 0 -> 255 -> 0 at the least threshold the table allows: 4095 candidates
        lut = np.arange(256, dtype=np.int64) * 257
        th_on, th_off = np.full((h, w), 16), np.full((h, w), 16)                         # 65535 // 16 = 4095; 15 would give 4369
        swing = (np.arange(P) % 61 == 3).reshape(h, w)                                   # on some pixels: the restatement is plain Python
        frames = np.full((4, h, w), 7, dtype=np.uint8)
        frames[:, swing] = np.array([0, 255, 0, 255], dtype=np.uint8)[:, None]
        times = np.array([1000, 6000, 11000, 11900])
    elif name == 'identical':
        frames = np.repeat(frames[:1], 5, axis=0)
    elif name == 'one_us':                                       # a span of 1 us: no pass of the sort
        frames, times = frames[:2], np.array([777, 778])
    elif name == 'three_passes':                                 # a span above 2^16
        times = np.arange(5) * 30000 + 5
    elif name == 'refractory':
        th_on, th_off = rng.randint(50, 900, (h, w)), rng.randint(50, 900, (h, w))
        refr = 150
    return dict(frames=frames, times=times.astype(np.int64), lut=lut, th_on=th_on.astype(np.int32), th_off=th_off.astype(np.int32), refr=refr)


@functools.lru_cache(maxsize=None)
def reference(name, h, w):
    """-> (records [n, 2] u32, state block int64, counters, kept events per interval) of the restatement, computed once."""
    c = case(name, h, w)
    s = sr.Sim(h, w, c['lut'], c['th_on'], c['th_off'], c['refr'])
    rec = s.feed(c['frames'], c['times'])
    assert s.invariant
    rec.setflags(write=False)
    return rec, s.state(), s.counters(), [len(ev) for _, _, ev in s.intervals]


def run(ops, c, cuts=(), **kw):
    """The frames of a case fed in calls cut at ``cuts`` -> (records [n, 2] u32 on the host, state tensor)."""
    edges = [0] + list(cuts) + [len(c['frames'])]
    frames = torch.from_numpy(c['frames']).to(DEV)
    state, parts = None, []
    for a, b in zip(edges[:-1], edges[1:]):
        before = None if state is None else state.clone()
        rec, new = ops.simulate_events(frames[a:b], c['times'][a:b], c['lut'], c['th_on'], c['th_off'], c['refr'], state, **kw)
        assert rec.dtype == torch.uint8 and rec.dim() == 2 and rec.shape[1] == 8 and new.dtype == torch.int64
        assert before is None or (torch.equal(before, state) and new.data_ptr() != state.data_ptr())   # the given state is not modified
        parts.append(rec.cpu().numpy().reshape(-1).view('<u4').reshape(-1, 2))
        state = new
    return np.concatenate(parts), state


def same(got, state, want):
    rec, block, counters, _ = want
    assert got.shape == rec.shape and np.array_equal(got, rec)
    assert np.array_equal(state.cpu().numpy(), block)


@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('hw', GEOMETRIES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_records_and_state_are_the_restatements(ops, hw, name):
    c, want = case(name, *hw), reference(name, *hw)
    n = len(c['frames'])
    got, state = run(ops, c)                                     # one call
    same(got, state, want)
    assert ops.simulate_counters(state) == want[2]
    got, state = run(ops, c, cuts=range(1, n))                   # a frame per call
    same(got, state, want)
    if n > 3:
        got, state = run(ops, c, cuts=(3,))                      # 3 + the rest
        same(got, state, want)


def test_the_cases_are_what_they_say(ops):
    for hw in GEOMETRIES:
        P = hw[0] * hw[1]
        rec, block, counters, per = reference('together', *hw)
        assert len(per) == 5 and all(k % P == 0 and k > 0 for k in (per[0], per[1], per[3], per[4])) and per[2] == 0
        assert len(np.unique(rec[:, 0])) <= len(rec) // P        # every pixel has every time: whole frames of pixels tie
        rec, block, counters, per = reference('swing', *hw)
        n_swing = len(range(3, P, 61))
        assert per == [4095 * n_swing] * 3 and counters['on'] == 2 * 4095 * n_swing
        rec, block, counters, per = reference('identical', *hw)
        assert len(rec) == 0 and counters['frames'] == 5 and counters['kept'] == 0
        rec, block, counters, per = reference('one_us', *hw)
        assert len(rec) > P and np.all(rec[:, 0] == 778)
        rec, block, counters, per = reference('three_passes', *hw)
        assert int(rec[-1, 0]) - 5 > 1 << 16
        rec, block, counters, per = reference('refractory', *hw)
        assert counters['dropped'] > P and counters['kept'] > P
    assert len(reference('random', 33, 67)[0]) > 8 * 2048        # more than one sort tile of events (8 x 256 records) in a call
    tile, digit, n_state, n_count, _ = ops.simulate_query(0, 16, 17)
    assert (tile, digit) == (256, 8) and 16 * 17 > tile > 5 * 7 and n_state == len(reference('random', 16, 17)[1])


def test_identical_frames_give_an_empty_tensor_and_an_updated_state(ops):
    c = case('identical', 16, 17)
    frames = torch.from_numpy(c['frames']).to(DEV)
    rec, state = ops.simulate_events(frames, c['times'], c['lut'], c['th_on'], c['th_off'])
    assert tuple(rec.shape) == (0, 8) and rec.dtype == torch.uint8
    assert ops.simulate_counters(state) == dict(frames=5, kept=0, on=0, off=0, dropped=0, t_last=int(c['times'][-1]))
    rec, again = ops.simulate_events(frames[:0], [], c['lut'], c['th_on'], c['th_off'], state=state)      # no frame: nothing changes
    assert tuple(rec.shape) == (0, 8) and torch.equal(again, state)


def test_a_small_workspace_takes_prefixes_of_the_intervals(ops):
    c, want = case('random', 33, 67), reference('random', 33, 67)
    per, total = want[3], len(want[0])
    third = ops.simulate_query(total // 3, 33, 67)[4]
    assert max(ops.simulate_query(k, 33, 67)[4] for k in per) <= third < ops.simulate_query(total, 33, 67)[4]     # it splits, and every interval fits
    got, state = run(ops, c, ws_bytes=third)
    same(got, state, want)
    got, state = run(ops, c, cuts=(2,), ws_bytes=third)
    same(got, state, want)
    # below the need of one interval: refused with the bytes it needs, before anything is emitted
    need = ops.simulate_query(max(per), 33, 67)[4]
    first = next(k for k in per if ops.simulate_query(k, 33, 67)[4] > need - 8)         # the first interval that does not fit is named
    with pytest.raises(_err(), match=f'{first} events.* need {ops.simulate_query(first, 33, 67)[4]} bytes'):
        run(ops, c, ws_bytes=need - 8)
    frames = torch.from_numpy(c['frames']).to(DEV)
    rec, state = ops.simulate_events(frames[:2], c['times'][:2], c['lut'], c['th_on'], c['th_off'])
    before = state.clone()
    with pytest.raises(_err(), match='bytes'):
        ops.simulate_events(frames[2:], c['times'][2:], c['lut'], c['th_on'], c['th_off'], state=state, ws_bytes=1024)
    assert torch.equal(state, before)


@pytest.mark.parametrize('name', ['random', 'refractory'])
def test_two_runs_give_identical_bytes(ops, name):
    c = case(name, 33, 67)
    frames = torch.from_numpy(c['frames']).to(DEV)
    a = ops.simulate_events(frames, c['times'], c['lut'], c['th_on'], c['th_off'], c['refr'])
    b = ops.simulate_events(frames, c['times'], c['lut'], c['th_on'], c['th_off'], c['refr'])
    assert a[0].numel() > 0 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_argument_checks(ops):
    c = case('random', 5, 7)
    frames = torch.from_numpy(c['frames']).to(DEV)
    a = (c['lut'], c['th_on'], c['th_off'])
    rec, state = ops.simulate_events(frames[:3], c['times'][:3], *a)
    with pytest.raises(ValueError, match='not later'):           # the carried time
        ops.simulate_events(frames[3:], c['times'][2:4], *a, state=state)
    with pytest.raises(ValueError):
        ops.simulate_events(frames, c['times'][:4], *a)
    with pytest.raises(ValueError):
        ops.simulate_events(frames, c['times'][::-1].copy(), *a)
    with pytest.raises(ValueError):
        ops.simulate_events(frames, c['times'], c['lut'], np.zeros((5, 7), np.int32), c['th_off'])
    with pytest.raises(ValueError):
        ops.simulate_events(frames, c['times'], c['lut'], torch.from_numpy(c['th_on']).to(DEV), c['th_off'])
    for bad in (torch.from_numpy(c['frames']), frames.to(torch.int32), frames[0], frames[:, :, ::2]):
        with pytest.raises(_err()):
            ops.simulate_events(bad, c['times'], *a)
    with pytest.raises(_err()):
        ops.simulate_events(frames, c['times'], *a, state=state[:-1])
    with pytest.raises(_err()):
        ops.simulate_counters(state[:4])
    # a threshold may be one integer; the table may be a CPU tensor
    one, _ = ops.simulate_events(frames, c['times'], torch.from_numpy(c['lut']), 900, 700)
    two, _ = ops.simulate_events(frames, c['times'], c['lut'], np.full((5, 7), 900), np.full((5, 7), 700))
    assert one.numel() > 0 and torch.equal(one, two)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
H, W, SIDE, STEP = 240, 304, 20, 4
X0, Y0 = 50, 100


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    """8 frames of 304 x 240: a bright square that moves 4 pixels to the right per frame over a flat background."""
    root = tmp_path_factory.mktemp('simulate')
    frames = np.full((8, H, W), 40, dtype=np.uint8)
    for i in range(8):
        frames[i, Y0:Y0 + SIDE, X0 + STEP * i:X0 + STEP * i + SIDE] = 200
    np.save(str(root / 'square.npy'), frames)
    from leod_amd.data import simulate
    lut = simulate.response_table('linlog')
    th_on, th_off = simulate.thresholds(lut, H, W, 0.2, 0.2)
    times = simulate.frame_times(8, fps=30)
    s = sr.Sim(H, W, lut, th_on, th_off)
    rec = s.feed(frames, times)
    return dict(root=str(root), src=str(root / 'square.npy'), rec=rec, counters=s.counters(), times=times)


def test_a_moving_square_goes_to_a_dat_file_a_raw_file_and_through_the_ingestion(ops, clip, tmp_path):
    from leod_amd.data import ingest, simulate
    from leod_amd.data.utils import dat_events, misc, raw_events
    want = clip['rec']
    assert len(want) > 1000
    dat_dir, raw_dir = str(tmp_path / 'dat'), str(tmp_path / 'raw')
    boxes = simulate.boxes_from_frames(np.arange(8), [[X0 + STEP * i, Y0, SIDE, SIDE] for i in range(8)], np.zeros(8, np.int64), clip['times'])
    rep = simulate.simulate_video(clip['src'], dat_dir, fps=30, batch_frames=3, boxes=boxes)
    assert sorted(os.listdir(dat_dir)) == ['square_bbox.npy', 'square_td.dat'] and rep['file'] == os.path.join(dat_dir, 'square_td.dat')
    hdr, records = dat_events.open_records(rep['file'])
    assert (hdr.height, hdr.width) == (H, W) and np.array_equal(np.asarray(records).reshape(-1, 2), want)
    c = clip['counters']
    assert (rep['frames'], rep['events'], rep['on'], rep['off'], rep['dropped']) == (8, c['kept'], c['on'], c['off'], 0)
    assert rep['payload_bytes'] == 8 * len(want) and rep['duration_us'] == 233333 and rep['boxes'] == 8
    assert rep['events_per_pixel_per_s'] == round(len(want) / (H * W) / 0.233333, 6)
    assert np.array_equal(np.load(os.path.join(dat_dir, 'square_bbox.npy')), boxes)
    # EVT3, with vectors: this project's decoder returns the records
    rep3 = simulate.simulate_video(clip['src'], raw_dir, fps=30, write_events='evt3', evt3_vectors=True, batch_frames=5)
    assert os.listdir(raw_dir) == ['square.raw'] and rep3['events'] == len(want)
    rh, payload = raw_events.open_words(rep3['file'])
    assert rh.encoding == 'evt3' and (rh.height, rh.width) == (H, W)
    words = torch.from_numpy(np.asarray(payload).view(np.uint8).reshape(-1).copy()).to(DEV)
    back, _ = ops.decode_evt(words, 'evt3')
    assert np.array_equal(back.cpu().numpy().reshape(-1).view('<u4').reshape(-1, 2), want)
    assert rep3['payload_bytes'] < rep['payload_bytes']
    # the directory is a source directory of the ingestion
    tree = str(tmp_path / 'tree')
    assert ingest.main([raw_dir, tree, '--dataset', 'gen1', '--unlabelled', 'ok']) == 0
    frames = np.load(misc.get_ev_raw_fn(os.path.join(tree, 'square'), 'gen1'))
    assert frames.shape[-2:] == (H, W) and frames.any()
    swept = np.zeros((H, W), dtype=bool)
    swept[Y0:Y0 + SIDE, X0:X0 + SIDE + 7 * STEP] = True          # the rows and columns the square's edges passed
    assert not frames[..., ~swept].any()
    reps = ingest.ingest_split(dat_dir, str(tmp_path / 'tree2'), 'gen1')                 # and with the boxes: labelled
    assert len(reps) == 1 and reps[0]['events'] == len(want)
    assert np.array_equal(np.load(misc.get_ev_raw_fn(os.path.join(str(tmp_path / 'tree2'), 'square'), 'gen1')), frames)
