"""Recording ingestion on the device: ``ops.voxelize_dat_windows`` (csrc/k_ingest.hip) window by window against the oracle's
``stacked_histogram`` and against the single-window kernel, chunking, the half-resolution output, the coordinate guard, and the whole
path from a raw .dat + _bbox.npy to a tree the loaders open."""
import os

import numpy as np
import pytest
import torch

from oracle import postproc as op

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BINS, H, W = 10, 24, 30
D = 50_000


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as _ops
    return _ops


def _eight_windows():
    """(t, x, y, p) of all events and the offsets [9] of eight windows: empty, one event, one shared timestamp, a pixel hit 300 times (and
    one hit 256 times: wraps to 0 in fast mode), four random ones of different sizes (one of them a single bin wide: t1 - t0 = 1)."""
    rng = np.random.RandomState(31)
    parts = []

    def rand(n, t_lo, t_hi):
        return [np.sort(rng.randint(t_lo, t_hi, n)), rng.randint(0, W, n), rng.randint(0, H, n), rng.randint(0, 2, n)]

    parts.append([np.zeros(0, np.int64)] * 4)                                     # 0: empty
    parts.append([np.array([D + 17]), np.array([W - 1]), np.array([H - 1]), np.array([1])])        # 1: a single event
    same = rand(50, 0, 1)
    same[0][:] = 2 * D + 5                                                        # 2: every event at one timestamp (denominator max(0, 1))
    parts.append(same)
    hot = rand(700, 3 * D + 1, 4 * D)                                             # 3: 300 hits on one cell (one pixel, one timestamp):
    hot[1][:300], hot[2][:300], hot[3][:300], hot[0][:300] = 7, 11, 1, hot[0][350]     # 300 -> 44 in fast mode, 255 / the cutoff otherwise
    hot[1][300:556], hot[2][300:556], hot[3][300:556], hot[0][300:556] = 29, 0, 0, hot[0][600]     # and 256 on another: -> 0 in fast mode
    order = np.argsort(hot[0], kind='stable')
    hot = [a[order] for a in hot]
    parts.append(hot)
    parts.append(rand(1000, 4 * D + 1, 5 * D))                                    # 4-7: random
    parts.append(rand(777, 5 * D + 1, 5 * D + 3))
    parts.append(rand(2, 6 * D + 1, 6 * D + 3))
    parts.append(rand(2500, 7 * D + 1, 8 * D + 1))
    off = np.concatenate([[0], np.cumsum([len(q[0]) for q in parts])]).astype(np.int64)
    t, x, y, p = (np.concatenate([q[k] for q in parts]).astype(np.int64) for k in range(4))
    return (t, x, y, p), off


@pytest.fixture(scope='module')
def eight():
    """The events, the offsets and, computed once, the oracle's histogram of every window for the four (fastmode, cutoff) settings."""
    ev, off = _eight_windows()
    ref = {}
    for fast in (True, False):
        for cutoff in (None, 10):
            ref[fast, cutoff] = np.stack([op.stacked_histogram(*(a[off[w]:off[w + 1]] for a in (ev[1], ev[2], ev[3], ev[0])), BINS, H, W,
                                                               count_cutoff=cutoff, fastmode=fast) for w in range(8)])
    for r in ref.values():
        r.setflags(write=False)
    return ev, off, ref


def _records(t, x, y, p):
    from leod_amd.data.utils import dat_events
    return torch.from_numpy(dat_events.encode(t, x, y, p).view(np.uint8).reshape(-1)).to(DEV)


def test_the_cases_are_the_cases(eight):
    (t, x, y, p), off, ref = eight
    assert off.tolist() == [0, 0, 1, 51, 751, 1751, 2528, 2530, 5030]
    assert np.all(np.diff(t) >= 0)
    assert not ref[True, None][0].any()
    slow3, fast3 = ref[False, None][3], ref[True, None][3]
    cells = np.argwhere(slow3 == 255)                                            # the two hot cells saturate without fast mode ...
    assert len(cells) == 2 and all(fast3[tuple(c)] < 100 for c in cells)         # ... and wrap with it
    assert ref[True, 10][3].max() == 10


@pytest.mark.parametrize('fast', [True, False])
@pytest.mark.parametrize('cutoff', [None, 10])
def test_batched_windows_equal_the_oracle(ops, eight, fast, cutoff):
    (t, x, y, p), off, ref = eight
    rec = _records(t, x, y, p)
    out, dropped = ops.voxelize_dat_windows(rec, off, BINS, H, W, count_cutoff=cutoff, fastmode=fast)
    assert out.shape == (8, 2 * BINS, H, W) and out.dtype is torch.uint8 and int(dropped) == 0
    got = out.cpu().numpy()
    for w in range(8):
        assert np.array_equal(got[w], ref[fast, cutoff][w]), f'window {w}'


@pytest.mark.parametrize('fast,cutoff', [(True, None), (False, 10)])
def test_chunking_changes_nothing(ops, eight, fast, cutoff):
    """ws_windows = 3: chunks of 3 + 3 + 2 windows, a chunk boundary behind the empty / single-event windows and one in the middle of the
    random ones; 8: one chunk; 1: one window per chunk; 5 and 100: a partial chunk and a chunk larger than the call."""
    (t, x, y, p), off, ref = eight
    rec = _records(t, x, y, p)
    whole = ops.voxelize_dat_windows(rec, off, BINS, H, W, count_cutoff=cutoff, fastmode=fast, ws_windows=8)[0]
    assert np.array_equal(whole.cpu().numpy(), ref[fast, cutoff])
    for ws in (3, 1, 5, 100):
        part = ops.voxelize_dat_windows(rec, off, BINS, H, W, count_cutoff=cutoff, fastmode=fast, ws_windows=ws)[0]
        assert torch.equal(part, whole), ws
    # offsets handed over on the device, and a sub-range of the windows that starts in the middle of the records
    sub = ops.voxelize_dat_windows(rec, torch.from_numpy(off[2:7]).to(DEV), BINS, H, W, count_cutoff=cutoff, fastmode=fast, ws_windows=3)[0]
    assert torch.equal(sub, whole[2:6])


def test_same_as_the_single_window_kernel(ops, eight):
    (t, x, y, p), off, _ = eight
    rec = _records(t, x, y, p)
    dev = [torch.from_numpy(a).to(DEV) for a in (x, y, p, t)]
    for fast, cutoff in ((True, None), (False, 10), (True, 3)):
        out = ops.voxelize_dat_windows(rec, off, BINS, H, W, count_cutoff=cutoff, fastmode=fast, ws_windows=3)[0]
        for w in range(8):
            one = ops.voxelize_u8(*(a[off[w]:off[w + 1]].contiguous() for a in dev), BINS, H, W, count_cutoff=cutoff, fastmode=fast)
            assert torch.equal(out[w], one), (fast, cutoff, w)


def test_golden_recordings_as_one_call(ops, golden_dir):
    """The three event sets the reference's StackedHistogram was recorded on (g10) as three windows of one call."""
    g = np.load(os.path.join(golden_dir, 'g10_voxel.npz'))
    ev = {k: np.concatenate([g[f'{n}_{k}'].astype(np.int64) for n in 'abc']) for k in 'xypt'}
    off = np.concatenate([[0], np.cumsum([len(g[f'{n}_t']) for n in 'abc'])])
    rec = _records(ev['t'] - ev['t'].min(), ev['x'], ev['y'], ev['p'])           # the bin depends on time differences only
    for name, w, fast, cutoff in (('a', 0, True, None), ('b', 1, False, 10), ('c', 2, True, 3)):
        out = ops.voxelize_dat_windows(rec, off, 10, 24, 30, count_cutoff=cutoff, fastmode=fast, ws_windows=2)[0]
        assert np.array_equal(out[w].cpu().numpy(), g[f'{name}_rep']), name


@pytest.mark.parametrize('ws', [3, 8])
def test_ds2_is_the_odd_pixels_of_the_full_histogram(ops, eight, ws):
    (t, x, y, p), off, ref = eight
    rec = _records(t, x, y, p)
    for fast, cutoff in ((True, None), (False, 10)):
        out, dropped = ops.voxelize_dat_windows(rec, off, BINS, H, W, ds2=True, count_cutoff=cutoff, fastmode=fast, ws_windows=ws)
        assert out.shape == (8, 2 * BINS, H // 2, W // 2) and int(dropped) == 0
        assert np.array_equal(out.cpu().numpy(), ref[fast, cutoff][..., 1::2, 1::2]), (fast, cutoff)


def test_sizes_that_are_no_multiple_of_four(ops):
    """2 * bins * H * W = 210: the finalise pass cannot pack four counts into one store and takes its byte-wise form; the second chunk then
    starts at an output address that is no multiple of four."""
    bins, h, w = 3, 5, 7
    rng = np.random.RandomState(8)
    off = np.array([0, 400, 400, 1000, 1003])
    n = int(off[-1])
    t, x, y, p = np.sort(rng.randint(0, 4 * D, n)), rng.randint(0, w, n), rng.randint(0, h, n), rng.randint(0, 2, n)
    for ws in (1, 2, 4):
        out = ops.voxelize_dat_windows(_records(t, x, y, p), off, bins, h, w, count_cutoff=40, ws_windows=ws)[0].cpu().numpy()
        for k in range(4):
            s = slice(off[k], off[k + 1])
            assert np.array_equal(out[k], op.stacked_histogram(x[s], y[s], p[s], t[s], bins, h, w, count_cutoff=40)), (ws, k)


def test_ds2_needs_even_sizes(ops):
    from leod_amd._lib import LeodHipError, lib
    rec = _records(np.array([1]), np.array([1]), np.array([1]), np.array([1]))
    with pytest.raises(LeodHipError):
        ops.voxelize_dat_windows(rec, np.array([0, 1]), BINS, 23, W, ds2=True)
    # the C entry point itself: LEOD_ERR_ARG before any launch
    ws = torch.zeros(16, dtype=torch.int32, device=DEV)
    out = torch.zeros(16, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 1], device=DEV)
    rc = lib().leod_voxelize_dat_windows(ops._p(rec), 1, ops._p(off), 1, ops._p(ws), 1, ops._p(out), 1, 2, 3, 1, 0, 1, None, ops._stream())
    assert rc == -1
    with pytest.raises(LeodHipError):
        ops.voxelize_dat_windows(rec, np.array([0, 2]), BINS, H, W)              # an offset behind the last event
    with pytest.raises(LeodHipError):
        ops.voxelize_dat_windows(rec[:7], np.array([0, 0]), BINS, H, W)          # no whole number of records


@pytest.mark.parametrize('ds2', [False, True])
def test_events_outside_the_sensor_are_skipped_and_counted(ops, eight, ds2):
    """x = W with y <= H - 2, and y = H with p = 0: a kernel WITHOUT the guard would count these on the next row / in the next plane, still
    inside the workspace, so a wrong build fails this comparison and faults nothing."""
    (t, x, y, p), off, ref = eight
    rng = np.random.RandomState(5)
    lo, hi = int(off[4]), int(off[5])                                             # into random window 4: 40 + 30 events
    at = np.sort(rng.randint(lo + 1, hi - 1, 70))                                 # not first / last: t0 and t1 of the window stay
    bx = np.concatenate([np.full(40, W), rng.randint(0, W, 30)])
    by = np.concatenate([rng.randint(0, H - 1, 40), np.full(30, H)])
    bp = np.concatenate([rng.randint(0, 2, 40), np.zeros(30, np.int64)])
    t2, x2, y2, p2 = (np.insert(a, at, b) for a, b in ((t, t[at]), (x, bx), (y, by), (p, bp)))
    off2 = off.copy()
    off2[5:] += 70
    assert np.all(np.diff(t2[off2[4]:off2[5]]) >= 0) and t2[off2[4]] == t[lo] and t2[off2[5] - 1] == t[hi - 1]
    out, dropped = ops.voxelize_dat_windows(_records(t2, x2, y2, p2), off2, BINS, H, W, ds2=ds2, ws_windows=3)
    want = ref[True, None][..., 1::2, 1::2] if ds2 else ref[True, None]
    assert int(dropped) == 70
    assert np.array_equal(out.cpu().numpy(), want)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
PROPHESEE_BBOX = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                           'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                           'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})


def _write_recording(src_dir, name, seed, hw, n_events, duration_s, box_times, n_classes):
    """A synthetic raw recording: <name>_td.dat (events up to exactly duration_s, two at t = 0, none in frame 5) + <name>_bbox.npy."""
    from leod_amd.data.utils import dat_events
    os.makedirs(src_dir, exist_ok=True)
    rng = np.random.RandomState(seed)
    h, w = hw
    t_end = int(duration_s * 1e6)
    t = rng.randint(1, t_end, n_events - 3)
    t = t[(t <= 5 * D) | (t > 6 * D)]                                             # frame 5 stays empty
    t = np.sort(np.concatenate([[0, 0], t, [t_end]]))
    n = len(t)
    x, y, p = rng.randint(0, w, n), rng.randint(0, h, n), rng.randint(0, 2, n)
    dat_events.write_dat(os.path.join(src_dir, name + '_td.dat'), dat_events.encode(t, x, y, p), h, w)
    boxes = np.zeros((len(box_times),), dtype=PROPHESEE_BBOX)
    for i, bt in enumerate(box_times):
        # whole-number coordinates: the loaders rebuild w as (x + w) - x in fp32 when they clamp boxes to the frame, exact on these
        boxes[i] = (bt, rng.randint(0, w - 60), rng.randint(0, h - 50), rng.randint(10, 50), rng.randint(10, 40), i % n_classes, 7 + i,
                    rng.randint(32, 65) / 64)
    np.save(os.path.join(src_dir, name + '_bbox.npy'), boxes)
    return (t, x, y, p), boxes


BOX_TIMES = [3 * D, 3 * D, 3 * D + 5, 4 * D, 4 * D, 10 * D + 1, 20 * D, 20 * D + 1, 30 * D]
#            frame 2 (two boxes)  frame 3: the later timestamp wins   10     19 (the end of the last frame)   beyond: dropped


def test_raw_recording_to_a_tree_the_loaders_open(ops, tmp_path):
    from leod_amd.data import ingest
    from leod_amd.data.genx_utils.sequence_rnd import SequenceForRandomAccess
    from leod_amd.data.utils import dat_events, misc
    from leod_amd.data.utils.types import DatasetType, DataType
    src = str(tmp_path / 'raw')
    (t, x, y, p), boxes = _write_recording(src, 'rec0', 1, (240, 304), 6000, 1.0, BOX_TIMES, 2)
    seq_dir = str(tmp_path / 'gen1' / 'train' / 'rec0')
    rep = ingest.ingest_recording(os.path.join(src, 'rec0_td.dat'), os.path.join(src, 'rec0_bbox.npy'), seq_dir, 'gen1')
    assert rep['frames'] == 20 and rep['events'] == len(t) and rep['dropped_events'] == 0 and rep['labelled_frames'] == 4 and rep['boxes'] == 6

    off = dat_events.window_offsets(t, D)
    assert len(off) == 21 and off[5] == off[6] and off[1] > 2
    want = [op.stacked_histogram(x[off[k]:off[k + 1]], y[off[k]:off[k + 1]], p[off[k]:off[k + 1]], t[off[k]:off[k + 1]], 10, 240, 304)
            for k in range(20)]
    frames = np.load(misc.get_ev_raw_fn(seq_dir, 'gen1'), mmap_mode='r')
    assert frames.shape == (20, 20, 240, 304) and frames.dtype == np.uint8
    for k in range(20):
        assert np.array_equal(frames[k], want[k]), f'frame {k}'
    assert misc.read_objframe_idx_2_repr_idx(seq_dir).tolist() == [2, 3, 10, 19]
    labels, starts = misc.read_npz_labels(seq_dir)
    assert starts.tolist() == [0, 2, 4, 5] and labels['t'].tolist() == [3 * D, 3 * D, 4 * D, 4 * D, 10 * D + 1, 20 * D]

    L = 3
    seq = SequenceForRandomAccess(seq_dir, misc.EV_REPR_NAME, L, DatasetType.GEN1, downsample_by_factor_2=False, only_load_end_labels=False)
    assert len(seq) == 4
    kept = boxes[[0, 1, 3, 4, 5, 6]]
    for i, (r, rows) in enumerate(zip([2, 3, 10, 19], [kept[0:2], kept[2:4], kept[4:5], kept[5:6]])):
        s = seq[i]
        assert s[DataType.EV_IDX] == list(range(r - L + 1, r + 1))
        for j, k in enumerate(s[DataType.EV_IDX]):
            assert np.array_equal(s[DataType.EV_REPR][j].numpy(), want[k]), (i, k)
        lab = s[DataType.OBJLABELS_SEQ][L - 1]
        assert len(lab) == len(rows)
        for name in ('t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence'):
            assert np.array_equal(lab.get(name).numpy(), rows[name].astype(np.float32)), (i, name)
        assert lab.objectness.tolist() == [1.0] * len(rows)


def test_command_line_split_and_data_module(ops, tmp_path):
    """``python -m leod_amd.data.ingest SRC DST --dataset gen1`` (its ``main``, in this process) over a directory with a test split of two
    recordings, then the tree through the DataModule's evaluation loader."""
    from leod_amd.config import full_config
    from leod_amd.data import ingest
    from leod_amd.data.utils import misc
    from leod_amd.data.utils.types import DataType
    from leod_amd.modules.data.genx import DataModule
    src, dst = str(tmp_path / 'raw'), str(tmp_path / 'gen1')
    for name, seed in (('recA', 3), ('recB', 4)):
        _write_recording(os.path.join(src, 'test'), name, seed, (240, 304), 3000, 1.0, BOX_TIMES, 2)
    assert ingest.main([src, dst, '--dataset', 'gen1']) == 0
    assert sorted(os.listdir(os.path.join(dst, 'test'))) == ['recA', 'recB']
    stored = {n: np.load(misc.get_ev_raw_fn(os.path.join(dst, 'test', n), 'gen1')) for n in ('recA', 'recB')}
    cfg = full_config('gen1', 'small', overrides=dict(dataset=dict(path=dst, sequence_length=5)))
    dm = DataModule(cfg.dataset, num_workers_train=1, num_workers_eval=1, batch_size_train=1, batch_size_eval=1, prefetch=2, io_threads=1)
    dm.setup('test')
    n_batches = 0
    for batch in dm.test_dataloader():
        ev = torch.stack([e.cpu() for e in batch['data'][DataType.EV_REPR]])[:, 0].numpy()       # [L, 20, 240, 304] of batch slot 0
        assert ev.shape == (5, 20, 240, 304)
        if n_batches == 0:                                        # the first batch is the head of one of the two recordings
            assert any(np.array_equal(ev, fr[:5]) for fr in stored.values())
        n_batches += 1
    assert n_batches >= 4


def test_gen4_recording_is_written_at_half_resolution(ops, tmp_path):
    from leod_amd.data import ingest
    from leod_amd.data.genx_utils.sequence_rnd import SequenceForRandomAccess
    from leod_amd.data.utils import dat_events, misc
    from leod_amd.data.utils.types import DatasetType, DataType
    src = str(tmp_path / 'raw')
    times = [D, 2 * D, 2 * D, 2 * D, 2 * D, 3 * D]
    (t, x, y, p), boxes = _write_recording(src, 'rec4', 9, (720, 1280), 8000, 0.15, times, 5)      # classes 0 1 2 3 4 0: 3 and 4 are dropped
    seq_dir = str(tmp_path / 'gen4' / 'train' / 'rec4')
    rep = ingest.ingest_recording(os.path.join(src, 'rec4_td.dat'), os.path.join(src, 'rec4_bbox.npy'), seq_dir, DatasetType.GEN4)
    assert rep['frames'] == 3 and rep['boxes'] == 4
    fn = misc.get_ev_raw_fn(seq_dir, 'gen4')
    assert fn.endswith('event_representations_ds2_nearest.npy')
    frames = np.load(fn)
    assert frames.shape == (3, 20, 360, 640)
    off = dat_events.window_offsets(t, D)
    for k in range(3):
        full = op.stacked_histogram(x[off[k]:off[k + 1]], y[off[k]:off[k + 1]], p[off[k]:off[k + 1]], t[off[k]:off[k + 1]], 10, 720, 1280)
        assert np.array_equal(frames[k], full[:, 1::2, 1::2]), k
    labels, starts = misc.read_npz_labels(seq_dir)
    assert labels['class_id'].tolist() == [0, 1, 2, 0] and starts.tolist() == [0, 1, 3]
    seq = SequenceForRandomAccess(seq_dir, misc.EV_REPR_NAME, 2, DatasetType.GEN4, downsample_by_factor_2=True, only_load_end_labels=False)
    assert len(seq) == 2                                           # labelled frames 1 and 2 have a frame of history; frame 0 has none
    s = seq[0]
    assert s[DataType.EV_IDX] == [0, 1] and np.array_equal(s[DataType.EV_REPR][1].numpy(), frames[1])
    assert np.allclose(s[DataType.OBJLABELS_SEQ][1].w.numpy(), boxes['w'][[1, 2]] / 2)
