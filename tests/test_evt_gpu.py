"""``ops.decode_evt`` (csrc/k_evt.hip) against the tests' sequential decoder (tests/evt_ref.py), bit for bit: records, the carried state and
the counters, for EVT2 and EVT3; then ``.raw`` recordings through ``ingest_recording`` against the same events as ``.dat``.  The stream
sizes follow the kernel's own constants (``ops.evt_query``): a tile of words per workgroup, four waves per tile, sixteen words per lane."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evt_ref  # noqa: E402
from evt_cases import AX, AY, HAND, TH, TL, V12, VB, P1, random_words  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
D = 50_000


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as _ops
    return _ops


def _dev(words, fmt):
    return torch.from_numpy(evt_ref.as_bytes(words, fmt).copy()).to(DEV)


def _decode(ops, words, fmt, state=None, out=None):
    rec, state = ops.decode_evt(_dev(words, fmt), 'evt%d' % fmt, state=state, out=out)
    assert rec.dtype == torch.uint8 and rec.dim() == 2 and rec.shape[1] == 8 and state.dtype == torch.int64
    return rec.cpu().numpy().view('<u4').reshape(-1, 2), state


def _check(ops, words, fmt, what=''):
    """One call on the device against the sequential decoder: records, state block, counters."""
    ref = evt_ref.Decoder(fmt)
    want = ref.feed(words)
    got, state = _decode(ops, words, fmt)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, f'record {bad[0]} of {len(want)}', got[bad[0]].tolist(), want[bad[0]].tolist())
    assert state.cpu().tolist() == ref.state(), what
    assert ops.evt_state_counters(state) == ref.counters(), what
    return got, ref


@pytest.mark.parametrize('case', HAND, ids=[c[0] for c in HAND])
def test_hand_written_words(ops, case):
    name, fmt, words, events, _ = case
    got, _ = _check(ops, words, fmt, name)
    w = got.astype(np.int64)
    assert list(zip(w[:, 0].tolist(), (w[:, 1] & 16383).tolist(), ((w[:, 1] >> 14) & 16383).tolist(), (w[:, 1] >> 28).tolist())) == events


@pytest.mark.parametrize('fmt', [3, 2])
def test_random_streams_of_the_sizes_where_the_kernel_changes_path(ops, fmt):
    tile = ops.evt_query()[0]
    rng = np.random.RandomState(17 + fmt)
    for n in (1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5):
        _check(ops, random_words(rng, n, fmt), fmt, f'{n} words')
    _check(ops, np.zeros((0,), dtype=np.int64), fmt, 'no words')


def _repeated_block(rng, fmt, n_blocks, per, first_high):
    """A block = TIME_HIGH + a random body without TIME_HIGH words; the stream repeats it with TIME_HIGH rising by one per block.
    -> (words, records, early events, ignored words).  Blocks 0 and 1 are decoded by the sequential decoder.  Every block from 1 on
    starts from the state the same body left behind, so block r holds the records of block 1 with r - 1 TIME_HIGH steps added to t
    (checked against the sequential decoder on the first five blocks)."""
    time_shift, kind_shift, mask = (12, 12, 4095) if fmt == 3 else (6, 28, (1 << 28) - 1)
    body = random_words(rng, 2 * per, fmt)
    body = body[(body >> kind_shift) != 0x8][:per - 1]
    assert len(body) == per - 1
    words = np.tile(np.concatenate([[0], body]), n_blocks)
    words[::per] = (0x8 << kind_shift) | ((first_high + np.arange(n_blocks)) & mask)
    ref = evt_ref.Decoder(fmt)
    head = ref.feed(words[:per]).astype(np.int64)
    early0 = ref.early
    one = ref.feed(words[per:2 * per]).astype(np.int64)
    early1 = ref.early - early0
    rest = np.tile(one, (n_blocks - 1, 1))
    rest[:, 0] += np.repeat(np.arange(n_blocks - 1), len(one)) << time_shift
    records = np.concatenate([head, rest])
    assert records[:, 0].max() < 2 ** 32 and len(one) > per // 4
    few = evt_ref.Decoder(fmt).feed(words[:5 * per]).astype(np.int64)
    assert np.array_equal(few, records[:len(few)])
    ignored = int(np.isin(body >> kind_shift, evt_ref.IGNORED[fmt]).sum()) * n_blocks
    return words, records.astype('<u4'), early0 + early1 * (n_blocks - 1), ignored


@pytest.mark.parametrize('fmt', [3, 2])
def test_a_stream_that_takes_the_scan_workgroup_three_passes(ops, fmt):
    tile, per_pass, _ = ops.evt_query()
    per = 1000                                                   # no divisor of the tile: the blocks drift through lanes, waves and tiles
    n_blocks = (2 * per_pass * tile + tile) // per + 2
    # EVT3 starts at TIME_HIGH 3000: the clock wraps at block 1096
    words, want, early, ignored = _repeated_block(np.random.RandomState(3), fmt, n_blocks, per, 3000 if fmt == 3 else 5)
    assert len(words) > 2 * per_pass * tile
    got, state = _decode(ops, words, fmt)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (f'record {bad[0]} of {len(want)}', got[bad[0]].tolist(), want[bad[0]].tolist())
    c = ops.evt_state_counters(state)
    assert c['events'] == len(want) and c['overflow'] == 0 and c['wraps'] == (1 if fmt == 3 else 0)
    assert c['ignored_words'] == ignored and c['early_events'] == early


def _boundary_streams(tile):
    """(name, words): each pattern placed so that every cut between two of its words falls on a lane, a wave and a tile boundary."""
    patterns = {'base_then_vect12': [VB | P1 | 50, V12 | 0xA05], 'row_then_event': [AY | 77, AX | 5],
                'high_low_event': [TH | 4001, TL | 9, AX | P1 | 6], 'wrap': [TH | 4095, TH | 2, AX | 3]}
    prefix = [TH | 4000, TL | 1, AY | 2, VB | 10]
    for at_name, at in (('lane', 16), ('wave', tile // 4), ('tile', tile), ('second_tile', 2 * tile)):
        for name, pat in patterns.items():
            for k in range(1, len(pat)):                         # pat[k] is the first word behind the boundary
                filler = [AX | (i % 300) for i in range(at - k - len(prefix))]
                yield f'{name}_cut{k}_at_{at_name}', prefix + filler + pat + [AX | 7, V12 | 0x3, AX | 8]


def test_state_words_on_either_side_of_a_lane_wave_and_tile_boundary(ops):
    tile = ops.evt_query()[0]
    n = 0
    for name, words in _boundary_streams(tile):
        got, ref = _check(ops, words, 3, name)
        assert ref.early == 0 and len(got) > 10
        n += 1
    assert n == 4 * 6
    # EVT2: TIME_HIGH on the last word before the boundary, the event behind it
    for at in (16, tile // 4, tile):
        words = [(0x8 << 28) | 7] + [(i % 2 << 28) | (i % 64 << 22) | (i % 1280 << 11) | (i % 720) for i in range(at - 2)] \
            + [(0x8 << 28) | 9, (0x1 << 28) | (3 << 22) | (5 << 11) | 6]
        got, _ = _check(ops, words, 2, f'evt2 at {at}')
        assert got[-1].tolist() == [(2 << 6) | 3, 5 | (6 << 14) | (1 << 28)]


@pytest.mark.parametrize('fmt', [3, 2])
def test_chunk_carry_at_every_split(ops, fmt):
    words = random_words(np.random.RandomState(41 + fmt), 200, fmt)
    whole, _ = _check(ops, words, fmt)
    for cut in range(201):
        ref = evt_ref.Decoder(fmt)
        want = [ref.feed(words[:cut]), ref.feed(words[cut:])]
        a, state = _decode(ops, words[:cut], fmt)
        b, state2 = _decode(ops, words[cut:], fmt, state=state)
        assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]), cut
        assert np.array_equal(np.concatenate([a, b]), whole), cut
        assert state2.cpu().tolist() == ref.state(), cut
        assert ops.evt_state_counters(state2) == ref.counters(), cut
        assert state2 is not state


def test_every_vect12_mask_of_one_bit_and_of_twelve(ops):
    words = [TH | 0, TL | 4, AY | 6]
    want = []
    for i in range(12):
        words += [VB | 100, V12 | (1 << i)]
        want.append((4, 100 + i, 6, 0))
    words += [VB | P1 | 200, V12 | 0xFFF]
    want += [(4, 200 + i, 6, 1) for i in range(12)]
    got, _ = _check(ops, words, 3)
    w = got.astype(np.int64)
    assert list(zip(w[:, 0].tolist(), (w[:, 1] & 16383).tolist(), ((w[:, 1] >> 14) & 16383).tolist(), (w[:, 1] >> 28).tolist())) == want


def test_overflow_flag_and_nothing_behind_the_records(ops):
    from leod_amd._lib import LeodHipError
    words = [TH | 0, TL | 0, AY | 0, AX | 1] + [TH | ((k * 1024) & 4095) for k in range(1, 1025)] + [AX | 2, AX | 3]     # 256 wraps: t = 2^32
    ref = evt_ref.Decoder(3)
    want = ref.feed(words)
    assert ref.overflow == 1 and len(want) == 3
    big = torch.full((3 * 8 + 4096,), 0xAB, dtype=torch.uint8, device=DEV)
    got, state = _decode(ops, words, 3, out=big[:24])
    assert np.array_equal(got, want) and got[:, 0].tolist() == [0, 0, 0]
    assert bool((big[24:] == 0xAB).all()) and big[:24].cpu().numpy().tobytes() == want.tobytes()
    c = ops.evt_state_counters(state)
    assert c['overflow'] == 1 and c['wraps'] == 256 and c == ref.counters()
    _, state = _decode(ops, [AX | 1], 3, state=state)             # the flag is carried
    assert ops.evt_state_counters(state)['overflow'] == 1
    # a buffer that does not hold the chunk is refused before anything is stored
    big.fill_(0xAB)
    with pytest.raises(LeodHipError):
        _decode(ops, words, 3, out=big[:16])
    assert bool((big == 0xAB).all())
    # the kernel's own guard: capacity 1 stores one record of the three
    dev_words = _dev(words, 3)
    ws_bytes = ops.evt_query(len(words))[2]
    ws = torch.empty((ws_bytes // 8 + 1,), dtype=torch.int64, device=DEV)
    s0, s1 = torch.zeros(16, dtype=torch.int64, device=DEV), torch.zeros(16, dtype=torch.int64, device=DEV)
    lib, p, st = ops._l(), ops._p, ops._stream()
    assert lib.leod_evt_scan(p(dev_words), len(words), 3, p(s0), p(s1), p(ws), ws_bytes, st) == 0
    assert lib.leod_evt_emit(p(dev_words), len(words), 3, p(ws), ws_bytes, p(big), 1, p(s1), st) == 0
    torch.cuda.synchronize()
    assert big[:8].cpu().numpy().tobytes() == want[:1].tobytes() and bool((big[8:] == 0xAB).all()) and int(s1[14]) == 3
    # arguments the entry points refuse
    assert lib.leod_evt_scan(p(dev_words), len(words), 4, p(s0), p(s1), p(ws), ws_bytes, st) == -1
    assert lib.leod_evt_scan(p(dev_words), len(words), 3, p(s0), p(s1), p(ws), ws_bytes - 1, st) == -1


def test_refusals(ops):
    from leod_amd._lib import LeodHipError
    words = _dev([TH | 1, TL | 1], 3)
    with pytest.raises(LeodHipError):
        ops.decode_evt(words.cpu(), 'evt3')
    for bad in ('evt21', 'evt4', 'dat', 1, None):
        with pytest.raises(LeodHipError):
            ops.decode_evt(words, bad)
    with pytest.raises(LeodHipError):
        ops.decode_evt(words[:3], 'evt3')
    with pytest.raises(LeodHipError):
        ops.decode_evt(words, 'evt2', state=torch.zeros(8, dtype=torch.int64, device=DEV))
    # a view that is not 16-byte aligned is decoded all the same
    rec, _ = ops.decode_evt(_dev([0, TH | 1, TL | 1, AY | 1, AX | 1], 3)[2:], 'evt3')
    assert rec.shape == (1, 8)


# ---- recordings -----------------------------------------------------------------------------------------------------------------------
BINS, H, W = 10, 24, 30


def _eight_windows():
    """The events of tests/test_ingest_gpu.py (a copy of its generator): eight windows -- empty, one event, one shared timestamp, a pixel
    hit 300 times and one hit 256 times, four random ones of different sizes."""
    rng = np.random.RandomState(31)
    parts = []

    def rand(n, t_lo, t_hi):
        return [np.sort(rng.randint(t_lo, t_hi, n)), rng.randint(0, W, n), rng.randint(0, H, n), rng.randint(0, 2, n)]

    parts.append([np.zeros(0, np.int64)] * 4)
    parts.append([np.array([D + 17]), np.array([W - 1]), np.array([H - 1]), np.array([1])])
    same = rand(50, 0, 1)
    same[0][:] = 2 * D + 5
    parts.append(same)
    hot = rand(700, 3 * D + 1, 4 * D)
    hot[1][:300], hot[2][:300], hot[3][:300], hot[0][:300] = 7, 11, 1, hot[0][350]
    hot[1][300:556], hot[2][300:556], hot[3][300:556], hot[0][300:556] = 29, 0, 0, hot[0][600]
    order = np.argsort(hot[0], kind='stable')
    hot = [a[order] for a in hot]
    parts.append(hot)
    parts.append(rand(1000, 4 * D + 1, 5 * D))
    parts.append(rand(777, 5 * D + 1, 5 * D + 3))
    parts.append(rand(2, 6 * D + 1, 6 * D + 3))
    parts.append(rand(2500, 7 * D + 1, 8 * D + 1))
    off = np.concatenate([[0], np.cumsum([len(q[0]) for q in parts])]).astype(np.int64)
    t, x, y, p = (np.concatenate([q[k] for q in parts]).astype(np.int64) for k in range(4))
    return (t, x, y, p), off


PROPHESEE_BBOX = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                           'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                           'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})


def _tree_files(seq_dir):
    out = {}
    for dirpath, _, files in os.walk(seq_dir):
        for f in files:
            out[os.path.relpath(os.path.join(dirpath, f), seq_dir)] = os.path.join(dirpath, f)
    return out


@pytest.mark.parametrize('write', ['npy', 'packed'])
def test_raw_recordings_give_the_tree_of_the_same_events_as_dat(ops, tmp_path, monkeypatch, write):
    """The anchor: the eight windows as EVT3 with vectors forced and as EVT2, decoded 64 payload bytes at a time, against the .dat path."""
    from leod_amd.data import ingest
    from leod_amd.data.utils import dat_events, raw_events
    from leod_amd.data.utils.types import DatasetType
    monkeypatch.setitem(ingest.SENSOR_HW, DatasetType.GEN1, (H, W))
    (t, x, y, p), off = _eight_windows()
    order = np.lexsort((x, p, y, t))                             # events of one timestamp row by row, so that neighbours can share a vector word
    t, x, y, p = t[order], x[order], y[order], p[order]
    src = tmp_path / 'src'
    src.mkdir()
    boxes = np.zeros((4,), dtype=PROPHESEE_BBOX)
    for i, bt in enumerate([2 * D, 4 * D, 4 * D, 8 * D]):
        boxes[i] = (bt, 2 + i, 3, 10, 8, i % 2, i, 0.5)
    np.save(str(src / 'box.npy'), boxes)
    dat_events.write_dat(str(src / 'a_td.dat'), dat_events.encode(t, x, y, p), H, W)
    w3 = raw_events.encode_evt3(t, x, y, p, first_time_high=777, vectors=True)
    assert {0x3, 0x4, 0x5} <= set((w3 >> 12).tolist())           # the window of one shared timestamp holds neighbours in a row
    raw_events.write_raw(str(src / 'evt3.raw'), w3, 'evt3', height=H, width=W)
    raw_events.write_raw(str(src / 'evt2.raw'), raw_events.encode_evt2(t, x, y, p, first_time_high=123_456), 'evt2', height=H, width=W,
                         style='evt')
    want_rep = ingest.ingest_recording(str(src / 'a_td.dat'), str(src / 'box.npy'), str(tmp_path / 'dat'), 'gen1', write=write)
    want = _tree_files(str(tmp_path / 'dat'))
    assert want_rep['frames'] == 8 and want_rep['labelled_frames'] == 3
    for name in ('evt3', 'evt2'):
        rep = ingest.ingest_recording(str(src / f'{name}.raw'), str(src / 'box.npy'), str(tmp_path / name), 'gen1', write=write,
                                      raw_chunk_bytes=64)
        got = _tree_files(str(tmp_path / name))
        assert sorted(got) == sorted(want), name
        for rel in want:
            if rel.endswith('.npz'):
                a, b = np.load(got[rel]), np.load(want[rel])
                assert sorted(a.files) == sorted(b.files)
                for k in b.files:
                    assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, rel, k)
            else:
                assert open(got[rel], 'rb').read() == open(want[rel], 'rb').read(), (name, rel)
        for k in ('frames', 'events', 'dropped_events', 'labelled_frames', 'boxes'):
            assert rep[k] == want_rep[k], (name, k)
        assert (rep['early_events'], rep['ignored_words'], rep['unknown_words'], rep['clock_wraps']) == (0, 0, 0, 0)


def test_unsorted_and_overflowing_recordings_are_refused(ops, tmp_path, monkeypatch):
    from leod_amd.data import ingest
    from leod_amd.data.utils import raw_events
    from leod_amd.data.utils.types import DatasetType
    monkeypatch.setitem(ingest.SENSOR_HW, DatasetType.GEN1, (H, W))
    unsorted = [c for c in HAND if c[0].startswith('time_high_100')][0][2]
    raw_events.write_raw(str(tmp_path / 'u.raw'), np.array(unsorted), 'evt3')
    for chunk in (4, 1 << 20):                                    # the decrease inside a chunk and across two
        with pytest.raises(ValueError, match='sorted in time'):
            ingest.ingest_recording(str(tmp_path / 'u.raw'), None, str(tmp_path / 'u'), 'gen1', raw_chunk_bytes=chunk)
    over = [TH | 0, TL | 0, AY | 0, AX | 1] + [TH | ((k * 1024) & 4095) for k in range(1, 1025)] + [AX | 2]
    raw_events.write_raw(str(tmp_path / 'o.raw'), np.array(over), 'evt3')
    with pytest.raises(ValueError, match='o.raw'):
        ingest.ingest_recording(str(tmp_path / 'o.raw'), None, str(tmp_path / 'o'), 'gen1')
    assert not [f for f in _tree_files(str(tmp_path)) if f.endswith(('.tmp', '.body'))]


def test_gen4_sized_header_gives_the_half_resolution_frame_file(ops, tmp_path):
    from oracle import postproc as op
    from leod_amd.data import ingest
    from leod_amd.data.utils import misc, raw_events
    rng = np.random.RandomState(8)
    t = np.sort(rng.randint(0, 2 * D + 1, 50))
    x, y, p = rng.randint(0, 1280, 50), rng.randint(0, 720, 50), rng.randint(0, 2, 50)
    x[:10], y[:10] = x[:10] | 1, y[:10] | 1                      # some events on the odd pixels that survive ds2
    fn = str(tmp_path / 'g4.raw')
    raw_events.write_raw(fn, raw_events.encode_evt3(t, x, y, p, first_time_high=9, vectors=True), 'evt3', height=720, width=1280)
    seq_dir = str(tmp_path / 'gen4' / 'train' / 'g4')
    rep = ingest.ingest_recording(fn, None, seq_dir, 'gen4')
    out = misc.get_ev_raw_fn(seq_dir, 'gen4')
    assert out.endswith('event_representations_ds2_nearest.npy') and rep['events'] == 50 and rep['boxes'] == 0
    frames = np.load(out)
    assert frames.shape == (rep['frames'], 20, 360, 640) and frames.any()
    off = np.searchsorted(t, np.arange(rep['frames'] + 1) * D, side='right')
    off[0] = 0
    for k in range(rep['frames']):
        s = slice(off[k], off[k + 1])
        assert np.array_equal(frames[k], op.stacked_histogram(x[s], y[s], p[s], t[s], 10, 720, 1280)[:, 1::2, 1::2]), k


def test_unlabelled_raw_recording_opens_as_a_stream(ops, tmp_path):
    from leod_amd.data import ingest
    from leod_amd.data.genx_utils.sequence_streaming import SequenceForIter
    from leod_amd.data.utils import misc, raw_events
    from leod_amd.data.utils.types import DatasetType, DataType
    rng = np.random.RandomState(2)
    n = 3000
    t = np.sort(rng.randint(0, 7 * D, n))
    ev = (t, rng.randint(0, 304, n), rng.randint(0, 240, n), rng.randint(0, 2, n))
    src = tmp_path / 'src'
    src.mkdir()
    raw_events.write_raw(str(src / 'mine.raw'), raw_events.encode_evt3(*ev, first_time_high=55, vectors=True), 'evt3', 240, 304)
    with pytest.raises(FileNotFoundError):
        ingest.ingest_split(str(src), str(tmp_path / 'gen1' / 'test'), 'gen1')
    rep, = ingest.ingest_split(str(src), str(tmp_path / 'gen1' / 'test'), 'gen1', unlabelled='ok', raw_chunk_bytes=4096)
    assert rep['frames'] == 7 and rep['events'] == n and rep['boxes'] == 0 and rep['labelled_frames'] == 0
    seq_dir = str(tmp_path / 'gen1' / 'test' / 'mine')
    frames = np.load(misc.get_ev_raw_fn(seq_dir, 'gen1'))
    assert frames.shape == (7, 20, 240, 304)
    seq = SequenceForIter(seq_dir, misc.EV_REPR_NAME, 3, DatasetType.GEN1, downsample_by_factor_2=False, start_from_zero=True)
    assert len(seq) == 3
    seen = []
    for i in range(len(seq)):
        s = seq.sample(i)
        for k, fr, lab, pad in zip(s[DataType.EV_IDX], s[DataType.EV_REPR], s[DataType.OBJLABELS_SEQ], s[DataType.IS_PADDED_MASK]):
            assert lab is None
            if not pad:
                assert np.array_equal(np.asarray(fr), frames[k])
                seen.append(k)
    assert seen == list(range(7))
