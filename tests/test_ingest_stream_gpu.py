"""The streaming route of the ingestion -- chunk reader, filter chain, carry of the incomplete window -- on one hand-built recording
that holds every place the carry logic can go wrong, as ``.dat`` and as EVT3 ``.raw``, with every chunk a single record, with chunks of
40 bytes and with the whole file in one chunk.  The trees must not depend on the chunk size or the container, and the frames are those
of ``ops.voxelize_u8`` per window on what the tests' sequential restatements keep (tests/filter_ref.py, tests/pixfilter_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref  # noqa: E402
import pixfilter_ref  # noqa: E402
from evt_cases import AX, AY, TH, TL  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
H, W, D, BINS = 24, 30, 1000, 10
N_FRAMES = 7
PM = (7, 5)                                                      # (x, y) of the masked pixel: it carries the long stretch
FLICKER_PIXEL = (20, 10)
TAU, TRAIL, STC, HOT_RATE = 150, 200, 50, 1800
BAND, BAND_US, LOCK = '2000:3000', (334, 500), 2                 # a period of 400 us is in the band
WHOLE = 1 << 20
CHUNKS = dict(dat=(8, 40, WHOLE), raw=(4, 40, WHOLE))            # a single record (.dat) / two EVT3 words, 40 bytes, the whole file
RAW_ONLY = ('early_events', 'ignored_words', 'unknown_words', 'clock_wraps')

# name -> (keywords of ingest_recording, the restatements that say what reaches the voxeliser)
OPTIONS = {
    'none': dict(),
    'denoise': dict(denoise_us=TAU),
    'mask': dict(pixel_mask='MASK'),
    'trail': dict(trail_us=TRAIL),
    'stc_flicker': dict(stc_us=STC, anti_flicker=BAND, flicker_lock=LOCK),
    'all': dict(denoise_us=TAU, hot_rate_hz=HOT_RATE, trail_us=TRAIL),
}


def _events():
    ev = [(0, 3, 3, 1), (0, 4, 3, 0)]                                                             # two events at t = 0
    ev += [(100, 3, 4, 1), (150, 4, 4, 1), (200, 5, 4, 0), (260, 5, 5, 1)]                        # neighbours in time and space
    ev += [(300, 18, 18, 1), (310, 19, 18, 1), (330, 18, 18, 1), (360, 18, 18, 1)]                # a burst of three on one pixel
    for k in range(5):                                                                            # 2.5 kHz on one pixel, into window 1
        ev += [(100 + 400 * k, *FLICKER_PIXEL, 1), (300 + 400 * k, *FLICKER_PIXEL, 0)]
    ev += [(400, 25, 20, 1), (700, 1, 20, 0), (1500, 31, 2, 1), (1600, 5, 25, 0), (1700, 27, 3, 1)]      # lone events; two beyond the sensor
    ev += [(990, 11, 10, 1), (1000, 10, 10, 1)]                                                   # exactly at 1 * D: the last of window 0
    ev += [(1100, 10, 11, 0), (1200, 11, 11, 1)]
    # windows 2, 3 and 4 are empty
    ev += [(5001, 3, 3, 1), (5050, 4, 3, 1), (5300, 22, 22, 0)]
    ev += [(5400, 14, 8, 1), (5420, 15, 8, 1), (5440, 15, 9, 0), (5460, 14, 9, 1), (5480, 14, 8, 0), (5600, 2, 12, 1)]
    ev += [(5900 + 20 * k, *PM, 1) for k in range(12)]                                            # the stretch: across 6 * D, one event at it
    ev += [(6300, 15, 15, 0), (6350, 16, 15, 0), (6400, 16, 16, 1), (6600, 25, 5, 1)]
    ev += [(6800, *PM, 0), (6900, *PM, 0)]                                                        # the last event continues a burst, alone, masked
    t, x, y, p = (np.array(c, dtype=np.int64) for c in zip(*ev))
    order = np.lexsort((x, y, t))
    return t[order], x[order], y[order], p[order]


def _kept(name, rec, mask, hot):
    """What reaches the voxeliser and the filters' part of the report, by the restatements."""
    if name == 'none':
        return rec, {}
    if name in ('denoise', 'mask'):
        f = filter_ref.Filter(H, W, TAU if name == 'denoise' else None, mask if name == 'mask' else None)
        kept, c = f.feed(rec), f.counters()
        return kept, dict(events=c['seen'], kept_events=c['kept'], masked_events=c['masked'], unsupported_events=c['unsupported'],
                          dropped_events=c['outside'], masked_pixels=int(name == 'mask'))
    first = dict(trail=dict(burst_us=TRAIL, burst_keep='first'),
                 stc_flicker=dict(burst_us=STC, burst_keep='from_second', flicker=BAND_US + (LOCK,)),
                 all=dict(burst_us=TRAIL, burst_keep='first', mask=hot))[name]
    pf = pixfilter_ref.PixelFilter(H, W, **first)
    kept, c = pf.feed(rec), pf.counters()
    rep = dict(events=c['seen'], kept_events=c['kept'], masked_events=c['masked'], unsupported_events=0, dropped_events=c['outside'],
               flicker_events=c['flicker'], burst_events=c['burst'], masked_pixels=int(name == 'all'))
    if name == 'all':
        f = filter_ref.Filter(H, W, TAU, None)
        kept = f.feed(kept)
        rep.update(kept_events=f.counters()['kept'], unsupported_events=f.counters()['unsupported'])
    return kept, rep


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def case(ops, tmp_path_factory):
    """The recording in both containers and, computed once, per option set the expected frames and report."""
    from leod_amd.data.utils import dat_events, event_filter as ef, raw_events
    t, x, y, p = _events()
    src = str(tmp_path_factory.mktemp('src'))
    dat_events.write_dat(os.path.join(src, 'a_td.dat'), dat_events.encode(t, x, y, p), H, W)
    raw_events.write_raw(os.path.join(src, 'a.raw'), raw_events.encode_evt3(t, x, y, p, first_time_high=777, vectors=True), 'evt3',
                         height=H, width=W)
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[PM[1], PM[0]] = 1
    np.save(os.path.join(src, 'mask.npy'), mask)
    inside = (x < W) & (y < H)
    counts = np.zeros((H, W), dtype=np.int64)
    np.add.at(counts, (y[inside], x[inside]), 1)
    hot = ef.hot_pixel_mask(counts, int(t[-1] - t[0]), HOT_RATE)
    rec = filter_ref.records(t, x, y, p)
    want = {}
    for name in OPTIONS:
        kept, rep = _kept(name, rec, mask, hot)
        kt, kx, ky, kp = filter_ref.unpack(kept)
        ok = (kx < W) & (ky < H)                                  # without a filter the voxeliser drops the events beyond the sensor
        off = dat_events.window_offsets(kt[ok], D, N_FRAMES)
        frames = np.zeros((N_FRAMES, 2 * BINS, H, W), dtype=np.uint8)
        for k in range(N_FRAMES):
            s = slice(int(off[k]), int(off[k + 1]))
            if s.start < s.stop:
                frames[k] = ops.voxelize_u8(*(torch.from_numpy(np.ascontiguousarray(a[ok][s])).to(DEV) for a in (kx, ky, kp, kt)),
                                            BINS, H, W).cpu().numpy()
        base = dict(frames=N_FRAMES, events=len(t), dropped_events=int((~inside).sum()), labelled_frames=0, boxes=0)
        want[name] = dict(kept=kept, frames=frames, report=dict(base, **rep))
    return dict(src=src, ev=(t, x, y, p), rec=rec, mask=mask, hot=hot, want=want)


@pytest.fixture()
def small_sensor(monkeypatch):
    from leod_amd.data import ingest
    from leod_amd.data.utils.types import DatasetType
    monkeypatch.setitem(ingest.SENSOR_HW, DatasetType.GEN1, (H, W))
    return ingest


def _tree_files(seq_dir):
    return {os.path.relpath(os.path.join(d, f), seq_dir): os.path.join(d, f) for d, _, files in os.walk(seq_dir) for f in files}


def _same_trees(got_dir, want_dir, what):
    got, want = _tree_files(got_dir), _tree_files(want_dir)
    assert sorted(got) == sorted(want), what
    for rel in want:
        if rel.endswith('.npz'):                                 # a zip archive states the time it was written: its arrays are compared
            a, b = np.load(got[rel]), np.load(want[rel])
            assert sorted(a.files) == sorted(b.files), (what, rel)
            for k in b.files:
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, rel, k)
        else:
            assert open(got[rel], 'rb').read() == open(want[rel], 'rb').read(), (what, rel)


def test_the_recording_is_what_it_says(case):
    t, x, y, p = case['ev']
    rec, want = case['rec'], case['want']
    assert 50 <= len(t) <= 70 and np.all(np.diff(t) >= 0) and (t == 0).sum() == 2 and (t == D).sum() == 1 and (t == 6 * D).sum() == 1
    assert not ((t > 2 * D) & (t <= 5 * D)).any() and -(-int(t[-1]) // D) == N_FRAMES            # three empty windows
    assert case['hot'].sum() == 1 and case['hot'][PM[1], PM[0]] and np.array_equal(case['hot'], case['mask'])
    on_pm = (x == PM[0]) & (y == PM[1])
    stretch = np.flatnonzero(on_pm & (t >= 5900) & (t <= 6120))
    assert len(stretch) == 12 and np.all(np.diff(stretch) == 1) and on_pm[-1] and on_pm[-2]
    for name in ('denoise', 'mask', 'trail', 'all'):
        kept = {tuple(r) for r in want[name]['kept'].tolist()}
        gone = [tuple(rec[i].tolist()) not in kept for i in stretch]
        # more than the 5 records of a 40-byte chunk in a row are removed, and so is the last event of the recording
        assert sum(gone[1:]) == 11 and (name == 'trail' or gone[0]), name
        assert tuple(rec[-1].tolist()) not in kept, name
        assert len(kept) > 5, name
    assert want['stc_flicker']['report']['flicker_events'] > 0 and want['stc_flicker']['report']['burst_events'] > 0
    assert want['all']['report']['unsupported_events'] > 0 and want['denoise']['report']['unsupported_events'] > 12
    assert want['none']['report']['dropped_events'] == 2
    for name in OPTIONS:
        r = want[name]['report']
        if name != 'none':
            assert r['kept_events'] + r.get('flicker_events', 0) + r.get('burst_events', 0) + r['masked_events'] + \
                r['unsupported_events'] + r['dropped_events'] == r['events'], name
        assert not want[name]['frames'][2:5].any() and want[name]['frames'][0].any(), name


@pytest.mark.parametrize('name', list(OPTIONS))
def test_trees_and_reports_do_not_depend_on_the_chunk_size_or_the_container(ops, tmp_path, case, small_sensor, name):
    ingest = small_sensor
    kw = dict(OPTIONS[name])
    if 'pixel_mask' in kw:
        kw['pixel_mask'] = os.path.join(case['src'], 'mask.npy')
    want = case['want'][name]
    first = None
    for cont, fn in (('dat', 'a_td.dat'), ('raw', 'a.raw')):
        for chunk in CHUNKS[cont]:
            out = str(tmp_path / f'{cont}{chunk}')
            rep = ingest.ingest_recording(os.path.join(case['src'], fn), None, out, 'gen1', duration_us=D, bins=BINS,
                                          raw_chunk_bytes=chunk, **kw)
            assert rep.pop('recording') == out
            if cont == 'raw':
                assert [rep.pop(k) for k in RAW_ONLY] == [0, 0, 0, 0], (name, cont, chunk)
            assert rep == want['report'], (name, cont, chunk)
            if first is None:
                first = out
                frames = np.load(os.path.join(out, 'event_representations_v2', ingest.ev_repr_name(D, BINS), 'event_representations.npy'))
                assert frames.shape == want['frames'].shape and frames.dtype == np.uint8
                for k in range(N_FRAMES):
                    assert np.array_equal(frames[k], want['frames'][k]), (name, f'frame {k}')
                if name == 'all':
                    hot_fn = [f for f in _tree_files(out) if f.endswith('hot_pixels.npy')]
                    assert len(hot_fn) == 1 and np.array_equal(np.load(_tree_files(out)[hot_fn[0]]), case['hot'])
            else:
                _same_trees(out, first, f'{name}: {cont} in chunks of {chunk} against the first tree')


@pytest.mark.parametrize('cont', ['dat', 'raw'])
def test_the_chunk_reader_alone(ops, case, cont):
    """The chunks of every size, joined, are the records of the whole file: for a .raw file one ``ops.decode_evt`` of the whole payload."""
    from leod_amd.data import ingest
    from leod_amd.data.utils import dat_events, raw_events
    if cont == 'dat':
        _, records = dat_events.open_records(os.path.join(case['src'], 'a_td.dat'))
        payload, encoding = records.view(np.uint8).reshape(-1), 'dat'
        whole = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 8)
    else:
        hdr, payload = raw_events.open_words(os.path.join(case['src'], 'a.raw'))
        encoding = hdr.encoding
        rec, state = ops.decode_evt(torch.from_numpy(np.array(payload)).to(DEV), encoding)
        whole = rec.cpu().numpy()
        whole_counters = ops.evt_state_counters(state)
    assert whole.shape == (len(case['rec']), 8) and np.array_equal(whole.view('<u4'), case['rec'])
    for chunk in CHUNKS[cont]:
        reader = ingest._RecordChunks(payload, encoding, chunk, torch.device(DEV), 'a')
        got = []
        for rec in reader:
            assert rec.is_cuda and rec.dtype == torch.uint8 and rec.dim() == 2 and rec.shape[1] == 8
            got.append(rec.cpu().numpy())                        # copied before the reader writes its pinned buffer again
        n_chunks = -(-len(payload) // (chunk if cont == 'raw' else max(chunk // 8, 1) * 8))
        assert len(got) == n_chunks, (cont, chunk)
        assert np.array_equal(np.concatenate(got), whole), (cont, chunk)
        if cont == 'raw':
            assert reader.counters() == whole_counters
        else:
            assert reader.counters() == dict(events=0, early_events=0, ignored_words=0, unknown_words=0, overflow=0, wraps=0)
    with pytest.raises(ValueError, match='raw_chunk_bytes=6'):
        ingest._RecordChunks(payload, encoding, 6, torch.device(DEV), 'a')


@pytest.mark.parametrize('name', list(OPTIONS))
def test_a_decrease_across_two_chunks_is_refused_alike_on_every_route(ops, tmp_path, case, small_sensor, name):
    """Times 8292 -> 4196 between the records 4 and 5: with a record per chunk and with 40-byte chunks (5 .dat records) the two lie in
    different chunks.  Every streaming route states it in the same words.  A .dat file without a filter is checked on the host by
    ``dat_events.scan_windows``, which also names the position; it names the same two times."""
    from leod_amd.data.utils import dat_events, raw_events
    ingest = small_sensor
    ts = [5, 9, 50, 4096 + 7, 2 * 4096 + 100, 4096 + 100, 4096 + 104]
    xs = list(range(1, 8))
    words = [TH | 0, TL | 5, AY | 2, AX | 1, TL | 9, AX | 2, TL | 50, AX | 3, TH | 1, TL | 7, AX | 4, TH | 2, TL | 100, AX | 5, TH | 1, AX | 6,
             TL | 104, AX | 7]
    dat_fn, raw_fn = str(tmp_path / 'u_td.dat'), str(tmp_path / 'u.raw')
    dat_events.write_dat(dat_fn, dat_events.encode(np.array(ts), np.array(xs), np.full(7, 2), np.zeros(7, dtype=np.int64)), H, W)
    raw_events.write_raw(raw_fn, np.array(words), 'evt3')
    kw = dict(OPTIONS[name])
    if 'pixel_mask' in kw:
        kw['pixel_mask'] = case['mask']
    tail = 'timestamps decrease (8292 -> 4196); a recording must be sorted in time'
    for fn, chunks in ((dat_fn, (8, 40, WHOLE)), (raw_fn, (4, WHOLE))):
        for chunk in chunks:
            with pytest.raises(ValueError) as info:
                ingest.ingest_recording(fn, None, str(tmp_path / 'out'), 'gen1', duration_us=D, bins=BINS, raw_chunk_bytes=chunk, **kw)
            if name == 'none' and fn == dat_fn:
                assert str(info.value).startswith(f'{fn}: timestamps decrease at event 5 (8292 -> 4196); a recording must be sorted in time')
            else:
                assert str(info.value) == f'{fn}: {tail}', (name, fn, chunk)
    assert not [f for f in _tree_files(str(tmp_path)) if f.endswith(('.tmp', '.body'))]
