"""Metavision RAW recordings without a GPU: the header reader, the encoders against the tests' own sequential decoder (tests/evt_ref.py),
hand-written word lists with their events stated literally, the associativity of the transform the device decoder scans with
(``raw_events.compose``, the algebra of csrc/k_evt.hip), and how ``ingest_split`` finds recordings."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evt_ref  # noqa: E402
from evt_cases import AX, AY, HAND, TH, TL, random_words  # noqa: E402

from leod_amd.data.utils import raw_events as rw  # noqa: E402

def _counters(expected, n):
    return dict(dict(events=n, early_events=0, ignored_words=0, unknown_words=0, overflow=0, wraps=0), **expected)


@pytest.mark.parametrize('case', HAND, ids=[c[0] for c in HAND])
def test_hand_written_words(case):
    _, fmt, words, events, counters = case
    (t, x, y, p), d = evt_ref.decode(words, fmt)
    assert list(zip(t.tolist(), x.tolist(), y.tolist(), p.tolist())) == events
    assert d.counters() == _counters(counters, len(events))
    t2, x2, y2, p2, c2 = rw.decode(np.array(words), 'evt%d' % fmt)                 # the tools' decoder reads them the same way
    assert list(zip(t2.tolist(), x2.tolist(), y2.tolist(), p2.tolist())) == events and c2 == _counters(counters, len(events))
    if case[0].startswith('time_high_100'):
        assert (np.diff(t) < 0).any()


def _random_events(rng, n, t_max, w=304, h=240):
    t = np.sort(rng.randint(0, t_max, n))
    return t, rng.randint(0, w, n), rng.randint(0, h, n), rng.randint(0, 2, n)


def _clustered_events(rng, n_groups):
    """Events that share t, y and p in runs of neighbouring columns: what the vector words are for."""
    t, x, y, p = [], [], [], []
    now = 0
    for _ in range(n_groups):
        now += int(rng.randint(0, 3000))
        cols = np.unique(rng.randint(0, 30, rng.randint(1, 9))) + rng.randint(0, 270)
        t += [now] * len(cols); x += cols.tolist(); y += [int(rng.randint(0, 240))] * len(cols); p += [int(rng.randint(0, 2))] * len(cols)
    return tuple(np.array(a, dtype=np.int64) for a in (t, x, y, p))


@pytest.mark.parametrize('first_high', [0, 1234])
@pytest.mark.parametrize('vectors', [False, True])
def test_evt3_round_trip(first_high, vectors):
    rng = np.random.RandomState(5 + first_high + vectors)
    for clustered, ev in ((False, _random_events(rng, 400, 3_000_000)), (True, _clustered_events(rng, 150))):
        words = rw.encode_evt3(*ev, first_time_high=first_high, vectors=vectors)
        got, d = evt_ref.decode(words, 3)
        for a, b in zip(got, ev):
            assert np.array_equal(a, b)
        assert d.counters() == _counters({}, len(ev[0])) and d.time_base == first_high << 12
        kinds = set((words >> 12).tolist())
        if not vectors:
            assert not kinds & {0x3, 0x4, 0x5}
        elif clustered:                                           # vectors are forced wherever neighbours share t, y and p
            assert {0x3, 0x4, 0x5} <= kinds
        assert (words >> 12 == 0x8).sum() > len(np.unique((ev[0] + (first_high << 12)) >> 12))      # TIME_HIGH is repeated


def test_evt3_round_trip_over_a_clock_wrap():
    rng = np.random.RandomState(9)
    t = np.sort(rng.randint(0, 40_000_000, 300))                  # 40 s from TIME_HIGH 3000: 3000 + 9765 = 3 x 4096 + 477
    ev = (t, rng.randint(0, 304, 300), rng.randint(0, 240, 300), rng.randint(0, 2, 300))
    words = rw.encode_evt3(*ev, first_time_high=3000, vectors=True)
    got, d = evt_ref.decode(words, 3)
    for a, b in zip(got, ev):
        assert np.array_equal(a, b)
    assert d.wraps == (3000 + (int(t[-1]) >> 12)) >> 12 == 3 and d.overflow == 0
    # a long pause is bridged by TIME_HIGH words so that it does not look like a wrap
    pause = (np.array([0, 9_000_000, 9_000_001]), np.array([1, 2, 3]), np.array([4, 5, 6]), np.array([0, 1, 0]))
    got, d = evt_ref.decode(rw.encode_evt3(*pause, first_time_high=4000), 3)
    assert np.array_equal(got[0], pause[0]) and d.wraps == 1


@pytest.mark.parametrize('first_high', [0, 77_000])
def test_evt2_round_trip(first_high):
    rng = np.random.RandomState(3)
    ev = _random_events(rng, 500, 2_000_000, w=1280, h=720)
    words = rw.encode_evt2(*ev, first_time_high=first_high)
    got, d = evt_ref.decode(words, 2)
    for a, b in zip(got, ev):
        assert np.array_equal(a, b)
    assert d.counters() == _counters({}, 500) and d.time_base == first_high << 6


def test_overflow_is_flagged():
    words = [TH | 0, TL | 0, AY | 0, AX | 1] + [TH | ((k * 1024) & 4095) for k in range(1, 1025)] + [AX | 2]     # 256 wraps: t = 2^32
    (t, x, y, p), d = evt_ref.decode(words, 3)
    assert d.wraps == 256 and d.overflow == 1 and t.tolist() == [0, 0]
    assert rw.decode(np.array(words), 'evt3')[4]['overflow'] == 1


# ---- the header ---------------------------------------------------------------------------------------------------------------------
def _write(tmp_path, name, header: bytes, payload: bytes):
    fn = str(tmp_path / name)
    with open(fn, 'wb') as f:
        f.write(header + payload)
    return fn


def test_header_variants(tmp_path):
    pay3 = np.array([TH | 1, TL | 2, AY | 3, AX | 4], dtype='<u2').tobytes()
    fn = _write(tmp_path, 'a.raw', b'% date 2023-03-01\n% evt 3.0\n% geometry 304x240\n% end\n', pay3)
    hdr = rw.parse_header(fn)
    assert hdr == rw.RawHeader('evt3', os.path.getsize(fn) - 8, 240, 304)
    h2, payload = rw.open_words(fn)
    assert h2 == hdr and payload.dtype == np.uint8 and bytes(payload) == pay3 and not payload.flags.writeable
    # no "% end": the header ends before the first byte that begins no "% " line (here the low byte of TIME_HIGH | 1)
    fn = _write(tmp_path, 'b.raw', b'% evt 3.0\n', pay3)
    assert rw.parse_header(fn) == rw.RawHeader('evt3', 10, None, None)
    fn = _write(tmp_path, 'c.raw', b'% format EVT3;height=720;width=1280\n% end\n', pay3)
    assert rw.parse_header(fn)[0::2] == ('evt3', 720) and rw.parse_header(fn).width == 1280
    fn = _write(tmp_path, 'd.raw', b'% format EVT2\n% geometry 1280x720\n% end\n', pay3)
    assert rw.parse_header(fn) == rw.RawHeader('evt2', os.path.getsize(fn) - 8, 720, 1280)
    # a payload whose first bytes happen to be "% " is still payload behind "% end"
    fn = _write(tmp_path, 'e.raw', b'% evt 3.0\n% end\n', b'% ' + pay3)
    assert rw.parse_header(fn).data_offset == 16


@pytest.mark.parametrize('header, payload, needle', [
    (b'% evt 2.1\n% end\n', b'\0' * 8, 'evt 2.1'),
    (b'% format EVT21\n% end\n', b'\0' * 8, 'EVT21'),
    (b'% evt 4.0\n% end\n', b'\0' * 8, 'evt 4.0'),
    (b'% date today\n% end\n', b'\0' * 8, 'no encoding'),
    (b'', b'\0' * 8, 'no encoding'),
    (b'% evt 3.0\n% end\n', b'\0' * 7, 'whole number'),
    (b'% evt 2.0\n% end\n', b'\0' * 6, 'whole number'),
    (b'% evt 3.0\n% format EVT2\n% end\n', b'\0' * 8, 'evt2 / evt3'),
])
def test_header_refusals_name_the_file(tmp_path, header, payload, needle):
    fn = _write(tmp_path, 'refused.raw', header, payload)
    with pytest.raises(ValueError) as e:
        rw.parse_header(fn)
    assert fn in str(e.value) and needle in str(e.value)


def test_geometry_mismatch_is_refused_before_the_device_is_touched(tmp_path):
    from leod_amd.data import ingest
    fn = str(tmp_path / 'g.raw')
    rw.write_raw(fn, rw.encode_evt3([1], [2], [3], [1]), 'evt3', height=480, width=640)
    with pytest.raises(ValueError) as e:
        ingest.ingest_recording(fn, None, str(tmp_path / 'out'), 'gen1')
    assert fn in str(e.value) and '480' in str(e.value) and '240' in str(e.value)


def test_write_raw_styles(tmp_path):
    words = rw.encode_evt2([5], [6], [7], [1])
    for style, end in (('format', True), ('evt', True), ('evt', False)):
        fn = str(tmp_path / f'{style}{end}.raw')
        rw.write_raw(fn, words, 'evt2', height=720, width=1280, style=style, end=end)
        hdr, payload = rw.open_words(fn)
        assert (hdr.encoding, hdr.height, hdr.width) == ('evt2', 720, 1280) and bytes(payload) == words.tobytes()


# ---- the algebra ---------------------------------------------------------------------------------------------------------------------
def _sequential_state(words, fmt):
    d = evt_ref.Decoder(fmt)
    d.feed(words)
    first = d.time_base >> (12 if fmt == 3 else 6)
    s = d.state()
    return dict(set=s[0], low=s[3], y=s[4], vpol=s[6], first=first, last=s[1], wraps=s[2], base=s[5])


def _visible(t):
    """A transform as a state: the fields a decoder can read (values of unset fields and the base offset of an unset base are not)."""
    o = dict(set=t['set'], wraps=t['wraps'])
    for bit, names in ((rw.F_HIGH, ('first', 'last')), (rw.F_LOW, ('low',)), (rw.F_Y, ('y',)), (rw.F_BASE, ('base', 'vpol'))):
        for n in names:
            o[n] = t[n] if t['set'] & bit else None
    return o


@pytest.mark.parametrize('fmt', [3, 2])
def test_transform_composition_in_any_order_is_the_sequential_state(fmt):
    """3 000 random streams of 1-40 words: the words' transforms combined pairwise in a random order (adjacent pairs only: the operation
    is associative, not commutative), also across a random chunk split, give the state of the sequential decoder."""
    rng = np.random.RandomState(2024 + fmt)
    enc = 'evt%d' % fmt
    for _ in range(3000):
        words = random_words(rng, rng.randint(1, 41), fmt).tolist()
        parts = [rw.word_transform(w, enc) for w in words]
        cut = rng.randint(0, len(parts) + 1)                      # the chunk split: each side is reduced on its own, then the two halves
        halves = []
        for side in (parts[:cut], parts[cut:]):
            side = list(side) or [dict(rw.IDENTITY)]
            while len(side) > 1:
                i = rng.randint(0, len(side) - 1)
                side[i:i + 2] = [rw.compose(side[i], side[i + 1], enc)]
            halves.append(side[0])
        got = rw.compose(halves[0], halves[1], enc)
        assert _visible(got) == _visible(_sequential_state(words, fmt)), words


# ---- ingest_split ---------------------------------------------------------------------------------------------------------------------
def test_ingest_split_finds_raw_and_handles_box_files(tmp_path, monkeypatch):
    from leod_amd.data import ingest
    src = tmp_path / 'src'
    src.mkdir()
    calls = []

    def fake(ev_fn, bbox_fn, out_dir, dataset_type, **kw):
        calls.append((os.path.basename(ev_fn), None if bbox_fn is None else os.path.basename(bbox_fn), os.path.basename(out_dir)))
        return dict(recording=out_dir)

    monkeypatch.setattr(ingest, 'ingest_recording', fake)
    for name in ('b.raw', 'a_td.dat', 'a_bbox.npy', 'b_bbox.npy'):
        (src / name).write_bytes(b'')
    assert len(ingest.ingest_split(str(src), str(tmp_path / 'dst'), 'gen1')) == 2
    assert calls == [('a_td.dat', 'a_bbox.npy', 'a'), ('b.raw', 'b_bbox.npy', 'b')]
    # a recording without a box file: today's FileNotFoundError by default, a tree without labels on request
    (src / 'c.raw').write_bytes(b'')
    with pytest.raises(FileNotFoundError):
        ingest.ingest_split(str(src), str(tmp_path / 'dst'), 'gen1')
    del calls[:]
    ingest.ingest_split(str(src), str(tmp_path / 'dst'), 'gen1', unlabelled='ok')
    assert calls[-1] == ('c.raw', None, 'c') and len(calls) == 3
    with pytest.raises(ValueError):
        ingest.ingest_split(str(src), str(tmp_path / 'dst'), 'gen1', unlabelled='maybe')
    # the same stem in both containers
    (src / 'b_td.dat').write_bytes(b'')
    with pytest.raises(ValueError) as e:
        ingest.ingest_split(str(src), str(tmp_path / 'dst'), 'gen1', unlabelled='ok')
    assert "'b'" in str(e.value)


def test_command_line_knows_unlabelled(tmp_path, monkeypatch):
    from leod_amd.data import ingest
    seen = {}
    monkeypatch.setattr(ingest, 'ingest_split', lambda src, dst, ds, **kw: seen.update(kw) or [1])
    (tmp_path / 'src').mkdir()
    assert ingest.main([str(tmp_path / 'src'), str(tmp_path / 'dst'), '--dataset', 'gen1', '--unlabelled', 'ok']) == 0
    assert seen['unlabelled'] == 'ok'
    assert ingest.main([str(tmp_path / 'src'), str(tmp_path / 'dst'), '--dataset', 'gen1']) == 0 and seen['unlabelled'] == 'error'


def test_empty_box_array_gives_empty_labels():
    from leod_amd.data import ingest
    lab, starts, repr_idx = ingest.convert_labels(np.zeros((0,), dtype=ingest.LABEL_DTYPE), 8, 50_000, None)
    assert len(lab) == 0 and len(starts) == 0 and len(repr_idx) == 0 and lab.dtype == ingest.LABEL_DTYPE


@pytest.mark.parametrize('reserve', [None, 64, 4096])
def test_streamed_npy_file_is_the_file_open_memmap_writes(tmp_path, reserve):
    """The dense frame file of the .raw path, whose length is known only at the end: with the header's room reserved (None) and with a
    reserve that does not fit, which moves the frames once."""
    from leod_amd.data import ingest
    frames = np.random.RandomState(1).randint(0, 256, (11, 4, 6, 5)).astype(np.uint8)
    want = str(tmp_path / 'want.npy')
    mm = np.lib.format.open_memmap(want, mode='w+', dtype=np.uint8, shape=frames.shape)
    mm[:] = frames
    mm.flush()
    del mm
    for n_frames in (11, 0):
        fn = str(tmp_path / f'got{n_frames}.npy')
        sink = ingest._NpyStream(fn, frames.shape[1:], reserve=reserve)
        for a in range(0, n_frames, 4):
            sink.append(frames[a:a + 4])
        sink.close()
        assert sorted(os.listdir(str(tmp_path))) == sorted({'want.npy', 'got11.npy', f'got{n_frames}.npy'})
        got = np.load(fn)
        assert got.dtype == np.uint8 and got.shape == (n_frames,) + frames.shape[1:] and np.array_equal(got, frames[:n_frames])
        if n_frames == 11:
            assert open(fn, 'rb').read() == open(want, 'rb').read()
    sink = ingest._NpyStream(str(tmp_path / 'gone.npy'), frames.shape[1:], reserve=reserve)
    sink.append(frames[:2])
    sink.abort()
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith('gone')]
