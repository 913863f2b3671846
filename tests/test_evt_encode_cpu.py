"""The event-file writer without a GPU: the tests' sequential streaming encoder (tests/evt_encode_ref.py) against the normative numpy
encoders ``raw_events.encode_evt2`` / ``encode_evt3`` word for word and through the tests' decoder (tests/evt_ref.py); the files
``event_writer.EventFileWriter`` writes; every refusal of the new ingestion options that needs no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evt_encode_ref as er  # noqa: E402
import evt_ref  # noqa: E402

from leod_amd.data.utils import dat_events, event_writer, raw_events  # noqa: E402

PERIODS, FIRST_HIGHS = (1, 3, 64), (0, 4095)
MODES = ((2, False), (3, False), (3, True))


def host_encode(ev, fmt, vectors, period, first):
    if fmt == 2:
        return raw_events.encode_evt2(*ev, first_time_high=first, high_period=period)
    return raw_events.encode_evt3(*ev, first_time_high=first, vectors=vectors, high_period=period)


def test_the_sequential_encoder_is_the_numpy_encoder_on_the_hand_cases():
    for name, ev in er.hand_cases().items():
        for fmt, vectors in MODES:
            for period in PERIODS:
                for first in FIRST_HIGHS:
                    want = host_encode(ev, fmt, vectors, period, first)
                    got = er.encode(*ev, fmt, vectors, period, first)
                    assert got.dtype == want.dtype and np.array_equal(got, want), (name, fmt, vectors, period, first)


def test_the_sequential_encoder_is_the_numpy_encoder_on_random_streams_and_the_words_decode_to_the_events():
    rng = np.random.RandomState(11)
    seen = dict(vector_groups=0, pause_1024=0, pause_4096=0, beyond_2_24=0)
    for i in range(300):
        ev = er.random_stream(rng, int(rng.randint(1, 260)))
        t = ev[0]
        hi = t >> 12
        seen['pause_1024'] += int((np.diff(hi) > 1024).any())
        seen['pause_4096'] += int((np.diff(hi) > 4096).any())
        seen['beyond_2_24'] += int(t.max() >= 1 << 24)
        for fmt, vectors in MODES:
            for period in PERIODS:
                for first in FIRST_HIGHS:
                    want = host_encode(ev, fmt, vectors, period, first)
                    e = er.Encoder(fmt, vectors, period, first)
                    for one in zip(*(a.tolist() for a in ev)):
                        e.push(*one)
                    e.flush()
                    assert np.array_equal(np.array(e.words, dtype=want.dtype), want), (i, fmt, vectors, period, first)
                    seen['vector_groups'] += e.vector_groups
        fmt, vectors = MODES[i % 3]
        (dt, dx, dy, dp), d = evt_ref.decode(host_encode(ev, fmt, vectors, PERIODS[i % 3], FIRST_HIGHS[i % 2]), fmt)
        assert all(np.array_equal(a, b) for a, b in zip((dt, dx, dy, dp), ev)), (i, fmt, vectors)
        c = d.counters()
        assert (c['early_events'], c['ignored_words'], c['unknown_words'], c['overflow']) == (0, 0, 0, 0) and c['events'] == len(t)
    assert seen['vector_groups'] > 10000 and min(seen['pause_1024'], seen['pause_4096'], seen['beyond_2_24']) > 20, seen


def _records(n=500, seed=3):
    rng = np.random.RandomState(seed)
    ev = er.random_stream(rng, n)
    return ev, dat_events.encode(*ev)


def test_a_dat_file_reads_back_and_is_the_file_write_dat_writes(tmp_path):
    import torch
    ev, rec = _records()
    fn = str(tmp_path / 'a_td.dat')
    w = event_writer.EventFileWriter(fn, 'dat', 240, 304)
    assert os.path.exists(fn + '.tmp') and not os.path.exists(fn)
    for a, b in ((0, 7), (7, 7), (7, 300), (300, len(rec))):     # an empty chunk among them
        w.append(torch.from_numpy(rec[a:b].view(np.uint8).copy()))
    w.close()
    assert not os.path.exists(fn + '.tmp') and (w.events, w.payload_bytes) == (len(rec), 8 * len(rec))
    hdr, got = dat_events.open_records(fn)
    assert (hdr.height, hdr.width, hdr.n_events) == (240, 304, len(rec)) and np.array_equal(got, rec)
    assert all(np.array_equal(a, b) for a, b in zip(dat_events.decode(got), ev))
    dat_events.write_dat(str(tmp_path / 'want.dat'), rec, 240, 304)
    assert open(fn, 'rb').read() == open(str(tmp_path / 'want.dat'), 'rb').read()


@pytest.mark.parametrize('fmt', ['evt2', 'evt3'])
def test_a_raw_file_of_host_words_parses_and_is_the_file_write_raw_writes(tmp_path, fmt):
    ev, _ = _records()
    words = raw_events.encode_evt2(*ev) if fmt == 'evt2' else raw_events.encode_evt3(*ev, vectors=True)
    fn = str(tmp_path / 'a.raw')
    w = event_writer.EventFileWriter(fn, fmt, 240, 304, vectors=fmt == 'evt3')
    half = len(words) // 2
    w.append_bytes(words[:half].view(np.uint8))
    w.append_bytes(words[half:])
    w.close()                                                    # fed by append_bytes alone: no device is needed
    assert not os.path.exists(fn + '.tmp') and w.words == len(words)
    hdr = raw_events.parse_header(fn)
    assert (hdr.encoding, hdr.height, hdr.width) == (fmt, 240, 304)
    _, payload = raw_events.open_words(fn)
    assert np.array_equal(np.asarray(payload).view(raw_events.WORD_DTYPE[fmt]), words)
    t, x, y, p, c = raw_events.decode(payload, fmt)
    assert all(np.array_equal(a, b) for a, b in zip((t, x, y, p), ev)) and c['early_events'] == c['unknown_words'] == 0
    raw_events.write_raw(str(tmp_path / 'want.raw'), words, fmt, 240, 304)
    assert open(fn, 'rb').read() == open(str(tmp_path / 'want.raw'), 'rb').read()
    with pytest.raises(ValueError, match='whole number'):
        event_writer.EventFileWriter(str(tmp_path / 'b.raw'), fmt, 240, 304).append_bytes(np.zeros(3, dtype=np.uint8))


def test_abort_leaves_nothing(tmp_path):
    for fmt, name in (('dat', 'a_td.dat'), ('evt3', 'a.raw')):
        fn = str(tmp_path / name)
        w = event_writer.EventFileWriter(fn, fmt, 240, 304)
        w.append_bytes(np.zeros(16, dtype=np.uint8))
        w.abort()
        assert os.listdir(str(tmp_path)) == []


def test_the_writer_refuses_what_no_file_holds(tmp_path):
    fn = str(tmp_path / 'a.raw')
    for kw in (dict(fmt='evt4'), dict(fmt='evt2', vectors=True), dict(fmt='dat', vectors=True), dict(fmt='evt3', width=2049),
               dict(fmt='evt2', height=2049), dict(fmt='evt3', height=0), dict(fmt='evt3', vectors=1.5)):
        args = dict(dict(fmt='evt3', height=240, width=304, vectors=False), **kw)
        with pytest.raises(ValueError):
            event_writer.EventFileWriter(fn, args['fmt'], args['height'], args['width'], vectors=args['vectors'])
    event_writer.check_format('evt3', 2048, 2048, True)
    event_writer.check_format('dat', 4096, 16384)                # .dat records hold 14 bits of each
    assert os.listdir(str(tmp_path)) == []


def test_the_options_are_checked_before_anything_is_opened():
    from leod_amd.data import ingest
    assert ingest.check_write_options() is None
    assert ingest.check_write_options('evt3', 'd', True) == dict(fmt='evt3', dir='d', vectors=True)
    assert ingest.check_write_options('dat', 'd') == dict(fmt='dat', dir='d', vectors=False)
    for args in (('evt3',), ('evt3', None, True), ('evt2', 'd', True), ('dat', 'd', True), (None, 'd'), (None, None, True), ('evt1', 'd'),
                 ('evt3', ''), ('evt3', 'd', 1.5)):
        with pytest.raises(ValueError):
            ingest.check_write_options(*args)


def _source(tmp_path, hw=(240, 304)):
    ev, rec = _records()
    src = tmp_path / 'src'
    src.mkdir()
    dat_events.write_dat(str(src / 'a_td.dat'), rec, *hw)
    return str(src)


def test_the_event_files_get_a_directory_of_their_own(tmp_path):
    """Refused on the host, before a device is touched and before anything is written."""
    from leod_amd.data import ingest
    src = _source(tmp_path)
    dst = str(tmp_path / 'dst')
    link = str(tmp_path / 'link')
    os.symlink(src, link)                                        # real paths are compared
    for events_out in (src, link, os.path.join(src, '..', 'src'), dst, os.path.join(dst, 'a')):
        with pytest.raises(ValueError, match='events_out'):
            ingest.ingest_recording(os.path.join(src, 'a_td.dat'), None, os.path.join(dst, 'a'), 'gen1', write_events='dat', events_out=events_out)
    for events_out in (src, link, dst):
        with pytest.raises(ValueError, match='events_out'):
            ingest.ingest_split(src, dst, 'gen1', unlabelled='ok', write_events='evt3', events_out=events_out)
    with pytest.raises(ValueError, match='needs events_out'):
        ingest.ingest_split(src, dst, 'gen1', unlabelled='ok', write_events='evt3')
    with pytest.raises(ValueError, match='evt3_vectors'):
        ingest.ingest_recording(os.path.join(src, 'a_td.dat'), None, os.path.join(dst, 'a'), 'gen1', write_events='evt2',
                                events_out=str(tmp_path / 'ev'), evt3_vectors=True)
    assert sorted(os.listdir(str(tmp_path))) == ['link', 'src'] and os.listdir(src) == ['a_td.dat']


def test_a_geometry_beyond_2048_does_not_fit_evt(tmp_path, monkeypatch):
    from leod_amd.data import ingest
    from leod_amd.data.utils.types import DatasetType
    monkeypatch.setitem(ingest.SENSOR_HW, DatasetType.GEN1, (240, 4096))
    src = _source(tmp_path, (240, 4096))
    for fmt in ('evt2', 'evt3'):
        with pytest.raises(ValueError, match='11 bits'):
            ingest.ingest_recording(os.path.join(src, 'a_td.dat'), None, str(tmp_path / 'dst' / 'a'), 'gen1', write_events=fmt,
                                    events_out=str(tmp_path / 'ev'))
    assert sorted(os.listdir(str(tmp_path))) == ['src']


def test_the_command_line_refuses_the_same(tmp_path, capsys):
    from leod_amd.data import ingest
    src = _source(tmp_path)
    base = [src, str(tmp_path / 'dst'), '--dataset', 'gen1']
    for extra, word in ((['--write-events', 'evt3'], 'events_out'), (['--write-events', 'evt2', '--events-out', 'ev', '--evt3-vectors'], 'evt3_vectors'),
                        (['--write-events', 'dat', '--events-out', 'ev', '--evt3-vectors'], 'evt3_vectors'),
                        (['--events-out', 'ev'], 'write_events'), (['--write-events', 'evt1', '--events-out', 'ev'], 'invalid choice')):
        with pytest.raises(SystemExit) as e:
            ingest.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err
    assert sorted(os.listdir(str(tmp_path))) == ['src']
