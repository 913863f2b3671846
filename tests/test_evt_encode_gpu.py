"""``ops.encode_evt`` (csrc/k_evtenc.hip) against the normative host encoders ``raw_events.encode_evt2`` / ``encode_evt3`` byte for byte:
one call, any cut into chunks, the round trip through ``ops.decode_evt``, the refusals; then ``--write-events`` through
``ingest_recording`` at Gen1 size.  The random streams span several tiles of the encoder (``ops.evt_encode_query``)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evt_encode_ref as er  # noqa: E402
from test_evt_encode_cpu import FIRST_HIGHS, MODES, PERIODS, host_encode  # noqa: E402
from test_fit_cpu import BOX  # noqa: E402

from leod_amd.data.utils import dat_events, raw_events  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FMT = {2: 'evt2', 3: 'evt3'}
N_RANDOM = 20_000


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as _ops
    return _ops


def _err():
    from leod_amd._lib import LeodHipError
    return LeodHipError


def _dev(rec):
    return torch.from_numpy(np.ascontiguousarray(rec, dtype='<u4').view(np.uint8).reshape(-1).copy()).to(DEV)


def _encode(ops, rec, fmt, cuts=(), **kw):
    """The words of ``rec`` cut at ``cuts`` (ascending positions; the last chunk is final) -> (words, state, most events held)."""
    edges = [0] + list(cuts) + [len(rec)]
    state, parts, held = None, [], 0
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        final = i == len(edges) - 2
        words, state = ops.encode_evt(_dev(rec[a:b]), FMT[fmt], state, final=final, **kw)
        assert words.dtype == torch.uint8 and words.dim() == 1 and state.dtype == torch.int64 and state.numel() == 32
        parts.append(words.cpu().numpy())
        if not final:
            held = max(held, ops.evt_encode_counters(state)['held'])
    return np.concatenate(parts).view('<u4' if fmt == 2 else '<u2'), state, held


@pytest.fixture(scope='module')
def streams():
    """name -> (events, records): the hand cases and two random streams of several tiles; read-only, shared by the tests."""
    out = dict(er.hand_cases())
    for seed in (1, 2):
        out[f'random_{seed}'] = er.random_stream(np.random.RandomState(seed), N_RANDOM)
    out = {k: (ev, dat_events.encode(*ev)) for k, ev in out.items()}
    for ev, rec in out.values():
        for a in ev + (rec,):
            a.setflags(write=False)
    return out


_WANT = {}


def _want(streams, name, fmt, vectors, period, first):
    key = (name, fmt, vectors, period, first)
    if key not in _WANT:
        _WANT[key] = host_encode(streams[name][0], fmt, vectors, period, first)
    return _WANT[key]


def test_the_streams_are_what_they_say(ops, streams):
    tile, ws, bound = ops.evt_encode_query(N_RANDOM, 'evt3')
    assert tile >= 64 and N_RANDOM >= 4 * tile and ws > 0
    ev, rec = streams['random_1']
    t = ev[0]
    assert len(rec) >= N_RANDOM and (np.diff(t >> 12) > 4096).any() and t.max() >= 1 << 24 and t.max() < 1 << 32
    words = _want(streams, 'random_1', 3, True, 64, 0)
    assert ((words >> 12) == 0x4).sum() > 500 and ((words >> 12) == 0x5).sum() > 500 and len(words) <= bound


@pytest.mark.parametrize('first', FIRST_HIGHS)
@pytest.mark.parametrize('period', PERIODS)
@pytest.mark.parametrize('fmt,vectors', MODES)
def test_one_final_call_writes_the_words_of_the_host_encoder(ops, streams, fmt, vectors, period, first):
    kw = dict(vectors=vectors, high_period=period, first_time_high=first)
    for name, (ev, rec) in streams.items():
        got, state, _ = _encode(ops, rec, fmt, **kw)
        want = _want(streams, name, fmt, vectors, period, first)
        assert got.dtype == want.dtype and len(got) == len(want) and np.array_equal(got, want), (name, np.flatnonzero(got != want)[:4])
        c = ops.evt_encode_counters(state)
        groups = int(((want >> 12) == 0x2).sum() + ((want >> 12) == 0x3).sum()) if fmt == 3 else len(rec)
        assert c == dict(events=len(rec), words=len(want), groups=groups, held=0,
                         vector_groups=int(((want >> 12) == 0x3).sum()) if fmt == 3 else 0), name


def _kinds(ev, cuts):
    """Which kinds of cut occur: inside a run, inside a group, directly after a pause, an empty chunk, a one-event chunk."""
    t, x, y, p = ev
    n = len(t)
    same = np.zeros(n, dtype=bool)
    same[1:] = (t[1:] == t[:-1]) & (y[1:] == y[:-1]) & (p[1:] == p[:-1]) & (x[1:] > x[:-1])
    words = raw_events.encode_evt3(t, x, y, p, vectors=True)
    sizes = []                                                   # of the groups, from the host encoder's words
    for w in words.tolist():
        if w >> 12 == 0x2:
            sizes.append(1)
        elif w >> 12 in (0x4, 0x5):
            sizes.append(bin(w & 4095).count('1'))
    pos = np.cumsum([0] + sizes)
    assert pos[-1] == n
    start = np.zeros(n + 1, dtype=bool)
    start[pos] = True
    after_pause = np.zeros(n, dtype=bool)
    after_pause[1:] = (t[1:] >> 12) - (t[:-1] >> 12) > 1024
    edges = [0] + list(cuts) + [n]
    inner = [c for c in cuts if 0 < c < n]
    return dict(run=any(same[c] for c in inner), group=any(not start[c] for c in inner), pause=any(after_pause[c] for c in inner),
                empty=any(a == b for a, b in zip(edges[:-1], edges[1:])), one=any(b - a == 1 for a, b in zip(edges[:-1], edges[1:])))


@pytest.mark.parametrize('fmt,vectors', MODES)
def test_the_words_do_not_depend_on_the_cut_into_chunks(ops, streams, fmt, vectors):
    rng = np.random.RandomState(5)
    seen = dict(run=False, group=False, pause=False, empty=False, one=False)
    # every single cut of a short stream: a run of 30 columns, a pause, a change of polarity
    ev, _ = streams['row']
    short = tuple(np.concatenate([a[:30], b]) for a, b in zip(ev, er._cols([(7000 + 1025 * er.U, 3, 100, 1), (7000 + 1025 * er.U, 4, 100, 1),
                                                                             (7000 + 1025 * er.U, 5, 100, 0), (7001 + 1025 * er.U, 5, 100, 0)])))
    rec = dat_events.encode(*short)
    want = host_encode(short, fmt, vectors, 3, 4095)
    for c in range(len(rec) + 1):
        got, state, held = _encode(ops, rec, fmt, [c], vectors=vectors, high_period=3, first_time_high=4095)
        assert np.array_equal(got, want) and held <= 12 and ops.evt_encode_counters(state)['held'] == 0, c
        assert held == 0 or vectors
        for k, v in _kinds(short, [c]).items():
            seen[k] |= v
    # random cuts of the random streams, with empty and one-event chunks among them
    for name, period, first in (('random_1', 64, 0), ('random_2', 3, 4095), ('row', 1, 0), ('pause_5000', 1, 4095)):
        ev, rec = streams[name]
        want = _want(streams, name, fmt, vectors, period, first)
        for _ in range(3):
            cuts = np.sort(rng.randint(0, len(rec) + 1, 12))
            cuts = np.sort(np.concatenate([cuts, cuts[:3], np.minimum(cuts[3:6] + 1, len(rec))])).tolist()
            got, state, held = _encode(ops, rec, fmt, cuts, vectors=vectors, high_period=period, first_time_high=first)
            assert len(got) == len(want) and np.array_equal(got, want), (name, cuts)
            assert held <= 12 and ops.evt_encode_counters(state)['held'] == 0
            for k, v in _kinds(ev, cuts).items():
                seen[k] |= v
    assert all(seen.values()), seen


@pytest.mark.parametrize('fmt,vectors', MODES)
def test_the_decoder_gives_the_records_back(ops, streams, fmt, vectors):
    for name, first in (('random_1', 0), ('random_2', 4095), ('late', 4095), ('zero', 0), ('row', 0), ('none', 0)):
        ev, rec = streams[name]
        words, _ = ops.encode_evt(_dev(rec), FMT[fmt], final=True, vectors=vectors, first_time_high=first)
        back, dstate = ops.decode_evt(words, FMT[fmt])
        assert np.array_equal(back.cpu().numpy().view('<u4').reshape(-1, 2), rec), name
        c = ops.evt_state_counters(dstate)
        assert (c['events'], c['early_events'], c['unknown_words'], c['overflow'], c['ignored_words']) == (len(rec), 0, 0, 0, 0), name


def test_a_column_or_a_row_beyond_11_bits_is_refused_with_its_position(ops, streams):
    ev, rec = streams['random_1']
    for fmt, vectors in MODES:
        for col, v in ((1, 2048), (1, 16383), (2, 2048)):
            bad = [a[:5000].copy() for a in ev]
            bad[col][3000] = v
            bad[col][4100] = v
            with pytest.raises(_err(), match=r'event 3000 of the chunk \(event 3000 of the recording\).*2 such records'):
                ops.encode_evt(_dev(dat_events.encode(*bad)), FMT[fmt], final=True, vectors=vectors)
            words, state = ops.encode_evt(_dev(rec[:1000]), FMT[fmt], vectors=vectors)
            with pytest.raises(_err(), match=r'event 2000 of the chunk \(event 3000 of the recording\)'):
                ops.encode_evt(_dev(dat_events.encode(*bad)[1000:]), FMT[fmt], state, vectors=vectors)
    ok = [a[:100].copy() for a in ev]
    ok[1][50], ok[2][60] = 2047, 2047                            # the last column and row an EVT word holds
    got, _, _ = _encode(ops, dat_events.encode(*ok), 3, vectors=True)
    assert np.array_equal(got, raw_events.encode_evt3(*ok, vectors=True))


def test_a_decreasing_time_is_refused_and_the_given_state_is_not_touched(ops, streams):
    ev, rec = streams['random_1']
    for fmt, vectors in MODES:
        bad = rec[:6000].copy()
        bad[4000, 0] = bad[3999, 0] - 1
        with pytest.raises(ops.EventOrderError) as e:
            ops.encode_evt(_dev(bad), FMT[fmt], vectors=vectors)
        assert (e.value.position, e.value.t_before, e.value.t_at) == (4000, int(bad[3999, 0]), int(bad[4000, 0]))
        # across a chunk boundary: position 0, against the last time of the chunk before (held back or not)
        words, state = ops.encode_evt(_dev(bad[:4000]), FMT[fmt], vectors=vectors)
        kept = state.clone()
        with pytest.raises(ops.EventOrderError) as e:
            ops.encode_evt(_dev(bad[4000:]), FMT[fmt], state, vectors=vectors)
        assert (e.value.position, e.value.t_before, e.value.t_at) == (0, int(bad[3999, 0]), int(bad[4000, 0]))
        assert torch.equal(state, kept)
        more, state2 = ops.encode_evt(_dev(rec[4000:6000]), FMT[fmt], state, final=True, vectors=vectors)
        assert torch.equal(state, kept) and state2.data_ptr() != state.data_ptr()
        want = host_encode(tuple(a[:6000] for a in ev), fmt, vectors, 64, 0)
        assert np.array_equal(np.concatenate([words.cpu().numpy(), more.cpu().numpy()]).view(want.dtype), want)


def test_nothing_is_written_behind_the_words_and_a_small_buffer_is_refused(ops, streams):
    ev, rec = streams['random_2']
    for fmt, vectors in MODES:
        want = _want(streams, 'random_2', fmt, vectors, 64, 0)
        nbytes = want.nbytes
        out = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        words, _ = ops.encode_evt(_dev(rec), FMT[fmt], final=True, vectors=vectors, out=out)
        assert words.data_ptr() == out.data_ptr() and np.array_equal(words.cpu().numpy().view(want.dtype), want)
        assert bool((out[nbytes:] == 0xA5).all())
        small = torch.full((nbytes - want.itemsize + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        with pytest.raises(_err(), match='do not hold'):
            ops.encode_evt(_dev(rec), FMT[fmt], final=True, vectors=vectors, out=small[:nbytes - want.itemsize])
        assert bool((small == 0xA5).all())


def test_argument_checks(ops, streams):
    rec = _dev(streams['one'][1])
    E = _err()
    for kw in (dict(fmt='evt2', vectors=True), dict(fmt='evt4'), dict(fmt='evt3', high_period=0), dict(fmt='evt3', high_period=1.5),
               dict(fmt='evt3', first_time_high=4096), dict(fmt='evt3', first_time_high=-1), dict(fmt='evt2', first_time_high=1 << 27),
               dict(fmt='evt3', state=torch.zeros(16, dtype=torch.int64, device=DEV)), dict(fmt='evt3', final=1.5),
               dict(fmt='evt3', state=torch.zeros(32, dtype=torch.int32, device=DEV))):
        with pytest.raises(E):
            ops.encode_evt(rec, **kw)
    with pytest.raises(E, match='no CPU fallback'):
        ops.encode_evt(rec.cpu(), 'evt3')
    with pytest.raises(E, match='whole number'):
        ops.encode_evt(rec[:7], 'evt3')
    with pytest.raises(E):
        ops.evt_encode_query(-1)
    assert ops.evt_encode_query(0, 'evt2')[2] == 1 and ops.evt_encode_query(10, 'evt2')[2] == 21


# ---- ingestion at Gen1 size ---------------------------------------------------------------------------------------------------------------
D, BINS = 50_000, 10
FILTERS = dict(trail_us=2000, denoise_us=20_000)


def _clustered(seed, n, hw, x0, y0, w, h, windows=4):
    """``windows`` windows of events dense enough on a w x h patch for the filters to keep a good part; the last event at windows * D."""
    rng = np.random.RandomState(seed)
    t = np.sort(rng.randint(1, windows * D, n))
    x, y, p = x0 + rng.randint(0, w, n), y0 + rng.randint(0, h, n), rng.randint(0, 2, n)
    far = rng.rand(n) < 0.05
    x[far], y[far] = rng.randint(0, hw[1], int(far.sum())), rng.randint(0, hw[0], int(far.sum()))
    t, x, y, p = (np.append(a, v) for a, v in ((t, windows * D), (x, x0), (y, y0), (p, 1)))
    return tuple(a.astype(np.int64) for a in (t, x, y, p))


def _boxes(scale=1):
    rows = [(40_000, 100, 50, 30, 20, 0), (40_000, 10, 10, 20, 12, 1), (120_000, 110, 60, 10, 6, 0), (190_000, 120, 55, 13, 9, 1)]
    b = np.zeros((len(rows),), dtype=BOX)
    for i, (t, x, y, w, h, c) in enumerate(rows):
        b[i] = (t, x * scale, y * scale, w * scale, h * scale, c, 1.0, i)
    return b


@pytest.fixture(scope='module')
def gen1(tmp_path_factory):
    """A Gen1-size .dat recording with boxes, its trees with and without the filters, and an upside-down 640 x 480 .raw one."""
    from leod_amd.data import ingest
    root = tmp_path_factory.mktemp('evtenc')
    src = root / 'src'
    src.mkdir()
    ev = _clustered(7, 30_000, (240, 304), 100, 50, 40, 30)
    dat_events.write_dat(str(src / 'a_td.dat'), dat_events.encode(*ev), 240, 304)
    np.save(str(src / 'a_bbox.npy'), _boxes())
    vga = root / 'vga'
    vga.mkdir()
    ev_vga = _clustered(8, 30_000, (480, 640), 200, 100, 80, 60)
    raw_events.write_raw(str(vga / 'v.raw'), raw_events.encode_evt3(*ev_vga, first_time_high=5, vectors=True), 'evt3', height=480, width=640)
    np.save(str(vga / 'v_bbox.npy'), _boxes(2))
    plain, filtered = str(root / 'plain' / 'a'), str(root / 'filtered' / 'a')
    plain_report = None
    if torch.cuda.is_available():
        plain_report = ingest.ingest_recording(str(src / 'a_td.dat'), str(src / 'a_bbox.npy'), plain, 'gen1')
        ingest.ingest_recording(str(src / 'a_td.dat'), str(src / 'a_bbox.npy'), filtered, 'gen1', **FILTERS)
    return dict(root=root, src=str(src), vga=str(vga), ev=ev, plain=plain, filtered=filtered, plain_report=plain_report)


def _tree_files(seq_dir):
    out = {}
    for dirpath, _, files in os.walk(seq_dir):
        for f in files:
            out[os.path.relpath(os.path.join(dirpath, f), seq_dir)] = os.path.join(dirpath, f)
    return out


def _same_trees(got_dir, want_dir, what):
    got, want = _tree_files(got_dir), _tree_files(want_dir)
    assert sorted(got) == sorted(want), what
    for rel in want:
        if rel.endswith('.npz'):
            a, b = np.load(got[rel]), np.load(want[rel])
            assert sorted(a.files) == sorted(b.files)
            for k in b.files:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, rel, k)
        else:
            assert open(got[rel], 'rb').read() == open(want[rel], 'rb').read(), (what, rel)


def _frames_and_labels(seq_dir):
    from leod_amd.data.utils import misc
    lab = np.load(os.path.join(seq_dir, 'labels_v2', 'labels.npz'))
    repr_idx = [f for rel, f in _tree_files(seq_dir).items() if rel.endswith('objframe_idx_2_repr_idx.npy')]
    return np.load(misc.get_ev_raw_fn(seq_dir, 'gen1')), lab['labels'], lab['objframe_idx_2_label_idx'], np.load(repr_idx[0])


def _is_the_head_of(ingest, again_dir, tree_dir, what):
    """The N' <= N frames of ``again_dir`` are the first N' of ``tree_dir``, whose other frames are all zero; the labels of the frames
    below N' are equal."""
    fa, la, ia, ra = _frames_and_labels(again_dir)
    ft, lt, it, rt = _frames_and_labels(tree_dir)
    n = len(fa)
    assert 1 <= n <= len(ft) and np.array_equal(fa, ft[:n]) and not ft[n:].any() and fa.any(), what
    below = ingest.label_frame(lt['t'], D) < n
    assert np.array_equal(la, lt[below]) and np.array_equal(ra, rt[rt < n]) and np.array_equal(ia, it[:len(ia)]) and len(la) > 0, what
    return n


def _file_events(fn):
    """(t, x, y, p) of a written event file, decoded on the host."""
    if fn.endswith('.dat'):
        return dat_events.decode(dat_events.open_records(fn)[1])
    hdr, payload = raw_events.open_words(fn)
    t, x, y, p, c = raw_events.decode(payload, hdr.encoding)
    assert c['early_events'] == c['unknown_words'] == c['ignored_words'] == c['overflow'] == 0
    return t, x, y, p


@pytest.mark.parametrize('fmt,vectors', [('evt3', True), ('evt3', False), ('evt2', False), ('dat', False)])
def test_the_filtered_stream_is_written_and_ingests_to_the_same_frames(ops, tmp_path, gen1, fmt, vectors):
    from leod_amd.data import ingest
    out, again, evd = str(tmp_path / 'out' / 'a'), str(tmp_path / 'again'), str(tmp_path / 'events')
    rep = ingest.ingest_recording(os.path.join(gen1['src'], 'a_td.dat'), os.path.join(gen1['src'], 'a_bbox.npy'), out, 'gen1',
                                  raw_chunk_bytes=64 << 10, write_events=fmt, events_out=evd, evt3_vectors=vectors, **FILTERS)
    _same_trees(out, gen1['filtered'], 'the tree with the event file against the tree without')
    name = 'a_td.dat' if fmt == 'dat' else 'a.raw'
    assert sorted(os.listdir(evd)) == sorted([name, 'a_bbox.npy']) and rep['events_file'] == os.path.join(evd, name)
    assert 0 < rep['written_events'] == rep['kept_events'] < rep['events'] and rep['written_bytes'] == os.path.getsize(rep['events_file'])
    assert ('written_words' in rep) == (fmt != 'dat')
    boxes = np.load(os.path.join(evd, 'a_bbox.npy'))
    assert boxes.dtype == BOX and np.array_equal(boxes, _boxes())
    t, x, y, p = _file_events(rep['events_file'])
    assert len(t) == rep['written_events'] and (np.diff(t) >= 0).all()
    if fmt == 'dat':
        hdr = dat_events.parse_header(rep['events_file'])
    else:
        hdr = raw_events.parse_header(rep['events_file'])
        assert hdr.encoding == fmt and rep['written_words'] * raw_events.WORD_BYTES[fmt] == os.path.getsize(rep['events_file']) - hdr.data_offset
        want = host_encode((t, x, y, p), int(fmt[-1]), vectors, 64, 0)       # the file's words are the host encoder's of its own events
        assert np.array_equal(np.asarray(raw_events.open_words(rep['events_file'])[1]).view(want.dtype), want)
    assert (hdr.height, hdr.width) == (240, 304)
    reps = ingest.ingest_split(evd, again, 'gen1')               # the directory written is a source directory
    assert len(reps) == 1 and reps[0]['events'] == rep['written_events']
    n = _is_the_head_of(ingest, os.path.join(again, 'a'), out, fmt)
    assert n == dat_events.num_windows(int(t[-1]), D)


@pytest.mark.parametrize('reduce', ['pick', 'fire'])
def test_an_upside_down_vga_recording_is_written_upright_at_gen1_size(ops, tmp_path, gen1, reduce):
    from leod_amd.data import ingest
    out, again, evd = str(tmp_path / 'out' / 'v'), str(tmp_path / 'again' / 'v'), str(tmp_path / 'events')
    fit = dict(scale='auto', orient=180, reduce=reduce)
    rep = ingest.ingest_recording(os.path.join(gen1['vga'], 'v.raw'), os.path.join(gen1['vga'], 'v_bbox.npy'), out, 'gen1', fit=fit,
                                  raw_chunk_bytes=64 << 10, write_events='evt3', events_out=evd, evt3_vectors=True)
    hdr = raw_events.parse_header(rep['events_file'])
    assert (hdr.encoding, hdr.height, hdr.width) == ('evt3', 240, 304) and 0 < rep['written_events'] == rep['kept_events']
    t, x, y, p = _file_events(rep['events_file'])
    assert x.max() < 304 and y.max() < 240
    rep2 = ingest.ingest_recording(rep['events_file'], os.path.join(evd, 'v_bbox.npy'), again, 'gen1')      # no fit
    assert rep2['events'] == rep['written_events'] and rep2['dropped_events'] == 0
    _is_the_head_of(ingest, again, out, reduce)


def test_an_unfiltered_dat_recording_is_copied_and_the_tree_is_that_of_the_unfiltered_route(ops, tmp_path, gen1):
    from leod_amd.data import ingest
    out, evd = str(tmp_path / 'out' / 'a'), str(tmp_path / 'events')
    rep = ingest.ingest_recording(os.path.join(gen1['src'], 'a_td.dat'), os.path.join(gen1['src'], 'a_bbox.npy'), out, 'gen1',
                                  raw_chunk_bytes=64 << 10, write_events='dat', events_out=evd)
    _same_trees(out, gen1['plain'], 'the streaming route with an event file against voxelize_recording')
    assert open(rep['events_file'], 'rb').read() == open(os.path.join(gen1['src'], 'a_td.dat'), 'rb').read()
    assert rep['written_events'] == rep['events'] == len(gen1['ev'][0]) and rep['frames'] == 4
    new = ('events_file', 'written_events', 'written_bytes')
    assert {k: v for k, v in rep.items() if k not in new + ('recording',)} == {k: v for k, v in gen1['plain_report'].items() if k != 'recording'}
    assert sorted(set(rep) - set(gen1['plain_report'])) == sorted(new)


@pytest.mark.parametrize('fmt', ['dat', 'evt3'])
def test_a_failure_in_the_middle_leaves_no_file(ops, tmp_path, gen1, fmt):
    from leod_amd.data import ingest
    t, x, y, p = (a.copy() for a in gen1['ev'])
    t[20_000] = t[19_999] - 1                                    # in the third of four chunks
    src = tmp_path / 'src'
    src.mkdir()
    dat_events.write_dat(str(src / 'a_td.dat'), np.stack([t, x | (y << 14) | (p << 28)], axis=1).astype('<u4'), 240, 304)
    evd = str(tmp_path / 'events')
    with pytest.raises(ValueError, match='timestamps decrease'):
        ingest.ingest_recording(str(src / 'a_td.dat'), os.path.join(gen1['src'], 'a_bbox.npy'), str(tmp_path / 'out' / 'a'), 'gen1',
                                raw_chunk_bytes=64 << 10, write_events=fmt, events_out=evd, evt3_vectors=fmt == 'evt3')
    assert os.listdir(evd) == []
    assert not [f for f in _tree_files(str(tmp_path / 'out')) if f.endswith('.tmp') or 'event_representations.npy' in f]
