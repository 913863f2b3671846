"""``ops.fit_events`` (csrc/k_fit.hip) against the tests' sequential restatement (tests/fit_ref.py): kept records byte for byte, the whole
state block and the counters; the anchor to the voxeliser's ``ds2``; then recordings of a foreign sensor size through ``ingest_recording``
with a fit on.  The stream sizes follow the kernel's own constants (``ops.fit_query``): a tile of 256 records per workgroup, 8 tiles per
workgroup of the sort, a digit of 8 key bits per pass of the sort."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref  # noqa: E402
import fit_ref as fr  # noqa: E402
from fit_ref import records as R  # noqa: E402
from test_fit_cpu import BOX, HAND, hand_case, random_case  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
D = 50_000
SORT_TILES = 8                                                   # tiles of records per workgroup of the sort (csrc/pixel_sort.hpp)
SRC, DST = (12, 20), (5, 8)
GEO = dict(scale=2, offset=(-1, -1))                             # what auto / center give for SRC onto DST
REDUCE_KW = dict(pick=dict(reduce='pick'), sum=dict(reduce='sum'), fire=dict(reduce='fire', threshold=3))


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


def _fit(ops, rec, src, dst, state=None, **kw):
    out, state = ops.fit_events(_dev(rec), src, dst, state=state, **kw)
    assert out.dtype == torch.uint8 and out.dim() == 2 and out.shape[1] == 8 and state.dtype == torch.int64
    return out.cpu().numpy().view('<u4').reshape(-1, 2), state


def _check(ops, rec, src, dst, what='', ws_bytes=None, **kw):
    """One call on the device against the restatement: kept records, the whole state block, the counters."""
    ref = fr.Fit(src, dst, **kw)
    want = ref.feed(rec)
    got, state = _fit(ops, rec, src, dst, ws_bytes=ws_bytes, **kw)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, f'kept record {bad[0]} of {len(want)}', got[bad[0]].tolist(), want[bad[0]].tolist())
    assert state.cpu().tolist() == ref.state(), what
    assert ops.fit_counters(state) == ref.counters(), what
    return got, ref


@pytest.mark.parametrize('case', HAND, ids=[c[0] for c in HAND])
def test_hand_written_streams(ops, case):
    rec, src, dst, kw, want, counts = hand_case(case)
    got, ref = _check(ops, rec, src, dst, what=case[0], **kw)
    assert np.array_equal(got, want) and ref.counters() == counts


@pytest.mark.parametrize('reduce', fr.REDUCES)
def test_bits_28_to_31_and_the_time_are_kept(ops, reduce):
    rec = R([7, 2 ** 32 - 1], [3, 2], [1, 0], [1, 0])
    rec[:, 1] |= np.array([0xE0000000, 0xA0000000], dtype='<u4')
    got, _ = _check(ops, rec, (2, 4), (2, 4), reduce=reduce, threshold=1 if reduce == 'fire' else None, mirror=True)
    assert got.tolist() == [[7, 0xF0000000 | (1 << 14) | 0], [2 ** 32 - 1, 0xA0000000 | 1]]


@pytest.mark.parametrize('reduce', fr.REDUCES)
def test_no_events(ops, reduce):
    empty = np.zeros((0, 2), dtype='<u4')
    kw = dict(REDUCE_KW[reduce], **GEO)
    got, state = _fit(ops, empty, SRC, DST, **kw)
    assert got.shape == (0, 2) and state.cpu().tolist() == fr.Fit(SRC, DST, **kw).state() == [0] * 6 + [-1, 0] + [0] * 40
    _, s1 = _fit(ops, random_case(0, 50), SRC, DST, **kw)
    got, s2 = _fit(ops, empty, SRC, DST, state=s1, **kw)
    assert got.shape == (0, 2) and torch.equal(s1, s2) and s2.data_ptr() != s1.data_ptr()


@pytest.mark.parametrize('reduce', fr.REDUCES)
def test_random_streams_at_the_tile_and_sort_tile_edges(ops, reduce):
    tile, per_pass, digit, _, _ = ops.fit_query(0, DST, reduce)
    assert (tile, per_pass, digit) == (256, 256, 8), 'the sizes below were chosen for these constants'
    for k, n in enumerate((1, tile - 1, tile, tile + 1, SORT_TILES * tile - 1, SORT_TILES * tile, SORT_TILES * tile + 1)):
        _, ref = _check(ops, random_case(k, n), SRC, DST, what=f'n = {n}', **REDUCE_KW[reduce], **GEO)
        c = ref.counters()
        if n > 1000:                                             # not vacuous
            assert min(c['kept'], c['outside'], c['cropped']) > 0 and (c['skipped'] > 0) == (reduce == 'pick') and \
                (c['merged'] > 0) == (reduce == 'fire'), (n, c)


@pytest.mark.parametrize('orient', fr.ORIENTS)
@pytest.mark.parametrize('mirror', [False, True])
def test_every_orientation_with_scale_offset_and_fire(ops, orient, mirror):
    rec = random_case(30 + orient, 1500, src=(13, 21))
    for reduce in fr.REDUCES:
        _, ref = _check(ops, rec, (13, 21), (6, 6), orient=orient, mirror=mirror, scale=2, offset=(-2, 1), **REDUCE_KW[reduce])
        assert ref.counters()['kept'] > 0 and ref.counters()['cropped'] > 0
    _check(ops, rec, (13, 21), (6, 6), orient=orient, mirror=mirror, scale=3, offset=(1, 1), reduce='pick')       # an odd scale: centre 1


@pytest.mark.parametrize('hw', [(1, 1), (1, 255), (1, 256), (1, 257), (256, 256), (257, 256), (1, 16384)])
def test_frames_on_each_side_of_a_sort_digit_boundary(ops, hw):
    """8-bit digits: 256 destination pixels take one pass of the sort, 257 two, 256 * 256 two, 257 * 256 three; a single pixel takes none.
    The source is the frame's size, so (1, 16384) runs source (1, 16384) onto (1, 16384)."""
    h, w = hw
    rng = np.random.RandomState(h * 1000 + w)
    n = 1500
    t = np.sort(rng.randint(0, 40 * n, n))
    # the top pixels of the frame occur, so the highest key bit is used; a few events lie beyond the sensor
    x, y = rng.randint(max(w - 300, 0), min(w + 2, 16384), n), rng.randint(max(h - 3, 0), h + 1, n)
    _, ref = _check(ops, R(t, x, y, rng.randint(0, 2, n)), hw, hw, what=str(hw), reduce='fire', threshold=2)
    c = ref.counters()
    assert c['kept'] > 0 and c['merged'] > 0 and (c['outside'] > 0 or hw == (1, 16384))
    _check(ops, R(t, x, y, rng.randint(0, 2, n)), hw, hw, what=str(hw), reduce='sum', mirror=True)


def test_all_events_on_one_destination_pixel(ops):
    rng = np.random.RandomState(9)
    n = 6000
    t = np.cumsum(rng.randint(0, 9, n))
    rec = R(t, 4 + rng.randint(0, 2, n), 2 + rng.randint(0, 2, n), (rng.rand(n) < 0.7).astype(np.int64))     # the cell of frame pixel (1, 0)
    _, ref = _check(ops, rec, SRC, DST, reduce='fire', **GEO)
    assert ref.counters()['kept'] > 300 and ref.counters()['merged'] > 3000 and ref.counters()['cropped'] == 0
    _check(ops, rec, SRC, DST, reduce='fire', ws_bytes=ops.fit_query(1024, DST)[3], **GEO)       # the run crosses the pieces


def test_forced_pieces_through_a_small_workspace(ops):
    tile = ops.fit_query(0, DST)[0]
    rec = random_case(11, 9 * tile + 17)
    one_tile = ops.fit_query(1, DST)[3]
    assert ops.fit_query(tile, DST)[3] == one_tile < ops.fit_query(tile + 1, DST)[3] < 2 * one_tile
    assert ops.fit_query(tile, DST, 'pick')[3] == ops.fit_query(tile, DST, 'sum')[3] == 0        # they sort nothing
    whole = ops.fit_query(len(rec), DST)[3]
    # pieces of 1, 1, 2, 8 (one whole workgroup of the sort) and 9 tiles, and the chunk in one piece
    for ws in (one_tile, ops.fit_query(2 * tile, DST)[3] - 1, ops.fit_query(2 * tile, DST)[3], ops.fit_query(SORT_TILES * tile, DST)[3],
               whole - 1, whole):
        _check(ops, rec, SRC, DST, what=f'ws {ws}', ws_bytes=ws, reduce='fire', threshold=3, **GEO)
    with pytest.raises(_err(), match='ws_bytes'):
        ops.fit_events(_dev(rec), SRC, DST, reduce='fire', ws_bytes=one_tile - 1, **GEO)


def test_chunk_carry_at_every_split(ops):
    rec = random_case(12, 60, src=(4, 6), outside=0.1)
    kw = dict(scale=2, reduce='fire', threshold=2)
    whole, ref = _check(ops, rec, (4, 6), (2, 3), **kw)
    assert ref.counters()['kept'] > 3 and ref.counters()['merged'] > 3 and ref.counters()['outside'] > 0 and any(ref.state()[8:])
    for split in range(len(rec) + 1):
        a, s1 = _fit(ops, rec[:split], (4, 6), (2, 3), **kw)
        keep1 = s1.clone()
        b, s2 = _fit(ops, rec[split:], (4, 6), (2, 3), state=s1, **kw)
        assert np.array_equal(np.concatenate([a, b]), whole), split
        assert s2.cpu().tolist() == ref.state(), split
        assert torch.equal(s1, keep1), f'split {split}: the given state was modified'


@pytest.mark.parametrize('reduce', fr.REDUCES)
def test_two_runs_are_byte_identical(ops, reduce):
    d = _dev(random_case(13, 30_000))
    kw = dict(REDUCE_KW[reduce], **GEO)
    a, sa = ops.fit_events(d, SRC, DST, **kw)
    b, sb = ops.fit_events(d, SRC, DST, **kw)
    assert torch.equal(a, b) and torch.equal(sa, sb) and a.shape[0] > 1000
    if reduce == 'fire':
        c, sc = ops.fit_events(d, SRC, DST, ws_bytes=ops.fit_query(2048, DST)[3], **kw)
        assert torch.equal(a, c) and torch.equal(sa, sc)


@pytest.mark.parametrize('reduce', fr.REDUCES)
def test_nothing_behind_the_kept_records_and_a_small_buffer_is_refused(ops, reduce):
    rec = random_case(14, 900)
    kw = dict(REDUCE_KW[reduce], **GEO)
    want = fr.Fit(SRC, DST, **kw).feed(rec)
    m = len(want)
    buf = torch.full(((m + 9) * 8,), 0xA5, dtype=torch.uint8, device=DEV)
    out, _ = ops.fit_events(_dev(rec), SRC, DST, out=buf, **kw)
    assert out.shape == (m, 8) and out.data_ptr() == buf.data_ptr() and m > 20
    assert np.array_equal(out.cpu().numpy().view('<u4').reshape(-1, 2), want)
    assert bool((buf[m * 8:] == 0xA5).all())
    exact = torch.empty((m * 8,), dtype=torch.uint8, device=DEV)
    assert ops.fit_events(_dev(rec), SRC, DST, out=exact, **kw)[0].shape == (m, 8)
    with pytest.raises(_err(), match='do not hold'):
        ops.fit_events(_dev(rec), SRC, DST, out=torch.empty((m * 8 - 8,), dtype=torch.uint8, device=DEV), **kw)


@pytest.mark.parametrize('reduce', ['pick', 'fire'])
def test_a_decreasing_time_is_refused_with_its_position(ops, reduce):
    tile = ops.fit_query(0, DST)[0]
    rec = random_case(15, 3 * tile)
    rec[:, 0] += 1                                               # no time is 0
    kw = dict(REDUCE_KW[reduce], **GEO)
    small = dict(ws_bytes=ops.fit_query(tile, DST)[3]) if reduce == 'fire' else {}
    for pos in (1, tile, 2 * tile + 7, 3 * tile - 1):            # every piece of one tile, their first and last record
        bad = rec.copy()
        bad[pos:, 0] = np.maximum(bad[pos:, 0], bad[pos - 1, 0] + 5)      # still sorted ...
        bad[pos, 0] = bad[pos - 1, 0] - 1                                   # ... but for this one
        with pytest.raises(ops.EventOrderError) as e:
            ops.fit_events(_dev(bad), SRC, DST, **kw, **small)
        assert (e.value.position, e.value.t_before, e.value.t_at) == (pos, int(bad[pos - 1, 0]), int(bad[pos, 0]))
        with pytest.raises(fr.OrderError) as r:
            fr.Fit(SRC, DST, **kw).feed(bad)
        assert (r.value.position, r.value.t_before, r.value.t_at) == (e.value.position, e.value.t_before, e.value.t_at)
    # across a chunk boundary: position 0, against the last time of the chunk before -- also where that event was outside the sensor
    _, s1 = _fit(ops, R([10, 500], [1, 99], [1, 1]), SRC, DST, **kw)
    with pytest.raises(ops.EventOrderError) as e:
        ops.fit_events(_dev(R([499, 600], [1, 1], [1, 1])), SRC, DST, state=s1, **kw)
    assert (e.value.position, e.value.t_before, e.value.t_at) == (0, 500, 499)
    _, s2 = _fit(ops, R([500, 600], [1, 1], [1, 1]), SRC, DST, state=s1, **kw)                  # an equal time is in order
    assert ops.fit_counters(s2)['seen'] == 4


def test_argument_checks(ops):
    rec = _dev(R([1, 2], [0, 1], [0, 0]))
    E = _err()
    for kw in (dict(orient=45), dict(orient=360), dict(orient=True), dict(mirror=1), dict(scale=0), dict(scale=65), dict(scale=2.0),
               dict(scale=True), dict(offset=(0,)), dict(offset=(16385, 0)), dict(offset=(0, -16385)), dict(offset=(0.5, 0)), dict(offset='0,0'),
               dict(reduce='max'), dict(reduce=2), dict(threshold=2), dict(reduce='sum', threshold=2), dict(reduce='fire', threshold=0),
               dict(reduce='fire', threshold=32768), dict(reduce='fire', threshold=1.0), dict(reduce='fire', ws_bytes=0)):
        with pytest.raises(E):
            ops.fit_events(rec, SRC, DST, **kw)
    for src, dst in (((0, 20), DST), ((12, 16385), DST), (SRC, (5, 0)), (SRC, (16385, 8)), ((12.0, 20), DST), (SRC, (5, True)), (12, DST),
                     (SRC, (5, 8, 1))):
        with pytest.raises(E):
            ops.fit_events(rec, src, dst)
    with pytest.raises(E):
        ops.fit_events(rec[:9], SRC, DST)                                       # no whole number of records
    with pytest.raises(E):
        ops.fit_events(rec.cpu(), SRC, DST)
    with pytest.raises(E):
        ops.fit_events(rec, SRC, DST, state=torch.zeros((8 + 12 * 20,), dtype=torch.int64, device=DEV))      # the source's size, not the frame's
    with pytest.raises(E):
        ops.fit_events(rec, SRC, DST, state=torch.zeros((8 + 40,), dtype=torch.int32, device=DEV))
    for bad in (lambda: ops.fit_query(-1, DST), lambda: ops.fit_query(5, (0, 8)), lambda: ops.fit_query(5, DST, 'max'),
                lambda: ops.fit_counters(torch.zeros((4,), dtype=torch.int64, device=DEV))):
        with pytest.raises(E):
            bad()
    got, st = ops.fit_events(rec, SRC, DST, scale=64, offset=(-16384, 16384), reduce='fire', threshold=32767)     # the limits themselves
    assert got.shape == (0, 8) and ops.fit_counters(st) == dict(seen=2, kept=0, outside=0, cropped=2, skipped=0, merged=0)
    # the entry points refuse buffers smaller than the query reports, and arguments beyond the limits
    n = 600
    many = _dev(R(np.arange(n), np.zeros(n), np.zeros(n)))
    st = torch.zeros((8 + 40,), dtype=torch.int64, device=DEV)
    io = torch.zeros((4,), dtype=torch.int64, device=DEV)
    _, _, _, ws_b, marks_b = ops.fit_query(n, DST)
    ws, marks, out = (torch.empty((b // 8 + 1,), dtype=torch.int64, device=DEV) for b in (ws_b, marks_b, n * 8))
    lib, p = ops._l(), ops._p

    def scan(wb=ws_b, mb=marks_b, geo=(12, 20, 5, 8, 0, 0, 2, -1, -1), reduce=2, theta=3):
        return lib.leod_event_fit_scan(p(many), n, *geo, reduce, theta, p(st), p(ws), wb, p(marks), mb, p(io), ops._stream())

    def emit(mb=marks_b, geo=(12, 20, 5, 8, 0, 0, 2, -1, -1), reduce=2, cap=n):
        return lib.leod_event_fit_emit(p(many), n, *geo, reduce, p(marks), mb, p(out), cap, ops._stream())
    assert scan(mb=marks_b - 8) != 0 and scan(wb=ops.fit_query(1, DST)[3] - 1) != 0 and emit(mb=marks_b - 8) != 0 and emit(cap=-1) != 0
    for geo in ((0, 20, 5, 8, 0, 0, 2, -1, -1), (12, 16385, 5, 8, 0, 0, 2, -1, -1), (12, 20, 5, 16385, 0, 0, 2, -1, -1),
                (12, 20, 5, 8, 45, 0, 2, -1, -1), (12, 20, 5, 8, 0, 2, 2, -1, -1), (12, 20, 5, 8, 0, 0, 0, -1, -1),
                (12, 20, 5, 8, 0, 0, 65, -1, -1), (12, 20, 5, 8, 0, 0, 2, -16385, -1), (12, 20, 5, 8, 0, 0, 2, -1, 16385)):
        assert scan(geo=geo) != 0 and emit(geo=geo) != 0, geo
    assert scan(reduce=3) != 0 and scan(theta=0) != 0 and scan(theta=32768) != 0 and emit(reduce=-1) != 0
    assert scan() == 0 and emit() == 0


def test_pick_at_scale_two_is_the_voxelisers_ds2(ops):
    """The anchor to existing behaviour: source (24, 32), scale 2, pick, voxelised at (12, 16) without ``ds2`` == the source voxelised at
    (24, 32) with ``ds2``.  A window's time bins are normalised over the events the voxeliser is given, so the two agree only where the
    first and the last event of every window survive the pick: the streams are built with those on odd-x, odd-y pixels."""
    rng = np.random.RandomState(3)
    sizes = (700, 1, 900, 2)
    n = sum(sizes)
    t = np.sort(rng.randint(0, 4 * D, n))
    x, y, p = rng.randint(0, 32, n), rng.randint(0, 24, n), rng.randint(0, 2, n)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for a, b in zip(off[:-1], off[1:]):
        for i in (a, b - 1):
            x[i] |= 1
            y[i] |= 1
    rec = R(t, x, y, p)
    kept, state = ops.fit_events(_dev(rec), (24, 32), (12, 16), scale=2, reduce='pick')
    odd = (x % 2 == 1) & (y % 2 == 1)
    assert ops.fit_counters(state) == dict(seen=n, kept=int(odd.sum()), outside=0, cropped=0, skipped=int(n - odd.sum()), merged=0)
    kept_off = np.concatenate([[0], np.cumsum(odd)])[off]
    got, _ = ops.voxelize_dat_windows(kept.reshape(-1), kept_off, 10, 12, 16, ds2=False)
    want, _ = ops.voxelize_dat_windows(_dev(rec), off, 10, 24, 32, ds2=True)
    assert got.shape == want.shape == (4, 20, 12, 16) and torch.equal(got, want) and int(want.sum()) > 300


# ---- ingestion ----------------------------------------------------------------------------------------------------------------------------
BINS = 10
TAU_ING = 30_000


def _synthetic_recording():
    """Four windows of 50 ms on a (12, 20) sensor: uniform events, some beyond the sensor, a busy pixel, and a last event at exactly 4 * D."""
    rng = np.random.RandomState(6)
    n = 2500
    t = np.sort(rng.randint(1, 4 * D, n))
    x, y, p = rng.randint(0, 20, n), rng.randint(0, 12, n), rng.randint(0, 2, n)
    x[rng.rand(n) < 0.02] += 20
    busy = rng.rand(n) < 0.1
    x[busy], y[busy] = 7, 5
    t, x, y, p = (np.append(a, v) for a, v in ((t, 4 * D), (x, 9), (y, 6), (p, 1)))
    return t.astype(np.int64), x.astype(np.int64), y.astype(np.int64), p.astype(np.int64)


def _boxes():
    rows = [(40_000, 2, 2, 6, 4, 0), (40_000, 0, 0, 2, 12, 1), (120_000, 10, 4, 10, 6, 0), (120_000, 18, 10, 2, 2, 1), (190_000, 4.5, 1.5, 3, 9, 1)]
    b = np.zeros((len(rows),), dtype=BOX)
    for i, (t, x, y, w, h, c) in enumerate(rows):
        b[i] = (t, x, y, w, h, c, 1.0, i)
    return b


@pytest.fixture(scope='module')
def recording():
    ev = _synthetic_recording()
    rec = R(*ev)
    mask = np.zeros(SRC, dtype=np.uint8)
    mask[5, 7] = 1                                               # the busy pixel, at SOURCE geometry
    kept = {}
    for reduce in fr.REDUCES:
        f = fr.Fit(SRC, DST, reduce=reduce, **GEO)               # fire: the default threshold k * k
        kept[reduce] = (f.feed(rec), f.counters())
    flt = filter_ref.Filter(SRC[0], SRC[1], TAU_ING, mask)
    stage1 = flt.feed(rec)
    f = fr.Fit(SRC, DST, reduce='fire', **GEO)
    kept['filtered'] = (f.feed(stage1), f.counters(), flt.counters())
    for a in ev + (rec, mask):
        a.setflags(write=False)
    return dict(ev=ev, rec=rec, mask=mask, kept=kept, boxes=_boxes())


@pytest.fixture()
def small_frames(monkeypatch):
    from leod_amd.data import ingest
    from leod_amd.data.utils.types import DatasetType
    monkeypatch.setitem(ingest.SENSOR_HW, DatasetType.GEN1, DST)
    return ingest


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


def _write_sources(src, recording, header_hw=SRC):
    from leod_amd.data.utils import dat_events, raw_events
    t, x, y, p = recording['ev']
    os.makedirs(src, exist_ok=True)
    dat_events.write_dat(os.path.join(src, 'a_td.dat'), dat_events.encode(t, x, y, p), *header_hw)
    raw_events.write_raw(os.path.join(src, 'a.raw'), raw_events.encode_evt3(t, x, y, p, first_time_high=777, vectors=True), 'evt3',
                         height=header_hw[0], width=header_hw[1])
    np.save(os.path.join(src, 'a_bbox.npy'), recording['boxes'])
    return os.path.join(src, 'a_bbox.npy')


def _voxelized(ops, kept, n_frames):
    """What the voxeliser makes of the restatement's records at the frame geometry."""
    from leod_amd.data.utils import dat_events
    off = dat_events.window_offsets(kept[:, 0].astype(np.int64), D, n_frames)
    out, dropped = ops.voxelize_dat_windows(_dev(kept), off, BINS, DST[0], DST[1], ds2=False)
    assert int(dropped.item()) == 0
    return out.cpu().numpy()


def _frames(seq_dir, write):
    from leod_amd.data.utils import misc, packed
    if write == 'npy':
        return np.load(misc.get_ev_raw_fn(seq_dir, 'gen1'))
    fn = [f for f in _tree_files(seq_dir).values() if f.endswith('.evp')]
    assert len(fn) == 1
    store = packed.PackedFrames(fn[0])
    try:
        return store.read(0, len(store))
    finally:
        store.close()


@pytest.mark.parametrize('write', ['npy', 'packed'])
@pytest.mark.parametrize('reduce', fr.REDUCES)
def test_a_foreign_sensor_is_fitted_onto_the_frames(ops, tmp_path, recording, small_frames, reduce, write):
    """(12, 20) onto (5, 8): auto / center give k = 2 and, with floor division, the offset (-1, -1) -- (8 - 10) // 2 and (5 - 6) // 2 -- so
    a column and a row of cells are cropped."""
    from leod_amd.data.utils import event_filter as ef
    ingest = small_frames
    src = str(tmp_path / 'src')
    bbox_fn = _write_sources(src, recording)
    want_kept, c = recording['kept'][reduce]
    reps = {}
    for cont, fn in (('dat', 'a_td.dat'), ('raw', 'a.raw')):
        # the .dat run names its sensor and resolves auto; the .raw run takes the size from the header and is given the scale
        kw = dict(sensor_hw='20x12', fit=dict(scale='auto', reduce=reduce)) if cont == 'dat' else \
            dict(fit='auto' if reduce == 'pick' else dict(scale=2, offset='center', reduce=reduce))
        reps[cont] = ingest.ingest_recording(os.path.join(src, fn), bbox_fn, str(tmp_path / cont), 'gen1', write=write, raw_chunk_bytes=4096, **kw)
    _same_trees(str(tmp_path / 'raw'), str(tmp_path / 'dat'), 'raw against dat')
    spec = ef.fit_spec(SRC, DST, reduce=reduce)
    assert (spec['scale'], spec['offset'], spec['threshold']) == (2, [-1, -1], 4 if reduce == 'fire' else None)
    for cont in ('dat', 'raw'):
        rep = reps[cont]
        assert rep['fit'] == spec and json.loads(json.dumps(rep['fit'])) == spec
        assert (rep['events'], rep['frames'], rep['kept_events'], rep['dropped_events'], rep['cropped_events'], rep['skipped_events'],
                rep['merged_events']) == (c['seen'], 4, c['kept'], c['outside'], c['cropped'], c['skipped'], c['merged'])
        assert rep['events'] == rep['kept_events'] + rep['dropped_events'] + rep['cropped_events'] + rep['skipped_events'] + rep['merged_events']
        assert min(c['kept'], c['outside'], c['cropped']) > 0 and rep['boxes_outside'] == 2
    frames = _frames(str(tmp_path / 'dat'), write)
    assert frames.shape == (4, 2 * BINS, DST[0], DST[1]) and np.array_equal(frames, _voxelized(ops, want_kept, 4)) and frames.any()
    assert not any(f.endswith('hot_pixels.npy') for f in _tree_files(str(tmp_path / 'dat')))
    lab = np.load(os.path.join(str(tmp_path / 'dat'), 'labels_v2', 'labels.npz'))
    fitted, n_out = ef.fit_boxes(recording['boxes'], spec)
    want_lab, want_idx, want_repr = ingest.convert_labels(fitted, 4, D, None)
    assert n_out == 2 and len(want_lab) == 3 and np.array_equal(lab['labels'], want_lab)
    assert np.array_equal(lab['objframe_idx_2_label_idx'], want_idx)
    assert [[float(r[k]) for k in 'xywh'] for r in lab['labels']] == [[0, 0, 3, 2], [4, 1, 4, 3], [1.25, 0, 1.5, 4.25]]


def test_the_filters_see_the_source_geometry_and_the_fit_what_they_keep(ops, tmp_path, recording, small_frames):
    ingest = small_frames
    src = str(tmp_path / 'src')
    _write_sources(src, recording)
    want_kept, c, fc = recording['kept']['filtered']
    mask_fn = str(tmp_path / 'mask.npy')
    np.save(mask_fn, recording['mask'])
    reps = []
    for cont, fn, extra in (('dat', 'a_td.dat', dict(pixel_mask=mask_fn)), ('raw', 'a.raw', dict(pixel_mask=recording['mask'], sensor_hw=SRC))):
        reps.append(ingest.ingest_recording(os.path.join(src, fn), None, str(tmp_path / cont), 'gen1', raw_chunk_bytes=4096,
                                            denoise_us=TAU_ING, fit=dict(scale='auto', reduce='fire'), **extra))
    _same_trees(str(tmp_path / 'raw'), str(tmp_path / 'dat'), 'raw against dat')
    for rep in reps:
        assert (rep['events'], rep['dropped_events'], rep['masked_events'], rep['unsupported_events'], rep['masked_pixels']) == \
            (fc['seen'], fc['outside'], fc['masked'], fc['unsupported'], 1)
        assert (rep['kept_events'], rep['cropped_events'], rep['skipped_events'], rep['merged_events']) == (c['kept'], c['cropped'], 0, c['merged'])
        assert c['seen'] == fc['kept'] and c['outside'] == 0 and min(fc['masked'], fc['unsupported'], fc['outside'], c['kept'], c['merged']) > 0
        assert rep['events'] == rep['dropped_events'] + rep['masked_events'] + rep['unsupported_events'] + rep['kept_events'] + \
            rep['cropped_events'] + rep['merged_events']
    assert np.array_equal(_frames(str(tmp_path / 'dat'), 'npy'), _voxelized(ops, want_kept, 4))
    # --hot-rate: the mask is made and written at source geometry
    rep = ingest.ingest_recording(os.path.join(src, 'a_td.dat'), None, str(tmp_path / 'hot'), 'gen1', hot_rate_hz=500, fit='auto')
    hot = [f for f in _tree_files(str(tmp_path / 'hot')).values() if f.endswith('hot_pixels.npy')]
    assert len(hot) == 1 and np.array_equal(np.load(hot[0]), recording['mask']) and rep['masked_pixels'] == 1
    # a mask at the frame geometry is refused once the header has given the source size
    with pytest.raises(ValueError, match='pixel mask'):
        ingest.ingest_recording(os.path.join(src, 'a_td.dat'), None, str(tmp_path / 'bad'), 'gen1', fit='auto', pixel_mask=np.zeros(DST, np.uint8))


def test_without_fit_a_foreign_size_is_the_error_it_was_and_the_sensor_must_agree_with_the_header(ops, tmp_path, recording, small_frames):
    ingest = small_frames
    src = str(tmp_path / 'src')
    _write_sources(src, recording)
    with pytest.raises(ValueError, match='a.raw: header says height 12, a GEN1 recording has 5'):
        ingest.ingest_recording(os.path.join(src, 'a.raw'), None, str(tmp_path / 'o1'), 'gen1')
    with pytest.raises(ValueError, match='a_td.dat: header says Height 12, a GEN1 recording has 5'):
        ingest.ingest_recording(os.path.join(src, 'a_td.dat'), None, str(tmp_path / 'o2'), 'gen1')
    with pytest.raises(ValueError, match='a_td.dat: header says Height 12, a GEN1 recording has 5'):
        ingest.ingest_recording(os.path.join(src, 'a_td.dat'), None, str(tmp_path / 'o2'), 'gen1', sensor_hw=DST)
    with pytest.raises(ValueError, match='header says width 20, the sensor given has 24'):
        ingest.ingest_recording(os.path.join(src, 'a.raw'), None, str(tmp_path / 'o3'), 'gen1', sensor_hw='24x12', fit='auto')
    assert not os.path.exists(str(tmp_path / 'o1')) and not os.path.exists(str(tmp_path / 'o3'))


def test_the_survey_reads_the_same_file_with_sensor(ops, tmp_path, recording, small_frames):
    from leod_amd.data import survey
    src = str(tmp_path / 'src')
    _write_sources(src, recording)
    t, x, y, p = recording['ev']
    for fn in ('a_td.dat', 'a.raw'):
        rep = survey.survey_recording(os.path.join(src, fn), 'gen1', edges_us=[100, 1000], sensor_hw='20x12')
        assert (rep['sensor'], rep['seen'], rep['outside']) == ([12, 20], len(t), int((x >= 20).sum())) and rep['candidates'] == len(t) - rep['outside']
        with pytest.raises(ValueError, match='a GEN1 recording has 5'):
            survey.survey_recording(os.path.join(src, fn), 'gen1', edges_us=[100, 1000])
        with pytest.raises(ValueError, match='the sensor given has 13'):
            survey.survey_recording(os.path.join(src, fn), 'gen1', edges_us=[100, 1000], sensor_hw=(13, 20))


def test_without_a_new_option_the_tree_is_that_of_a_run_that_cannot_reach_the_new_functions(ops, tmp_path, recording, small_frames, monkeypatch):
    from leod_amd.data.utils import event_filter as ef
    ingest = small_frames
    src = str(tmp_path / 'src')
    t, x, y, p = recording['ev']
    inside = (x < DST[1]) & (y < DST[0])
    _write_sources(src, dict(ev=(t[inside], x[inside], y[inside], p[inside]), boxes=recording['boxes']), header_hw=DST)
    for name, ev_fn, extra in (('dat', 'a_td.dat', {}), ('raw', 'a.raw', {}), ('flt', 'a_td.dat', dict(denoise_us=TAU_ING, trail_us=100))):
        first = ingest.ingest_recording(os.path.join(src, ev_fn), None, str(tmp_path / name), 'gen1', raw_chunk_bytes=4096, **extra)
        with monkeypatch.context() as mp:
            def never(*a, **kw):
                raise AssertionError('a run without the new options reached the sensor fit')
            for mod, names in ((ef, ('fit_spec', 'fit_boxes')), (ops, ('fit_events', 'fit_query', 'fit_counters')), (ingest, ('parse_sensor', ))):
                for fn in names:
                    mp.setattr(mod, fn, never)
            mp.setattr(ingest, 'check_fit_options', lambda *a, **kw: None)
            second = ingest.ingest_recording(os.path.join(src, ev_fn), None, str(tmp_path / (name + '2')), 'gen1', raw_chunk_bytes=4096, **extra)
        _same_trees(str(tmp_path / name), str(tmp_path / (name + '2')), name)
        assert {k: v for k, v in first.items() if k != 'recording'} == {k: v for k, v in second.items() if k != 'recording'}
        assert not any(k in first for k in ('fit', 'cropped_events', 'skipped_events', 'merged_events', 'boxes_outside'))
