"""``ops.pixel_filter_events`` (csrc/k_pixfilter.hip) against the tests' sequential restatement (tests/pixfilter_ref.py): kept records byte
for byte, the whole state block and the counters; then recordings through ``ingest_recording`` with the per-pixel filters on.  The
stream sizes follow the kernel's own constants (``ops.pixel_filter_query``): a record per lane, a wave of 64, a tile of records per
workgroup, a pass of tile counts of the scan workgroup, a digit of key bits per pass of the sort."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref  # noqa: E402
import pixfilter_ref as pr  # noqa: E402
from pixfilter_ref import records as R  # noqa: E402
from test_pixfilter_cpu import BAND, HAND, HH, HW, TAU, hand_case, random_case  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
D = 50_000
SORT_TILES = 8                                                   # tiles of records per workgroup of the sort (csrc/k_pixfilter.hip)


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


def _mask_dev(mask):
    return None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)


def _filter(ops, rec, h, w, state=None, mask=None, **kw):
    out, state = ops.pixel_filter_events(_dev(rec), h, w, state=state, pixel_mask=_mask_dev(mask), **kw)
    assert out.dtype == torch.uint8 and out.dim() == 2 and out.shape[1] == 8 and state.dtype == torch.int64
    return out.cpu().numpy().view('<u4').reshape(-1, 2), state


def _check(ops, rec, h, w, mask=None, what='', ws_bytes=None, **kw):
    """One call on the device against the restatement: kept records, the whole state block, the counters."""
    ref = pr.PixelFilter(h, w, mask=mask, **kw)
    want = ref.feed(rec)
    got, state = _filter(ops, rec, h, w, mask=mask, ws_bytes=ws_bytes, **kw)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, f'kept record {bad[0]} of {len(want)}', got[bad[0]].tolist(), want[bad[0]].tolist())
    assert state.cpu().tolist() == ref.state(), what
    assert ops.pixel_filter_counters(state) == ref.counters(), what
    return got, ref


@pytest.mark.parametrize('case', HAND, ids=[c[0] for c in HAND])
def test_hand_written_streams(ops, case):
    rec, mask, kw, want, counts = hand_case(case)
    got, ref = _check(ops, rec, HH, HW, mask=mask, what=case[0], **kw)
    assert np.array_equal(got, want) and ref.counters() == counts


def test_no_events(ops):
    empty = np.zeros((0, 2), dtype='<u4')
    got, state = _filter(ops, empty, HH, HW, burst_us=5, flicker=BAND)
    assert got.shape == (0, 2) and state.cpu().tolist() == pr.PixelFilter(HH, HW).state()
    rec = R([1, 2], [0, 0], [0, 0], [1, 1])
    _, s1 = _filter(ops, rec, HH, HW, burst_us=5)
    got, s2 = _filter(ops, empty, HH, HW, state=s1, burst_us=5)
    assert got.shape == (0, 2) and torch.equal(s1, s2) and s2.data_ptr() != s1.data_ptr()
    assert ops.pixel_filter_counters(s2) == dict(seen=2, kept=1, outside=0, masked=0, flicker=0, burst=1)


def _sizes(ops):
    tile, per_pass, digit, _, _ = ops.pixel_filter_query(0, 12, 16)
    assert (tile, per_pass, digit) == (256, 256, 8), 'the sizes below were chosen for these constants'
    return [1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5, SORT_TILES * tile - 1, SORT_TILES * tile, SORT_TILES * tile + 1,
            tile * per_pass - 1, tile * per_pass + tile + 1]


@pytest.mark.parametrize('flicker', [None, BAND], ids=['burst_only', 'with_flicker'])
@pytest.mark.parametrize('keep', pr.KEEP)
def test_random_streams_of_the_sizes_where_the_kernel_changes_path(ops, keep, flicker):
    for k, n in enumerate(_sizes(ops)):
        rec, mask = random_case(k, n)
        _, ref = _check(ops, rec, 12, 16, mask=mask, what=f'n = {n}', burst_us=TAU, burst_keep=keep, flicker=flicker)
        c = ref.counters()
        if n > 1000:                                             # not vacuous
            assert min(c['kept'], c['outside'], c['masked'], c['burst']) > 0 and (flicker is None or c['flicker'] > 0), (n, c)


def test_flicker_alone_and_both_families_off(ops):
    rec, mask = random_case(21, 6000)
    _, ref = _check(ops, rec, 12, 16, mask=mask, flicker=BAND)
    assert ref.counters()['flicker'] > 0 and ref.counters()['burst'] == 0
    got, ref = _check(ops, rec, 12, 16, mask=mask)
    c = ref.counters()
    assert c['flicker'] == c['burst'] == 0 and c['kept'] == len(got) == 6000 - c['outside'] - c['masked']
    # steps 1 and 2 are the whole rule: the activity filter with its third rule off keeps the same records
    other, _ = ops.filter_events(_dev(rec), 12, 16, None, pixel_mask=_mask_dev(mask))
    assert np.array_equal(other.cpu().numpy().view('<u4').reshape(-1, 2), got)


@pytest.mark.parametrize('hw', [(1, 1), (1, 2), (1, 255), (1, 256), (1, 257), (16, 16), (257, 255), (256, 256), (1, 16384)])
def test_sensors_on_each_side_of_a_sort_digit_boundary(ops, hw):
    """8-bit digits: 256 pixels take one pass of the sort, 257 two, 256 * 256 two, 257 * 255 = 65535 two; a single pixel takes none."""
    h, w = hw
    rng = np.random.RandomState(h * 1000 + w)
    n = 1500
    t = np.sort(rng.randint(0, 40 * n, n))
    # the top pixels of the sensor occur, so the highest key bit is used
    x, y = rng.randint(max(w - 300, 0), min(w + 2, 16384), n), rng.randint(max(h - 3, 0), h + 1, n)
    _, ref = _check(ops, R(t, x, y, rng.randint(0, 2, n)), h, w, what=str(hw), burst_us=3000, burst_keep='from_second', flicker=BAND)
    assert ref.counters()['kept'] > 0 and ref.counters()['outside'] > 0 and ref.counters()['burst'] > 0


def test_the_1_megapixel_sensor_with_a_few_thousand_events(ops):
    rng = np.random.RandomState(5)
    lamps = ((1279, 719), (0, 0), (640, 360))
    rec = pr.lamp_stream(rng, 5000, 720, 1280, lamps)
    x, y = filter_ref.unpack(rec)[1:3]
    x[:2000], y[:2000] = 600 + x[:2000] % 8, 300 + y[:2000] % 8         # a busy patch, so that bursts occur
    rec = R(rec[:, 0], x, y, filter_ref.unpack(rec)[3])
    mask = np.zeros((720, 1280), dtype=np.uint8)
    mask[300:304, 600:602] = 1
    _, ref = _check(ops, rec, 720, 1280, mask=mask, burst_us=TAU, flicker=BAND)
    assert min(ref.counters().values()) > 0, ref.counters()


def test_tau_zero_and_a_gap_beyond_two_to_the_31(ops):
    rng = np.random.RandomState(8)
    n = 700
    t = np.sort(rng.randint(0, 200, n))                          # many equal times
    rec = R(t, rng.randint(0, 5, n), rng.randint(0, 4, n), rng.randint(0, 2, n))
    for keep in pr.KEEP:
        _, ref = _check(ops, rec, HH, HW, burst_us=0, burst_keep=keep)
        assert ref.counters()['burst'] > 0 and ref.counters()['kept'] > 0
    # times up to 2^32 - 1: differences are taken in 64 bits
    big = 2 ** 31 + 12345
    t = [0, 5, big, big + 3, 2 ** 32 - 10, 2 ** 32 - 1]
    rec = R(t, [1] * 6, [1] * 6, [1, 1, 1, 1, 1, 1])
    got, _ = _check(ops, rec, HH, HW, burst_us=2 ** 31 - 1, burst_keep='first', flicker=(1, 2 ** 31 - 1, 1))
    assert got[:, 0].tolist() == [0, big]                        # big - 5 > tau: a new burst; 2^32 - 10 - (big + 3) <= tau: connected
    _check(ops, rec, HH, HW, burst_us=10, burst_keep='from_second', flicker=(2 ** 31 - 1, 2 ** 31 - 1, 1))


def test_all_events_on_one_pixel(ops):
    rng = np.random.RandomState(9)
    n = 20_000
    t = np.cumsum(rng.randint(0, 9, n))
    rec = R(t, np.full(n, 7), np.full(n, 5), rng.randint(0, 2, n))
    for kw in (dict(burst_us=4, burst_keep='first'), dict(burst_us=4, burst_keep='second', flicker=(10, 30, 2))):
        _, ref = _check(ops, rec, 12, 16, **kw)
        assert ref.counters()['burst'] > 1000 and ref.counters()['kept'] > 1000
    _check(ops, rec, 12, 16, burst_us=4, ws_bytes=ops.pixel_filter_query(1024, 12, 16)[3])      # the run crosses the pieces


def test_forced_pieces_through_a_small_workspace(ops):
    tile = ops.pixel_filter_query(0, 12, 16)[0]
    rec, mask = random_case(11, 9 * tile + 17)
    one_tile = ops.pixel_filter_query(1, 12, 16)[3]
    assert ops.pixel_filter_query(tile, 12, 16)[3] == one_tile < ops.pixel_filter_query(tile + 1, 12, 16)[3] < 2 * one_tile
    whole = ops.pixel_filter_query(len(rec), 12, 16)[3]
    # pieces of 1, 1, 2, 8 (one whole workgroup of the sort) and 9 tiles, and the chunk in one piece
    for ws in (one_tile, ops.pixel_filter_query(2 * tile, 12, 16)[3] - 1, ops.pixel_filter_query(2 * tile, 12, 16)[3],
               ops.pixel_filter_query(SORT_TILES * tile, 12, 16)[3], whole - 1, whole):
        _check(ops, rec, 12, 16, mask=mask, what=f'ws {ws}', ws_bytes=ws, burst_us=TAU, burst_keep='from_second', flicker=BAND)
    with pytest.raises(_err(), match='ws_bytes'):
        ops.pixel_filter_events(_dev(rec), 12, 16, burst_us=5, ws_bytes=one_tile - 1)


def test_chunk_carry_at_every_split(ops):
    rng = np.random.RandomState(12)
    rec = pr.lamp_stream(rng, 200, HH, HW, ((2, 2),), period=1000, jitter=30)
    rec[:, 0] //= 4                                              # 2000 us, lamp period 250 us
    kw = dict(burst_us=40, burst_keep='from_second', flicker=(200, 300, 2))
    mask = np.zeros((HH, HW), dtype=np.uint8)
    mask[1, 1] = 1
    whole, ref = _check(ops, rec, HH, HW, mask=mask, **kw)
    assert min(ref.counters().values()) > 0, ref.counters()
    for split in range(len(rec) + 1):
        a, s1 = _filter(ops, rec[:split], HH, HW, mask=mask, **kw)
        keep1 = s1.clone()
        b, s2 = _filter(ops, rec[split:], HH, HW, state=s1, mask=mask, **kw)
        assert np.array_equal(np.concatenate([a, b]), whole), split
        assert s2.cpu().tolist() == ref.state(), split
        assert torch.equal(s1, keep1), f'split {split}: the given state was modified'


def test_two_runs_are_byte_identical(ops):
    rec, mask = random_case(13, 30_000)
    d, m = _dev(rec), _mask_dev(mask)
    kw = dict(burst_us=TAU, burst_keep='second', flicker=BAND, pixel_mask=m)
    a, sa = ops.pixel_filter_events(d, 12, 16, **kw)
    b, sb = ops.pixel_filter_events(d, 12, 16, **kw)
    c, sc = ops.pixel_filter_events(d, 12, 16, ws_bytes=ops.pixel_filter_query(2048, 12, 16)[3], **kw)
    assert torch.equal(a, b) and torch.equal(sa, sb) and torch.equal(a, c) and torch.equal(sa, sc) and a.shape[0] > 1000


def test_nothing_behind_the_kept_records_and_a_small_buffer_is_refused(ops):
    rec, mask = random_case(14, 900)
    want = pr.PixelFilter(12, 16, TAU, mask=mask).feed(rec)
    m = len(want)
    buf = torch.full(((m + 9) * 8,), 0xA5, dtype=torch.uint8, device=DEV)
    out, _ = ops.pixel_filter_events(_dev(rec), 12, 16, burst_us=TAU, pixel_mask=_mask_dev(mask), out=buf)
    assert out.shape == (m, 8) and out.data_ptr() == buf.data_ptr()
    assert np.array_equal(out.cpu().numpy().view('<u4').reshape(-1, 2), want)
    assert bool((buf[m * 8:] == 0xA5).all())
    exact = torch.empty((m * 8,), dtype=torch.uint8, device=DEV)
    assert ops.pixel_filter_events(_dev(rec), 12, 16, burst_us=TAU, pixel_mask=_mask_dev(mask), out=exact)[0].shape == (m, 8)
    with pytest.raises(_err(), match='do not hold'):
        ops.pixel_filter_events(_dev(rec), 12, 16, burst_us=TAU, pixel_mask=_mask_dev(mask),
                                out=torch.empty((m * 8 - 8,), dtype=torch.uint8, device=DEV))


def test_a_decreasing_time_is_refused_with_its_position(ops):
    tile = ops.pixel_filter_query(0, 12, 16)[0]
    rec, _ = random_case(15, 3 * tile)
    rec[:, 0] += 1                                               # no time is 0
    for pos in (1, tile, 2 * tile + 7, 3 * tile - 1):            # every piece of one tile, their first and last record
        bad = rec.copy()
        bad[pos:, 0] = np.maximum(bad[pos:, 0], bad[pos - 1, 0] + 5)      # still sorted ...
        bad[pos, 0] = bad[pos - 1, 0] - 1                                   # ... but for this one
        with pytest.raises(ops.EventOrderError) as e:
            ops.pixel_filter_events(_dev(bad), 12, 16, burst_us=5, ws_bytes=ops.pixel_filter_query(tile, 12, 16)[3])
        assert (e.value.position, e.value.t_before, e.value.t_at) == (pos, int(bad[pos - 1, 0]), int(bad[pos, 0]))
        with pytest.raises(pr.OrderError) as r:
            pr.PixelFilter(12, 16, 5).feed(bad)
        assert (r.value.position, r.value.t_before, r.value.t_at) == (e.value.position, e.value.t_before, e.value.t_at)
    # across a chunk boundary: position 0, against the last time of the chunk before -- also where that event was outside the sensor
    _, s1 = _filter(ops, R([10, 500], [1, 99], [1, 1]), 12, 16, burst_us=5)
    with pytest.raises(ops.EventOrderError) as e:
        ops.pixel_filter_events(_dev(R([499, 600], [1, 1], [1, 1])), 12, 16, burst_us=5, state=s1)
    assert (e.value.position, e.value.t_before, e.value.t_at) == (0, 500, 499)
    got, _ = _filter(ops, R([500, 600], [1, 1], [1, 1]), 12, 16, state=s1, burst_us=5)        # an equal time is in order
    assert len(got) == 2


def test_argument_checks(ops):
    rec = _dev(R([1, 2], [0, 1], [0, 0]))
    E = _err()
    ok = dict(burst_us=5)
    for kw in (dict(burst_us=-1), dict(burst_us=2 ** 31), dict(burst_us=1.0), dict(burst_us=True), dict(burst_us=5, burst_keep='third'),
               dict(burst_keep=1), dict(flicker=(0, 5, 1)), dict(flicker=(6, 5, 1)), dict(flicker=(1, 2 ** 31, 1)), dict(flicker=(1, 5, 0)),
               dict(flicker=(1, 5, 256)), dict(flicker=(1, 5)), dict(flicker=(1.0, 5, 1)), dict(flicker='1:5')):
        with pytest.raises(E):
            ops.pixel_filter_events(rec, 12, 16, **kw)
    for h, w in ((0, 16), (12, 16385), (12.0, 16), (True, 16)):
        with pytest.raises(E):
            ops.pixel_filter_events(rec, h, w, **ok)
    with pytest.raises(E):
        ops.pixel_filter_events(rec[:9], 12, 16, **ok)                         # no whole number of records
    with pytest.raises(E):
        ops.pixel_filter_events(rec.cpu(), 12, 16, **ok)
    with pytest.raises(E):
        ops.pixel_filter_events(rec, 12, 16, state=torch.zeros((8 + 12 * 16,), dtype=torch.int64, device=DEV), **ok)     # the other filter's
    with pytest.raises(E):
        ops.pixel_filter_events(rec, 12, 16, state=torch.zeros((8 + 4 * 12 * 16,), dtype=torch.int32, device=DEV), **ok)
    with pytest.raises(E):
        ops.pixel_filter_events(rec, 12, 16, pixel_mask=torch.zeros((16, 12), dtype=torch.uint8, device=DEV), **ok)
    with pytest.raises(E):
        ops.pixel_filter_events(rec, 12, 16, pixel_mask=torch.zeros((12, 16), dtype=torch.int32, device=DEV), **ok)
    with pytest.raises(E):
        ops.pixel_filter_events(rec, 12, 16, ws_bytes=0, **ok)
    with pytest.raises(E):
        ops.pixel_filter_query(-1, 12, 16)
    with pytest.raises(E):
        ops.pixel_filter_query(5, 0, 16)
    with pytest.raises(E):
        ops.pixel_filter_counters(torch.zeros((4,), dtype=torch.int64, device=DEV))
    # a bool mask is taken; the entry point refuses marks smaller than the query reports
    got, _ = ops.pixel_filter_events(rec, 12, 16, pixel_mask=torch.ones((12, 16), dtype=torch.bool, device=DEV), **ok)
    assert got.shape == (0, 8)
    n = 600
    many = _dev(R(np.arange(n), np.zeros(n), np.zeros(n)))
    st = torch.zeros((8 + 4 * 12 * 16,), dtype=torch.int64, device=DEV)
    io = torch.zeros((4,), dtype=torch.int64, device=DEV)
    _, _, _, ws_b, marks_b = ops.pixel_filter_query(n, 12, 16)
    ws, marks = (torch.empty((b // 8 + 1,), dtype=torch.int64, device=DEV) for b in (ws_b, marks_b))
    call = lambda wb, mb: ops._l().leod_pixel_filter_scan(ops._p(many), n, 12, 16, 5, 0, 0, 0, 0, None, ops._p(st), ops._p(ws), wb,      # noqa: E731
                                                           ops._p(marks), mb, ops._p(io), ops._stream())
    assert call(ws_b, marks_b - 8) != 0 and call(ops.pixel_filter_query(1, 12, 16)[3] - 1, marks_b) != 0
    assert call(ws_b, marks_b) == 0


# ---- ingestion ----------------------------------------------------------------------------------------------------------------------------
BINS, GH, GW = 10, 48, 64                                        # the sensor is shrunk through ingest.SENSOR_HW
LAMPS = ((10, 7), (50, 40))
HOT = (33, 20)
ING = dict(trail_us=3000, anti_flicker='80:125', flicker_lock=3)
ING_OPS = dict(burst_us=3000, burst_keep='first', flicker=(8000, 12500, 3))
TAU_ING = 20_000


def _synthetic_recording():
    """Six windows of 50 ms on a 48 x 64 sensor: a 5 x 5 block that moves a pixel every 4 ms and fires in bursts, sparse uniform noise, two
    lamps at 100 Hz, a hot pixel that fires every 300 us with alternating polarity; window 3 holds the lamps only, which are locked by
    then -- the filter empties it -- and the last event of the recording is a lone noise event at exactly 6 * D."""
    rng = np.random.RandomState(6)
    parts = []
    for ms in range(0, 300, 2):
        if 150 <= ms < 200:
            continue
        n = 10
        tt = ms * 1000 + np.sort(rng.randint(1, 2000, n))
        parts.append((tt, 5 + ms // 8 + rng.randint(0, 5, n), 20 + rng.randint(0, 5, n), np.full(n, (ms // 2) % 2)))
    n_noise = 300
    tn = rng.randint(1, 6 * D, n_noise)
    tn = tn[(tn <= 3 * D) | (tn > 4 * D)]
    nx, ny = rng.randint(0, GW, len(tn)), rng.randint(0, GH, len(tn))
    for lx, ly in LAMPS:
        nx[(nx == lx) & (ny == ly)] += 1
    parts.append((tn, nx, ny, rng.randint(0, 2, len(tn))))
    for lx, ly in LAMPS:
        starts = np.arange(700, 6 * D - 10_000, 10_000)
        for half, pol in ((0, 1), (5000, 0)):
            for rep in range(2):
                tt = starts + half + rep * 60 + rng.randint(-200, 201, len(starts))
                parts.append((tt, np.full(len(tt), lx), np.full(len(tt), ly), np.full(len(tt), pol)))
    th = np.arange(150, 6 * D, 300)
    th = th[(th <= 3 * D) | (th > 4 * D)]
    parts.append((th, np.full(len(th), HOT[0]), np.full(len(th), HOT[1]), np.arange(len(th)) % 2))
    parts.append((np.array([6 * D]), np.array([60]), np.array([3]), np.array([1])))
    t, x, y, p = (np.concatenate([q[k] for q in parts]).astype(np.int64) for k in range(4))
    order = np.lexsort((x, y, t))
    return t[order], x[order], y[order], p[order]


@pytest.fixture(scope='module')
def recording():
    """The events and, computed once, what the restatements keep of them: the per-pixel stage with the hot-pixel mask, then the activity
    filter's restatement on its output."""
    from leod_amd.data.utils import event_filter as ef
    t, x, y, p = _synthetic_recording()
    counts = np.zeros((GH, GW), dtype=np.int64)
    np.add.at(counts, (y, x), 1)
    mask = ef.hot_pixel_mask(counts, int(t[-1] - t[0]), 1000)
    rec = R(t, x, y, p)
    first = pr.PixelFilter(GH, GW, mask=mask, **ING_OPS)
    stage1 = first.feed(rec)
    second = filter_ref.Filter(GH, GW, TAU_ING, None)
    stage2 = second.feed(stage1)
    nomask = pr.PixelFilter(GH, GW, **ING_OPS)
    stage1_nomask = nomask.feed(rec)
    for a in (t, x, y, p, mask, stage1, stage2, stage1_nomask):
        a.setflags(write=False)
    return dict(ev=(t, x, y, p), rec=rec, mask=mask, stage1=stage1, stage2=stage2, c1=first.counters(), c2=second.counters(),
                stage1_nomask=stage1_nomask, c1_nomask=nomask.counters())


@pytest.fixture()
def small_sensor(monkeypatch):
    from leod_amd.data import ingest
    from leod_amd.data.utils.types import DatasetType
    monkeypatch.setitem(ingest.SENSOR_HW, DatasetType.GEN1, (GH, GW))
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


def _write_sources(src, ev):
    from leod_amd.data.utils import dat_events, raw_events
    t, x, y, p = ev
    os.makedirs(src, exist_ok=True)
    dat_events.write_dat(os.path.join(src, 'a_td.dat'), dat_events.encode(t, x, y, p), GH, GW)
    raw_events.write_raw(os.path.join(src, 'a.raw'), raw_events.encode_evt3(t, x, y, p, first_time_high=777, vectors=True), 'evt3',
                         height=GH, width=GW)


def _voxelized(ops, kept, n_frames):
    """What the voxeliser makes of kept records, window by window."""
    from leod_amd.data.utils import dat_events
    kt, kx, ky, kp = filter_ref.unpack(kept)
    off = dat_events.window_offsets(kt, D, n_frames)
    frames = np.zeros((n_frames, 2 * BINS, GH, GW), dtype=np.uint8)
    for k in range(n_frames):
        s = slice(int(off[k]), int(off[k + 1]))
        if s.start < s.stop:
            one = ops.voxelize_u8(*(torch.from_numpy(np.ascontiguousarray(a[s])).to(DEV) for a in (kx, ky, kp, kt)), BINS, GH, GW)
            frames[k] = one.cpu().numpy()
    return frames


def test_the_recording_is_what_it_says(recording):
    t = recording['ev'][0]
    c1, c2 = recording['c1'], recording['c2']
    assert 2000 < len(t) < 4000 and np.all(np.diff(t) >= 0) and t[-1] == 6 * D
    assert recording['mask'].sum() == 1 and recording['mask'][HOT[1], HOT[0]]
    assert c1['masked'] > 500 and c1['outside'] == 0 and c1['flicker'] > 150 and c1['burst'] > 150 and c1['kept'] > 300
    assert c2['seen'] == c1['kept'] and c2['unsupported'] > 50 and c2['kept'] > 200
    for kept in (recording['stage1'], recording['stage2']):
        kt = kept[:, 0].astype(np.int64)
        assert not ((kt > 3 * D) & (kt <= 4 * D)).any() and ((t > 3 * D) & (t <= 4 * D)).sum() > 30      # window 3 is emptied
    assert recording['stage2'][-1, 0] < 6 * D                                 # the last event seen does not reach the voxeliser
    assert recording['c1_nomask']['masked'] == 0 and recording['c1_nomask']['kept'] > c1['kept']


@pytest.mark.parametrize('write', ['npy', 'packed'])
def test_filtered_ingestion_of_both_containers(ops, tmp_path, recording, small_sensor, write):
    from leod_amd.data.utils import misc
    ingest = small_sensor
    src = str(tmp_path / 'src')
    _write_sources(src, recording['ev'])
    c1, c2 = recording['c1'], recording['c2']
    kw = dict(write=write, raw_chunk_bytes=4096, **ING)
    plain = ingest.ingest_recording(os.path.join(src, 'a_td.dat'), None, str(tmp_path / 'plain'), 'gen1', write=write)
    reps = {}
    for name, extra in (('pix', {}), ('all', dict(denoise_us=TAU_ING, hot_rate_hz=1000))):
        for cont, fn in (('dat', 'a_td.dat'), ('raw', 'a.raw')):
            reps[name, cont] = ingest.ingest_recording(os.path.join(src, fn), None, str(tmp_path / (name + cont)), 'gen1', **kw, **extra)
        _same_trees(str(tmp_path / (name + 'raw')), str(tmp_path / (name + 'dat')), name + ': raw against dat')
    for cont in ('dat', 'raw'):
        rep = reps['pix', cont]
        cn = recording['c1_nomask']
        assert (rep['events'], rep['frames'], rep['kept_events'], rep['flicker_events'], rep['burst_events'], rep['masked_events'],
                rep['unsupported_events'], rep['dropped_events'], rep['masked_pixels']) == \
            (len(recording['rec']), 6, cn['kept'], cn['flicker'], cn['burst'], 0, 0, 0, 0)
        rep = reps['all', cont]
        assert (rep['events'], rep['frames'], rep['kept_events'], rep['flicker_events'], rep['burst_events'], rep['masked_events'],
                rep['unsupported_events'], rep['dropped_events'], rep['masked_pixels']) == \
            (len(recording['rec']), plain['frames'], c2['kept'], c1['flicker'], c1['burst'], c1['masked'], c2['unsupported'], 0, 1)
        assert rep['kept_events'] + rep['flicker_events'] + rep['burst_events'] + rep['masked_events'] + rep['unsupported_events'] + \
            rep['dropped_events'] == rep['events']
    files = _tree_files(str(tmp_path / 'alldat'))
    hot_fn = [f for f in files if f.endswith('hot_pixels.npy')]
    assert len(hot_fn) == 1 and np.array_equal(np.load(files[hot_fn[0]]), recording['mask'])
    assert sorted(set(files) - set(hot_fn)) == sorted(_tree_files(str(tmp_path / 'plain'))) == sorted(_tree_files(str(tmp_path / 'pixdat')))
    if write == 'packed':
        return
    # the frames are those of voxelising the restatements' output; window 3 is a zero frame
    for name, kept in (('pix', recording['stage1_nomask']), ('all', recording['stage2'])):
        frames = np.load(misc.get_ev_raw_fn(str(tmp_path / (name + 'dat')), 'gen1'))
        assert frames.shape == (6, 2 * BINS, GH, GW)
        want = _voxelized(ops, kept, 6)
        for k in range(6):
            assert np.array_equal(frames[k], want[k]), (name, f'frame {k}')
        assert not frames[3].any() and frames[2].any() and frames[4].any()
    unfiltered = np.load(misc.get_ev_raw_fn(str(tmp_path / 'plain'), 'gen1'))
    assert unfiltered[3].any() and unfiltered[3][:, LAMPS[0][1], LAMPS[0][0]].any()


@pytest.mark.parametrize('kw,ops_kw', [(dict(stc_us=1500), dict(burst_us=1500, burst_keep='from_second')),
                                       (dict(stc_us=1500, stc_cut_trail=True), dict(burst_us=1500, burst_keep='second')),
                                       (dict(anti_flicker=(90, 110), flicker_lock=5), dict(flicker=(9091, 11111, 5)))],
                         ids=['stc', 'stc_cut_trail', 'anti_flicker'])
def test_each_option_reaches_the_op_as_it_says(ops, tmp_path, recording, small_sensor, kw, ops_kw):
    from leod_amd.data.utils import misc
    ingest = small_sensor
    src = str(tmp_path / 'src')
    _write_sources(src, recording['ev'])
    rep = ingest.ingest_recording(os.path.join(src, 'a_td.dat'), None, str(tmp_path / 'out'), 'gen1', raw_chunk_bytes=1 << 20, **kw)
    ref = pr.PixelFilter(GH, GW, **ops_kw)
    kept = ref.feed(recording['rec'])
    c = ref.counters()
    assert (rep['kept_events'], rep['flicker_events'], rep['burst_events']) == (c['kept'], c['flicker'], c['burst']) and c['kept'] > 0
    assert c['flicker'] + c['burst'] > 100
    assert np.array_equal(np.load(misc.get_ev_raw_fn(str(tmp_path / 'out'), 'gen1')), _voxelized(ops, kept, 6))


def test_without_a_new_option_the_tree_is_that_of_a_run_that_cannot_reach_the_new_functions(ops, tmp_path, recording, small_sensor,
                                                                                              monkeypatch):
    ingest = small_sensor
    src = str(tmp_path / 'src')
    _write_sources(src, recording['ev'])
    for name, ev_fn, extra in (('dat', 'a_td.dat', {}), ('raw', 'a.raw', {}), ('flt', 'a_td.dat', dict(denoise_us=TAU_ING, hot_rate_hz=1000))):
        first = ingest.ingest_recording(os.path.join(src, ev_fn), None, str(tmp_path / name), 'gen1', raw_chunk_bytes=4096, **extra)
        with monkeypatch.context() as mp:
            def never(*a, **kw):
                raise AssertionError('a run without the new options reached the per-pixel filter')
            for fn in ('pixel_filter_events', 'pixel_filter_query', 'pixel_filter_counters'):
                mp.setattr(ops, fn, never)
            mp.setattr(ingest, 'check_pixel_filter_options', lambda *a, **kw: None)
            second = ingest.ingest_recording(os.path.join(src, ev_fn), None, str(tmp_path / (name + '2')), 'gen1', raw_chunk_bytes=4096,
                                             **extra)
        _same_trees(str(tmp_path / name), str(tmp_path / (name + '2')), name)
        assert {k: v for k, v in first.items() if k != 'recording'} == {k: v for k, v in second.items() if k != 'recording'}
        assert not any(k in first for k in ('flicker_events', 'burst_events'))
    # with the activity filter alone its mask is applied by that filter, as before: the report counts the masked events there
    assert first['masked_events'] == recording['c1']['masked'] and first['masked_pixels'] == 1


def test_an_emptied_window_is_a_zero_frame_and_shifts_nothing(ops, tmp_path, small_sensor):
    """A pixel fires every 100 us through windows 0 to 2; with a trail filter of 150 us only its first event survives, so windows 1 and 2
    are zero frames, and the last event SEEN sets the number of frames.  Every event in a chunk of its own, then all in one."""
    from leod_amd.data.utils import dat_events, misc
    ingest = small_sensor
    t = np.arange(100, 3 * D + 1, 100)
    x, y, p = np.full(len(t), 9), np.full(len(t), 4), np.ones(len(t), dtype=np.int64)
    fn = str(tmp_path / 'w_td.dat')
    dat_events.write_dat(fn, dat_events.encode(t, x, y, p), GH, GW)
    for chunk in (8, 1 << 20):
        out = str(tmp_path / f'out{chunk}')
        rep = ingest.ingest_recording(fn, None, out, 'gen1', trail_us=150, raw_chunk_bytes=chunk)
        assert (rep['frames'], rep['events'], rep['kept_events'], rep['burst_events']) == (3, len(t), 1, len(t) - 1)
        frames = np.load(misc.get_ev_raw_fn(out, 'gen1'))
        assert frames.shape == (3, 20, GH, GW) and frames[0].sum() == 1 and frames[0][:, 4, 9].sum() == 1
        assert not frames[1].any() and not frames[2].any()


def test_gen4_is_filtered_at_sensor_resolution(ops, tmp_path):
    """Bursts on the pixels (501, 301) and (500, 300), which share the half-resolution pixel (250, 150): at sensor resolution they are two
    pixels with a burst each."""
    from leod_amd.data import ingest
    from leod_amd.data.utils import dat_events, misc
    t, x, y, p = [100, 150, 200, 250], [501, 500, 501, 500], [301, 300, 301, 300], [1, 1, 1, 1]
    fn = str(tmp_path / 'g_td.dat')
    dat_events.write_dat(fn, dat_events.encode(t, x, y, p), 720, 1280)
    rep = ingest.ingest_recording(fn, None, str(tmp_path / 'g4'), 'gen4', trail_us=60)
    assert (rep['frames'], rep['kept_events'], rep['burst_events']) == (1, 4, 0)       # 100 us apart on each pixel: no burst
    rep = ingest.ingest_recording(fn, None, str(tmp_path / 'g4b'), 'gen4', trail_us=100)
    assert (rep['frames'], rep['kept_events'], rep['burst_events']) == (1, 2, 2)
    frames = np.load(misc.get_ev_raw_fn(str(tmp_path / 'g4b'), 'gen4'))
    assert frames.shape == (1, 20, 360, 640) and frames.sum() == 1 and frames[0][:, 150, 250].sum() == 1
