"""``ops.filter_events`` / ``ops.event_pixel_counts`` (csrc/k_filter.hip) against the tests' sequential restatement (tests/filter_ref.py):
kept records byte for byte, the counters and the surface; then recordings through ``ingest_recording`` with the filters on.  The stream
sizes follow the kernel's own constants (``ops.event_filter_query``): a record per lane, a wave of 64, a tile of records per workgroup,
a pass of tile counts of the scan workgroup."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref  # noqa: E402
from filter_ref import records as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
D = 50_000


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as _ops
    return _ops


def _dev(rec):
    return torch.from_numpy(np.ascontiguousarray(rec, dtype='<u4').view(np.uint8).reshape(-1).copy()).to(DEV)


def _mask_dev(mask):
    return None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)


def _filter(ops, rec, h, w, tau, state=None, mask=None, **kw):
    out, state = ops.filter_events(_dev(rec), h, w, tau, state=state, pixel_mask=_mask_dev(mask), **kw)
    assert out.dtype == torch.uint8 and out.dim() == 2 and out.shape[1] == 8 and state.dtype == torch.int64
    return out.cpu().numpy().view('<u4').reshape(-1, 2), state


def _check(ops, rec, h, w, tau, mask=None, what='', **kw):
    """One call on the device against the restatement: kept records, the whole state block, the counters."""
    ref = filter_ref.Filter(h, w, tau, mask)
    want = ref.feed(rec)
    got, state = _filter(ops, rec, h, w, tau, mask=mask, **kw)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, f'kept record {bad[0]} of {len(want)}', got[bad[0]].tolist(), want[bad[0]].tolist())
    assert state.cpu().tolist() == ref.state(), what
    assert ops.event_filter_counters(state) == ref.counters(), what
    return got, ref


# ---- hand-written streams on a 5 x 4 sensor ----------------------------------------------------------------------------------------------
HH, HW, TAU = 4, 5, 10
# (name, t, x, y, mask pixels (x, y), times of the kept events)
HAND = [
    ('lone_event', [5], [2], [2], (), []),
    ('neighbours_tau_apart', [100, 110], [1, 2], [1, 2], (), [110]),
    ('neighbours_tau_plus_one_apart', [100, 111], [1, 2], [1, 2], (), []),
    ('same_pixel_twice', [100, 101], [2, 2], [1, 1], (), []),
    ('removed_event_supports', [0, 100, 105], [0, 1, 2], [0, 0, 0], (), [105]),
    ('equal_times_in_stream_order', [7, 7], [1, 2], [1, 1], (), [7]),
    ('equal_times_in_the_other_order', [7, 7], [2, 1], [1, 1], (), [7]),
    ('three_at_one_time', [7, 7, 7], [3, 0, 4], [3, 0, 3], (), [7]),
    # every corner and an edge pixel alone (nothing beyond the sensor supports them), then each with one neighbour inside
    ('corners_and_an_edge_alone', [0, 20, 40, 60, 80], [0, 4, 0, 4, 2], [0, 0, 3, 3, 0], (), []),
    ('corners_and_an_edge_supported', [0, 1, 20, 21, 40, 41, 60, 61, 80, 81], [1, 0, 3, 4, 1, 0, 3, 4, 1, 2], [1, 0, 1, 0, 2, 3, 2, 3, 1, 0],
     (), [1, 21, 41, 61, 81]),
    # x = 4 and x = 0 of the next row are neighbours in memory, not on the sensor
    ('row_ends_are_no_neighbours', [0, 1, 2, 3], [4, 0, 0, 4], [0, 1, 3, 2], (), []),
    ('masked_neighbour_does_not_support', [0, 1, 2], [1, 2, 3], [1, 1, 1], ((1, 1),), [2]),
    ('masked_event_is_removed', [0, 1], [1, 2], [1, 1], ((2, 1),), []),
    ('outside_event_between_two_inside', [0, 1, 2], [3, 5, 4], [3, 3, 3], (), [2]),
    ('outside_by_y_and_by_both', [0, 1, 2, 3], [0, 0, 9000, 1], [0, 4, 9000, 0], (), [3]),
    ('tau_across_slots', [9, 11, 19, 22, 33], [0, 1, 0, 1, 0], [0, 0, 0, 0, 0], (), [11, 19, 22]),
]


def _hand_mask(pixels):
    if not pixels:
        return None
    m = np.zeros((HH, HW), dtype=np.uint8)
    for x, y in pixels:
        m[y, x] = 1
    return m


def test_the_hand_written_cases_are_what_they_say():
    for name, t, x, y, masked, kept in HAND:
        f = filter_ref.Filter(HH, HW, TAU, _hand_mask(masked))
        assert f.feed(R(t, x, y))[:, 0].tolist() == kept, name


@pytest.mark.parametrize('case', HAND, ids=[c[0] for c in HAND])
def test_hand_written_streams(ops, case):
    name, t, x, y, masked, kept = case
    got, _ = _check(ops, R(t, x, y, [i % 2 for i in range(len(t))]), HH, HW, TAU, mask=_hand_mask(masked), what=name)
    assert got[:, 0].tolist() == kept
    # the same stream far from time zero, where t - tau does not clamp
    got, _ = _check(ops, R(np.asarray(t) + 3_000_000_000, x, y), HH, HW, TAU, mask=_hand_mask(masked), what=name + ' late')
    assert (got[:, 0].astype(np.int64) - 3_000_000_000).tolist() == kept


def test_no_events(ops):
    got, state = _filter(ops, np.zeros((0, 2), '<u4'), HH, HW, TAU)
    assert got.shape == (0, 2) and state.cpu().tolist() == filter_ref.Filter(HH, HW, TAU).state()
    # and between two chunks: the state goes through unchanged
    a, s1 = _filter(ops, R([5, 6], [1, 2], [1, 1]), HH, HW, TAU)
    b, s2 = _filter(ops, np.zeros((0, 2), '<u4'), HH, HW, TAU, state=s1)
    assert len(b) == 0 and torch.equal(s1, s2) and s2 is not s1
    c, _ = _filter(ops, R([16], [3], [1]), HH, HW, TAU, state=s2)
    assert c[:, 0].tolist() == [16]


# ---- random streams on a 16 x 12 sensor --------------------------------------------------------------------------------------------------
RH, RW = 12, 16


def _random_stream(rng, n, t_max, outside=0.03):
    t = np.sort(rng.randint(0, t_max + 1, n))
    x, y = rng.randint(0, RW, n), rng.randint(0, RH, n)
    out = rng.rand(n) < outside
    x[out] = RW + rng.randint(0, 3, int(out.sum()))
    return R(t, x, y, rng.randint(0, 2, n))


def _sizes(ops):
    tile, per_pass = ops.event_filter_query()[:2]
    assert tile % 64 == 0 and tile >= 64
    return [1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5, tile * per_pass - 1, tile * per_pass + tile + 1]


@pytest.mark.parametrize('tau_kind', ['one_slot', 'one_event_per_slot', 'zero'])
def test_random_streams_of_the_sizes_where_the_kernel_changes_path(ops, tau_kind):
    rng = np.random.RandomState(['one_slot', 'one_event_per_slot', 'zero'].index(tau_kind) + 5)
    mask = (rng.rand(RH, RW) < 0.05).astype(np.uint8)
    for n in _sizes(ops):
        if tau_kind == 'one_slot':                               # every time below tau + 1
            rec, tau = _random_stream(rng, n, 4000), 4000
        elif tau_kind == 'one_event_per_slot':                   # distinct times 3 apart, slots 3 wide: support comes from the slot before
            rec, tau = _random_stream(rng, n, 10), 2
            rec[:, 0] = 3 * np.arange(n) + rng.randint(0, 2, n)
            assert len(set((rec[:, 0] // 3).tolist())) == n
        else:                                                    # support at equal times only
            rec, tau = _random_stream(rng, n, max(n // 3, 1)), 0
        got, ref = _check(ops, rec, RH, RW, tau, mask=mask if n % 2 else None, what=(tau_kind, n))
        if n > 1000:
            c = ref.counters()
            assert min(c['kept'], c['unsupported'], c['outside']) > 0, (tau_kind, n, c)


def test_rule_three_off_applies_bounds_and_mask_only(ops):
    rng = np.random.RandomState(12)
    mask = (rng.rand(RH, RW) < 0.2).astype(np.uint8)
    rec = _random_stream(rng, 700, 10_000)
    got, ref = _check(ops, rec, RH, RW, None, mask=mask)
    c = ref.counters()
    assert c['unsupported'] == 0 and c['masked'] > 0 and c['outside'] > 0 and c['kept'] == len(got)
    _check(ops, rec, RH, RW, None, mask=(mask != 0))              # a bool mask is the same mask


# ---- forced splits: the table's bound lowered until a chunk is cut into pieces -----------------------------------------------------------
def test_forced_splits_and_a_gap_beyond_two_to_the_31(ops):
    tile = ops.event_filter_query()[0]
    small = ops.FILTER_WS_MIN_BYTES                               # takes one tile of records per piece
    assert ops.event_filter_query(tile)[2] == small and ops.event_filter_query(5 * tile)[2] > 4 * small
    rng = np.random.RandomState(77)
    n = 5 * tile + 17
    # dense enough that pieces depend on each other: support across every cut comes from the surface
    rec = _random_stream(rng, n, 3 * n)
    whole, ref = _check(ops, rec, RH, RW, 40, what='one piece')
    assert 0 < ref.counters()['kept'] < n - 100
    for ws in (small, 2 * small, 4 * small):
        got, _ = _check(ops, rec, RH, RW, 40, ws_bytes=ws, what=f'ws_bytes={ws}')
        assert np.array_equal(got, whole)
    # two bursts more than 2^31 microseconds apart (in slots of 41 and of 1), the second one cut into pieces as well
    late = rec.copy()
    late[2 * tile + 9:, 0] += np.uint32(2 ** 31 + 12345)
    assert int(late[-1, 0]) < 2 ** 32 and int(late[2 * tile + 9, 0]) - int(late[2 * tile + 8, 0]) > 2 ** 31
    for tau in (40, 0, 2 ** 31 - 1):
        one, _ = _check(ops, late, RH, RW, tau, what=f'gap, tau={tau}')
        cut, _ = _check(ops, late, RH, RW, tau, ws_bytes=small, what=f'gap, tau={tau}, pieces')
        assert np.array_equal(one, cut)
    from leod_amd._lib import LeodHipError
    with pytest.raises(LeodHipError):
        _filter(ops, rec, RH, RW, 40, ws_bytes=small - 1)


# ---- chunk carry --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tau', [25, 0])
def test_chunk_carry_at_every_split(ops, tau):
    rng = np.random.RandomState(41 + tau)
    rec = _random_stream(rng, 200, 700 if tau else 8)
    mask = (rng.rand(RH, RW) < 0.05).astype(np.uint8)
    whole, ref = _check(ops, rec, RH, RW, tau, mask=mask)
    assert 20 < len(whole) < 180
    whole_state = ref.state()
    for cut in range(201):
        a, state = _filter(ops, rec[:cut], RH, RW, tau, mask=mask)
        before = state.clone()
        b, state2 = _filter(ops, rec[cut:], RH, RW, tau, state=state, mask=mask)
        assert np.array_equal(np.concatenate([a, b]), whole), cut
        assert state2.cpu().tolist() == whole_state, cut
        assert state2 is not state and torch.equal(state, before), cut          # the given state is not modified


# ---- out buffer, refusals -----------------------------------------------------------------------------------------------------------------
def test_nothing_behind_the_kept_records_and_a_small_buffer_is_refused(ops):
    from leod_amd._lib import LeodHipError
    rng = np.random.RandomState(3)
    rec = _random_stream(rng, 900, 2000)
    ref = filter_ref.Filter(RH, RW, 30)
    want = ref.feed(rec)
    m = len(want)
    assert 100 < m < 800
    big = torch.full((m * 8 + 4096,), 0xAB, dtype=torch.uint8, device=DEV)
    got, _ = _filter(ops, rec, RH, RW, 30, out=big)
    assert np.array_equal(got, want)
    assert big[:m * 8].cpu().numpy().tobytes() == want.tobytes() and bool((big[m * 8:] == 0xAB).all())
    big.fill_(0xAB)
    got, _ = _filter(ops, rec, RH, RW, 30, out=big[:m * 8])        # exactly enough
    assert np.array_equal(got, want) and bool((big[m * 8:] == 0xAB).all())
    big.fill_(0xAB)
    with pytest.raises(LeodHipError):
        _filter(ops, rec, RH, RW, 30, out=big[:m * 8 - 8])         # refused before anything is stored
    assert bool((big == 0xAB).all())
    with pytest.raises(LeodHipError):
        _filter(ops, rec, RH, RW, 30, out=big[4:])                 # not 8-byte aligned
    with pytest.raises(LeodHipError):
        _filter(ops, rec, RH, RW, 30, out=big.cpu())
    # the kernel's own guard: capacity 3 stores three records of the m
    big.fill_(0xAB)
    lib, p, st = ops._l(), ops._p, ops._stream()
    d = _dev(rec)
    _, _, table_bytes, marks_bytes = ops.event_filter_query(len(rec))
    table = torch.empty((table_bytes // 8,), dtype=torch.int64, device=DEV)
    marks = torch.empty((marks_bytes // 8,), dtype=torch.int64, device=DEV)
    state = torch.tensor(filter_ref.Filter(RH, RW, 30).state(), dtype=torch.int64, device=DEV)
    io = torch.tensor([0, 2 ** 63 - 1, 0, 0], dtype=torch.int64, device=DEV)
    assert lib.leod_event_filter_scan(p(d), len(rec), RH, RW, 30, None, p(state), p(table), table_bytes, p(marks), marks_bytes, p(io), st) == 0
    assert lib.leod_event_filter_emit(p(d), len(rec), p(marks), marks_bytes, p(big), 3, st) == 0
    torch.cuda.synchronize()
    assert int(io[0]) == m and big[:24].cpu().numpy().tobytes() == want[:3].tobytes() and bool((big[24:] == 0xAB).all())
    assert state.cpu().tolist() == ref.state()
    # arguments the entry points refuse
    assert lib.leod_event_filter_scan(p(d), len(rec), RH, RW, 2 ** 31, None, p(state), p(table), table_bytes, p(marks), marks_bytes, p(io), st) == -1
    assert lib.leod_event_filter_scan(p(d), len(rec), RH, RW, -2, None, p(state), p(table), table_bytes, p(marks), marks_bytes, p(io), st) == -1
    assert lib.leod_event_filter_scan(p(d), len(rec), 0, RW, 30, None, p(state), p(table), table_bytes, p(marks), marks_bytes, p(io), st) == -1
    assert lib.leod_event_filter_scan(p(d), len(rec), RH, 16385, 30, None, p(state), p(table), table_bytes, p(marks), marks_bytes, p(io), st) == -1
    assert lib.leod_event_filter_scan(p(d), len(rec), RH, RW, 30, None, p(state), p(table), 1000, p(marks), marks_bytes, p(io), st) == -1
    assert lib.leod_event_filter_scan(p(d), len(rec), RH, RW, 30, None, p(state), p(table), table_bytes, p(marks), marks_bytes - 1, p(io), st) == -1
    assert lib.leod_event_filter_emit(p(d), len(rec), p(marks), marks_bytes - 1, p(big), 3, st) == -1


def test_a_decreasing_time_is_refused_with_its_position(ops):
    rng = np.random.RandomState(9)
    tile = ops.event_filter_query()[0]
    rec = _random_stream(rng, 2 * tile + 50, 5000)
    rec[:, 0] += 5
    for pos in (1, 64, tile, tile + 7, 2 * tile + 49):            # inside a wave, on a wave and a tile boundary, at the end
        bad = rec.copy()
        bad[pos, 0] = bad[pos - 1, 0] - 1                         # the first decrease (what follows is >= the event before it) ...
        if pos + 20 < len(bad):
            bad[pos + 20, 0] = 0                                  # ... and a later, larger one
        with pytest.raises(ops.EventOrderError) as e:
            _filter(ops, bad, RH, RW, 50)
        assert (e.value.position, e.value.t_before, e.value.t_at) == (pos, int(bad[pos - 1, 0]), int(bad[pos, 0])), pos
        assert f'event {pos} ' in str(e.value)
        with pytest.raises(filter_ref.OrderError) as r:
            filter_ref.Filter(RH, RW, 50).feed(bad)
        assert (r.value.position, r.value.t_before, r.value.t_at) == (pos, int(bad[pos - 1, 0]), int(bad[pos, 0]))
        if pos >= tile:                                          # the same in pieces: the position is that of the chunk
            with pytest.raises(ops.EventOrderError) as e:
                _filter(ops, bad, RH, RW, 50, ws_bytes=ops.FILTER_WS_MIN_BYTES)
            assert e.value.position == pos
    # against the chunk before
    _, state = _filter(ops, R([100, 200], [1, 2], [1, 1]), RH, RW, 50)
    with pytest.raises(ops.EventOrderError) as e:
        _filter(ops, R([199, 300], [1, 2], [1, 1]), RH, RW, 50, state=state)
    assert (e.value.position, e.value.t_before, e.value.t_at) == (0, 200, 199)
    got, _ = _filter(ops, R([200, 300], [1, 2], [2, 2]), RH, RW, 50, state=state)      # equal to the last time seen is in order
    assert got[:, 0].tolist() == [200]


def test_argument_checks(ops):
    from leod_amd._lib import LeodHipError
    rec = _dev(R([1, 2], [1, 2], [1, 1]))
    ok_mask = torch.zeros((RH, RW), dtype=torch.uint8, device=DEV)
    ops.filter_events(rec, RH, RW, 5, pixel_mask=ok_mask)
    assert issubclass(ops.EventOrderError, LeodHipError)
    bad_calls = [
        lambda: ops.filter_events(rec.cpu(), RH, RW, 5),                                            # a CPU tensor
        lambda: ops.filter_events(rec.view(torch.int8), RH, RW, 5),                                 # a wrong dtype
        lambda: ops.filter_events(rec.to(torch.int32), RH, RW, 5),
        lambda: ops.filter_events(rec[:12], RH, RW, 5),                                             # a partial record
        lambda: ops.filter_events(rec, RH, RW, -1),                                                 # tau out of range
        lambda: ops.filter_events(rec, RH, RW, 2 ** 31),
        lambda: ops.filter_events(rec, RH, RW, 5.0),
        lambda: ops.filter_events(rec, RH, RW, True),
        lambda: ops.filter_events(rec, 0, RW, 5),
        lambda: ops.filter_events(rec, RH, 16385, 5),
        lambda: ops.filter_events(rec, RH, RW, 5, pixel_mask=ok_mask.t()),                          # a mask of the wrong shape
        lambda: ops.filter_events(rec, RH, RW, 5, pixel_mask=ok_mask[:, :-1]),
        lambda: ops.filter_events(rec, RH, RW, 5, pixel_mask=ok_mask.reshape(-1)),
        lambda: ops.filter_events(rec, RH, RW, 5, pixel_mask=ok_mask.to(torch.int32)),
        lambda: ops.filter_events(rec, RH, RW, 5, pixel_mask=ok_mask.cpu()),
        lambda: ops.filter_events(rec, RH, RW, 5, pixel_mask=ok_mask.cpu().numpy()),
        lambda: ops.filter_events(rec, RH, RW, 5, state=torch.zeros(8 + RH * RW - 1, dtype=torch.int64, device=DEV)),
        lambda: ops.filter_events(rec, RH, RW, 5, state=torch.zeros(8 + RH * RW, dtype=torch.int32, device=DEV)),
        lambda: ops.filter_events(rec, RH, RW, 5, state=torch.zeros(8 + RH * RW, dtype=torch.int64)),
        lambda: ops.filter_events(rec, RH, RW, 5, out=torch.zeros(64, dtype=torch.int32, device=DEV)),
        lambda: ops.event_filter_counters(torch.zeros(8, dtype=torch.int64)),
        lambda: ops.event_filter_counters(torch.zeros(8, dtype=torch.int32, device=DEV)),
        lambda: ops.event_pixel_counts(rec.cpu(), RH, RW),
        lambda: ops.event_pixel_counts(rec.to(torch.int64), RH, RW),
        lambda: ops.event_pixel_counts(rec[:9], RH, RW),
        lambda: ops.event_pixel_counts(rec, RH, RW, counts=torch.zeros((RW, RH), dtype=torch.int64, device=DEV)),
        lambda: ops.event_pixel_counts(rec, RH, RW, counts=torch.zeros((RH, RW), dtype=torch.int32, device=DEV)),
        lambda: ops.event_pixel_counts(rec, RH, RW, counts=torch.zeros((RH, RW), dtype=torch.int64)),
        lambda: ops.event_pixel_counts(rec, RH, 0),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(LeodHipError):
            call()
            pytest.fail(f'call {i} was accepted')
    # a view that is not 8-byte aligned is filtered all the same
    shifted = torch.cat([torch.zeros(4, dtype=torch.uint8, device=DEV), rec])[4:]
    out, _ = ops.filter_events(shifted, RH, RW, 5)
    assert out.cpu().numpy().view('<u4').reshape(-1, 2)[:, 0].tolist() == [2]


def test_event_pixel_counts(ops):
    rng = np.random.RandomState(21)
    tile = ops.event_filter_query()[0]
    a, b = _random_stream(rng, 3 * tile + 11, 1000, outside=0.1), _random_stream(rng, 500, 1000, outside=0.1)
    a[:300, 1] = 3 | (7 << 14)                                    # a hot pixel: 300 adds to one address
    want = np.zeros((RH, RW), dtype=np.int64)
    outs = []
    for rec in (a, b):
        _, x, y, _ = filter_ref.unpack(rec)
        inside = (x < RW) & (y < RH)
        np.add.at(want, (y[inside], x[inside]), 1)
        outs.append(int((~inside).sum()))
    counts, o1 = ops.event_pixel_counts(_dev(a), RH, RW)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (RH, RW) and int(o1) == outs[0] > 0
    same, o2 = ops.event_pixel_counts(_dev(b), RH, RW, counts)     # accumulated into the tensor given
    assert same is counts and int(o2) == outs[1] > 0
    assert np.array_equal(counts.cpu().numpy(), want) and want[7, 3] >= 300
    empty, o3 = ops.event_pixel_counts(_dev(np.zeros((0, 2), '<u4')), RH, RW)
    assert int(empty.sum()) == 0 and int(o3) == 0
    # y beyond the sensor with x inside, and the largest coordinates a record can hold
    edge = R([1, 2, 3], [0, RW - 1, 16383], [RH, RH - 1, 16383])
    c, o = ops.event_pixel_counts(_dev(edge), RH, RW)
    assert int(o) == 2 and int(c.sum()) == 1 and int(c[RH - 1, RW - 1]) == 1


# ---- ingestion ----------------------------------------------------------------------------------------------------------------------------
BINS, GH, GW = 10, 240, 304
TAU_ING = 10_000
HOT = ((17, 33), (250, 200))                                     # (x, y) of the two hot pixels
PROPHESEE_BBOX = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                           'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                           'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})


def _synthetic_recording():
    """Eight windows of 50 ms on the Gen1 sensor: a 6 x 6 block that moves a pixel per millisecond (dense: its events support each
    other), uniform noise, two hot pixels that fire every 400 us; window 5 holds noise only -- the filter empties it -- and the last event
    of the recording is a lone noise event at exactly 8 * D."""
    rng = np.random.RandomState(4)
    parts = []
    for ms in range(400):
        if 250 <= ms < 300:
            continue
        n = 14
        parts.append((ms * 1000 + np.sort(rng.randint(1, 1000, n)), 20 + ms // 2 + rng.randint(0, 6, n), 60 + rng.randint(0, 6, n)))
    n_noise = 700
    tn = np.concatenate([rng.randint(1, 8 * D, n_noise - 40), rng.randint(5 * D + 1, 6 * D, 40)])
    parts.append((tn, rng.randint(0, GW, n_noise), rng.randint(0, GH, n_noise)))
    for hx, hy in HOT:
        th = np.arange(200, 8 * D, 400)
        parts.append((th, np.full(len(th), hx), np.full(len(th), hy)))
    parts.append((np.array([8 * D]), np.array([150]), np.array([120])))
    t, x, y = (np.concatenate([q[k] for q in parts]).astype(np.int64) for k in range(3))
    order = np.lexsort((x, y, t))
    t, x, y = t[order], x[order], y[order]
    return t, x, y, rng.randint(0, 2, len(t))


@pytest.fixture(scope='module')
def recording():
    """The events and, computed once, what the restatement keeps of them with the hot-pixel mask and tau = 10 ms."""
    from leod_amd.data.utils import event_filter as ef
    t, x, y, p = _synthetic_recording()
    counts = np.zeros((GH, GW), dtype=np.int64)
    np.add.at(counts, (y, x), 1)
    mask = ef.hot_pixel_mask(counts, int(t[-1] - t[0]), 1000)
    ref = filter_ref.Filter(GH, GW, TAU_ING, mask)
    rec = R(t, x, y, p)
    kept = ref.feed(rec)
    for a in (t, x, y, p, mask, kept):
        a.setflags(write=False)
    return dict(ev=(t, x, y, p), rec=rec, mask=mask, kept=kept, counters=ref.counters())


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
    boxes = np.zeros((4,), dtype=PROPHESEE_BBOX)
    for i, bt in enumerate([2 * D, 6 * D, 6 * D, 8 * D]):        # a box at the end of the window that the filter empties
        boxes[i] = (bt, 20 + i, 30, 40, 30, i % 2, i, 0.5)
    np.save(os.path.join(src, 'box.npy'), boxes)
    dat_events.write_dat(os.path.join(src, 'a_td.dat'), dat_events.encode(t, x, y, p), GH, GW)
    raw_events.write_raw(os.path.join(src, 'a.raw'), raw_events.encode_evt3(t, x, y, p, first_time_high=777, vectors=True), 'evt3',
                         height=GH, width=GW)


def test_the_recording_is_what_it_says(recording):
    t, x, y, p = recording['ev']
    c = recording['counters']
    assert 5000 < len(t) < 9000 and np.all(np.diff(t) >= 0) and t[-1] == 8 * D
    assert recording['mask'].sum() == 2 and all(recording['mask'][hy, hx] for hx, hy in HOT)
    assert c['masked'] == 2 * len(np.arange(200, 8 * D, 400)) and c['outside'] == 0
    assert c['kept'] > 4000 and c['unsupported'] > 500                       # the block survives, the noise does not
    kt = recording['kept'][:, 0].astype(np.int64)
    assert not ((kt > 5 * D) & (kt <= 6 * D)).any() and ((t > 5 * D) & (t <= 6 * D)).sum() > 40      # window 5 is emptied
    assert kt[-1] < 8 * D                                                     # the last event seen is not kept


@pytest.mark.parametrize('write', ['npy', 'packed'])
def test_filtered_ingestion_of_both_containers(ops, tmp_path, recording, write):
    from leod_amd.data import ingest
    from leod_amd.data.utils import dat_events, misc
    src = str(tmp_path / 'src')
    _write_sources(src, recording['ev'])
    box = os.path.join(src, 'box.npy')
    kw = dict(write=write, denoise_us=TAU_ING, hot_rate_hz=1000, raw_chunk_bytes=8192)
    plain = ingest.ingest_recording(os.path.join(src, 'a_td.dat'), box, str(tmp_path / 'plain'), 'gen1', write=write)
    rep_dat = ingest.ingest_recording(os.path.join(src, 'a_td.dat'), box, str(tmp_path / 'dat'), 'gen1', **kw)
    rep_raw = ingest.ingest_recording(os.path.join(src, 'a.raw'), box, str(tmp_path / 'raw'), 'gen1', **kw)
    _same_trees(str(tmp_path / 'raw'), str(tmp_path / 'dat'), 'raw against dat')
    # the reports: the counters are the restatement's and add up
    c = recording['counters']
    for rep in (rep_dat, rep_raw):
        assert rep['events'] == len(recording['rec']) == plain['events']
        assert (rep['kept_events'], rep['masked_events'], rep['unsupported_events'], rep['dropped_events'], rep['masked_pixels']) == \
            (c['kept'], c['masked'], c['unsupported'], c['outside'], 2)
        assert rep['kept_events'] + rep['masked_events'] + rep['unsupported_events'] + rep['dropped_events'] == rep['events']
        # frames and labels are those of the unfiltered recording
        assert (rep['frames'], rep['labelled_frames'], rep['boxes']) == (plain['frames'], plain['labelled_frames'], plain['boxes']) == (8, 3, 4)
    files, plain_files = _tree_files(str(tmp_path / 'dat')), _tree_files(str(tmp_path / 'plain'))
    hot_fn = [f for f in files if f.endswith('hot_pixels.npy')]
    assert sorted(set(files) - set(hot_fn)) == sorted(plain_files) and len(hot_fn) == 1
    assert np.array_equal(np.load(files[hot_fn[0]]), recording['mask']) and np.load(files[hot_fn[0]]).dtype == np.uint8
    for rel in plain_files:
        if rel.endswith('labels.npz') or rel.endswith('objframe_idx_2_repr_idx.npy'):
            if rel.endswith('.npz'):
                a, b = np.load(files[rel]), np.load(plain_files[rel])
                assert all(np.array_equal(a[k], b[k]) for k in b.files) and sorted(a.files) == sorted(b.files)
            else:
                assert open(files[rel], 'rb').read() == open(plain_files[rel], 'rb').read()
    if write == 'packed':
        return
    # the frames: voxelize_u8 per window on what the restatement keeps; the hot pixels' columns are zero; window 5 is a zero frame
    frames = np.load(misc.get_ev_raw_fn(str(tmp_path / 'dat'), 'gen1'))
    assert frames.shape == (8, 2 * BINS, GH, GW)
    kt, kx, ky, kp = filter_ref.unpack(recording['kept'])
    off = dat_events.window_offsets(kt, D, 8)
    assert off[5] == off[6] and off[8] == len(kt)
    for k in range(8):
        s = slice(int(off[k]), int(off[k + 1]))
        if s.start == s.stop:
            assert not frames[k].any(), f'frame {k}'
            continue
        one = ops.voxelize_u8(*(torch.from_numpy(np.ascontiguousarray(a[s])).to(DEV) for a in (kx, ky, kp, kt)), BINS, GH, GW)
        assert np.array_equal(frames[k], one.cpu().numpy()), f'frame {k}'
    assert not frames[5].any() and frames[4].any() and frames[6].any() and frames[7].any()
    for hx, hy in HOT:
        assert not frames[:, :, hy, hx].any()
    unfiltered = np.load(misc.get_ev_raw_fn(str(tmp_path / 'plain'), 'gen1'))
    assert unfiltered[5].any() and all(unfiltered[:, :, hy, hx].any() for hx, hy in HOT)
    # the written mask repeats the run
    again = ingest.ingest_recording(os.path.join(src, 'a_td.dat'), box, str(tmp_path / 'again'), 'gen1', denoise_us=TAU_ING,
                                    pixel_mask=files[hot_fn[0]], raw_chunk_bytes=1 << 20)
    assert np.array_equal(np.load(misc.get_ev_raw_fn(str(tmp_path / 'again'), 'gen1')), frames)
    assert again['kept_events'] == c['kept'] and not [f for f in _tree_files(str(tmp_path / 'again')) if f.endswith('hot_pixels.npy')]


def test_without_an_option_the_tree_is_that_of_the_unchanged_path(ops, tmp_path, recording, monkeypatch):
    """No option given: ``ingest_recording`` against a second call that is kept from reaching anything this change added -- which shows
    that the filter is not reached and the run is deterministic, not by itself that the bytes are the parent's: both calls run this
    tree's ``ingest_recording``.  So the .dat frames are also compared with a direct call of ``voxelize_recording`` on the memory-mapped
    records and the host's window offsets, the functions the unfiltered .dat path always consisted of and that this change did not touch,
    and the .raw tree with the .dat tree.  Beyond that, the backstop is that the ingestion and RAW tests from before this change
    (tests/test_ingest_gpu.py, tests/test_evt_gpu.py), which compare with independent references, pass unchanged."""
    from leod_amd.data import ingest
    from leod_amd.data.utils import dat_events, misc
    src = str(tmp_path / 'src')
    _write_sources(src, recording['ev'])
    box = os.path.join(src, 'box.npy')
    for name, ev_fn in (('dat', 'a_td.dat'), ('raw', 'a.raw')):
        first = ingest.ingest_recording(os.path.join(src, ev_fn), box, str(tmp_path / name), 'gen1', raw_chunk_bytes=8192)
        with monkeypatch.context() as mp:
            def never(*a, **kw):
                raise AssertionError('the unfiltered path reached the filter')
            for mod, fn in ((ops, 'filter_events'), (ops, 'event_pixel_counts'), (ingest, 'count_pixel_events')):
                mp.setattr(mod, fn, never)
            second = ingest.ingest_recording(os.path.join(src, ev_fn), box, str(tmp_path / (name + '2')), 'gen1', raw_chunk_bytes=8192)
        _same_trees(str(tmp_path / name), str(tmp_path / (name + '2')), name)
        assert {k: v for k, v in first.items() if k != 'recording'} == {k: v for k, v in second.items() if k != 'recording'}
        assert not any(k in first for k in ('kept_events', 'masked_events', 'unsupported_events', 'masked_pixels'))
        assert not [f for f in _tree_files(str(tmp_path / name)) if f.endswith('hot_pixels.npy')]
    _same_trees(str(tmp_path / 'raw'), str(tmp_path / 'dat'), 'raw against dat, unfiltered')
    hdr, records = dat_events.open_records(os.path.join(src, 'a_td.dat'))
    offsets = dat_events.scan_windows(records, D)
    direct = np.zeros((len(offsets) - 1, 2 * BINS, GH, GW), dtype=np.uint8)
    assert ingest.voxelize_recording(records, offsets, direct, BINS, GH, GW, False) == 0
    assert np.array_equal(np.load(misc.get_ev_raw_fn(str(tmp_path / 'dat'), 'gen1')), direct) and direct.any()


def test_an_emptied_window_is_a_zero_frame_and_shifts_nothing(ops, tmp_path, monkeypatch):
    """Three windows on a small sensor: a pair, a lone event (removed: its window is all zeros), a pair; the last event SEEN is a lone one
    in window 3, which therefore exists and is empty.  Every event in a chunk of its own."""
    from leod_amd.data import ingest
    from leod_amd.data.utils import dat_events, misc
    from leod_amd.data.utils.types import DatasetType
    monkeypatch.setitem(ingest.SENSOR_HW, DatasetType.GEN1, (24, 30))
    t = [10, 20, D + 5, 2 * D + 10, 2 * D + 30, 3 * D + 1]
    x, y, p = [3, 4, 20, 8, 9, 25], [3, 3, 20, 8, 9, 2], [1, 0, 1, 0, 1, 1]
    fn = str(tmp_path / 'w_td.dat')
    dat_events.write_dat(fn, dat_events.encode(t, x, y, p), 24, 30)
    for chunk in (8, 1 << 20):
        out = str(tmp_path / f'out{chunk}')
        rep = ingest.ingest_recording(fn, None, out, 'gen1', denoise_us=100, raw_chunk_bytes=chunk)
        assert (rep['frames'], rep['kept_events'], rep['unsupported_events'], rep['masked_pixels']) == (4, 2, 4, 0)
        frames = np.load(misc.get_ev_raw_fn(out, 'gen1'))
        assert frames.shape == (4, 20, 24, 30)
        assert frames[0].sum() == 1 and frames[0][:, 3, 4].sum() == 1
        assert not frames[1].any() and not frames[3].any()
        assert frames[2].sum() == 1 and frames[2][:, 9, 9].sum() == 1
    # a mask alone (rule 3 off) on the same recording: only the masked pixel's event goes
    mask = np.zeros((24, 30), dtype=bool)
    mask[20, 20] = True
    rep = ingest.ingest_recording(fn, None, str(tmp_path / 'masked'), 'gen1', pixel_mask=mask)
    assert (rep['frames'], rep['kept_events'], rep['masked_events'], rep['unsupported_events'], rep['masked_pixels']) == (4, 5, 1, 0, 1)
    frames = np.load(misc.get_ev_raw_fn(str(tmp_path / 'masked'), 'gen1'))
    assert not frames[1].any() and frames[3].sum() == 1


def test_gen4_is_filtered_at_sensor_resolution(ops, tmp_path):
    """Two events on EVEN pixels support one on an odd pixel: the half-resolution frame keeps only odd pixels, so the supporter is not in
    the frame -- the filter saw it all the same."""
    from leod_amd.data import ingest
    from leod_amd.data.utils import dat_events, misc
    t, x, y, p = [100, 150, 900, 950], [500, 501, 800, 801], [300, 301, 400, 400], [1, 1, 0, 0]
    fn = str(tmp_path / 'g_td.dat')
    dat_events.write_dat(fn, dat_events.encode(t, x, y, p), 720, 1280)
    rep = ingest.ingest_recording(fn, None, str(tmp_path / 'g4'), 'gen4', denoise_us=100)
    assert (rep['frames'], rep['kept_events'], rep['unsupported_events']) == (1, 2, 2)
    frames = np.load(misc.get_ev_raw_fn(str(tmp_path / 'g4'), 'gen4'))
    assert frames.shape == (1, 20, 360, 640) and frames.sum() == 1 and frames[0][:, 150, 250].sum() == 1
