"""``ops.survey_events`` (csrc/k_survey.hip) against the tests' sequential restatement (tests/survey_ref.py): the whole state block, byte
for byte, on small sensors and streams chosen for the kernel's own boundaries (a record per lane, a tile of 256 records per workgroup,
pieces of whole tiles); then one stream of 200 000 events on which the five identities of DESIGN.md section 1 are checked against
``ops.filter_events`` and ``ops.pixel_filter_events`` themselves."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixfilter_ref as pr  # noqa: E402
import survey_ref  # noqa: E402
from pixfilter_ref import records as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EDGES = [0, 40, 200, 390, 410, 2_000, 50_000]
BAND = (350, 450)                                                # around the lamps' period of 400 us
TILE = 256


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


def _lamps(n, h, w, seed=5, **kw):
    kw = dict(dict(lamps=[(w // 2, h // 2)], period=400, jitter=10, outside=0.05), **kw)
    return pr.lamp_stream(np.random.RandomState(seed), n, h, w, **kw)


def _survey(ops, chunks, h, w, edges=EDGES, band=BAND, mask=None, ws_bytes=None):
    state = None
    for part in chunks:
        state = ops.survey_events(_dev(part), h, w, edges, flicker=band, state=state, pixel_mask=_mask_dev(mask), ws_bytes=ws_bytes)
        assert state.dtype == torch.int64 and state.dim() == 1
    return state


def _check(ops, chunks, h, w, edges=EDGES, band=BAND, mask=None, ws_bytes=None, what=''):
    """The chunks through the op against the restatement: the whole state block and the counters."""
    ref = survey_ref.Survey(h, w, edges, flicker=band, mask=mask)
    for part in chunks:
        ref.feed(part)
    state = _survey(ops, chunks, h, w, edges, band, mask, ws_bytes)
    got, want = state.cpu().tolist(), ref.state()
    assert len(got) == len(want), (what, len(got), len(want))
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (what, f'state word {bad[0]} (of {len(bad)} that differ)', got[bad[0]], want[bad[0]])
    c, r = ops.survey_counters(state, len(edges)), ref.counters()
    assert sorted(c) == sorted(r)
    for k in r:
        assert np.array_equal(c[k], r[k]), (what, k)
    return state, ref


@pytest.mark.parametrize('h,w', [(1, 1), (1, 9), (5, 1), (5, 7)])
def test_small_sensors(ops, h, w):
    rec = _lamps(1_500, h, w)                                    # six tiles; on 1 x 1 no neighbour is inside, on a line two at most
    _, ref = _check(ops, [rec], h, w, what=f'{h}x{w}')
    c = ref.counters()
    assert c['outside'] > 0 and c['same'].sum() > 0 and c['period'].sum() > 0 and c['run'][1:].sum() > 0
    if h * w == 1:
        assert c['nb'][:-1].sum() == 0 and c['nb'][-1] == c['candidates']
    else:
        assert c['nb'][:-1].sum() > 0


def test_one_edge_at_zero_and_sixty_four_edges(ops):
    rec = _lamps(1_000, 5, 7)
    rec[:, 0] = rec[:, 0] // 64 * 64                             # many equal times, in the lamp's pairs of events too
    _, ref = _check(ops, [rec], 5, 7, edges=[0], what='K=1')
    c = ref.counters()
    assert c['same'][0] > 0 and c['same'][1] > 0 and c['nb'][0] > 0      # d = 0 is not above the edge 0
    edges = [0] + list(range(7, 7 + 63 * 37, 37))
    assert len(edges) == 64
    _, ref = _check(ops, [_lamps(1_000, 5, 7)], 5, 7, edges=edges, what='K=64')
    assert np.count_nonzero(ref.counters()['nb']) > 40 and ref.counters()['nb'][64] > 0


def test_all_events_at_one_time(ops):
    rng = np.random.RandomState(2)
    n = 700
    rec = R(np.full(n, 1_000), rng.randint(0, 7, n), rng.randint(0, 5, n), rng.randint(0, 2, n))
    _, ref = _check(ops, [rec], 5, 7, what='one time')
    assert ref.counters()['nb'][0] > n // 2 and ref.counters()['same'][0] > 0


def test_every_event_on_one_pixel(ops):
    rng = np.random.RandomState(3)
    n = 1_500
    rec = R(np.cumsum(rng.randint(0, 300, n)), np.full(n, 3), np.full(n, 2), rng.randint(0, 2, n))
    _, ref = _check(ops, [rec], 5, 7, what='one pixel')
    assert ref.counters()['nb'][-1] == n                         # no neighbour ever fires


def test_every_candidate_is_its_pixel_s_first(ops):
    h = w = 24                                                   # 576 events: more than two tiles
    order = np.random.RandomState(4).permutation(h * w)
    rec = R(np.arange(h * w) * 3, order % w, order // w, order & 1)
    _, ref = _check(ops, [rec], h, w, what='firsts')
    c = ref.counters()
    assert c['same'].sum() == c['sec_on'].sum() == c['period'].sum() == 0 and c['candidates'] == h * w


def test_empty_chunks_and_single_events_one_by_one(ops):
    rec = _lamps(60, 5, 7)
    empty = np.zeros((0, 2), dtype='<u4')
    chunks = [empty]
    for i in range(len(rec)):
        chunks += [rec[i:i + 1]] + ([empty] if i % 7 == 0 else [])
    state, _ = _check(ops, chunks, 5, 7, what='one by one')
    again = ops.survey_events(_dev(empty), 5, 7, EDGES, flicker=BAND, state=state)
    assert torch.equal(again, state) and again.data_ptr() != state.data_ptr()
    fresh = ops.survey_events(_dev(empty), 5, 7, EDGES, flicker=BAND)
    assert fresh.cpu().tolist() == survey_ref.Survey(5, 7, EDGES, flicker=BAND).state()


def test_split_at_every_record_boundary(ops):
    rec = _lamps(300, 5, 7)                                      # more than one tile
    whole, _ = _check(ops, [rec], 5, 7, what='whole')
    for k in range(len(rec) + 1):
        state = _survey(ops, [rec[:k], rec[k:]], 5, 7)
        assert torch.equal(state, whole), f'split at {k}'


def test_small_workspaces_cut_a_chunk_into_pieces(ops):
    rec = _lamps(2_000, 5, 7)
    mask = np.zeros((5, 7), np.uint8)
    mask[0, 0] = 1
    _, _, least, _ = ops.survey_query(1, 5, 7, len(EDGES))
    _, _, three, _ = ops.survey_query(3 * TILE, 5, 7, len(EDGES))
    assert ops.survey_query(len(rec), 5, 7, len(EDGES))[2] > three > least
    whole, _ = _check(ops, [rec], 5, 7, mask=mask, what='one piece')
    for ws in (least, three, three + 100):                       # 8 pieces of a tile, 3 of three tiles
        state = _survey(ops, [rec], 5, 7, mask=mask, ws_bytes=ws)
        assert torch.equal(state, whole), ws
    with pytest.raises(_err()):
        ops.survey_events(_dev(rec), 5, 7, EDGES, ws_bytes=least - 1)


def test_masked_and_outside_events(ops):
    rec = _lamps(1_200, 5, 7, outside=0.2)
    mask = np.zeros((5, 7), np.uint8)
    mask[2, 2] = mask[2, 4] = mask[4, 6] = 1                     # both sides of the lamp pixel (3, 2)
    _, ref = _check(ops, np.array_split(rec, 3), 5, 7, mask=mask, what='mask')
    c = ref.counters()
    assert c['masked'] > 20 and c['outside'] > 100 and c['seen'] == c['candidates'] + c['masked'] + c['outside']
    state = _survey(ops, [rec], 5, 7, mask=mask.astype(bool))
    assert state.cpu().tolist() == ref.state()


def test_without_a_band_run_stays_empty(ops):
    rec = _lamps(600, 5, 7)
    _, ref = _check(ops, [rec], 5, 7, band=None, what='no band')
    assert ref.counters()['run'].sum() == 0 and ref.counters()['period'].sum() > 0


def test_a_decreasing_time_is_an_error_and_the_state_stays(ops):
    rec = _lamps(600, 5, 7)
    state = _survey(ops, [rec[:300]], 5, 7)
    kept = state.clone()
    bad = rec[300:].copy()
    bad[200, 0] = bad[199, 0] - 1                                # inside the chunk
    with pytest.raises(ops.EventOrderError) as info:
        ops.survey_events(_dev(bad), 5, 7, EDGES, flicker=BAND, state=state)
    assert (info.value.position, info.value.t_before, info.value.t_at) == (200, int(bad[199, 0]), int(bad[199, 0]) - 1)
    assert torch.equal(state, kept)
    with pytest.raises(ops.EventOrderError) as info:             # against the chunk before
        ops.survey_events(_dev(rec[299:]), 5, 7, EDGES, flicker=BAND, state=_survey(ops, [rec[:300], rec[300:400]], 5, 7))
    assert (info.value.position, info.value.t_before, info.value.t_at) == (0, int(rec[399, 0]), int(rec[299, 0]))
    after = ops.survey_events(_dev(rec[300:]), 5, 7, EDGES, flicker=BAND, state=state)      # the state is as good as before
    assert torch.equal(after, _survey(ops, [rec], 5, 7)) and torch.equal(state, kept)


def test_argument_checks(ops):
    rec = _dev(_lamps(100, 5, 7))
    for edges in ([], list(range(65)), [5, 5], [9, 3], [-1], [2 ** 31], [1.5], [True], None):
        with pytest.raises(_err()):
            ops.survey_events(rec, 5, 7, edges)
    for flicker in ((0, 5), (9, 5), (5, 2 ** 31), (5,), (350, 450, 3), 'x'):
        with pytest.raises(_err()):
            ops.survey_events(rec, 5, 7, EDGES, flicker=flicker)
    state = ops.survey_events(rec, 5, 7, EDGES)
    with pytest.raises(_err()):
        ops.survey_events(rec, 5, 7, EDGES[:-1], state=state)    # another number of edges: another state block
    with pytest.raises(_err()):
        ops.survey_events(rec, 5, 8, EDGES, state=state)
    with pytest.raises(_err()):
        ops.survey_events(rec[:-1], 5, 7, EDGES)
    with pytest.raises(_err()):
        ops.survey_events(rec, 5, 7, EDGES, pixel_mask=torch.zeros((5, 8), dtype=torch.uint8, device=DEV))
    with pytest.raises(_err()):
        ops.survey_counters(state, len(EDGES) + 1)
    with pytest.raises(_err()):
        ops.survey_counters(state, 0)


def test_a_recording_through_the_command_line_s_reader(ops, tmp_path):
    """A small Gen1 ``.dat`` file through ``survey_recording`` -- the ingestion's chunk reader, three chunks -- against the restatement."""
    from leod_amd.data import survey
    from leod_amd.data.utils import dat_events
    h, w = 240, 304
    rec = pr.lamp_stream(np.random.RandomState(8), 2_000, 24, 24, lamps=[(10, 5)], period=2_000, jitter=20, clear_lamps=True)
    rec[[100, 1_400], 1] = 310 | (5 << 14)                       # beyond the sensor
    mask = np.zeros((h, w), np.uint8)
    mask[3, 4] = 1
    dat_events.write_dat(str(tmp_path / 'a_td.dat'), rec, h, w)
    rep = survey.survey_recording(str(tmp_path / 'a_td.dat'), 'gen1', edges_us=[50, 500, 5_000], anti_flicker='400:600', pixel_mask=mask,
                                  hot_rates=[100, 10 ** 6], raw_chunk_bytes=8 * 700)
    ref = survey_ref.Survey(h, w, [50, 500, 5_000], flicker=(1_667, 2_500), mask=mask)
    ref.feed(rec)
    c = ref.counters()
    assert {k: rep[k] for k in survey_ref.HEAD} == {k: c[k] for k in survey_ref.HEAD} and rep['masked'] > 0 and rep['outside'] >= 2
    for k in ('nb', 'same', 'sec_on', 'sec_off', 'period', 'run'):
        assert rep['histograms'][k] == c[k].tolist(), k
    assert rep['removed']['flicker_by_lock'][2] == int(c['run'][3:].sum()) > 0
    assert rep['hot_pixels'] == {'100': rep['hot_pixels']['100'], '1000000': 0} and rep['hot_pixels']['100'] >= 1


# ---- 200 000 events on 32 x 32: the identities against the filters themselves

BIG_HW = (32, 32)
BIG_BAND = (9_000, 11_000)                                       # the lamps' period of 10 000 us, jittered by at most 200
BIG_AT = (1, 8, 15)                                              # 200, 5 000 and 100 000 us of the default edges
BIG_LOCKS = (1, 3, 200)


@pytest.fixture(scope='module')
def big(ops):
    from leod_amd.data.survey import DEFAULT_EDGES_US
    from leod_amd.data.utils.event_filter import survey_responses
    edges = list(DEFAULT_EDGES_US)
    rec = pr.lamp_stream(np.random.RandomState(9), 200_000, *BIG_HW, lamps=[(5, 6), (20, 17), (31, 31)], jitter=100, clear_lamps=True)
    mask = np.zeros(BIG_HW, np.uint8)
    mask[3, 3] = mask[10, 30] = mask[0, 0] = 1
    dev, mask_dev = _dev(rec), _mask_dev(mask)
    first = ops.survey_events(dev[:8 * 120_000], *BIG_HW, edges, flicker=BIG_BAND, pixel_mask=mask_dev)
    held = first.clone()
    state = ops.survey_events(dev[8 * 120_000:], *BIG_HW, edges, flicker=BIG_BAND, state=first, pixel_mask=mask_dev)
    assert torch.equal(first, held)                              # the state passed in is not modified
    c = ops.survey_counters(state, len(edges))
    return dict(rec=dev, mask=mask_dev, edges=edges, state=state, counters=c, responses=survey_responses(c, edges))


def test_big_case_is_not_empty(big):
    c = big['counters']
    assert c['seen'] == 200_000 and min(c['candidates'], c['outside'], c['masked']) > 0
    assert c['seen'] == c['candidates'] + c['outside'] + c['masked'] and 0 <= c['t_first'] < c['t_last']
    for k in ('nb', 'same', 'sec_on', 'sec_off', 'period', 'run'):
        assert c[k].sum() > 0 and c[k].min() >= 0, k
    assert c['nb'].sum() == c['candidates'] == c['run'].sum()
    assert np.count_nonzero(c['nb']) >= 16 and np.count_nonzero(c['same']) >= 16 and c['run'][255] > 0


def test_big_case_two_runs_are_byte_identical(ops, big):
    again = ops.survey_events(big['rec'], *BIG_HW, big['edges'], flicker=BIG_BAND, pixel_mask=big['mask'])
    assert torch.equal(again, big['state'])                      # one chunk or two, first run or second


@pytest.mark.parametrize('b', BIG_AT)
def test_big_case_activity_identity(ops, big, b):
    _, fstate = ops.filter_events(big['rec'], *BIG_HW, big['edges'][b], pixel_mask=big['mask'])
    got = ops.event_filter_counters(fstate)
    assert got['unsupported'] > 0 and got['unsupported'] == big['responses']['denoise'][b]
    assert got['seen'] - got['outside'] - got['masked'] == big['counters']['candidates']


@pytest.mark.parametrize('keep,curve', [('first', 'trail'), ('from_second', 'stc'), ('second', 'stc_cut_trail')])
@pytest.mark.parametrize('b', BIG_AT)
def test_big_case_burst_identities(ops, big, b, keep, curve):
    _, pstate = ops.pixel_filter_events(big['rec'], *BIG_HW, burst_us=big['edges'][b], burst_keep=keep, pixel_mask=big['mask'])
    got = ops.pixel_filter_counters(pstate)
    assert got['burst'] > 0 and got['kept'] > 0 and got['burst'] == big['responses'][curve][b]


@pytest.mark.parametrize('lock', BIG_LOCKS)
def test_big_case_flicker_identity(ops, big, lock):
    _, pstate = ops.pixel_filter_events(big['rec'], *BIG_HW, flicker=BIG_BAND + (lock,), pixel_mask=big['mask'])
    got = ops.pixel_filter_counters(pstate)
    assert got['flicker'] > 0 and got['flicker'] == big['responses']['flicker'][lock]
