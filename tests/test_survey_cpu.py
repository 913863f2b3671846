"""The filter survey without a GPU: the sequential restatement (tests/survey_ref.py) against the five identities,
with the filters' own restatements run once per edge, per ``burst_keep`` and per lock; ``event_filter.survey_responses`` on hand-made
counters; the option checks and the command line of ``leod_amd.data.survey`` with the op replaced by the restatement."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import filter_ref                                                # noqa: E402
import pixfilter_ref                                             # noqa: E402
import survey_ref                                                # noqa: E402
from leod_amd.data import survey                                 # noqa: E402
from leod_amd.data.utils import dat_events, event_filter as ef   # noqa: E402

H, W = 6, 7
EDGES = [0, 40, 200, 390, 410, 2_000, 50_000]
LOCKS = (1, 2, 3, 7, 255)
# name -> (lamp_stream keywords, band)
STREAMS = {
    'slow_lamps': (dict(lamps=[(2, 3), (5, 0)], period=2_000, jitter=60), (1_900, 2_100)),
    'fast_lamp': (dict(lamps=[(3, 2)], period=400, jitter=10, clear_lamps=True), (350, 450)),
}


def _mask():
    m = np.zeros((H, W), np.uint8)
    m[1, 1] = m[4, 6] = 1
    return m


@pytest.fixture(scope='module', params=sorted(STREAMS))
def case(request):
    kw, band = STREAMS[request.param]
    rec = pixfilter_ref.lamp_stream(np.random.RandomState(11), 3_000, H, W, outside=0.05, **kw)
    t, x, y, _ = filter_ref.unpack(rec)
    assert np.any(t[1:] == t[:-1]) and np.any(x >= W) and np.any(_mask()[np.minimum(y, H - 1), np.minimum(x, W - 1)][x < W] == 1)
    sv = survey_ref.Survey(H, W, EDGES, flicker=band, mask=_mask())
    for part in np.array_split(rec, [0, 1, 700, 701, 2_500]):    # pieces, an empty one and single events among them
        sv.feed(part)
    return rec, band, sv


def test_split_stream_gives_the_state_of_one_piece(case):
    rec, band, sv = case
    whole = survey_ref.Survey(H, W, EDGES, flicker=band, mask=_mask())
    whole.feed(rec)
    assert whole.state() == sv.state()
    assert len(sv.state()) == 8 + 5 * len(EDGES) + 262 + 4 * H * W


def test_head_and_histogram_totals(case):
    rec, band, sv = case
    c = sv.counters()
    t, x, y, _ = filter_ref.unpack(rec)
    assert c['seen'] == len(rec) and c['seen'] == c['candidates'] + c['outside'] + c['masked']
    assert c['outside'] == int(np.sum((x >= W) | (y >= H))) and c['masked'] > 0
    assert (c['t_first'], c['t_last']) == (int(t[0]), int(t[-1]))
    assert c['nb'].sum() == c['candidates'] == c['run'].sum()
    assert all(c[k].min() >= 0 for k in ('nb', 'same', 'sec_on', 'sec_off', 'period', 'run'))
    assert c['same'].sum() > 0 and c['sec_on'].sum() > 0 and c['sec_off'].sum() > 0 and c['period'].sum() > 0


def test_activity_identity_at_every_edge(case):
    rec, _, sv = case
    resp = ef.survey_responses(sv.counters(), EDGES)
    for b, e in enumerate(EDGES):
        f = filter_ref.Filter(H, W, e, mask=_mask())
        f.feed(rec)
        assert f.counters()['unsupported'] == resp['denoise'][b], (b, e)
    assert resp['denoise'][0] > resp['denoise'][-1] > 0


@pytest.mark.parametrize('keep,curve', [('first', 'trail'), ('from_second', 'stc'), ('second', 'stc_cut_trail')])
def test_burst_identities_at_every_edge(case, keep, curve):
    rec, _, sv = case
    resp = ef.survey_responses(sv.counters(), EDGES)
    got = []
    for b, e in enumerate(EDGES):
        f = pixfilter_ref.PixelFilter(H, W, burst_us=e, burst_keep=keep, mask=_mask())
        f.feed(rec)
        got.append(f.counters()['burst'])
        assert got[-1] == resp[curve][b], (keep, b, e)
    assert len(set(got)) > 2                                     # the curve moves over the edges: the case is not empty


def test_flicker_identity_at_the_locks(case):
    rec, band, sv = case
    resp = ef.survey_responses(sv.counters(), EDGES)
    got = {}
    for lock in LOCKS:
        f = pixfilter_ref.PixelFilter(H, W, flicker=(band[0], band[1], lock), mask=_mask())
        f.feed(rec)
        got[lock] = f.counters()['flicker']
        assert got[lock] == resp['flicker'][lock], lock
    assert got[1] > got[7] > 0
    assert resp['flicker'][0] == 0 and np.all(np.diff(resp['flicker'][1:]) <= 0)


def test_the_fast_lamp_reaches_lock_255():
    kw, band = STREAMS['fast_lamp']
    rec = pixfilter_ref.lamp_stream(np.random.RandomState(11), 3_000, H, W, outside=0.05, **kw)
    sv = survey_ref.Survey(H, W, EDGES, flicker=band)
    sv.feed(rec)
    assert sv.counters()['run'][255] > 0


def test_without_a_band_run_stays_empty_and_the_rest_is_the_same(case):
    rec, band, sv = case
    plain = survey_ref.Survey(H, W, EDGES, mask=_mask())
    plain.feed(rec)
    a, b = plain.counters(), sv.counters()
    assert a['run'].sum() == 0
    for k in ('nb', 'same', 'sec_on', 'sec_off', 'period'):
        assert np.array_equal(a[k], b[k]), k


def test_a_decreasing_time_raises_before_anything_changes():
    sv = survey_ref.Survey(H, W, EDGES)
    sv.feed(filter_ref.records([5, 9], [1, 2], [1, 1], [1, 0]))
    before = sv.state()
    with pytest.raises(filter_ref.OrderError) as info:
        sv.feed(filter_ref.records([9, 8], [1, 2], [1, 1]))
    assert (info.value.position, info.value.t_before, info.value.t_at) == (1, 9, 8) and sv.state() == before
    with pytest.raises(filter_ref.OrderError) as info:
        sv.feed(filter_ref.records([8], [1], [1]))
    assert info.value.position == 0 and sv.state() == before


def test_by_hand():
    """Five events on a 1 x 3 sensor, edges 10 and 100: every histogram entry is worked out here."""
    #            t   x  p
    events = [(0, 0, 1),         # first of pixel 0: rising edge, no period; no earlier neighbour -> nb[3]
              (5, 1, 1),         # first of pixel 1; neighbour 0 fired 5 ago -> nb[0]
              (12, 0, 1),        # same polarity, d = 12 -> same[1]; c = 1 < INF, 1 < K: sec_on[1]; c' = INF: no sec_off; nb: 12 - 5 = 7 -> nb[0]
              (20, 0, 1),        # d = 8 -> same[0]; c = 0 < c' = 1: sec_on[0], sec_off[1]; nb: 20 - 5 = 15 -> nb[1]
              (400, 0, 0),       # polarity changes: c = INF; nb: 400 - 5 = 395 -> nb[2]
              (500, 0, 1)]       # rising edge, t_edge = 0: period 500 -> period[2]; c = INF; nb: 495 -> nb[2]
    t, x, p = zip(*events)
    sv = survey_ref.Survey(1, 3, [10, 100], flicker=(450, 550))
    sv.feed(filter_ref.records(t, x, [0] * len(t), p))
    c = sv.counters()
    assert c['nb'].tolist() == [2, 1, 2, 1]
    assert c['same'].tolist() == [1, 1, 0]
    assert c['sec_on'].tolist() == [1, 1, 0] and c['sec_off'].tolist() == [0, 1, 0]
    assert c['period'].tolist() == [0, 0, 1]
    assert c['run'][:3].tolist() == [5, 1, 0]                    # the period of 500 is in the band: the last event sees n_per = 1


def test_survey_responses_on_hand_made_counters():
    counters = dict(candidates=100, nb=[10, 20, 30, 5], same=[7, 11, 13], sec_on=[4, 6, 0], sec_off=[0, 3, 2],
                    run=[90, 6, 3, 1] + [0] * 252)
    r = ef.survey_responses(counters, [50, 500])
    assert r['denoise'].tolist() == [20 + 30 + 5, 30 + 5]
    assert r['trail'].tolist() == [7, 18]
    assert r['stc'].tolist() == [93, 82]
    assert r['stc_cut_trail'].tolist() == [100 - 4, 100 - (10 - 3)]
    assert r['flicker'][:5].tolist() == [0, 10, 4, 1, 0] and r['flicker'].shape == (256,)
    assert all(v.dtype == np.int64 for v in r.values())
    with pytest.raises(ValueError):
        ef.survey_responses(dict(counters, nb=[1, 2, 3]), [50, 500])
    with pytest.raises(ValueError):
        ef.survey_responses(dict(counters, same=np.zeros(3)), [50, 500])


def test_edge_list_checks():
    assert survey.check_edges([0]) == [0] and survey.check_edges(range(64)) == list(range(64))
    assert len(survey.DEFAULT_EDGES_US) == 16 and survey.check_edges(survey.DEFAULT_EDGES_US)[0] == 100
    assert survey.DEFAULT_EDGES_US[-1] == 100_000
    for bad in ([], list(range(65)), [5, 5], [7, 3], [-1], [2 ** 31], [1.5], [True], 7):
        with pytest.raises(ValueError):
            survey.check_edges(bad)


def test_option_checks(tmp_path):
    opt = survey.check_survey_options('gen1')
    assert opt == dict(edges=list(survey.DEFAULT_EDGES_US), band=None, mask=None, hot_rates=[])
    opt = survey.check_survey_options('gen1', [10, 20], '80:125', np.zeros((240, 304), bool), [100, 0])
    assert opt['band'] == (8_000, 12_500) and opt['mask'].dtype == np.uint8 and opt['hot_rates'] == [100, 0]
    np.save(tmp_path / 'm.npy', np.zeros((3, 3), np.uint8))
    for kw in (dict(anti_flicker='125:80'), dict(pixel_mask=str(tmp_path / 'm.npy')), dict(hot_rates=[-1]), dict(hot_rates=[2.5]),
               dict(edges_us=[3, 2])):
        with pytest.raises(ValueError):
            survey.check_survey_options('gen1', **kw)
    with pytest.raises(ValueError):
        survey.check_survey_options('gen7')


@pytest.fixture
def on_the_restatement(monkeypatch):
    """``leod_amd.data.survey`` with the device out of it: chunks of host tensors, the ops replaced by the restatement."""
    from leod_amd import ops
    made = {}

    def chunks(payload, encoding, raw_chunk_bytes, what):
        assert encoding == 'dat'
        step = max(int(raw_chunk_bytes) // 8, 1) * 8
        for pos in range(0, len(payload), step):
            yield torch.from_numpy(np.array(payload[pos:pos + step])).view(-1, 8)

    def survey_events(rec, height, width, edges_us, flicker=None, state=None, pixel_mask=None, ws_bytes=None):
        if state is None:
            made['sv'] = survey_ref.Survey(height, width, edges_us, flicker=flicker, mask=None if pixel_mask is None else pixel_mask.numpy())
        try:
            made['sv'].feed(rec.numpy().view('<u4'))
        except filter_ref.OrderError as e:
            raise ops.EventOrderError(e.position, e.t_before, e.t_at) from None
        return torch.tensor(made['sv'].state(), dtype=torch.int64)

    def event_pixel_counts(rec, height, width, counts=None):
        counts = torch.zeros((height, width), dtype=torch.int64) if counts is None else counts
        _, x, y, _ = filter_ref.unpack(rec.numpy().view('<u4'))
        inside = (x < width) & (y < height)
        np.add.at(counts.numpy(), (y[inside], x[inside]), 1)
        return counts, torch.tensor([int((~inside).sum())])

    monkeypatch.setattr(survey, '_record_chunks', chunks)
    monkeypatch.setattr(ops, 'survey_events', survey_events)
    monkeypatch.setattr(ops, 'survey_counters', lambda state, n_edges: made['sv'].counters())
    monkeypatch.setattr(ops, 'event_pixel_counts', event_pixel_counts)
    return made


def _tiny_recording(dirname):
    """600 events on a 16 x 16 corner of a Gen1 sensor (so that neighbours meet), two of them moved beyond the sensor."""
    rec = pixfilter_ref.lamp_stream(np.random.RandomState(3), 600, 16, 16, lamps=[(10, 5)], period=2_000, jitter=20, clear_lamps=True)
    rec[[100, 400], 1] = 310 | (5 << 14)
    dat_events.write_dat(os.path.join(dirname, 'a_td.dat'), rec, 240, 304)
    return rec


def test_command_line_on_a_tiny_recording(tmp_path, capsys, on_the_restatement, monkeypatch):
    rec = _tiny_recording(str(tmp_path))
    monkeypatch.setattr(survey, 'RAW_CHUNK_BYTES', 8 * 250)      # three chunks
    out_fn = str(tmp_path / 'rep.json')
    assert survey.main([str(tmp_path), '--dataset', 'gen1', '--edges-us', '50', '500', '5000', '--anti-flicker', '400:600',
                        '--hot-rates', '100', '1000000', '--out', out_fn]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    rep = json.loads(lines[0])
    assert json.load(open(out_fn)) == [rep]
    assert rep['recording'].endswith('a_td.dat') and rep['sensor'] == [240, 304] and rep['edges_us'] == [50, 500, 5000]
    assert rep['band_us'] == [1_667, 2_500] and rep['seen'] == 600 and rep['outside'] >= 2 and rep['masked'] == 0
    assert rep['candidates'] + rep['outside'] == 600
    assert 'applied alone to the unfiltered stream' in rep['note'] and 'combined ingestion' in rep['note']
    assert sorted(rep['histograms']) == ['nb', 'period', 'run', 'same', 'sec_off', 'sec_on']
    assert [len(rep['histograms'][k]) for k in ('nb', 'same', 'period', 'run')] == [5, 4, 4, 256]
    # the curves are those of the filters' restatements on the whole recording
    for b, e in enumerate(rep['edges_us']):
        f = filter_ref.Filter(240, 304, e)
        f.feed(rec)
        assert rep['removed']['denoise'][b] == f.counters()['unsupported']
        for keep, curve in (('first', 'trail'), ('from_second', 'stc'), ('second', 'stc_cut_trail')):
            p = pixfilter_ref.PixelFilter(240, 304, burst_us=e, burst_keep=keep)
            p.feed(rec)
            assert rep['removed'][curve][b] == p.counters()['burst']
    assert len(rep['removed']['flicker_by_lock']) == 255
    p = pixfilter_ref.PixelFilter(240, 304, flicker=(1_667, 2_500, 3))
    p.feed(rec)
    assert rep['removed']['flicker_by_lock'][2] == p.counters()['flicker'] > 0
    assert rep['hot_pixels']['1000000'] == 0 and rep['hot_pixels']['100'] >= 1


def test_command_line_refuses_bad_options_and_an_unsorted_recording(tmp_path, on_the_restatement):
    for argv in (['--edges-us', '5', '5'], ['--anti-flicker', '9'], ['--pixel-mask', str(tmp_path / 'none.txt')], ['--hot-rates', '-3']):
        with pytest.raises(SystemExit):
            survey.main([str(tmp_path), '--dataset', 'gen1'] + argv)
    with pytest.raises(SystemExit):                              # no recording under SRC
        survey.main([str(tmp_path), '--dataset', 'gen1'])
    dat_events.write_dat(str(tmp_path / 'b_td.dat'), filter_ref.records([5, 9, 8], [1, 2, 3], [1, 1, 1]), 240, 304)
    with pytest.raises(ValueError, match=r'timestamps decrease \(9 -> 8\)'):
        survey.main([str(tmp_path), '--dataset', 'gen1'])
    dat_events.write_dat(str(tmp_path / 'b_td.dat'), filter_ref.records([5], [1], [1]), 200, 304)
    with pytest.raises(ValueError, match='Height 200'):
        survey.main([str(tmp_path), '--dataset', 'gen1'])
