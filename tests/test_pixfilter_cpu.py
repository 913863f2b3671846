"""The per-pixel event filters without a GPU: the sequential restatement (tests/pixfilter_ref.py) against the transcription "by the
sentence" on random streams, hand-written streams that say what they show, and the host-side option checks of the ingestion."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixfilter_ref as pr  # noqa: E402
from pixfilter_ref import records as R  # noqa: E402

HH, HW = 4, 5                                                    # the hand-written streams' sensor: 4 rows, 5 columns
BAND = (8_000, 12_500, 3)
TAU = 4_000


def random_case(seed, n, clear_lamps=None):
    """The generator of the GPU tests on a 12 x 16 sensor: two lamps, 5 % of the pixels masked (never a lamp), 3 % of the events outside.
    Below 4000 events the stream spans only a few lamp cycles and one background hit on a lamp pixel can keep it from ever locking
    (n = 1500: no flicker event at all in two seeds of six), so there the background stays off the lamp pixels (``clear_lamps`` None);
    from 4000 on it hits them, and they lock, unlock and lock again."""
    rng = np.random.RandomState(seed)
    clear_lamps = n < 4000 if clear_lamps is None else clear_lamps
    lamps = ((3, 2), (11, 9))
    rec = pr.lamp_stream(rng, n, 12, 16, lamps if n >= 300 else (), clear_lamps=clear_lamps)
    mask = rng.rand(12, 16) < 0.05
    mask[0, 0] = True
    for lx, ly in lamps:
        mask[ly, lx] = False
    return rec, mask


def _restated(rec, h, w, mask=None, split=None, **kw):
    f = pr.PixelFilter(h, w, mask=mask, **kw)
    if split is None:
        kept = f.feed(rec)
    else:
        kept = np.concatenate([f.feed(rec[:split]), f.feed(rec[split:])])
    return kept, f


@pytest.mark.parametrize('keep', pr.KEEP)
@pytest.mark.parametrize('flicker', [None, BAND])
@pytest.mark.parametrize('n', [40, 300, 1500])
def test_restatement_against_the_transcription(keep, flicker, n):
    for seed in range(3):
        rec, mask = random_case(seed, n)
        kept, f = _restated(rec, 12, 16, mask, burst_us=TAU, burst_keep=keep, flicker=flicker)
        idx, counts = pr.by_the_sentence(rec, 12, 16, TAU, keep, flicker, mask)
        assert np.array_equal(kept, rec[idx]) and f.counters() == counts
        c = f.counters()
        assert c['seen'] == n == c['kept'] + c['outside'] + c['masked'] + c['flicker'] + c['burst']
        if n > 1000:                                             # the streams are not vacuous
            assert min(c['kept'], c['outside'], c['masked'], c['burst']) > 0, c
            assert flicker is None or c['flicker'] > 0, c
    # the families alone and tau = 0
    rec, mask = random_case(7, 600)
    for kw in (dict(burst_us=None, flicker=BAND), dict(burst_us=0, burst_keep=keep), dict()):
        kept, f = _restated(rec, 12, 16, mask, **kw)
        idx, counts = pr.by_the_sentence(rec, 12, 16, mask=mask, **kw)
        assert np.array_equal(kept, rec[idx]) and f.counters() == counts


def test_the_counts_of_the_generator():
    """n = 1500 (60 ms, six lamp cycles): with the background on the lamp pixels a handful of flicker events or none, with it kept off
    them locking is certain; bursts by the hundred.  n = 6000: every counter is positive either way."""
    for seed in range(3):
        rec, mask = random_case(seed, 1500, clear_lamps=False)
        first = _restated(rec, 12, 16, mask, burst_us=TAU, burst_keep='first', flicker=BAND)[1].counters()
        second = _restated(rec, 12, 16, mask, burst_us=TAU, burst_keep='second', flicker=BAND)[1].counters()
        assert 0 <= first['flicker'] <= 25 and first['flicker'] == second['flicker']
        assert 100 < first['burst'] < 600 and 900 < second['burst'] < 1450
        rec, mask = random_case(seed, 1500)
        assert _restated(rec, 12, 16, mask, flicker=BAND)[1].counters()['flicker'] >= 8
        for clear in (False, True):
            rec, mask = random_case(seed, 6000, clear_lamps=clear)
            c = _restated(rec, 12, 16, mask, burst_us=TAU, burst_keep='from_second', flicker=BAND)[1].counters()
            assert min(c.values()) > 0 and c['flicker'] > 30, c


def test_splitting_changes_nothing():
    rec, mask = random_case(3, 400)
    whole, f = _restated(rec, 12, 16, mask, burst_us=TAU, burst_keep='from_second', flicker=BAND)
    for split in (0, 1, 77, 399, 400):
        kept, g = _restated(rec, 12, 16, mask, split=split, burst_us=TAU, burst_keep='from_second', flicker=BAND)
        assert np.array_equal(kept, whole) and g.state() == f.state()


# ---- hand-written streams on a 5 x 4 sensor -------------------------------------------------------------------------------------------------
# (name, keyword arguments, events (t, x, y, p), mask pixels (x, y), the verdict on every event: K kept, B burst, F flicker, M masked,
# O outside)
FL = (90, 110, 2)                                                # band 90..110 us, lock after 2 periods
HAND = [
    ('a trail keeps the first of a burst', dict(burst_us=10),
     [(0, 1, 1, 1), (5, 1, 1, 1), (15, 1, 1, 1), (100, 1, 1, 1)], (), 'KBBK'),
    ('a gap of exactly tau connects, tau + 1 does not', dict(burst_us=10),
     [(0, 2, 0, 0), (10, 2, 0, 0), (21, 2, 0, 0)], (), 'KBK'),
    ('a polarity change restarts', dict(burst_us=10),
     [(0, 0, 3, 1), (2, 0, 3, 0), (4, 0, 3, 0), (6, 0, 3, 1)], (), 'KKBK'),
    ('bursts belong to their pixel', dict(burst_us=10),
     [(0, 0, 0, 1), (1, 1, 0, 1), (2, 0, 0, 1), (3, 1, 0, 1)], (), 'KKBB'),
    ('second: the second of a burst of 4 alone', dict(burst_us=10, burst_keep='second'),
     [(0, 4, 3, 1), (3, 4, 3, 1), (6, 4, 3, 1), (9, 4, 3, 1), (50, 4, 3, 1)], (), 'BKBBB'),
    ('from_second: a burst of 4 from its second on', dict(burst_us=10, burst_keep='from_second'),
     [(0, 4, 3, 1), (3, 4, 3, 1), (6, 4, 3, 1), (9, 4, 3, 1), (50, 4, 3, 1)], (), 'BKKKB'),
    ('tau = 0 connects equal times only', dict(burst_us=0),
     [(5, 1, 2, 1), (5, 1, 2, 1), (6, 1, 2, 1)], (), 'KBK'),
    ('equal times order by position', dict(burst_us=10, burst_keep='second'),
     [(7, 3, 3, 0), (7, 3, 3, 0), (7, 3, 3, 0)], (), 'BKB'),
    ('lock after exactly `lock` in-band periods; then both polarities go', dict(flicker=FL),
     [(0, 2, 2, 1), (50, 2, 2, 0), (100, 2, 2, 1), (150, 2, 2, 0), (200, 2, 2, 1), (250, 2, 2, 0), (300, 2, 2, 1)], (), 'KKKKFFF'),
    ('periods of exactly p_min and p_max are in band', dict(flicker=FL),
     [(0, 0, 1, 1), (40, 0, 1, 0), (90, 0, 1, 1), (100, 0, 1, 0), (200, 0, 1, 1), (201, 0, 1, 0)], (), 'KKKKFF'),
    ('a period of p_min - 1 resets', dict(flicker=FL),
     [(0, 0, 1, 1), (40, 0, 1, 0), (100, 0, 1, 1), (140, 0, 1, 0), (189, 0, 1, 1), (230, 0, 1, 0), (289, 0, 1, 1), (300, 0, 1, 0),
      (389, 0, 1, 1)], (), 'KKKKKKKKF'),
    ('a period of p_max + 1 resets', dict(flicker=FL),
     [(0, 0, 1, 1), (40, 0, 1, 0), (100, 0, 1, 1), (140, 0, 1, 0), (211, 0, 1, 1), (250, 0, 1, 0), (311, 0, 1, 1)], (), 'KKKKKKK'),
    ('a non-edge event later than p_max unlocks and is itself kept', dict(flicker=FL),
     [(0, 3, 0, 1), (50, 3, 0, 0), (100, 3, 0, 1), (150, 3, 0, 0), (200, 3, 0, 1), (250, 3, 0, 0), (311, 3, 0, 0), (320, 3, 0, 0)], (),
     'KKKKFFKK'),
    ('a stray ON event between two edges is no edge; a stray OFF-ON pair unlocks', dict(flicker=FL),
     [(0, 3, 0, 1), (50, 3, 0, 0), (100, 3, 0, 1), (120, 3, 0, 1), (150, 3, 0, 0), (200, 3, 0, 1), (230, 3, 0, 0), (240, 3, 0, 1),
      (250, 3, 0, 0)], (), 'KKKKKFFKK'),
    ('flicker is tested before burst, and a removed event still counts in its burst', dict(burst_us=10, flicker=FL),
     [(0, 1, 3, 1), (50, 1, 3, 0), (100, 1, 3, 1), (150, 1, 3, 0), (200, 1, 3, 1), (205, 1, 3, 1), (316, 1, 3, 0), (320, 1, 3, 0)], (),
     'KKKKFFKB'),
    ('masked and outside events touch no state', dict(burst_us=10, flicker=FL),
     [(0, 4, 0, 1), (1, 9, 0, 1), (2, 4, 9, 1), (3, 2, 1, 1), (4, 4, 0, 1), (5, 2, 1, 1)], ((2, 1),), 'KOOMBM'),
    ('a masked pixel never locks or bursts: its state stays initial', dict(burst_us=10, burst_keep='from_second'),
     [(0, 2, 1, 1), (1, 2, 1, 1), (2, 1, 1, 1)], ((2, 1),), 'MMB'),
    ('both families off: bounds and mask are the whole rule', dict(),
     [(0, 4, 3, 1), (0, 5, 3, 1), (0, 4, 4, 0), (1, 0, 0, 1), (1, 4, 3, 1)], ((0, 0),), 'KOOMK'),
]
LETTER = dict(K='kept', B='burst', F='flicker', M='masked', O='outside')


def hand_case(case):
    name, kw, ev, mask_px, verdict = case
    rec = R(*(np.array([e[k] for e in ev]) for k in range(4)))
    mask = None
    if mask_px:
        mask = np.zeros((HH, HW), dtype=np.uint8)
        for mx, my in mask_px:
            mask[my, mx] = 1
    want = rec[[i for i, v in enumerate(verdict) if v == 'K']]
    counts = dict(seen=len(ev), kept=0, outside=0, masked=0, flicker=0, burst=0)
    for v in verdict:
        counts[LETTER[v]] += 1
    return rec, mask, kw, want, counts


@pytest.mark.parametrize('case', HAND, ids=[c[0] for c in HAND])
def test_hand_written_streams(case):
    rec, mask, kw, want, counts = hand_case(case)
    assert len(case[4]) == len(rec)
    kept, f = _restated(rec, HH, HW, mask, **kw)
    assert np.array_equal(kept, want), (case[0], kept[:, 0].tolist())
    assert f.counters() == counts
    idx, c2 = pr.by_the_sentence(rec, HH, HW, mask=mask, **kw)
    assert np.array_equal(rec[idx], want) and c2 == counts


def test_the_state_block():
    f = pr.PixelFilter(1, 2, burst_us=10, flicker=(5, 20, 2))
    assert f.state() == [0, 0, 0, 0, 0, 0, -1, 0, -1, -1, 0, 0, -1, -1, 0, 0]
    f.feed(R([3, 4, 5, 12, 13], [1, 1, 1, 1, 7], [0, 0, 0, 0, 0], [1, 1, 0, 1, 0]))
    # pixel 1: ON 3 (edge), ON 4 (k = 2, removed), OFF 5, ON 12 (edge, period 9 in band: n_per 1); the last event is outside
    assert f.state() == [5, 3, 1, 0, 0, 1, 13, 0, -1, -1, 0, 0, 12, 12, 1 + 2 * 1, 1]


def test_a_decreasing_time_is_refused_before_anything_changes():
    f = pr.PixelFilter(HH, HW, burst_us=5)
    f.feed(R([5, 9], [0, 0], [0, 0]))
    before = f.state()
    with pytest.raises(pr.OrderError) as e:
        f.feed(R([9, 10, 8], [1, 1, 1], [0, 0, 0]))
    assert (e.value.position, e.value.t_before, e.value.t_at) == (2, 10, 8) and f.state() == before
    with pytest.raises(pr.OrderError) as e:
        f.feed(R([8], [1], [0]))
    assert (e.value.position, e.value.t_before, e.value.t_at) == (0, 9, 8)


# ---- the options of the ingestion -------------------------------------------------------------------------------------------------------------
def test_flicker_band():
    from leod_amd.data.utils import event_filter as ef
    assert ef.flicker_band('80:125') == (8000, 12500) == ef.flicker_band((80, 125))
    assert ef.flicker_band('50:120') == (8334, 20000)            # ceil(10^6 / 120), floor(10^6 / 50)
    assert ef.flicker_band('1:1000000') == (1, 1_000_000) and ef.flicker_band('3:4') == (250_000, 333_333)
    assert ef.flicker_band('1000000:1000000') == (1, 1)
    for bad in ('3:3', '0:10', '10:5', '5:1000001', '50', '50:60:70', 'a:b', '50.5:60', '-5:60', (50.0, 60), (True, 60), 50, None):
        with pytest.raises(ValueError):
            ef.flicker_band(bad)


def test_option_checks():
    from leod_amd.data import ingest
    chk = ingest.check_pixel_filter_options
    assert chk() is None and chk(stc_cut_trail=False) is None
    assert chk(trail_us=3000) == dict(burst_us=3000, burst_keep='first', flicker=None)
    assert chk(stc_us=0) == dict(burst_us=0, burst_keep='from_second', flicker=None)
    assert chk(stc_us=7, stc_cut_trail=True) == dict(burst_us=7, burst_keep='second', flicker=None)
    assert chk(anti_flicker='50:120') == dict(burst_us=None, burst_keep='first', flicker=(8334, 20000, 3))
    assert chk(trail_us=1, anti_flicker=(80, 125), flicker_lock=255)['flicker'] == (8000, 12500, 255)
    for kw in (dict(trail_us=1, stc_us=1), dict(trail_us=-1), dict(trail_us=2 ** 31), dict(stc_us=1.5), dict(trail_us=True),
               dict(stc_cut_trail=True), dict(trail_us=5, stc_cut_trail=True), dict(anti_flicker='3:3'), dict(anti_flicker='100:50'),
               dict(anti_flicker='50:120', flicker_lock=0), dict(anti_flicker='50:120', flicker_lock=256), dict(flicker_lock=3),
               dict(anti_flicker='50:120', flicker_lock=2.0)):
        with pytest.raises(ValueError):
            chk(**kw)
    # they are checked before anything is opened: the recording does not exist
    for fn in (ingest.ingest_recording, ):
        with pytest.raises(ValueError, match='anti_flicker'):
            fn('/nonexistent/a_td.dat', None, '/nonexistent/out', 'gen1', anti_flicker='3:3')
    with pytest.raises(ValueError, match='one burst rule'):
        ingest.ingest_split('/nonexistent/src', '/nonexistent/dst', 'gen1', trail_us=1, stc_us=1)
    with pytest.raises(SystemExit):
        ingest.main(['/nonexistent/src', '/nonexistent/dst', '--dataset', 'gen1', '--trail-us', '5', '--stc-us', '5'])
    with pytest.raises(SystemExit):
        ingest.main(['/nonexistent/src', '/nonexistent/dst', '--dataset', 'gen1', '--anti-flicker', '3:3'])


def test_check_filter_options_is_unchanged():
    from leod_amd.data import ingest
    import inspect
    assert list(inspect.signature(ingest.check_filter_options).parameters) == ['dataset_type', 'denoise_us', 'pixel_mask', 'hot_rate_hz']
    assert ingest.check_filter_options('gen1') is None
    assert ingest.check_filter_options('gen1', denoise_us=5, hot_rate_hz=100) == dict(tau_us=5, mask=None, hot_rate_hz=100)
    got = ingest.check_filter_options('gen1', pixel_mask=np.ones((240, 304), dtype=bool))
    assert sorted(got) == ['hot_rate_hz', 'mask', 'tau_us'] and got['tau_us'] is None and got['mask'].dtype == np.uint8
