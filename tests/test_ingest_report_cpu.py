"""The report of the streaming route of the ingestion (``ingest._report_fragment``, the arithmetic behind ``_FilterChain.report``) on
hand-written counter dictionaries, for every combination of stages: no filter, the activity filter alone, the per-pixel filters alone,
both.  No device: the counters are those the ops' states would hold."""
import pytest
import torch

from leod_amd.data import ingest

DECODER = dict(events=100, early_events=3, ignored_words=5, unknown_words=1, overflow=0, wraps=2)       # of a .raw file
NO_DECODER = dict(events=0, early_events=0, ignored_words=0, unknown_words=0, overflow=0, wraps=0)      # of a .dat file
BASE_KEYS = {'frames', 'dropped_events', 'events', 'early_events', 'ignored_words', 'unknown_words', 'overflow', 'wraps'}
FILTER_KEYS = BASE_KEYS | {'kept_events', 'masked_events', 'unsupported_events'}
PIXEL_KEYS = FILTER_KEYS | {'flicker_events', 'burst_events'}
PIX = dict(seen=100, kept=50, outside=4, masked=10, flicker=16, burst=20)


def _adds_up(frag):
    """Every event seen is kept or counted by exactly one reason.  Without a filter nothing is counted but the voxeliser's drops: what
    reaches the frames is the rest."""
    kept = frag.get('kept_events', frag['events'] - frag['dropped_events'])
    return kept + frag.get('flicker_events', 0) + frag.get('burst_events', 0) + frag.get('masked_events', 0) + \
        frag.get('unsupported_events', 0) + frag['dropped_events'] == frag['events']


def test_no_filter_is_the_decoder_and_the_voxeliser():
    frag = ingest._report_fragment(7, 4, DECODER)
    assert frag == dict(frames=7, dropped_events=4, events=100, early_events=3, ignored_words=5, unknown_words=1, overflow=0, wraps=2)
    assert set(frag) == BASE_KEYS and _adds_up(frag)


@pytest.mark.parametrize('decoder', [DECODER, NO_DECODER], ids=['raw', 'dat'])
def test_activity_filter_alone(decoder):
    fc = dict(seen=100, kept=60, outside=4, masked=10, unsupported=26)
    frag = ingest._report_fragment(7, 0, decoder, first='activity', tau_on=True, activity=fc)
    assert set(frag) == FILTER_KEYS
    assert frag == dict(decoder, frames=7, events=100, dropped_events=4, kept_events=60, masked_events=10, unsupported_events=26)
    assert _adds_up(frag)
    # a mask without tau_us: the same stage, nothing is unsupported
    frag = ingest._report_fragment(7, 0, decoder, first='activity', tau_on=False,
                                   activity=dict(seen=100, kept=86, outside=4, masked=10, unsupported=0))
    assert frag == dict(decoder, frames=7, events=100, dropped_events=4, kept_events=86, masked_events=10, unsupported_events=0)
    assert _adds_up(frag)


def test_the_voxeliser_s_drops_join_the_first_stage_s():
    frag = ingest._report_fragment(2, 3, NO_DECODER, first='activity', tau_on=True,
                                   activity=dict(seen=10, kept=4, outside=1, masked=0, unsupported=5))
    assert frag['dropped_events'] == 4 and frag['kept_events'] == 4 and frag['events'] == 10


def test_pixel_filters_alone():
    frag = ingest._report_fragment(7, 0, DECODER, first='pixel', tau_on=False, pixel=PIX)
    assert set(frag) == PIXEL_KEYS
    assert frag == dict(DECODER, frames=7, events=100, dropped_events=4, kept_events=50, masked_events=10, unsupported_events=0,
                        flicker_events=16, burst_events=20)
    assert _adds_up(frag)


def test_pixel_filters_then_the_activity_filter():
    fc = dict(seen=50, kept=30, outside=0, masked=0, unsupported=20)       # the second stage saw what the first one kept
    frag = ingest._report_fragment(7, 0, DECODER, first='pixel', tau_on=True, activity=fc, pixel=PIX)
    assert set(frag) == PIXEL_KEYS
    assert frag == dict(DECODER, frames=7, events=100, dropped_events=4, kept_events=30, masked_events=10, unsupported_events=20,
                        flicker_events=16, burst_events=20)
    assert _adds_up(frag)
    # tau_us is set but the first stage never kept a record: the second one has no state, and nothing reached the voxeliser
    none_kept = dict(seen=100, kept=0, outside=4, masked=10, flicker=16, burst=70)
    frag = ingest._report_fragment(7, 0, DECODER, first='pixel', tau_on=True, activity=None, pixel=none_kept)
    assert frag == dict(DECODER, frames=7, events=100, dropped_events=4, kept_events=0, masked_events=10, unsupported_events=0,
                        flicker_events=16, burst_events=70)
    assert _adds_up(frag)


@pytest.mark.parametrize('first,tau_on,keys', [(None, False, BASE_KEYS), ('activity', True, FILTER_KEYS), ('activity', False, FILTER_KEYS),
                                               ('pixel', False, PIXEL_KEYS), ('pixel', True, PIXEL_KEYS)])
def test_a_recording_of_zero_events_has_no_state_yet_and_reports_zeros(first, tau_on, keys):
    frag = ingest._report_fragment(1, 0, NO_DECODER, first=first, tau_on=tau_on)
    assert set(frag) == keys
    assert frag == dict({k: 0 for k in keys}, frames=1)
    assert _adds_up(frag)


def test_the_order_error_reads_as_it_always_did(monkeypatch):
    from leod_amd import ops
    want = 'rec_td.dat: timestamps decrease (5 -> 3); a recording must be sorted in time'
    e = ingest._order_error('rec_td.dat', 5, 3)
    assert isinstance(e, ValueError) and str(e) == want

    def refuse(*a, **kw):
        raise ops.EventOrderError(7, 5, 3)
    monkeypatch.setattr(ops, 'filter_events', refuse)
    monkeypatch.setattr(ops, 'pixel_filter_events', refuse)
    rec = torch.zeros((2, 8), dtype=torch.uint8)
    for pixel in (None, dict(burst_us=10, burst_keep='first', flicker=None)):
        chain = ingest._FilterChain(dict(tau_us=5, mask=None, pixel=pixel), (4, 4), 'cpu', 'rec_td.dat')
        with pytest.raises(ValueError) as info:
            chain(rec)
        assert str(info.value) == want and not isinstance(info.value, ops.EventOrderError)
