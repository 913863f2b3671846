"""The host side of the event noise filters: the tests' sequential restatement (tests/filter_ref.py) against the rule's sentence, the
hot-pixel threshold, the mask file, and the options of the ingestion up to the point where the device is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref  # noqa: E402

from leod_amd.data import ingest  # noqa: E402
from leod_amd.data.utils import event_filter as ef  # noqa: E402

H, W = 6, 8


def _stream(rng, n, t_max, outside=True):
    """n events on the 8 x 6 sensor with many equal times; some of them outside it."""
    t = np.sort(rng.randint(0, t_max + 1, n))
    x, y = rng.randint(0, W + (2 if outside else 0), n), rng.randint(0, H + (1 if outside else 0), n)
    return filter_ref.records(t, x, y, rng.randint(0, 2, n))


@pytest.mark.parametrize('tau', [0, 1, 7, 10_000])
def test_restatement_equals_the_rule_as_written(tau):
    rng = np.random.RandomState(100 + tau % 97)
    for trial in range(12):
        n = int(rng.randint(1, 301))
        # spans from "everything at a few times" to "most gaps exceed tau"
        rec = _stream(rng, n, t_max=[3, 40, 6 * max(tau, 1), 40 * max(tau, 1) + 50][trial % 4])
        mask = (rng.rand(H, W) < 0.15).astype(np.uint8) if trial % 3 else None
        f = filter_ref.Filter(H, W, tau, mask)
        got = f.feed(rec)
        want = by = filter_ref.by_the_sentence(rec, H, W, tau, mask)
        assert np.array_equal(got, rec[by]), (tau, trial)
        c = f.counters()
        assert c['seen'] == n and c['kept'] == len(want) and c['kept'] + c['outside'] + c['masked'] + c['unsupported'] == n
        # fed in two chunks the restatement gives the same
        cut = int(rng.randint(0, n + 1))
        g = filter_ref.Filter(H, W, tau, mask)
        assert np.array_equal(np.concatenate([g.feed(rec[:cut]), g.feed(rec[cut:])]), got) and g.state() == f.state()


def test_restatement_on_the_cases_one_can_do_by_hand():
    R = filter_ref.records
    f = filter_ref.Filter(4, 5, 10)
    assert len(f.feed(R([5], [2], [2]))) == 0                                            # a lone event
    f = filter_ref.Filter(4, 5, 10)
    assert f.feed(R([0, 10, 21], [1, 2, 3], [1, 1, 1]))[:, 0].tolist() == [10]           # tau apart: kept; tau + 1: not
    f = filter_ref.Filter(4, 5, 10)
    assert len(f.feed(R([0, 1], [1, 1], [1, 1]))) == 0                                   # the pixel itself is no neighbour
    f = filter_ref.Filter(4, 5, 10)
    assert f.feed(R([0, 100, 105], [0, 1, 2], [0, 0, 0]))[:, 0].tolist() == [105]        # a removed event supports
    with pytest.raises(filter_ref.OrderError) as e:
        f.feed(R([200, 199], [0, 0], [0, 0]))
    assert (e.value.position, e.value.t_before, e.value.t_at) == (1, 200, 199)
    with pytest.raises(filter_ref.OrderError) as e:                                      # against the chunk before
        f.feed(R([104], [0], [0]))
    assert (e.value.position, e.value.t_before, e.value.t_at) == (0, 105, 104) and f.counters()['seen'] == 3
    f = filter_ref.Filter(4, 5, None, mask=np.eye(4, 5))                                 # rule 3 off: bounds and mask only
    assert f.feed(R([1, 2, 3], [0, 1, 5], [0, 0, 0]))[:, 0].tolist() == [2] and f.counters()['unsupported'] == 0


def test_hot_pixel_threshold_is_exact():
    # 50 Hz over 3.5 s: 175 events are exactly the rate -- not hot; 176 are
    counts = np.array([[0, 174, 175], [176, 177, 10 ** 12]], dtype=np.int64)
    m = ef.hot_pixel_mask(counts, 3_500_000, 50)
    assert m.dtype == np.uint8 and m.tolist() == [[0, 0, 0], [1, 1, 1]]
    # a duration that is no whole number of periods: count * 10^6 > 3 * 333_333 = 999_999 from one event on
    assert ef.hot_pixel_mask(np.array([[0, 1]]), 333_333, 3).tolist() == [[0, 1]]
    assert ef.hot_pixel_mask(np.array([[1, 2]]), 333_334, 3).tolist() == [[0, 1]]          # 1_000_002: one event is below it
    assert ef.hot_pixel_mask(np.array([[0, 1]], dtype=np.uint16), 1, 0).tolist() == [[0, 1]]
    # beyond float precision: 2^53 + 1 against 2^53
    big = np.array([[2 ** 53, 2 ** 53 + 1]], dtype=np.int64)
    assert ef.hot_pixel_mask(big, 1_000_000, 2 ** 53).tolist() == [[0, 1]]
    for bad in (dict(counts=np.zeros((2, 2))), dict(counts=np.zeros(4, np.int64)), dict(duration_us=-1), dict(max_rate_hz=2.5),
                dict(counts=np.array([[-1]]))):
        kw = dict(dict(counts=np.zeros((2, 2), np.int64), duration_us=10, max_rate_hz=1), **bad)
        with pytest.raises(ValueError):
            ef.hot_pixel_mask(**kw)


def test_mask_files_are_validated(tmp_path):
    good = np.zeros((H, W), dtype=np.uint8)
    good[2, 3] = 7
    np.save(str(tmp_path / 'u8.npy'), good)
    np.save(str(tmp_path / 'bool.npy'), good != 0)
    for name in ('u8.npy', 'bool.npy'):
        m = ef.read_pixel_mask(str(tmp_path / name), (H, W))
        assert m.dtype == np.uint8 and m.shape == (H, W) and m.sum() == 1 and m[2, 3] == 1
    np.save(str(tmp_path / 'transposed.npy'), good.T.copy())
    np.save(str(tmp_path / 'flat.npy'), good.reshape(-1))
    np.save(str(tmp_path / 'float.npy'), good.astype(np.float32))
    np.save(str(tmp_path / 'int64.npy'), good.astype(np.int64))
    np.save(str(tmp_path / 'pickled.npy'), np.array([good, None], dtype=object), allow_pickle=True)
    (tmp_path / 'text.npy').write_bytes(b'not an array')
    np.savez(str(tmp_path / 'mask.npz'), mask=good)
    for name in ('transposed.npy', 'flat.npy', 'float.npy', 'int64.npy', 'pickled.npy', 'text.npy', 'mask.npz'):
        with pytest.raises(ValueError):
            ef.read_pixel_mask(str(tmp_path / name), (H, W))
    with pytest.raises(FileNotFoundError):
        ef.read_pixel_mask(str(tmp_path / 'none.npy'), (H, W))
    with pytest.raises(ValueError):
        ef.check_pixel_mask(good, (W, H))


def test_filter_options_are_checked_on_the_host(tmp_path, monkeypatch):
    from leod_amd.data.utils.types import DatasetType
    assert ingest.check_filter_options('gen1') is None
    assert ingest.check_filter_options('gen1', denoise_us=0) == dict(tau_us=0, mask=None, hot_rate_hz=None)
    flt = ingest.check_filter_options('gen4', hot_rate_hz=50, pixel_mask=np.ones((720, 1280), dtype=bool))
    assert flt['tau_us'] is None and flt['hot_rate_hz'] == 50 and flt['mask'].dtype == np.uint8 and flt['mask'].all()
    for kw in (dict(denoise_us=-1), dict(denoise_us=2 ** 31), dict(denoise_us=1.5), dict(denoise_us=True), dict(hot_rate_hz=-1),
               dict(hot_rate_hz=0.5), dict(pixel_mask=np.zeros((240, 304), np.int32)), dict(pixel_mask=np.zeros((304, 240), np.uint8)),
               dict(pixel_mask=str(tmp_path / 'mask.txt'))):
        with pytest.raises(ValueError):
            ingest.check_filter_options('gen1', **kw)
    assert ingest.check_filter_options('gen1', denoise_us=2 ** 31 - 1)['tau_us'] == 2 ** 31 - 1


def test_command_line_options_reach_ingest_split(tmp_path, monkeypatch, capsys):
    """``main`` up to the point where the device is needed: the options are parsed, checked and handed to ``ingest_split``."""
    calls = []
    monkeypatch.setattr(ingest, 'ingest_split', lambda src, dst, dataset, **kw: calls.append((src, dst, dataset, kw)) or [{}])
    src, dst = str(tmp_path / 'src'), str(tmp_path / 'dst')
    os.makedirs(src)
    assert ingest.main([src, dst, '--dataset', 'gen1']) == 0
    kw = calls[-1][3]
    assert (kw['denoise_us'], kw['pixel_mask'], kw['hot_rate_hz']) == (None, None, None)       # all three are off by default
    mask = np.zeros((240, 304), dtype=np.uint8)
    np.save(str(tmp_path / 'mask.npy'), mask)
    assert ingest.main([src, dst, '--dataset', 'gen1', '--denoise-us', '10000', '--pixel-mask', str(tmp_path / 'mask.npy'), '--hot-rate', '50',
                        '--write', 'packed']) == 0
    kw = calls[-1][3]
    assert (kw['denoise_us'], kw['pixel_mask'], kw['hot_rate_hz'], kw['write']) == (10000, str(tmp_path / 'mask.npy'), 50, 'packed')
    # refused before anything is ingested: values out of range, a mask of another sensor, a mask that is not there
    n = len(calls)
    for bad in (['--denoise-us', '-1'], ['--denoise-us', str(2 ** 31)], ['--denoise-us', '1.5'], ['--hot-rate', '-3'],
                ['--pixel-mask', str(tmp_path / 'none.npy')]):
        with pytest.raises(SystemExit) as e:
            ingest.main([src, dst, '--dataset', 'gen1'] + bad)
        assert e.value.code == 2, bad
    with pytest.raises(SystemExit):
        ingest.main([src, dst, '--dataset', 'gen4', '--pixel-mask', str(tmp_path / 'mask.npy')])     # a Gen1 mask for a Gen4 sensor
    assert len(calls) == n
    capsys.readouterr()


def test_the_keyword_arguments_reach_every_recording(tmp_path, monkeypatch):
    """``ingest_split`` reads a mask file once and hands the three options to ``ingest_recording``; without them it hands over none."""
    from leod_amd.data.utils import dat_events
    calls = []
    monkeypatch.setattr(ingest, 'ingest_recording', lambda *a, **kw: calls.append(kw) or {})
    src = tmp_path / 'src'
    src.mkdir()
    for name in ('a', 'b'):
        dat_events.write_dat(str(src / f'{name}_td.dat'), filter_ref.records([1], [1], [1]), 240, 304)
    ingest.ingest_split(str(src), str(tmp_path / 'dst'), 'gen1', unlabelled='ok')
    assert len(calls) == 2 and not any(k in calls[0] for k in ('denoise_us', 'pixel_mask', 'hot_rate_hz'))
    mask = np.zeros((240, 304), dtype=bool)
    mask[5, 6] = True
    np.save(str(tmp_path / 'mask.npy'), mask)
    ingest.ingest_split(str(src), str(tmp_path / 'dst'), 'gen1', unlabelled='ok', denoise_us=5000, pixel_mask=str(tmp_path / 'mask.npy'))
    assert len(calls) == 4
    for kw in calls[2:]:
        assert kw['denoise_us'] == 5000 and kw['hot_rate_hz'] is None
        assert isinstance(kw['pixel_mask'], np.ndarray) and kw['pixel_mask'].dtype == np.uint8 and kw['pixel_mask'].sum() == 1
    with pytest.raises(ValueError):
        ingest.ingest_split(str(src), str(tmp_path / 'dst'), 'gen1', unlabelled='ok', denoise_us=-5)
    assert len(calls) == 4
