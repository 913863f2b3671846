"""The sensor fit of the ingestion on the host: the auto / center table, the pixel map as a bijection, the boxes'
map tied to the events', box clipping, the integrate-and-fire rule on the tests' restatement (tests/fit_ref.py), and the options."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_ref as fr  # noqa: E402
from fit_ref import records as R  # noqa: E402
from leod_amd.data.utils import event_filter as ef  # noqa: E402

BOX = np.dtype([('t', '<i8'), ('x', '<f4'), ('y', '<f4'), ('w', '<f4'), ('h', '<f4'), ('class_id', '<u4'), ('class_confidence', '<f4'),
                ('track_id', '<u4')])

# name, src (H, W), dst (H, W), keyword arguments, events (t, x, y, p), kept (t, xd, yd, p), counters other than seen and kept
HAND = [
    ('pick', (4, 6), (2, 3), dict(scale=2), [(1, 1, 1, 1), (2, 0, 0, 1), (3, 3, 1, 0), (4, 5, 3, 1), (5, 6, 0, 1), (6, 4, 3, 0)],
     [(1, 0, 0, 1), (3, 1, 0, 0), (4, 2, 1, 1)], dict(outside=1, skipped=2)),
    ('sum', (4, 6), (2, 3), dict(scale=2, reduce='sum'), [(1, 1, 1, 1), (2, 0, 0, 1), (3, 3, 1, 0), (4, 5, 3, 1), (5, 6, 0, 1), (6, 4, 3, 0)],
     [(1, 0, 0, 1), (2, 0, 0, 1), (3, 1, 0, 0), (4, 2, 1, 1), (6, 2, 1, 0)], dict(outside=1)),
    # pixel (0, 0): +1, +2 fires ON, -1, 0, -1, -2 fires OFF; pixel (1, 0): +1
    ('fire', (4, 6), (2, 3), dict(scale=2, reduce='fire', threshold=2),
     [(1, 0, 0, 1), (2, 1, 1, 1), (3, 0, 1, 0), (4, 1, 0, 1), (5, 1, 0, 0), (6, 0, 0, 0), (7, 2, 0, 1)],
     [(2, 0, 0, 1), (6, 0, 0, 0)], dict(merged=5)),
    ('fire_default_threshold_is_k_squared', (2, 2), (1, 1), dict(scale=2, reduce='fire'),
     [(1, 0, 0, 1), (1, 1, 0, 1), (2, 0, 1, 1), (2, 1, 1, 1), (3, 0, 0, 1)], [(2, 0, 0, 1)], dict(merged=4)),
    ('orient_90', (2, 3), (3, 2), dict(orient=90, reduce='sum'), [(1, 2, 0, 1), (2, 0, 1, 0)], [(1, 1, 2, 1), (2, 0, 0, 0)], {}),
    ('orient_180', (2, 3), (2, 3), dict(orient=180, reduce='sum'), [(1, 2, 0, 1), (2, 0, 1, 0)], [(1, 0, 1, 1), (2, 2, 0, 0)], {}),
    ('orient_270', (2, 3), (3, 2), dict(orient=270, reduce='sum'), [(1, 2, 0, 1), (2, 0, 1, 0)], [(1, 0, 0, 1), (2, 1, 2, 0)], {}),
    ('mirror', (2, 3), (2, 3), dict(mirror=True), [(1, 2, 0, 1), (2, 0, 1, 0)], [(1, 0, 0, 1), (2, 2, 1, 0)], {}),
    ('mirror_then_90', (2, 3), (3, 2), dict(mirror=True, orient=90), [(1, 2, 0, 1), (2, 0, 1, 0)], [(1, 1, 0, 1), (2, 0, 2, 0)], {}),
    # W' = 5: the scaled image is 2 wide, x' = 4 lies in the incomplete cell; offset -1: cell 0 leaves the frame on the left
    ('cropped', (2, 5), (1, 2), dict(scale=2, offset=(-1, 0), reduce='sum'), [(1, 4, 0, 1), (2, 0, 0, 1), (3, 2, 1, 0), (4, 3, 0, 1)],
     [(3, 0, 0, 0), (4, 0, 0, 1)], dict(cropped=2)),
    ('pad', (1, 2), (3, 4), dict(offset=(1, 2)), [(1, 0, 0, 1), (2, 1, 0, 0)], [(1, 1, 2, 1), (2, 2, 2, 0)], {}),
]


def hand_case(case):
    name, src, dst, kw, ev, kept, other = case
    rec = R(*zip(*ev))
    want = R(*zip(*kept)) if kept else np.zeros((0, 2), '<u4')
    counts = dict(seen=len(ev), kept=len(kept), outside=0, cropped=0, skipped=0, merged=0)
    counts.update(other)
    return rec, src, dst, kw, want, counts


def random_case(seed, n, src=(12, 20), outside=0.03):
    """n random events on a sensor ``src``, a share of them beyond it, times with repeats."""
    rng = np.random.RandomState(1000 + seed)
    h, w = src
    t = np.sort(rng.randint(0, 3 * n + 5, n))
    x, y = rng.randint(0, w, n), rng.randint(0, h, n)
    out = rng.rand(n) < outside
    x[out] += w
    return R(t, x, y, rng.randint(0, 2, n))


@pytest.mark.parametrize('case', HAND, ids=[c[0] for c in HAND])
def test_hand_written_streams(case):
    rec, src, dst, kw, want, counts = hand_case(case)
    f = fr.Fit(src, dst, **kw)
    got = f.feed(rec)
    assert np.array_equal(got, want), (case[0], got.tolist())
    assert f.counters() == counts and sum(counts.values()) == 2 * counts['seen']


def test_the_auto_center_table():
    table = [((480, 640), 'gen1', 2, (-8, 0)), ((480, 640), 'gen4', 1, (0, -60)), ((720, 1280), 'gen1', 3, (-61, 0)),
             ((720, 1280), 'gen4', 2, (0, 0)), ((320, 320), 'gen1', 1, (-8, -40)), ((240, 304), 'gen4', 1, (168, 60))]
    from leod_amd.data import ingest
    assert ingest.frame_hw('gen1') == (240, 304) and ingest.frame_hw('gen4') == (360, 640)
    for src, ds, k, off in table:
        spec = ef.fit_spec(src, ingest.frame_hw(ds))
        assert (spec['scale'], tuple(spec['offset'])) == (k, off), (src, ds, spec)
        assert spec == dict(src_hw=list(src), frame_hw=list(ingest.frame_hw(ds)), orient=0, mirror=False, scale=k, offset=list(off),
                            reduce='pick', threshold=None)
        assert all(type(v) is int for v in spec['src_hw'] + spec['frame_hw'] + spec['offset'] + [spec['scale'], spec['orient']])
    # a quarter turn swaps the sides before the scale is chosen; fire resolves its threshold to k * k
    spec = ef.fit_spec((640, 480), (240, 304), orient=90, reduce='fire')
    assert (spec['scale'], spec['offset'], spec['threshold']) == (2, [-8, 0], 4)
    assert ef.fit_spec((480, 640), (240, 304), scale='3', offset='5,-7')['offset'] == [5, -7]
    assert ef.fit_spec((12, 20), (5, 8))['offset'] == [-1, -1]   # (5 - 6) // 2 = -1: floor division


@pytest.mark.parametrize('src', [(3, 5), (4, 4), (1, 7)])
def test_orientation_is_a_bijection_of_the_pixels(src):
    h, w = src
    pixels = [(x, y) for y in range(h) for x in range(w)]
    for orient, mirror in itertools.product(fr.ORIENTS, (False, True)):
        ho, wo = fr.oriented_hw(src, orient)
        image = [fr.orient_pixel(x, y, src, orient, mirror) for x, y in pixels]
        assert sorted(image) == sorted((x, y) for y in range(ho) for x in range(wo)), (orient, mirror)
    for x, y in pixels:
        q, size = (x, y), src
        for _ in range(4):                                       # four quarter turns, each in the image the one before left
            q, size = fr.orient_pixel(*q, size, 90), fr.oriented_hw(size, 90)
        assert q == (x, y) and size == src
        assert fr.orient_pixel(*fr.orient_pixel(x, y, src, 90), fr.oriented_hw(src, 90), 90) == fr.orient_pixel(x, y, src, 180)
        assert fr.orient_pixel(*fr.orient_pixel(x, y, src, 180), src, 90) == fr.orient_pixel(x, y, src, 270)
        assert fr.orient_pixel(*fr.orient_pixel(x, y, src, 0, True), src, 0, True) == (x, y)


def _boxes(rows):
    b = np.zeros((len(rows),), dtype=BOX)
    for i, (x, y, w, h) in enumerate(rows):
        b[i] = (1000 + i, x, y, w, h, i % 3, 0.5, 7 + i)
    return b


def test_the_unit_box_of_a_pixel_maps_to_the_cell_of_the_mapped_pixel():
    src = (3, 5)
    for orient, mirror in itertools.product(fr.ORIENTS, (False, True)):
        dst = fr.oriented_hw(src, orient)
        spec = ef.fit_spec(src, dst, scale=1, offset=(0, 0), orient=orient, mirror=mirror)
        for y in range(3):
            for x in range(5):
                _, xd, yd, _ = fr.map_pixel(x, y, src, dst, orient, mirror)
                out, n_out = ef.fit_boxes(_boxes([(x, y, 1, 1)]), spec)
                assert n_out == 0 and [out[k][0] for k in 'xywh'] == [xd, yd, 1, 1], (orient, mirror, x, y)
    # and with a scale and an offset: the box of a whole cell is the unit box of the destination pixel
    spec = ef.fit_spec((4, 6), (4, 6), scale=2, offset=(1, 2))
    _, xd, yd, _ = fr.map_pixel(3, 1, (4, 6), (4, 6), scale=2, offset=(1, 2))
    out, _ = ef.fit_boxes(_boxes([(2, 0, 2, 2)]), spec)
    assert [out[k][0] for k in 'xywh'] == [xd, yd, 1, 1] == [2, 2, 1, 1]


def test_box_clipping_and_boxes_outside():
    # (6, 11) at k = 2 -> a 3 x 5 image (x' = 10 is a dropped edge cell) placed at (-1, 1) in a (5, 6) frame: it covers x in [0, 4), y in [1, 4)
    spec = ef.fit_spec((6, 11), (5, 6), scale=2, offset=(-1, 1))
    rows = [(4, 2, 4, 2),        # inside: (1, 2, 2, 1)
            (0, 0, 4, 4),        # half outside on the left: x from -1 -> (0, 1, 1, 2)
            (0, 0, 2, 2),        # wholly in the cropped column -> dropped
            (10, 0, 1, 6),       # wholly in the dropped edge cell (x' >= 10 -> x >= 4) -> dropped
            (8, 4, 3, 2),        # reaches into the edge cell: clipped at x = 4 -> (3, 3, 1, 1)
            (4, 2, 0, 2)]        # no width -> dropped
    boxes = _boxes(rows)
    out, n_out = ef.fit_boxes(boxes, spec)
    assert n_out == 3 and out.dtype == boxes.dtype
    assert [[float(r[k]) for k in 'xywh'] for r in out] == [[1, 2, 2, 1], [0, 1, 1, 2], [3, 3, 1, 1]]
    assert out['t'].tolist() == [1000, 1001, 1004] and out['track_id'].tolist() == [7, 8, 11] and out['class_id'].tolist() == [0, 1, 1]
    assert boxes['x'].tolist() == [4, 0, 0, 10, 8, 4]            # the input is not modified
    # wholly in the pad: a small image centred in a larger frame
    spec = ef.fit_spec((2, 2), (6, 6))
    assert spec['offset'] == [2, 2]
    out, n_out = ef.fit_boxes(_boxes([(0, 0, 2, 2), (-5, 0, 4, 1), (0.5, 0.5, 1, 1)]), spec)
    assert n_out == 1 and [[float(r[k]) for k in 'xywh'] for r in out] == [[2, 2, 2, 2], [2.5, 2.5, 1, 1]]
    # a quarter turn swaps w and h; mirror first
    spec = ef.fit_spec((4, 6), (6, 4), orient=90, mirror=True)
    out, _ = ef.fit_boxes(_boxes([(1, 0, 3, 1)]), spec)          # mirror: x = 6 - 4 = 2; 90: (4 - 1, 2, 1, 3)
    assert [float(out[k][0]) for k in 'xywh'] == [3, 2, 1, 3]
    empty, n_out = ef.fit_boxes(_boxes([]), spec)
    assert len(empty) == 0 and n_out == 0


def test_fire_with_threshold_one_is_sum():
    rec = random_case(1, 3000)
    geo = dict(scale=2, offset=(-1, -1))
    a, b = fr.Fit((12, 20), (5, 8), reduce='fire', threshold=1, **geo), fr.Fit((12, 20), (5, 8), reduce='sum', **geo)
    assert np.array_equal(a.feed(rec), b.feed(rec)) and a.counters() == b.counters() and a.merged == 0 and a.cropped > 0 and a.outside > 0
    assert a.state()[8:] == [0] * 40


@pytest.mark.parametrize('theta', [2, 4, 5])
def test_fire_conserves_polarity_per_destination_pixel(theta):
    src, dst, geo = (12, 20), (5, 8), dict(scale=2, offset=(-1, -1))
    rec = random_case(2 + theta, 4000)
    f = fr.Fit(src, dst, reduce='fire', threshold=theta, **geo)
    kept = f.feed(rec)
    assert f.max_abs < theta and f.kept > 50 and f.merged > f.kept
    net = np.zeros(dst, dtype=np.int64)                          # the sum of +-1 over each pixel's candidates
    t, x, y, p = fr.unpack(rec)
    for xi, yi, pi in zip(x.tolist(), y.tolist(), p.tolist()):
        if xi < src[1] and yi < src[0]:
            why, xd, yd, _ = fr.map_pixel(xi, yi, src, dst, **geo)
            if why is None:
                net[yd, xd] += 1 if pi else -1
    fired = np.zeros(dst, dtype=np.int64)
    _, kx, ky, kp = fr.unpack(kept)
    np.add.at(fired, (ky, kx), np.where(kp == 1, 1, -1))
    assert np.array_equal(theta * fired + np.array(f.state()[8:]).reshape(dst), net)
    assert np.all(np.diff(kept[:, 0].astype(np.int64)) >= 0)


def test_fire_split_at_every_position_equals_one_call():
    rec = random_case(9, 40, src=(4, 6), outside=0.1)
    kw = dict(scale=2, reduce='fire', threshold=2)
    whole = fr.Fit((4, 6), (2, 3), **kw)
    want = whole.feed(rec)
    assert whole.kept > 3 and whole.merged > 3 and any(whole.state()[8:])
    for split in range(len(rec) + 1):
        f = fr.Fit((4, 6), (2, 3), **kw)
        got = np.concatenate([f.feed(rec[:split]), f.feed(rec[split:])])
        assert np.array_equal(got, want) and f.state() == whole.state(), split


def test_a_decreasing_time_is_refused_before_anything_changes():
    f = fr.Fit((4, 6), (2, 3), scale=2, reduce='fire')
    f.feed(R([5, 9], [0, 0], [0, 0]))
    before = f.state()
    with pytest.raises(fr.OrderError) as e:
        f.feed(R([9, 10, 8], [1, 1, 1], [0, 0, 0]))
    assert (e.value.position, e.value.t_before, e.value.t_at) == (2, 10, 8) and f.state() == before


# ---- the options of the ingestion -------------------------------------------------------------------------------------------------------------
def test_fit_spec_checks():
    ok = dict(src_hw=(480, 640), frame_hw=(240, 304))
    for kw in (dict(scale=0), dict(scale=65), dict(scale='big'), dict(scale=2.0), dict(scale=True), dict(offset='middle'), dict(offset='1'),
               dict(offset=(1, 2, 3)), dict(offset=(16385, 0)), dict(offset=(0, -16385)), dict(offset=(1.5, 0)), dict(orient=45),
               dict(orient=360), dict(orient=-90), dict(mirror=2), dict(reduce='max'), dict(threshold=3), dict(reduce='sum', threshold=3),
               dict(reduce='fire', threshold=0), dict(reduce='fire', threshold=32768), dict(reduce='fire', threshold=2.5),
               dict(src_hw=(0, 640)), dict(src_hw=(480, 16385)), dict(src_hw=(480,)), dict(frame_hw=(240, 0)), dict(src_hw=(480.0, 640))):
        with pytest.raises(ValueError):
            ef.fit_spec(**{**ok, **kw})
    spec = ef.fit_spec(**ok, scale=64, offset=(-16384, 16384), reduce='fire')
    assert (spec['scale'], spec['offset'], spec['threshold']) == (64, [-16384, 16384], 4096)
    assert ef.fit_spec(**ok, reduce='fire', threshold=32767)['threshold'] == 32767


def test_option_checks_come_before_any_file_is_opened():
    from leod_amd.data import ingest
    chk = ingest.check_fit_options
    assert chk('gen1') is None and chk('gen1', fit_mirror=False) is None
    assert chk('gen1', '640x480', 'auto') == dict(sensor_hw=(480, 640), fit=dict(scale='auto', mirror=False))
    assert chk('gen1', (480, 640), 2, '1,2', 90, True, 'fire', 9) == \
        dict(sensor_hw=(480, 640), fit=dict(scale=2, mirror=True, offset='1,2', orient=90, reduce='fire', threshold=9))
    assert chk('gen1', '304x240') == dict(sensor_hw=(240, 304), fit=None)
    assert chk('gen4', None, dict(scale=3, reduce='sum')) == dict(sensor_hw=None, fit=dict(scale=3, reduce='sum'))
    assert ingest.parse_sensor('640x480') == (480, 640) == ingest.parse_sensor((480, 640)) == ingest.parse_sensor('640X480')
    bad = (dict(fit_offset='center'), dict(fit_orient=0), dict(fit_orient=90), dict(fit_mirror=True), dict(fit_reduce='pick'),
           dict(fit_threshold=4), dict(fit_reduce='fire', fit_threshold=4),              # any other fit option without fit
           dict(fit='auto', fit_threshold=4), dict(fit='auto', fit_reduce='sum', fit_threshold=4),    # a threshold without fire
           dict(sensor_hw='640x480'),                                                    # another sensor without a fit
           dict(sensor_hw='640'), dict(sensor_hw='axb'), dict(sensor_hw='0x480'), dict(sensor_hw=(480, 640, 3)), dict(sensor_hw=(480.0, 640)),
           dict(fit='huge'), dict(fit=0), dict(fit=65), dict(fit='auto', fit_orient=45), dict(fit='auto', fit_offset='1;2'),
           dict(fit='auto', fit_reduce='max'), dict(fit='auto', fit_reduce='fire', fit_threshold=0), dict(fit='auto', fit_mirror=3),
           dict(fit=dict(scale=2), fit_orient=90), dict(fit=dict(scale=2, colour='red')), dict(fit=dict(scale=2, threshold=3)))
    for kw in bad:
        with pytest.raises(ValueError):
            chk('gen1', **kw)
    # the recording does not exist: nothing was opened
    for kw in (dict(sensor_hw='640x480'), dict(sensor_hw='640', fit='auto'), dict(fit='huge'), dict(fit=0), dict(fit=dict(scale=2, threshold=3)),
               dict(fit=dict(scale='auto', orient=45)), dict(fit=dict(scale=2, reduce='fire', threshold=0)), dict(fit=dict(colour='red')),
               dict(fit=dict(offset='1;2'))):
        with pytest.raises(ValueError):
            ingest.ingest_recording('/nonexistent/a_td.dat', None, '/nonexistent/out', 'gen1', **kw)
    with pytest.raises(ValueError, match='fit_threshold'):
        ingest.ingest_split('/nonexistent/src', '/nonexistent/dst', 'gen1', fit=dict(scale='auto', threshold=5))
    with pytest.raises(ValueError, match='needs a fit'):
        ingest.ingest_split('/nonexistent/src', '/nonexistent/dst', 'gen1', sensor_hw='640x480')
    # a mask is checked against the sensor given, not the dataset's
    with pytest.raises(ValueError, match='pixel mask'):
        ingest.ingest_recording('/nonexistent/a_td.dat', None, '/nonexistent/out', 'gen1', sensor_hw='640x480', fit='auto',
                                pixel_mask=np.zeros((240, 304), np.uint8))
    with pytest.raises(FileNotFoundError):
        ingest.ingest_recording('/nonexistent/a_td.dat', None, '/nonexistent/out', 'gen1', sensor_hw='640x480', fit='auto',
                                pixel_mask=np.zeros((480, 640), np.uint8))
    base = ['/nonexistent/src', '/nonexistent/dst', '--dataset', 'gen1']
    for argv in (['--fit-orient', '90'], ['--fit-mirror'], ['--fit-offset', '1,2'], ['--fit-reduce', 'sum'], ['--fit-threshold', '3'],
                 ['--fit', 'auto', '--fit-threshold', '3'], ['--fit', 'auto', '--fit-reduce', 'pick', '--fit-threshold', '3'],
                 ['--sensor', '640x480'], ['--sensor', '640', '--fit', 'auto'], ['--fit', '0'], ['--fit', 'auto', '--fit-orient', '45'],
                 ['--fit', 'auto', '--fit-offset', 'left']):
        with pytest.raises(SystemExit):
            ingest.main(base + argv)


def test_without_the_new_options_ingest_recording_cannot_reach_the_new_functions(monkeypatch):
    """With ``fit_spec``, ``fit_boxes``, ``check_fit_options``' resolution and the op made unreachable, a call without the new options gets
    as far as opening its (missing) file; the byte-for-byte comparison of the trees is in tests/test_fit_gpu.py."""
    from leod_amd import ops
    from leod_amd.data import ingest

    def never(*a, **kw):
        raise AssertionError('a run without the new options reached the sensor fit')
    for mod, names in ((ef, ('fit_spec', 'fit_boxes', 'fit_oriented_hw')), (ops, ('fit_events', 'fit_query', 'fit_counters')),
                       (ingest, ('parse_sensor', 'frame_hw'))):
        for name in names:
            monkeypatch.setattr(mod, name, never)
    for kw in ({}, dict(denoise_us=5), dict(trail_us=5)):
        with pytest.raises(FileNotFoundError):
            ingest.ingest_recording('/nonexistent/a_td.dat', None, '/nonexistent/out', 'gen1', **kw)
    with pytest.raises(AssertionError, match='reached the sensor fit'):
        ingest.ingest_recording('/nonexistent/a_td.dat', None, '/nonexistent/out', 'gen1', fit='auto')
