"""Host side of the recording ingestion, without a GPU: the .dat header and record layout against what the reference's own reader
returns (g27, recorded by tests/golden/make_golden_dat.py), the refusals, the window rule at its edges, the label-to-frame rule, and
the statement the ds2 kernel rests on: nearest-exact interpolation at scale 0.5 selects full[.., 1::2, 1::2]."""
import os

import numpy as np
import pytest

from leod_amd.data import ingest
from leod_amd.data.utils import dat_events

D = 50_000


@pytest.fixture(scope='module')
def g27(golden_dir):
    return np.load(os.path.join(golden_dir, 'g27_dat_events.npz'))


def _write(path, data: bytes) -> str:
    with open(path, 'wb') as f:
        f.write(data)
    return str(path)


def test_header_and_records_match_the_reference_reader(g27, tmp_path):
    fn = _write(tmp_path / 'rec_td.dat', g27['dat_bytes'].tobytes())
    hdr, records = dat_events.open_records(fn)
    bod, ev_type, ev_size, h, w = (int(v) for v in g27['header'])
    assert (ev_type, ev_size) == (0, 8)
    assert hdr == dat_events.DatHeader(bod, h, w, len(g27['t'])) and (h, w) == (24, 30)
    assert records.dtype == np.dtype('<u4') and records.shape == (len(g27['t']), 2) and isinstance(records, np.memmap)
    t, x, y, p = dat_events.decode(records)
    for got, name in ((t, 't'), (x, 'x'), (y, 'y'), (p, 'p')):
        assert got.dtype == np.int64 and np.array_equal(got, g27[name]), name
    assert t[-1] == 2 ** 32 - 1 and t[0] == 0                          # t is unsigned in the file
    assert np.array_equal(dat_events.encode(t, x, y, p), np.asarray(records))
    dat_events.check_sorted(t)
    # the same bytes written again by the package's writer
    dat_events.write_dat(str(tmp_path / 'again_td.dat'), records, h, w)
    assert np.array_equal(np.fromfile(str(tmp_path / 'again_td.dat'), dtype=np.uint8), g27['dat_bytes'])


def test_bare_records_without_a_header(tmp_path):
    rec = dat_events.encode([1, 2, 3], [4, 5, 6], [7, 8, 9], [0, 1, 0])
    fn = _write(tmp_path / 'bare_td.dat', rec.tobytes())
    hdr, records = dat_events.open_records(fn)
    assert hdr == dat_events.DatHeader(0, None, None, 3) and np.array_equal(records, rec)


@pytest.mark.parametrize('ev_type,ev_size', [(12, 8), (0, 16), (1, 4)])
def test_other_event_types_and_sizes_are_refused(tmp_path, ev_type, ev_size):
    fn = _write(tmp_path / 'odd_td.dat', b'% Height 24\n% Width 30\n' + bytes([ev_type, ev_size]) + bytes(32))
    with pytest.raises(ValueError, match='odd_td.dat'):
        dat_events.parse_header(fn)


def test_truncated_records_are_refused(tmp_path):
    fn = _write(tmp_path / 'short_td.dat', b'% Height 24\n% Width 30\n' + bytes([0, 8]) + bytes(20))
    with pytest.raises(ValueError, match='short_td.dat'):
        dat_events.parse_header(fn)


def test_decreasing_time_is_refused(tmp_path):
    dat_events.check_sorted(np.array([0, 0, 5, 5, 9]))
    with pytest.raises(ValueError, match='decrease at event 3'):
        dat_events.check_sorted(np.array([0, 4, 9, 8, 10], dtype=np.uint32))
    t = np.array([0, 10, 20, 30, 25, 40, 50])
    fn = str(tmp_path / 'back_td.dat')
    dat_events.write_dat(fn, dat_events.encode(t, t * 0, t * 0, t * 0), 24, 30)
    _, records = dat_events.open_records(fn)
    for block in (1 << 22, 4, 2):                                       # the decrease inside a block and across a block boundary
        with pytest.raises(ValueError, match='back_td.dat'):
            dat_events.scan_windows(records, D, what=fn, block=block)


def test_window_offsets_edges():
    wo = dat_events.window_offsets
    # t = 0 belongs to frame 0; t = k*D exactly closes frame k - 1
    t = np.array([0, 0, 1, D - 1, D, D, D + 1, 2 * D, 2 * D + 1, 3 * D])
    assert wo(t, D).tolist() == [0, 6, 8, 10]
    # an empty window in the middle
    t = np.array([5, D, 3 * D + 1, 3 * D + 2])
    assert wo(t, D).tolist() == [0, 2, 2, 2, 4]
    # a single event, at 0, inside a frame, on an edge
    assert wo(np.array([0]), D).tolist() == [0, 1]
    assert wo(np.array([7]), D).tolist() == [0, 1]
    assert wo(np.array([D]), D).tolist() == [0, 1]
    assert wo(np.array([D + 1]), D).tolist() == [0, 0, 1]
    # no event at all: one empty frame
    assert wo(np.zeros(0, dtype=np.int64), D).tolist() == [0, 0]
    # u32 times beyond 2^31 (the file's type) do not wrap
    t = np.array([2 ** 32 - 1], dtype=np.uint32)
    off = wo(t, 2 ** 30)
    assert off.tolist() == [0, 0, 0, 0, 1] and off.dtype == np.int64
    assert dat_events.num_windows(0, D) == 1 and dat_events.num_windows(D, D) == 1 and dat_events.num_windows(D + 1, D) == 2


def test_scan_windows_equals_window_offsets_for_every_block_size(g27):
    rec = dat_events.encode(g27['t'], g27['x'], g27['y'], g27['p'])[:390]        # without the tail beyond 2^31: 8 frames instead of 85 900
    want = dat_events.window_offsets(rec[:, 0], D)
    assert want[-1] == 390 and len(want) == 9
    for block in (1 << 22, 390, 389, 64, 1):
        assert np.array_equal(dat_events.scan_windows(rec, D, block=block), want), block
    assert dat_events.scan_windows(rec[:0], D).tolist() == [0, 0]


PROPHESEE_BBOX = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                           'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                           'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})


def _boxes(rows):
    out = np.zeros((len(rows),), dtype=PROPHESEE_BBOX)
    for i, (t, cls) in enumerate(rows):
        out[i] = (t, 10 + i, 20 + i, 30 + i, 40 + i, cls, 100 + i, 0.5 + 0.01 * i)
    return out


def test_label_frame_rule():
    assert ingest.label_frame([0, 1, D - 1, D, D + 1, 2 * D, 2 * D + 1], D).tolist() == [0, 0, 0, 0, 1, 1, 2]
    #           frame 0 (t = 0)  frame 1, two timestamps     frame 3      frame 3 again   past the last frame (N = 5)
    boxes = _boxes([(0, 0), (D + 10, 1), (2 * D, 0), (2 * D, 1), (4 * D, 0), (3 * D + 1, 1), (5 * D + 1, 0), (9 * D, 1)])
    lab, starts, repr_idx = ingest.convert_labels(boxes, 5, D)
    assert repr_idx.tolist() == [0, 1, 3] and repr_idx.dtype == np.int64
    assert starts.tolist() == [0, 1, 3] and starts.dtype == np.int64
    assert lab['t'].tolist() == [0, 2 * D, 2 * D, 4 * D]                # D + 10 and 3*D + 1 gave way to the later timestamp of their frame
    assert lab.dtype == ingest.LABEL_DTYPE and lab.dtype.itemsize == 40 and 'track_id' not in lab.dtype.names
    assert np.all(lab['objectness'] == 1.0)
    src = boxes[[0, 2, 3, 4]]
    for name in ('t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence'):
        assert np.array_equal(lab[name], src[name]), name
    # class filter: only class 1 -> frame 1 keeps its later box, frame 3 now keeps 3*D + 1
    lab, starts, repr_idx = ingest.convert_labels(boxes, 5, D, keep_classes=(1,))
    assert repr_idx.tolist() == [1, 3] and starts.tolist() == [0, 1] and lab['t'].tolist() == [2 * D, 3 * D + 1]
    # a box exactly at the end of the last frame stays, one microsecond later it goes
    assert ingest.convert_labels(_boxes([(5 * D, 0)]), 5, D)[2].tolist() == [4]
    assert ingest.convert_labels(_boxes([(5 * D + 1, 0)]), 5, D)[2].tolist() == []
    # nothing left: empty arrays of the right types
    lab, starts, repr_idx = ingest.convert_labels(_boxes([]), 5, D)
    assert len(lab) == 0 and lab.dtype == ingest.LABEL_DTYPE and starts.dtype == np.int64 and len(repr_idx) == 0


def test_label_dtype_is_the_one_the_loaders_read():
    from leod_amd.data.genx_utils.labels import ObjectLabelFactory
    boxes = _boxes([(D, 0), (D, 1), (3 * D, 1)])
    lab, starts, repr_idx = ingest.convert_labels(boxes, 4, D)
    fac = ObjectLabelFactory.from_structured_array(lab, starts, (240, 304))
    assert len(fac) == 2 and repr_idx.tolist() == [0, 2]
    first = fac[0]
    assert first.t.tolist() == [D, D] and first.class_id.tolist() == [0, 1] and first.objectness.tolist() == [1.0, 1.0]
    assert first.x.tolist() == [10.0, 11.0] and first.h.tolist() == [40.0, 41.0]


def test_older_annotation_field_names():
    old = np.zeros((2,), dtype=[('ts', '<u8'), ('x', '<f4'), ('y', '<f4'), ('w', '<f4'), ('h', '<f4'), ('class_id', 'u1'),
                                ('confidence', '<f4'), ('track_id', '<u4')])
    old['ts'], old['confidence'], old['class_id'] = [D, 2 * D], [0.25, 0.75], [0, 1]
    lab, starts, repr_idx = ingest.convert_labels(old, 2, D)
    assert lab['t'].tolist() == [D, 2 * D] and lab['class_confidence'].tolist() == [0.25, 0.75] and repr_idx.tolist() == [0, 1]
    with pytest.raises(ValueError, match='lacks the fields'):
        ingest.convert_labels(np.zeros((1,), dtype=[('t', '<i8'), ('x', '<f4')]), 2, D)


def test_nearest_exact_half_scale_selects_the_odd_pixels():
    """The ds2 output of the kernel is full[.., 1::2, 1::2]; the tree's file name says '_ds2_nearest'.  torch's nearest-exact rule at
    scale 0.5 reads source index floor((i + 0.5) * 2) = 2i + 1."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    for H, W in ((24, 30), (240, 304), (720, 1280), (2, 2)):
        full = torch.randint(0, 256, (2, 20, H, W), generator=g, dtype=torch.uint8)
        half = F.interpolate(full.float(), scale_factor=0.5, mode='nearest-exact')
        assert half.shape[-2:] == (H // 2, W // 2)
        assert torch.equal(half.to(torch.uint8), full[..., 1::2, 1::2])
        assert torch.equal(F.interpolate(full.float(), size=(H // 2, W // 2), mode='nearest-exact').to(torch.uint8), full[..., 1::2, 1::2])


def test_ingest_refuses_what_it_does_not_write(tmp_path):
    with pytest.raises(ValueError, match='npy'):
        ingest.ingest_recording('a_td.dat', 'a_bbox.npy', str(tmp_path), 'gen1', write='h5')
    with pytest.raises(ValueError, match='gen1 or gen4'):
        ingest.ingest_recording('a_td.dat', 'a_bbox.npy', str(tmp_path), 'gen3')
    # a header of another sensor
    fn = str(tmp_path / 'small_td.dat')
    dat_events.write_dat(fn, dat_events.encode([1], [2], [3], [1]), 24, 30)
    with pytest.raises(ValueError, match='Height 24'):
        ingest.ingest_recording(fn, 'a_bbox.npy', str(tmp_path / 'out'), 'gen1')
    assert ingest.ev_repr_name(50_000, 10) == 'stacked_histogram_dt=50_nbins=10'
