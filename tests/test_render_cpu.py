"""Host side of the prediction videos (leod_amd/visualize.py) and the argument checks of ``ops.render_frames``: no GPU involved."""
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as g
    g.build()
    from leod_amd import _lib
    return _lib


def decode_png(path):
    """8-bit RGB PNG -> uint8 [H, W, 3] with zlib alone (all five scanline filters), independent of the writer."""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, seen = 8, b'', []
    while pos < len(data):
        n = struct.unpack('>I', data[pos:pos + 4])[0]
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, f'CRC of {tag}'
        seen.append(tag)
        if tag == b'IHDR':
            w, h, depth, colour, comp, filt, interlace = struct.unpack('>IIBBBBB', body)
            assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    assert seen[0] == b'IHDR' and seen[-1] == b'IEND'
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), dtype=np.uint8)
    for y in range(h):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        prev = out[y - 1].astype(np.int32) if y else np.zeros(3 * w, dtype=np.int32)
        cur = np.zeros(3 * w, dtype=np.int32)
        for i in range(3 * w):
            a = cur[i - 3] if i >= 3 else 0
            b, c = prev[i], (prev[i - 3] if i >= 3 else 0)
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[i] = (line[i] + pred) & 255
        out[y] = cur
    return out.reshape(h, w, 3)


@pytest.mark.parametrize('hw', [(1, 1), (5, 7), (24, 40)])
def test_png_round_trip(tmp_path, hw):
    from leod_amd.visualize import write_png, read_png
    img = np.random.RandomState(hw[0]).randint(0, 256, size=hw + (3,)).astype(np.uint8)
    fn = str(tmp_path / 'a.png')
    write_png(fn, img)
    assert np.array_equal(decode_png(fn), img)
    assert np.array_equal(read_png(fn), img)
    write_png(fn, torch.from_numpy(img))
    assert np.array_equal(decode_png(fn), img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(fn) as im:
            assert im.mode == 'RGB' and np.array_equal(np.asarray(im), img)
    with pytest.raises(ValueError):
        write_png(fn, img[..., 0])
    with pytest.raises(ValueError):
        write_png(fn, img.astype(np.float32))


def schedule_restated(has_label, n_classes):
    """vis_pred.py:216-224 as written there: a list of frames, labelled ones several times, then [::2]."""
    all_imgs = []
    for i, lab in enumerate(has_label):
        if not lab:
            all_imgs.append(i)
        elif n_classes == 3:
            all_imgs.extend([i] * 3)
        else:
            all_imgs.extend([i] * ((30 // 2) // 2))
    return all_imgs[::2]


@pytest.mark.parametrize('n_classes', [2, 3])
@pytest.mark.parametrize('labelled', [(0,), (8,), (3, 4), (0, 1, 8), (), (2, 5)])
def test_video_frame_indices(n_classes, labelled):
    from leod_amd.visualize import video_frame_indices, FPS
    assert FPS == 15
    has = [i in labelled for i in range(9)]
    got = video_frame_indices(has, n_classes)
    assert got == schedule_restated(has, n_classes)
    hold = 3 if n_classes == 3 else 7
    assert len(got) == -(-(9 + (hold - 1) * len(labelled)) // 2)
    assert got == sorted(got) and all(0 <= i < 9 for i in got)


class FakeLabels:
    """The two calls ``build_items`` makes on an ``ObjectLabels``."""

    def __init__(self, xyxy, cls):
        self.xyxy, self.cls = torch.tensor(xyxy, dtype=torch.float32), torch.tensor(cls, dtype=torch.float32)

    def get_xyxy(self):
        return self.xyxy

    def get(self, name):
        assert name == 'class_id'
        return self.cls


def item_text(items, text, i):
    return bytes(text[items[i, 5]:items[i, 5] + items[i, 6]]).decode()


def test_build_items():
    from leod_amd.visualize import build_items
    G, R, K = 0 | 255 << 8, 255, 0
    keep = [torch.tensor([[10.7, 20.2, 30.99, 41.5, 0.9, 0.8, 1.0]]), None]
    remove = [torch.tensor([[1.0, 2.0, 3.0, 4.0, 0.5, 0.25, 0.0]]), None]
    labels = [FakeLabels([[5.5, 6.5, 50.0, 40.0]], [1.0]), None]
    frame_off, items, text = build_items(keep, remove, labels, ('car', 'ped'), [0.35, 0.40], upsample=2)
    assert frame_off.dtype == np.int32 and items.dtype == np.int32 and text.dtype == np.uint8
    assert frame_off.tolist() == [0, 11, 12] and items.shape == (12, 8)
    assert items[:11, 0].tolist() == [0] * 11 and items[11, 0] == 1
    # kept prediction: rectangle with truncated corners (10.7 * 2 = 21.4 -> 21, 30.99 * 2 = 61.98 -> 61), thickness 2, green, then three lines
    assert items[0].tolist() == [0, 0, 21, 40, 61, 83, 2, G]
    assert [item_text(items, text, i) for i in (1, 2, 3)] == ['ped', '0.900x0.800', '0.720']
    assert items[1:4, 1].tolist() == [1, 1, 1] and items[1:4, 4].tolist() == [2, 2, 2] and items[1:4, 7].tolist() == [G] * 3
    assert items[1:4, 2].tolist() == [21] * 3 and items[1:4, 3].tolist() == [40, 56, 72]          # line pitch 8 * scale
    # removed prediction: red
    assert items[4].tolist() == [0, 0, 2, 4, 6, 8, 2, R]
    assert [item_text(items, text, i) for i in (5, 6, 7)] == ['car', '0.500x0.250', '0.125'] and items[5:8, 7].tolist() == [R] * 3
    # label: black, the class name only
    assert items[8].tolist() == [0, 0, 11, 13, 100, 80, 2, K]
    assert item_text(items, text, 9) == 'ped' and items[9, 7] == K and items[9, 2:4].tolist() == [11, 13]
    # timestamp last: red at (10, 10 + 10 * upsample)
    assert item_text(items, text, 10) == f'{0.35:.2f}s (N={int(0.35 / 0.05):04d})'
    assert items[10, 1:5].tolist() == [1, 10, 30, 2] and items[10, 7] == R
    assert item_text(items, text, 11).startswith('0.40s (N=')
    # every text range lies inside the buffer, back to back
    assert items[items[:, 1] == 1][:, 5].tolist() == np.cumsum([0] + items[items[:, 1] == 1][:-1, 6].tolist()).tolist()
    assert int(items[-1, 5] + items[-1, 6]) == len(text)
    # upsample 1: corners int(coord), thickness 1, scale 1
    _, it1, _ = build_items(keep, remove, labels, ('car', 'ped'), [0.35, 0.40], upsample=1)
    assert it1[0].tolist() == [0, 0, 10, 20, 30, 41, 1, G] and it1[10, 1:5].tolist() == [1, 10, 20, 1]


def test_filter_boxes_ssod_split():
    from leod_amd.visualize import filter_boxes_ssod
    assert filter_boxes_ssod(None) == (None, None) and filter_boxes_ssod(torch.zeros((0, 7))) == (None, None)
    boxes = torch.tensor([[-5.0, 10.0, 40.0, 50.0, 0.9, 0.9, 0.0],          # kept, clamped to x1 = 0
                          [10.0, 10.0, 12.0, 50.0, 0.9, 0.9, 1.0],          # narrower than 5 pixels: removed
                          [2.0, 2.0, 300.0, 100.0, 0.9, 0.9, 0.0]])         # wider than 90 % of the frame: removed
    before = boxes.clone()
    keep, remove = filter_boxes_ssod(boxes, 'gen1', False)
    assert torch.equal(boxes, before)
    assert keep[:, :4].tolist() == [[0.0, 10.0, 40.0, 50.0]] and len(remove) == 2 and remove[0, 6] == 1.0
    assert torch.equal(remove[1], before[2])


def test_vis_config():
    from leod_amd.config import vis_config
    cfg = vis_config('gen1', 'small')
    assert cfg.is_train is False and cfg.num_video == 5 and cfg.reverse is False
    assert cfg.batch_size.eval == 1 and cfg.tta.enable is False
    assert vis_config('gen4', 'tiny', overrides=dict(num_video=2, reverse=True)).num_video == 2


def good_overlay():
    items = [[0, 0, 1, 1, 5, 5, 1, 255], [0, 1, 2, 9, 1, 0, 3, 255], [1, 1, 0, 8, 2, 3, 2, 0]]
    return [0, 2, 3], items, b'abcde'


@pytest.mark.parametrize('case', ['descending', 'last', 'first', 'text_range', 'text_negative', 'scale', 'thickness', 'length', 'shape',
                                  'kind', 'upsample'])
def test_render_frames_refuses_bad_overlays(built, case):
    """Every check happens on the host before anything is uploaded: these all raise with CPU tensors and no GPU."""
    from leod_amd import ops
    ev = torch.zeros((2, 4, 3, 5), dtype=torch.uint8)
    fo, items, text = good_overlay()
    kw = {}
    if case == 'descending':
        fo = [0, 3, 2]
        items = items[:2]
    elif case == 'last':
        fo = [0, 2, 2]
    elif case == 'first':
        fo = [1, 2, 3]
    elif case == 'text_range':
        items[2][5], items[2][6] = 4, 2
    elif case == 'text_negative':
        items[1][5] = -1
    elif case == 'scale':
        items[1][4] = 0
    elif case == 'thickness':
        items[0][6] = 0
    elif case == 'length':
        fo = [0, 3]
    elif case == 'shape':
        items = [r[:7] for r in items]
    elif case == 'kind':
        items[0][1] = 2
    elif case == 'upsample':
        kw['upsample'] = 3
    with pytest.raises(ValueError):
        ops.render_frames(ev, fo, items, text, **kw)


def test_render_frames_refuses_cpu_tensors(built):
    from leod_amd import ops
    from leod_amd._lib import LeodHipError
    ev = torch.zeros((2, 4, 3, 5), dtype=torch.uint8)
    with pytest.raises(LeodHipError):
        ops.render_frames(ev)
    with pytest.raises(LeodHipError):
        ops.render_frames(ev, *good_overlay())                             # a valid overlay gets as far as the device check
    with pytest.raises(LeodHipError):
        ops.render_frames(ev.to(torch.int32))


def test_font_table(built):
    from leod_amd import ops
    table = ops.render_font()
    assert table.shape == (95, 7) and table.dtype == np.uint8
    assert int(table.max()) < 32                                           # five columns
    assert not table[0].any()                                              # space
    assert all(table[i].any() for i in range(1, 95))
    assert len({bytes(g) for g in table}) == 95
    # orientation: 'L' is a left column and a bottom row, '-' the middle row only
    L, dash = table[ord('L') - 0x20], table[ord('-') - 0x20]
    assert L.tolist() == [0x10] * 6 + [0x1F] and dash.tolist() == [0, 0, 0, 0x1F, 0, 0, 0]
    # the committed header is what tools/gen_font5x7.py writes
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_font5x7', os.path.join(ROOT, 'tools', 'gen_font5x7.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert np.array_equal(np.asarray(gen.table(), dtype=np.uint8), table)


def test_surface(built):
    from leod_amd import ops, visualize
    protos = built.parse_header()
    assert 'leod_render_frames_u8' in protos and 'leod_render_font' in protos
    assert len(protos['leod_render_frames_u8'][1]) == 15
    assert callable(ops.render_frames)
    for name in ('event2rgb', 'filter_boxes_ssod', 'build_items', 'video_frame_indices', 'write_png', 'render_sequence',
                 'run_visualization', 'main'):
        assert callable(getattr(visualize, name)), name
    header = open(built.HEADER_PATH).read()
    assert re.search(r'int leod_render_font\(unsigned char\* dst\);', header)
