"""The frame renderer on the device (``leod_render_frames_u8`` through ``ops.render_frames``) against the restatement in
tests/render_ref.py -- bit for bit: the base image is exact integer arithmetic, the overlay a set of integer raster rules -- and the
prediction-video drivers of leod_amd/visualize.py on top of it.  ``pytest -m gpu``."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import render_ref as rr  # noqa: E402

DEV = 'cuda'
REACHABLE = {255, 243, 219, 207, 183, 171, 147, 135, 112, 100, 76, 64}       # (16320 - 765 K + 32) >> 6 for K in 0 1 3 4 6 7 9 10 12 13 15 16


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return True


def events(shape, gen, density=0.12, dtype=torch.uint8):
    """Pixels with events at about ``density``; such a pixel has counts 1..7 in about half of its channels (at least in one)."""
    L, C, H, W = shape
    pix = torch.rand((L, 1, H, W), generator=gen) < density
    chan = torch.rand(shape, generator=gen) < 0.5
    chan[:, 0] |= ~chan.any(1)
    return (pix & chan).to(dtype) * torch.randint(1, 8, shape, generator=gen).to(dtype)


BASE_SHAPES = [((3, 4, 6, 10), torch.uint8), ((2, 4, 5, 7), torch.uint8), ((2, 4, 6, 10), torch.float32),
               ((1, 2, 1, 1), torch.uint8), ((1, 2, 1, 5), torch.uint8), ((1, 2, 4, 1), torch.uint8)]


@pytest.fixture(scope='module')
def base_cases():
    """(name, events, upsample, expected) of the base-render test; the expectation is computed once, on the CPU."""
    gen = torch.Generator().manual_seed(0)
    cases = []
    for shape, dtype in BASE_SHAPES:
        ev = events(shape, gen, dtype=dtype)
        cases.append((f'{list(shape)} {dtype}', ev, 2))
    ev = events((3, 4, 6, 10), gen)
    cases.append(('up=1', ev, 1))
    ev = events((3, 4, 6, 10), gen)
    ev[0], ev[1] = 0, 3
    cases.append(('all-zero and all-event frames', ev, 2))
    ev = events((2, 4, 6, 10), gen)
    ev[:, :2] = 0
    assert bool(ev[:, 2:].any())
    cases.append(('negative half only', ev, 2))
    ev = events((1, 2, 1, 1), gen)
    ev[:] = 5
    cases.append(('one event pixel', ev, 2))
    return [(name, ev, up, rr.base_image(ev, up)) for name, ev, up in cases]


def test_base_render_vs_restatement(gpu, base_cases):
    from leod_amd import ops
    seen = set()
    for name, ev, up, want in base_cases:
        got = ops.render_frames(ev.to(DEV), upsample=up)
        assert got.dtype is torch.uint8 and tuple(got.shape) == want.shape, name
        got = got.cpu().numpy()
        assert np.array_equal(got, want), f'{name}: {int((got != want).sum())} bytes differ'
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2]), name
        seen |= set(np.unique(want).tolist())
    assert seen == REACHABLE, sorted(REACHABLE - seen)
    name, ev, up, want = base_cases[7]
    assert name.startswith('all-zero') and (want[0] == 255).all() and (want[1] == 64).all()
    # into a caller's buffer, and through the module's own entry point
    from leod_amd.visualize import event2rgb
    name, ev, up, want = base_cases[0]
    out = torch.zeros(want.shape, dtype=torch.uint8, device=DEV)
    assert ops.render_frames(ev.to(DEV), upsample=2, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(event2rgb(ev.to(DEV)).cpu().numpy(), want)


def test_base_render_gen1_size(gpu):
    """One call at the real frame size: 72 960 bytes per plane, the 16-byte path of the mask pass and the 4-pixel path of the render."""
    from leod_amd import ops
    ev = events((2, 20, 240, 304), torch.Generator().manual_seed(1))
    want = rr.base_image(ev, 2)
    got = ops.render_frames(ev.to(DEV)).cpu().numpy()
    assert got.shape == (2, 480, 608, 3) and np.array_equal(got, want)
    assert set(np.unique(want).tolist()) == REACHABLE


def test_entry_point_refuses_bad_arguments(gpu):
    from leod_amd._lib import lib
    L, C2, H, W = 1, 2, 2, 4
    ev = torch.zeros((L, C2, H, W), dtype=torch.uint8, device=DEV)
    out = torch.zeros((L, 2 * H, 2 * W, 3), dtype=torch.uint8, device=DEV)
    ws = torch.zeros((L * H * W,), dtype=torch.uint8, device=DEV)
    fo = torch.zeros((L + 1,), dtype=torch.int32, device=DEV)
    it = torch.zeros((1, 8), dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    f = lib().leod_render_frames_u8
    e, o, w = ev.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert f(e, 0, o, L, C2, H, W, 3, None, None, 0, None, 0, w, s) == -1
    assert f(e, 0, o, L, C2, H, W, 0, None, None, 0, None, 0, w, s) == -1
    assert f(e, 0, o, L, 3, H, W, 2, None, None, 0, None, 0, w, s) == -1
    assert f(e, 0, o, 0, C2, H, W, 2, None, None, 0, None, 0, w, s) == -1
    assert f(e, 0, o, L, C2, 0, W, 2, None, None, 0, None, 0, w, s) == -1
    assert f(e, 0, o, L, C2, H, -1, 2, None, None, 0, None, 0, w, s) == -1
    assert f(None, 0, o, L, C2, H, W, 2, None, None, 0, None, 0, w, s) == -1
    assert f(e, 0, None, L, C2, H, W, 2, None, None, 0, None, 0, w, s) == -1
    assert f(e, 0, o, L, C2, H, W, 2, None, it.data_ptr(), 1, None, 0, w, s) == -1
    assert f(e, 0, o, L, C2, H, W, 2, fo.data_ptr(), None, 1, None, 0, w, s) == -1
    assert f(e, 0, o, L, C2, H, W, 2, None, None, 0, None, 0, w, s) == 0
    torch.cuda.synchronize()
    assert int(out.min()) == 255


def overlay_case():
    """[3, 4, 12, 20] at up = 2 -> frames of 24 x 40.  Frame 1 has no items."""
    R, G, B, K = rr.rgb(255, 0, 0), rr.rgb(0, 255, 0), rr.rgb(0, 0, 255), rr.rgb(0, 0, 0)
    text = bytearray()

    def txt(f, x, y, scale, s, col):
        raw = s if isinstance(s, bytes) else s.encode()
        row = [f, rr.TEXT, x, y, scale, len(text), len(raw), col]
        text.extend(raw)
        return row
    f0 = [[0, rr.RECT, 4, 3, 20, 15, 1, R],                                # thickness 1
          [0, rr.RECT, 8, 6, 30, 20, 2, G],                                # thickness 2, overlaps the first: the later one wins
          [0, rr.RECT, -6, -4, 9, 7, 2, B],                                # negative corners
          [0, rr.RECT, 33, 17, 47, 30, 1, K],                              # past the right and the bottom edge
          [0, rr.RECT, 60, 50, 70, 60, 2, R],                              # wholly outside
          [0, rr.RECT, 25, 2, 25, 12, 1, B],                               # x == a
          [0, rr.RECT, 38, 10, 34, 4, 1, G],                               # swapped corners
          txt(0, 2, 23, 1, 'car 0.5', K)]
    f2 = [[2, rr.RECT, 10, 10, 12, 12, 2, R],                              # thickness 2 on a 3 x 3 box: no interior left
          [2, rr.RECT, 11, 9, 30, 16, 3, B],                               # thickness 3, on top of it
          txt(2, 1, 14, 2, 'Hg', G),                                       # scale 2
          txt(2, -3, 9, 1, 'left', K),                                     # clipped at the left border
          txt(2, 30, 8, 1, 'right', R),                                    # ... the right
          txt(2, 12, 3, 1, 'top', B),                                      # ... the top
          txt(2, 15, 27, 1, 'bottom', R),                                  # ... the bottom
          txt(2, 31, 30, 2, 'q|', K),                                      # scale 2, clipped right and bottom
          txt(2, 2, 22, 1, b'a\x7f\x05\xffb', G)]                          # bytes outside the table: solid blocks
    items = np.asarray(f0 + f2, dtype=np.int32)
    return [0, len(f0), len(f0), len(f0) + len(f2)], items, bytes(text)


def test_overlays_vs_restatement(gpu):
    from leod_amd import ops
    ev = events((3, 4, 12, 20), torch.Generator().manual_seed(2))
    frame_off, items, text = overlay_case()
    base = rr.base_image(ev, 2)
    want = rr.draw_items(base, frame_off, items, text, rr.font())
    got = ops.render_frames(ev.to(DEV), frame_off, items, text, upsample=2).cpu().numpy()
    assert np.array_equal(got, want), f'{int((got != want).any(-1).sum())} pixels differ'
    assert np.array_equal(got[1], base[1])                                 # the frame without items
    # what the case is meant to exercise did reach the frames
    f0, f2 = want[0], want[2]
    assert f0[3, 4].tolist() == [255, 0, 0] and f0[3, 5].tolist() == [255, 0, 0] and np.array_equal(f0[4, 5], base[0, 4, 5])
    assert f0[5, 7].tolist() == [0, 255, 0] and f0[5, 20].tolist() == [0, 255, 0] and f0[15, 7].tolist() == [0, 255, 0]   # green over red
    assert f0[15, 10].tolist() == [255, 0, 0] and f0[6, 8].tolist() == [0, 0, 255]                                  # blue over green
    assert f0[7, 9].tolist() == [0, 0, 255] and f0[0, 9].tolist() == [0, 0, 255] and f0[0, 8].tolist() == [0, 0, 255]
    assert f0[17, 39].tolist() == [0, 0, 0] and f0[23, 33].tolist() == [0, 0, 0]
    assert all(f0[y, 25].tolist() == [0, 0, 255] for y in range(2, 13))
    assert f0[4, 34].tolist() == [0, 255, 0] and f0[10, 38].tolist() == [0, 255, 0]
    assert (f2 != base[2]).any() and (f2[:, 0] != base[2][:, 0]).any() and (f2[0] != base[2][0]).any()
    assert (f2[:, -1] != base[2][:, -1]).any() and (f2[-1] != base[2][-1]).any()
    # the same overlay at up = 1 (coordinates are output pixels: most of it now falls outside the 12 x 20 frame)
    got1 = ops.render_frames(ev.to(DEV), frame_off, items, text, upsample=1).cpu().numpy()
    assert np.array_equal(got1, rr.draw_items(rr.base_image(ev, 1), frame_off, items, text, rr.font()))


def many_items_case(Ho, Wo, n0, n1, seed):
    """Two frames of Ho x Wo: ``n0`` random rectangles and text lines on frame 0 (thickness / scale 1..3, a share of them partly or
    wholly outside), ``n1`` on frame 1.  Returns (frame_off, items, text)."""
    rng = np.random.RandomState(seed)
    text = bytearray()
    rows = []
    for f, n in ((0, n0), (1, n1)):
        for _ in range(n):
            col = int(rng.randint(0, 1 << 24))
            if rng.rand() < 0.5:
                x, y = int(rng.randint(-20, Wo + 10)), int(rng.randint(-20, Ho + 10))
                w, h = int(rng.randint(0, max(Wo // 3, 4))), int(rng.randint(0, max(Ho // 3, 4)))
                a, b = (x + w, y + h) if rng.rand() < 0.8 else (x - w, y - h)
                rows.append([f, rr.RECT, x, y, a, b, int(rng.randint(1, 4)), col])
            else:
                raw = bytes(rng.randint(0x20, 0x7F, size=int(rng.randint(1, 12))).astype(np.uint8))
                rows.append([f, rr.TEXT, int(rng.randint(-30, Wo)), int(rng.randint(0, Ho + 15)), int(rng.randint(1, 4)), len(text), len(raw), col])
                text.extend(raw)
    return [0, n0, n0 + n1], np.asarray(rows, dtype=np.int32), bytes(text)


def test_overlays_across_blocks_and_item_batches(gpu):
    """A Gen1-sized call, [2, 20, 240, 304] at up = 2: a frame of 480 x 608 is 72 960 groups of four pixels = 72 steps of 1 024 groups
    (6.7 rows each) spread over the blocks, so the row culling does drop items, boxes and text lines straddle step boundaries, and frame 0
    carries 600 items: three batches of 256 in the culling, with later-wins overlaps between items of different batches."""
    from leod_amd import ops
    Ho, Wo = 480, 608
    ev = events((2, 20, 240, 304), torch.Generator().manual_seed(5))
    frame_off, items, text = many_items_case(Ho, Wo, 600, 40, seed=6)
    # the same rectangle at item 3 (red), item 300 (green) and item 590 (blue), one pixel wider each time: what is left of each ring is known
    for i, (grow, col) in zip((3, 300, 590), ((0, rr.rgb(255, 0, 0)), (1, rr.rgb(0, 255, 0)), (2, rr.rgb(0, 0, 255)))):
        items[i] = [0, rr.RECT, 100 - grow, 50, 300, 200 + grow, 3, col]
    # a text line at item 10 and the same line in another colour at item 520; a step boundary (row 6.7) runs through a scale-3 line at y = 21
    text = text + b'straddle'
    for i, col in ((10, rr.rgb(1, 2, 3)), (520, rr.rgb(200, 100, 50))):
        items[i] = [0, rr.TEXT, 40, 21, 3, len(text) - 8, 8, col]
    base = rr.base_image(ev, 2)
    want = rr.draw_items(base, frame_off, items, text, rr.font())
    got = ops.render_frames(ev.to(DEV), frame_off, items, text, upsample=2).cpu().numpy()
    assert np.array_equal(got, want), f'{int((got != want).any(-1).sum())} pixels differ, first at {np.argwhere((got != want).any(-1))[:3].tolist()}'
    # the case does what it says: most of the frame is overdrawn, and the later of the planted items is what shows (unless a still later random
    # item covers the pixel: the probes below were checked against the expectation, which is computed independently of the kernel)
    assert (want[0] != base[0]).any(-1).mean() > 0.3 and (want[1] != base[1]).any()
    later = rr.draw_items(base, [0, 10, 10], items[590 - 9:591], text, rr.font())          # the ten last-but-nine items alone, item 590 among them
    ring = (later[0] == np.array([0, 0, 255], dtype=np.uint8)).all(-1) & ~(base[0] == np.array([0, 0, 255], dtype=np.uint8)).all(-1)
    assert ring.sum() > 500                                                # item 590's ring exists ...
    still = ring & (want[0] == np.array([0, 0, 255], dtype=np.uint8)).all(-1)
    assert still.sum() > 100                                               # ... and survives the nine items behind it on many pixels, above items 3 and 300


@pytest.mark.parametrize('shape,up', [((2, 4, 5, 7), 2), ((2, 4, 5, 7), 1), ((2, 4, 9, 6), 1)])
def test_overlays_on_rows_that_are_no_multiple_of_four_pixels(gpu, shape, up):
    """Output rows of 14, 7 and 6 pixels: the one-pixel-per-thread render path with items."""
    from leod_amd import ops
    Ho, Wo = up * shape[2], up * shape[3]
    assert Wo % 4
    ev = events(shape, torch.Generator().manual_seed(7))
    frame_off, items, text = many_items_case(Ho, Wo, 12, 5, seed=8 + up)
    items[0] = [0, rr.RECT, 1, 1, Wo - 2, Ho - 2, 1, rr.rgb(9, 8, 7)]
    items[1] = [0, rr.TEXT, 0, 7, 1, 0, min(2, len(text)), rr.rgb(250, 0, 250)]
    base = rr.base_image(ev, up)
    want = rr.draw_items(base, frame_off, items, text, rr.font())
    got = ops.render_frames(ev.to(DEV), frame_off, items, text, upsample=up).cpu().numpy()
    assert np.array_equal(got, want), f'{int((got != want).any(-1).sum())} pixels differ'
    assert (want[0] != base[0]).any() and (want[1] != base[1]).any()


class Labels:
    def __init__(self, xyxy, cls):
        self.xyxy, self.cls = torch.tensor(xyxy, dtype=torch.float32), torch.tensor(cls, dtype=torch.float32)

    def get_xyxy(self):
        return self.xyxy

    def get(self, name):
        return self.cls


def test_render_sequence(gpu, monkeypatch):
    """9 frames, 2 labelled: the frame count follows the schedule, every shown frame equals a direct render of its own inputs, and the
    chunks of 4 rendered frames meet inside the sequence."""
    from leod_amd import ops, visualize as V
    L, H, W = 9, 12, 20
    ev = events((L, 4, H, W), torch.Generator().manual_seed(3)).to(DEV)
    g = torch.Generator().manual_seed(4)
    preds = []
    for i in range(L):
        n = i % 3
        xy = torch.rand((n, 2), generator=g) * torch.tensor([W - 8.0, H - 7.0])
        wh = 5.5 + torch.rand((n, 2), generator=g) * 3
        rest = torch.cat([torch.rand((n, 2), generator=g), torch.randint(0, 2, (n, 1), generator=g).float()], 1)
        preds.append(torch.cat([xy, xy + wh, rest], 1).to(DEV) if n else None)
    labels = [None] * L
    labels[2], labels[7] = Labels([[1.5, 2.5, 9.0, 8.0]], [1.0]), Labels([[3.0, 1.0, 15.5, 10.0], [0.0, 0.0, 6.0, 6.0]], [0.0, 1.0])
    label_map = ('car', 'ped')

    def filter_fn(b):                                                      # keeps the left half: both colours occur
        if b is None or len(b) == 0:
            return None, None
        left = b[:, 0] < W / 2
        return b[left], b[~left]
    calls = []
    inner = ops.render_frames
    monkeypatch.setattr(V.ops, 'render_frames', lambda ev, *a, **k: (calls.append(ev.shape[0]), inner(ev, *a, **k))[1])
    monkeypatch.setattr(V, 'RENDER_CHUNK', 4)
    video, next_t = V.render_sequence(preds, ev, labels, filter_fn, label_map, prev_t=1.0)
    shown = V.video_frame_indices([l is not None for l in labels], 2)
    assert len(shown) == 11 and video.shape == (len(shown), 2 * H, 2 * W, 3) and video.dtype == np.uint8
    assert next_t == pytest.approx(1.0 + L * 0.05)
    distinct = sorted(set(shown))
    assert calls == [4] * (len(distinct) // 4) + ([len(distinct) % 4] if len(distinct) % 4 else []) and len(calls) >= 2
    table = rr.font()
    for k in (0, len(shown) - 1, shown.index(2), shown.index(7)):
        i = shown[k]
        kp, rm = filter_fn(None if preds[i] is None else preds[i].cpu())
        fo, items, text = V.build_items([kp], [rm], [labels[i]], label_map, [1.0 + i * 0.05], 2)
        direct = inner(ev[i:i + 1], fo, items, text, upsample=2).cpu().numpy()[0]
        assert np.array_equal(video[k], direct), f'video frame {k} (source {i})'
        assert np.array_equal(direct, rr.draw_items(rr.base_image(ev[i:i + 1], 2), fo, items, text, table)[0])
    assert shown[0] == 0
    held = [k for k, i in enumerate(shown) if i == 2]
    assert len(held) >= 3 and all(np.array_equal(video[k], video[held[0]]) for k in held)


HW = (60, 90)


def test_run_visualization(gpu, manifest, tmp_path):
    """Three short synthetic Gen1 recordings in the test split: the first one streamed is skipped (the rule of vis_pred.py:270-272), the other two
    are written -- PNG files of the upsampled frame size, ``frames.json`` in step with them, and with ``reverse`` the side-by-side
    frames.  The model is a randomly initialised micro network with a confidence threshold low enough for boxes to appear."""
    from oracle.synth import synth_recording, synth_state_dict
    from leod_amd.config import vis_config, dynamically_modify_train_config
    from leod_amd.modules.utils.fetch import fetch_model_module, fetch_data_module
    from leod_amd import visualize as V
    tree = str(tmp_path / 'gen1')
    recs = [('rec_a', 11, 6, [2]), ('rec_b', 12, 11, [1, 9]), ('rec_c', 13, 7, [3])]
    for split in ('train', 'val', 'test'):
        for name, seed, n, lab in recs:
            synth_recording(os.path.join(tree, split), name, seed, n, lab, dst_name='gen1', frame_hw=HW)
    over = dict(model=dict(backbone=dict(embed_dim=16, stage=dict(attention=dict(dim_head=8)))), dataset=dict(path=tree), num_video=2)
    cfg = dynamically_modify_train_config(vis_config('gen1', 'small', overrides=over))
    cfg.dataset.ev_repr_hw = HW
    cfg.model.backbone.in_res_hw = (64, 96)
    cfg.model.backbone.stage.attention.partition_size = (2, 3)
    cfg.model.postprocess.confidence_threshold = 0.001
    mod = fetch_model_module(cfg)
    mod.mdl.load_state_dict(synth_state_dict(manifest['micro'], 8))
    mod.to(DEV)
    seen = []
    inner = V.build_items
    try:
        V.build_items = lambda *a, **k: (lambda r: (seen.append(int((r[1][:, 1] == 0).sum())), r)[1])(inner(*a, **k))
        out = V.run_visualization(cfg, mod, fetch_data_module(cfg, prefetch=1), str(tmp_path / 'vis'), reverse=True, sequence_length=8)
    finally:
        V.build_items = inner
    assert sum(seen) > 3, 'no box was drawn: lower the confidence threshold'
    # the documented side effects and departures: 2 / 400 of three recordings would select none -> every recording; the caller's config is changed
    assert cfg.dataset.test_ratio == -1 and cfg.dataset.sequence_length == 8 and cfg.batch_size.eval == 1
    assert cfg.hardware.num_workers.eval == 1 and cfg.dataset.reverse_event_order is False
    # which recording the loader streams first is the loader's business (it deals the longest out first); that one is skipped
    shown = out['recordings']
    assert len(shown) == 2 and len(set(shown)) == 2 and set(shown) < {r[0] for r in recs} and out['both'] == shown
    skipped = ({r[0] for r in recs} - set(shown)).pop()
    assert out['dir'] == os.path.join(str(tmp_path / 'vis'), 'gen1_rnndet_dim16', 'pred_reverse')
    assert sorted(os.listdir(out['dir'])) == sorted(shown + [n + '_both' for n in shown]), f'{skipped} must not be written'
    Hp, Wp = 2 * HW[0], 2 * HW[1]
    for name, _, n, lab in (r for r in recs if r[0] in shown):
        for sub, width in ((name, Wp), (name + '_both', 2 * Wp + 5)):
            d = os.path.join(out['dir'], sub)
            meta = json.load(open(os.path.join(d, 'frames.json')))
            files = sorted(f for f in os.listdir(d) if f.endswith('.png'))
            assert meta['fps'] == 15 and [m['file'] for m in meta['frames']] == files == [f'{k:05d}.png' for k in range(len(files))]
            for fn in (files[0], files[-1]):
                assert V.read_png(os.path.join(d, fn)).shape == (Hp, width, 3)
            src = [m['source_frame'] for m in meta['frames']]
            assert src == sorted(src) and 0 <= src[0] and src[-1] < n and (sub != name or set(lab) <= set(src))
            assert all(m['t'] == pytest.approx(0.05 * m['source_frame']) for m in meta['frames'])
        # the samples of 8 frames each contribute their own schedule (vis_pred.py applies [::2] per sample)
        want = []
        for lo in range(0, n, 8):
            want += [lo + i for i in V.video_frame_indices([lo + j in lab for j in range(min(8, n - lo))], 2)]
        assert [m['source_frame'] for m in json.load(open(os.path.join(out['dir'], name, 'frames.json')))['frames']] == want
        both = V.read_png(os.path.join(out['dir'], name + '_both', '00000.png'))
        assert np.array_equal(both[:, :Wp], V.read_png(os.path.join(out['dir'], name, '00000.png'))) and not both[:, Wp:Wp + 5].any()
