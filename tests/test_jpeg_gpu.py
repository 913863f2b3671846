"""The JPEG encoder on the device (``leod_jpeg_scan`` / ``leod_jpeg_emit`` through ``ops.encode_jpeg``) against the sequential restatement
in tests/jpeg_ref.py -- byte for byte, offsets included: the stream is an integer pipeline with fixed tables -- and the Motion-JPEG mode of
leod_amd/visualize.py on top of it.  ``pytest -m gpu``."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_ref as jr  # noqa: E402

DEV = 'cuda'


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return True


def speckle(n, h, w, seed):
    """What the renderer's frames look like: white, 10 % dark speckle, a green and a red one-pixel line."""
    rng = np.random.RandomState(seed)
    a = np.full((n, h, w, 3), 255, dtype=np.uint8)
    a[rng.rand(n, h, w) < 0.1] = 64
    a[:, h // 3, :] = (0, 255, 0)
    a[:, :, w // 2] = (255, 0, 0)
    return a


def noise(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)


def block_alternating(h, w):
    """Black and white from one 8 x 8 block to the next: at quality 100 the DC differences are +-2040, category 11."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy // 8 + xx // 8) % 2) * 255).astype(np.uint8)[None, :, :, None], 3, axis=3)


def primaries(h, w, seed):
    """Every channel of every pixel 0 or 255: the corners of the colour cube, where the conversion reaches 0 and 255."""
    return (np.random.RandomState(seed).randint(0, 2, size=(1, h, w, 3)) * 255).astype(np.uint8)


def checker(h, w):
    """A one-pixel checker of amplitude 20 and one of 30 around 128: at quality 50 a luma block of the first keeps coefficients 53, 60 and 63 (a
    run of 52 zeros: three ZRL), one of the second 4, 11, 42, ... 63 (a run of 30: one ZRL); coefficient 63 is not zero, so no EOB follows."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([np.repeat((128 + a * (1 - 2 * ((yy + xx) % 2))).astype(np.uint8)[:, :, None], 3, axis=2) for a in (20, 30)])


def encode(frames, quality=90, **kw):
    from leod_amd import ops
    blob, off = ops.encode_jpeg(torch.from_numpy(frames).to(DEV), quality, **kw)
    assert blob.dtype is torch.uint8 and off.dtype is torch.int64 and blob.is_cuda and off.is_cuda
    return blob.cpu().numpy(), off.cpu().numpy()


def same(frames, quality=90, **kw):
    got, off = encode(frames, quality, **kw)
    want, want_off = jr.encode_many(frames, quality)
    assert off.tolist() == want_off.tolist(), f'offsets {off.tolist()} != {want_off.tolist()}'
    assert got.shape == want.shape and np.array_equal(got, want), f'first difference at byte {int(np.flatnonzero(got != want)[0])}'
    return want.tobytes()


CASES = {
    'one block': lambda: (speckle(1, 8, 8, 1), 90),
    'partial blocks both ways': lambda: (speckle(2, 13, 21, 2), 90),
    '66 blocks per interval': lambda: (speckle(1, 9, 523, 3), 90),
    'three frames, the second all white': lambda: (np.concatenate([speckle(1, 16, 21, 4), np.full((1, 16, 21, 3), 255, np.uint8),
                                                                   speckle(1, 16, 21, 5)]), 90),
    'noise at quality 100': lambda: (noise(2, 24, 40, 6), 100),
    'blocks alternating at quality 100': lambda: (block_alternating(16, 64), 100),
    'saturated primaries': lambda: (primaries(19, 30, 7), 90),
    'checker': lambda: (checker(16, 24), 50),
    'quality 1': lambda: (noise(1, 13, 21, 8), 1),
    'quality 50': lambda: (speckle(1, 13, 21, 9), 50),
    'noise at quality 90': lambda: (noise(1, 21, 13, 10), 90),
    'one pixel': lambda: (noise(1, 1, 1, 11), 90),
    'one column, 33 rows': lambda: (noise(1, 33, 1, 12), 75),
    '300 blocks per interval, noise': lambda: (noise(1, 8, 2400, 13), 100),
}


@pytest.mark.parametrize('name', list(CASES))
def test_encoder_vs_restatement(gpu, name):
    frames, quality = CASES[name]()
    data = same(frames, quality)
    coef = jr.coefficients(frames[0], quality)
    # the case does what its name says
    if name == 'three frames, the second all white':
        white = jr.coefficients(frames[1], quality)
        assert not white[..., 1:].any() and (white[..., 0] == white[:, :1, :, 0]).all() and white[0, 0, 0, 0] > 0   # every DC difference but the first is 0
    if name == 'noise at quality 100':
        assert data.count(b'\xFF\x00') > 3
    if name == 'blocks alternating at quality 100':
        assert int(np.abs(np.diff(coef[0, :, 0, 0])).max()) >= 1024                      # category 11
    if name == 'saturated primaries':
        ycc = jr.ycc(frames[0])
        assert ycc.min() == 0 and ycc.max() == 255
    if name == 'checker':
        for frame, longest in zip(frames, (52, 30)):
            for blk in jr.coefficients(frame, quality)[:, :, 0].reshape(-1, 64):
                k = np.flatnonzero(blk)
                assert k[-1] == 63 and int(np.diff(np.concatenate([[0], k])).max()) - 1 == longest
    if name == '300 blocks per interval, noise':
        assert len(data) > 300 * 3 * 64                                                  # several steps of 256 units and of 256 bytes per interval


def test_workspace_bound_splits_the_frames(gpu, monkeypatch):
    from leod_amd import ops
    from leod_amd._lib import LeodHipError
    frames = speckle(5, 16, 21, 20)
    frames[3] = noise(1, 16, 21, 21)[0]
    per_frame = ops.jpeg_query(1, 16, 21)[0]
    calls = []
    inner = ops._l().leod_jpeg_scan
    monkeypatch.setattr(ops._l(), 'leod_jpeg_scan', lambda rgb, n, *a: (calls.append(n), inner(rgb, n, *a))[1])
    want, want_off = jr.encode_many(frames, 90)
    for ws_bytes, sub in ((2 * per_frame + 5, [2, 2, 1]), (per_frame, [1] * 5), (5 * per_frame, [5]), (None, [5])):
        del calls[:]
        got, off = encode(frames, 90, ws_bytes=ws_bytes)
        assert calls == sub, (ws_bytes, calls)
        assert np.array_equal(got, want) and off.tolist() == want_off.tolist(), ws_bytes
    with pytest.raises(LeodHipError):
        ops.encode_jpeg(torch.from_numpy(frames).to(DEV), 90, ws_bytes=per_frame - 1)


def test_two_runs_give_the_same_bytes(gpu):
    frames = noise(3, 40, 72, 30)
    a, oa = encode(frames, 95)
    b, ob = encode(frames, 95)
    assert np.array_equal(a, b) and np.array_equal(oa, ob)


def test_caller_buffer(gpu):
    from leod_amd import ops
    from leod_amd._lib import LeodHipError
    frames = noise(3, 13, 21, 40)
    want, want_off = jr.encode_many(frames, 90)
    total = len(want)
    dev_frames = torch.from_numpy(frames).to(DEV)
    per_frame = ops.jpeg_query(1, 13, 21)[0]
    for ws_bytes in (None, per_frame):                                    # one sub-chunk, and one per frame
        buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        blob, off = ops.encode_jpeg(dev_frames, 90, out=buf[:total], ws_bytes=ws_bytes)
        assert blob.data_ptr() == buf.data_ptr() and np.array_equal(blob.cpu().numpy(), want) and off.cpu().tolist() == want_off.tolist()
        assert bool((buf[total:] == 0xA5).all())
        buf = torch.full((total - 1 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        with pytest.raises(LeodHipError):
            ops.encode_jpeg(dev_frames, 90, out=buf[:total - 1], ws_bytes=ws_bytes)
        torch.cuda.synchronize()
        assert bool((buf[total - 1:] == 0xA5).all()), 'bytes behind the end of a short buffer were written'


def test_refuses_bad_arguments(gpu):
    from leod_amd import ops
    from leod_amd._lib import LeodHipError, lib
    good = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    for bad in (good.cpu(), good.float(), good[0], good[..., :2], torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=DEV),
                torch.zeros((1, 8, 16, 3), dtype=torch.uint8, device=DEV)[:, :, ::2]):
        with pytest.raises(LeodHipError):
            ops.encode_jpeg(bad)
    for q in (0, 101, -5, 50.5, True):
        with pytest.raises(LeodHipError):
            ops.encode_jpeg(good, quality=q)
    with pytest.raises(LeodHipError):
        ops.encode_jpeg(good, out=torch.zeros((4096,), dtype=torch.uint8))
    with pytest.raises(LeodHipError):
        ops.encode_jpeg(good, out=torch.zeros((4096,), dtype=torch.int32, device=DEV))
    ws_bytes, bound, hdr = ops.jpeg_query(1, 8, 8)
    assert hdr == len(jr.header(8, 8, 90)) and bound == hdr + 3 * 432 + 2 and ws_bytes % 16 == 0
    ws = torch.zeros((ws_bytes // 8,), dtype=torch.int64, device=DEV)
    off = torch.zeros((2,), dtype=torch.int64, device=DEV)
    out = torch.zeros((bound,), dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    scan, emit = lib().leod_jpeg_scan, lib().leod_jpeg_emit
    g, w, o, b = good.data_ptr(), ws.data_ptr(), off.data_ptr(), out.data_ptr()
    assert scan(None, 1, 8, 8, 90, w, ws_bytes, o, 0, s) == -1
    assert scan(g, 1, 8, 8, 90, None, ws_bytes, o, 0, s) == -1
    assert scan(g, 1, 8, 8, 90, w, ws_bytes, None, 0, s) == -1
    assert scan(g, 0, 8, 8, 90, w, ws_bytes, o, 0, s) == -1
    assert scan(g, 1, 0, 8, 90, w, ws_bytes, o, 0, s) == -1
    assert scan(g, 1, 8, 65536, 90, w, ws_bytes, o, 0, s) == -1
    assert scan(g, 1, 8, 8, 0, w, ws_bytes, o, 0, s) == -1
    assert scan(g, 1, 8, 8, 101, w, ws_bytes, o, 0, s) == -1
    assert scan(g, 1, 8, 8, 90, w, ws_bytes - 1, o, 0, s) == -1
    assert scan(g, 1, 8, 8, 90, w + 8, ws_bytes, o, 0, s) == -1
    assert scan(g, 1, 8, 8, 90, w, ws_bytes, o, -1, s) == -1
    assert emit(None, ws_bytes, 1, 8, 8, 90, b, bound, 0, s) == -1
    assert emit(w, ws_bytes, 1, 8, 8, 90, None, bound, 0, s) == -1
    assert emit(w, ws_bytes - 1, 1, 8, 8, 90, b, bound, 0, s) == -1
    assert emit(w, ws_bytes, 1, 8, 8, 90, b, -1, 0, s) == -1
    assert lib().leod_jpeg_query(1, 8, 70000, None, None, None) == -1
    assert scan(g, 1, 8, 8, 90, w, ws_bytes, o, 0, s) == 0 and emit(w, ws_bytes, 1, 8, 8, 90, b, bound, 0, s) == 0
    torch.cuda.synchronize()
    n = int(off[1])
    assert bytes(out[:n].cpu().numpy()) == jr.encode(np.zeros((8, 8, 3), np.uint8), 90)


def boxes_overlay(n_frames, Ho, Wo, per_frame, seed):
    rng = np.random.RandomState(seed)
    rows = []
    for f in range(n_frames):
        for _ in range(per_frame):
            x, y = int(rng.randint(0, Wo - 40)), int(rng.randint(0, Ho - 40))
            rows.append([f, 0, x, y, x + int(rng.randint(10, 120)), y + int(rng.randint(10, 90)), 2,
                         (0x00FF00, 0x0000FF, 0x000000)[int(rng.randint(0, 3))]])
    return [per_frame * f for f in range(n_frames + 1)], np.asarray(rows, dtype=np.int32)


def test_gen1_size_on_rendered_frames(gpu):
    """[4, 480, 608, 3] with ten boxes a frame: 60 intervals of 76 blocks per frame, the whole-word path of the transform."""
    from leod_amd import ops
    g = torch.Generator().manual_seed(50)
    ev = ((torch.rand((4, 1, 240, 304), generator=g) < 0.1) & (torch.rand((4, 20, 240, 304), generator=g) < 0.5)).to(torch.uint8)
    frame_off, items = boxes_overlay(4, 480, 608, 10, 51)
    frames = ops.render_frames(ev.to(DEV), frame_off, items, b'', upsample=2)
    blob, off = ops.encode_jpeg(frames, 90)
    blob, off = blob.cpu().numpy().tobytes(), off.cpu().tolist()
    first = frames[0].cpu().numpy()
    assert len(np.unique(first.reshape(-1, 3), axis=0)) > 5
    assert blob[off[0]:off[1]] == jr.encode(first, 90)
    assert off[0] == 0 and off[4] == len(blob)
    for i in range(4):
        assert blob[off[i]:off[i] + 2] == b'\xFF\xD8' and blob[off[i + 1] - 2:off[i + 1]] == b'\xFF\xD9'
    assert jr.decode(blob[off[3]:off[4]]).shape == (480, 608, 3)


HW = (60, 90)


def test_run_visualization_avi(gpu, manifest, tmp_path):
    """The synthetic Gen1 tree of test_render_gpu.py::test_run_visualization, once as PNG files and once as Motion-JPEG: the same frames in
    the same order, every video frame the JPEG file of the PNG's pixels, ``frames.json`` in step, and the side-by-side video of ``reverse``
    (width 2 * 180 + 5 = 365: partial blocks at the right edge)."""
    from oracle.synth import synth_recording, synth_state_dict
    from leod_amd.config import vis_config, dynamically_modify_train_config
    from leod_amd.modules.utils.fetch import fetch_model_module, fetch_data_module
    from leod_amd.utils.mjpeg import read_avi_frames
    from leod_amd import ops, visualize as V
    tree = str(tmp_path / 'gen1')
    recs = [('rec_a', 11, 6, [2]), ('rec_b', 12, 11, [1, 9]), ('rec_c', 13, 7, [3])]
    for split in ('train', 'val', 'test'):
        for name, seed, n, lab in recs:
            synth_recording(os.path.join(tree, split), name, seed, n, lab, dst_name='gen1', frame_hw=HW)

    def run(out, **kw):
        over = dict(model=dict(backbone=dict(embed_dim=16, stage=dict(attention=dict(dim_head=8)))), dataset=dict(path=tree), num_video=2)
        cfg = dynamically_modify_train_config(vis_config('gen1', 'small', overrides=over))
        cfg.dataset.ev_repr_hw = HW
        cfg.model.backbone.in_res_hw = (64, 96)
        cfg.model.backbone.stage.attention.partition_size = (2, 3)
        cfg.model.postprocess.confidence_threshold = 0.001
        mod = fetch_model_module(cfg)
        mod.mdl.load_state_dict(synth_state_dict(manifest['micro'], 8))
        mod.to(DEV)
        return V.run_visualization(cfg, mod, fetch_data_module(cfg, prefetch=1), str(tmp_path / out), reverse=True, sequence_length=8, **kw)
    png = run('png')
    avi = run('avi', video='avi', jpeg_quality=85)
    assert avi['recordings'] == png['recordings'] and avi['both'] == png['both'] and len(avi['recordings']) == 2
    assert sorted(os.listdir(avi['dir'])) == sorted(n + s + e for n in avi['recordings'] for s in ('', '_both') for e in ('.avi', '.frames.json'))
    Hp, Wp = 2 * HW[0], 2 * HW[1]
    for name in avi['recordings']:
        for sub, width in ((name, Wp), (name + '_both', 2 * Wp + 5)):
            meta_png = json.load(open(os.path.join(png['dir'], sub, 'frames.json')))
            meta_avi = json.load(open(os.path.join(avi['dir'], sub + '.frames.json')))
            assert meta_avi['fps'] == meta_png['fps'] == 15 and meta_avi['video'] == [sub + '.avi']
            assert len(meta_avi['frames']) == len(meta_png['frames']) > 0
            for k, (a, p) in enumerate(zip(meta_avi['frames'], meta_png['frames'])):
                assert a == {'frame': k, 'source_frame': p['source_frame'], 't': p['t']} and set(p) == {'file', 'source_frame', 't'}
            frames = read_avi_frames(os.path.join(avi['dir'], sub + '.avi'))
            assert len(frames) == len(meta_png['frames'])
            pixels = np.stack([V.read_png(os.path.join(png['dir'], sub, p['file'])) for p in meta_png['frames']])
            assert pixels.shape[1:] == (Hp, width, 3)
            blob, off = ops.encode_jpeg(torch.from_numpy(pixels).to(DEV), 85)
            blob, off = blob.cpu().numpy().tobytes(), off.cpu().tolist()
            for k, f in enumerate(frames):
                assert f == blob[off[k]:off[k + 1]], f'{sub}: frame {k}'
                assert f[:2] == b'\xFF\xD8' and f[158:160] == b'\xFF\xC0' and (f[163] << 8 | f[164], f[165] << 8 | f[166]) == (Hp, width)   # SOF0
            back = jr.decode(frames[0])
            assert back.shape == (Hp, width, 3)
            assert frames[0] == jr.encode(pixels[0], 85)
    # the PNG mode with its default arguments is what it was: no video files in its tree
    assert not [f for _, _, fs in os.walk(png['dir']) for f in fs if f.endswith('.avi')]
    with pytest.raises(ValueError):
        V.run_visualization(None, None, None, str(tmp_path / 'x'), num_video=1, reverse=False, video='mp4')
