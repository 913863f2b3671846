#!/usr/bin/env python
"""The JPEG encoder at the chunk size of a Gen1 prediction video: [128, 480, 608, 3] uint8 frames as ``ops.render_frames`` draws them, with
10 boxes each (a rectangle and three text lines) and a timestamp, at quality 90.
 (a)  the launches alone: ``leod_jpeg_scan`` + ``leod_jpeg_emit`` over all 128 frames, workspace and output allocated beforehand, no read-back,
 (b)  ``ops.encode_jpeg`` with its default workspace bound of 16 MiB (sub-chunks of a few frames, one read-back each),
 (b+) ``ops.encode_jpeg`` with a workspace that takes the 128 frames at once (one read-back),
 (c)  what ``--video avi`` does per chunk: (b) plus the copy of blob and offsets to the host and the cut into files (``visualize.encode_frames``),
 (d)  what ``--video png`` does per chunk: the device -> host copy of the frames, then ``write_png`` of each to the null device (zlib on one
      host thread; no disk),
 (e)  Pillow's encoder on the host at the same quality and 4:4:4, after the same device -> host copy -- only if Pillow is installed.
Wall-clock time per call around a synchronised device, the variants alternating window by window; prints median, minimum and maximum, and the
bytes per frame of (b).  (d) and (e) run once per window: they take seconds.
usage: python tools/kbench_jpeg.py [calls per window] [windows]"""
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
from leod_amd import ops  # noqa: E402
from leod_amd._lib import lib, check  # noqa: E402
from leod_amd.visualize import build_items, encode_frames, write_png  # noqa: E402

DEV = 'cuda'
N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WINDOWS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
L, C, H, W = 128, 20, 240, 304
BOXES, QUALITY = 10, 90
assert torch.cuda.is_available(), 'kbench_jpeg needs the GPU'
g = torch.Generator().manual_seed(3)
ev = ((torch.rand((L, C, H, W), generator=g) < 0.02) * torch.randint(1, 12, (L, C, H, W), generator=g)).to(torch.uint8).to(DEV)
rng = np.random.RandomState(4)
preds = []
for _ in range(L):
    xy = rng.uniform(0, 1, (BOXES, 2)) * [W - 80, H - 60]
    wh = rng.uniform(20, 80, (BOXES, 2)) * [1.0, 0.75]
    preds.append(np.concatenate([xy, xy + wh, rng.uniform(0, 1, (BOXES, 2)), rng.randint(0, 2, (BOXES, 1))], 1).astype(np.float32))
frame_off, items, text = build_items(preds, [None] * L, [None] * L, ('car', 'ped'), [0.05 * i for i in range(L)], 2)
frames = ops.render_frames(ev, frame_off, items, text, upsample=2)
Ho, Wo = frames.shape[1:3]

ws_all = ops.jpeg_query(L, Ho, Wo)[0]
blob0, off0 = ops.encode_jpeg(frames, QUALITY)
total = int(off0[-1])
ws = torch.empty((ws_all // 8,), dtype=torch.int64, device=DEV)
out = torch.empty((total,), dtype=torch.uint8, device=DEV)
off = torch.zeros((L + 1,), dtype=torch.int64, device=DEV)


def launches_only():
    s = torch.cuda.current_stream().cuda_stream
    check(lib().leod_jpeg_scan(frames.data_ptr(), L, Ho, Wo, QUALITY, ws.data_ptr(), ws_all, off.data_ptr(), 0, s), 'scan')
    check(lib().leod_jpeg_emit(ws.data_ptr(), ws_all, L, Ho, Wo, QUALITY, out.data_ptr(), total, 0, s), 'emit')
    return out


def png_route():
    host = frames.cpu().numpy()
    for f in host:
        write_png(os.devnull, f)


variants = {
    '(a)  scan + emit launches alone': (launches_only, N),
    '(b)  ops.encode_jpeg, 16 MiB workspace': (lambda: ops.encode_jpeg(frames, QUALITY), N),
    '(b+) ops.encode_jpeg, one sub-chunk': (lambda: ops.encode_jpeg(frames, QUALITY, ws_bytes=ws_all), N),
    '(c)  encode_jpeg + copy + cut (avi route)': (lambda: encode_frames(frames, QUALITY), N),
    '(d)  copy + write_png (png route)': (png_route, 1),
}
try:
    from PIL import Image

    def pillow_route():
        host = frames.cpu().numpy()
        return sum(Image.fromarray(f).save(io.BytesIO(), 'JPEG', quality=QUALITY, subsampling=0) is None for f in host)
    variants['(e)  copy + Pillow JPEG on the host'] = (pillow_route, 1)
except ImportError:
    print('Pillow is not installed here: (e) is left out')

assert torch.equal(launches_only(), blob0) and torch.equal(off, off0), 'the launches alone and ops.encode_jpeg differ'
assert torch.equal(ops.encode_jpeg(frames, QUALITY, ws_bytes=ws_all)[0], blob0), 'one sub-chunk and many differ'
files = encode_frames(frames, QUALITY)
assert len(files) == L and b''.join(files) == blob0.cpu().numpy().tobytes()
times = {k: [] for k in variants}
for k, (fn, n) in variants.items():                             # warm-up: code object load, allocator pools
    if n > 1:
        fn()
torch.cuda.synchronize()
for _ in range(WINDOWS):
    for k, (fn, n) in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) * 1e3 / n)
print(f'frames {list(frames.shape)} uint8 ({frames.numel() / 1e6:.1f} MB), {len(items)} items ({BOXES} boxes per frame), quality {QUALITY}: '
      f'{total} bytes of JPEG files, {total / L:.0f} per frame ({frames.numel() / total:.1f} : 1); workspace of one frame '
      f'{ops.jpeg_query(1, Ho, Wo)[0]} bytes, of all {ws_all}; {WINDOWS} windows')
for k, v in times.items():
    v = sorted(v)
    print(f'{k:<44} median {v[len(v) // 2]:10.3f} ms per call  (min {v[0]:.3f}, max {v[-1]:.3f}; {variants[k][1]} calls per window)')
