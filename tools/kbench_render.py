#!/usr/bin/env python
"""The frame renderer at the chunk size of a Gen1 prediction video, [128, 20, 240, 304] uint8 -> [128, 480, 608, 3] uint8:
 (a) ``ops.render_frames`` without overlay items,
 (b) ``ops.render_frames`` with 10 boxes per frame (a rectangle and three text lines each) and a timestamp line,
 (c) the reference's formulation of the base image with torch ops on the same device (vis_pred.py:74-93: channel sums, mask, fp32
     canvas, F.interpolate x2, round, uint8) followed by the permute to HWC -- the only other way to these pixels.
Device events around windows of back-to-back calls on one stream, the variants alternating window by window; prints the median, minimum
and maximum time per call and the achieved bytes/s against the algorithmic bytes (the events read once + the frames written once).
(a) and (b) are whole ``ops.render_frames`` calls: the host-side check and the upload of the overlay arrays and the allocation of the mask
workspace are inside, so their bytes/s are over call time, not kernel time; (b*) is (b) with the overlay arrays already on the device: the
two kernel launches alone.  Not timed: what ``visualize.render_sequence`` does around the call (the Python loop of ``build_items``, the
gather of the shown frames' events, the device -> host copy of the frames).
usage: python tools/kbench_render.py [calls per window] [windows]"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
from leod_amd import ops  # noqa: E402
from leod_amd._lib import lib, check  # noqa: E402
from leod_amd.visualize import build_items  # noqa: E402

DEV = 'cuda'
N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WINDOWS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
L, C, H, W = 128, 20, 240, 304
BOXES = 10
assert torch.cuda.is_available(), 'kbench_render needs the GPU'
g = torch.Generator().manual_seed(3)
ev = ((torch.rand((L, C, H, W), generator=g) < 0.02) * torch.randint(1, 12, (L, C, H, W), generator=g)).to(torch.uint8).to(DEV)
rng = np.random.RandomState(4)
preds = []
for _ in range(L):
    xy = rng.uniform(0, 1, (BOXES, 2)) * [W - 80, H - 60]
    wh = rng.uniform(20, 80, (BOXES, 2)) * [1.0, 0.75]
    preds.append(np.concatenate([xy, xy + wh, rng.uniform(0, 1, (BOXES, 2)), rng.randint(0, 2, (BOXES, 1))], 1).astype(np.float32))
frame_off, items, text = build_items(preds, [None] * L, [None] * L, ('car', 'ped'), [0.05 * i for i in range(L)], 2)
out = torch.empty((L, 2 * H, 2 * W, 3), dtype=torch.uint8, device=DEV)


def torch_base():
    e = ev.reshape(L, 2, C // 2, H, W)
    pos, neg = e[:, 0].sum(1, keepdim=True), e[:, 1].sum(1, keepdim=True)
    img = torch.ones((L, 3, H, W), dtype=torch.float32, device=DEV)
    img[((pos > 0) | (neg > 0)).repeat(1, 3, 1, 1)] = 0.25
    img = F.interpolate(img, scale_factor=2, mode='bilinear', align_corners=False)
    return torch.round(img * 255.).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


d_fo, d_it, d_tx = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (frame_off, items, text))
ws = torch.empty((L * H * W,), dtype=torch.uint8, device=DEV)


def kernels_only():
    check(lib().leod_render_frames_u8(ev.data_ptr(), 0, out.data_ptr(), L, C, H, W, 2, d_fo.data_ptr(), d_it.data_ptr(), len(items),
                                      d_tx.data_ptr(), d_tx.numel(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream), 'render')
    return out


launch = {
    '(a) render_frames, no items': lambda: ops.render_frames(ev, out=out),
    f'(b) render_frames, {len(items)} items': lambda: ops.render_frames(ev, frame_off, items, text, out=out),
    '(b*) the two launches of (b) alone': kernels_only,
    '(c) torch ops (reference formulation)': torch_base,
}
assert torch.equal(launch['(a) render_frames, no items'](), torch_base()), 'the two base images differ'
assert torch.equal(ops.render_frames(ev, frame_off, items, text), kernels_only()), 'the two overlay paths differ'
times = {k: [] for k in launch}
for fn in launch.values():                                      # warm-up: code object load, allocator pools
    for _ in range(3):
        fn()
torch.cuda.synchronize()
for _ in range(WINDOWS):
    for k, fn in launch.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / N)
nbytes = ev.numel() + out.numel()
print(f'events {[L, C, H, W]} uint8 -> frames {list(out.shape)} uint8, {len(items)} items ({BOXES} boxes per frame), '
      f'{nbytes / 1e6:.1f} MB algorithmic, {N} calls per window, {WINDOWS} windows')
for k, v in times.items():
    v = sorted(v)
    med = v[len(v) // 2]
    print(f'{k:<42} median {med:9.1f} us  (min {v[0]:.1f}, max {v[-1]:.1f})  {nbytes / med / 1e6:6.3f} TB/s of the algorithmic bytes')
