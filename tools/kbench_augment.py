#!/usr/bin/env python
"""The two augmentation gather launches at the training shape [21, 8, 20, 240, 304] uint8: ``leod_augment_u8`` with eight zoom-in
states and ``leod_augment_rot_u8`` with eight rotated samples (rotation only, and rotation + hflip + zoom-in).
Device events around windows of back-to-back launches on one stream (the host enqueues faster than the kernels run), the variants
alternating window by window; prints the median, minimum and maximum window per launch and the bytes moved per second.
usage: python tools/kbench_augment.py [launches per window] [windows]"""
import os, sys
import torch
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
from leod_amd._lib import lib, check  # noqa: E402
from leod_amd.data.utils.augmentor import (AugmentationState, RotationState, ZoomInState, state_to_params, state_to_rot)  # noqa: E402

DEV = 'cuda'
N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
WINDOWS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
T, B, C, H, W = 21, 8, 20, 240, 304
g = torch.Generator().manual_seed(3)
ev = ((torch.rand((T, B, C, H, W), generator=g) < 0.15) * torch.randint(1, 12, (T, B, C, H, W), generator=g)).to(torch.uint8).to(DEV)
angles = [4.0, -7.5, 11.0, -15.0, 19.0, -2.5, 6.0, -12.0]
zooms = [ZoomInState(True, 10 + 5 * b, 8 + 3 * b, 1.1 + 0.05 * b) for b in range(B)]
variants = {
    'augment_u8      zoom-in x8': [AugmentationState(zoom_in=z) for z in zooms],
    'augment_rot_u8  rotation x8': [AugmentationState(rotation=RotationState(True, a)) for a in angles],
    'augment_rot_u8  rot+hflip+zoom-in x8': [AugmentationState(apply_h_flip=True, rotation=RotationState(True, a), zoom_in=z)
                                             for a, z in zip(angles, zooms)],
}
out = torch.empty_like(ev)
stream = torch.cuda.current_stream().cuda_stream


def launcher(name, states):
    """The launch ``augment_events`` makes for these states, with the parameter blocks uploaded once."""
    params = torch.tensor([state_to_params(s, (H, W)) for s in states], dtype=torch.int32).to(DEV)
    if name.startswith('augment_rot_u8'):
        rot = torch.tensor([state_to_rot(s) for s in states], dtype=torch.float32).to(DEV)
        return lambda: check(lib().leod_augment_rot_u8(ev.data_ptr(), out.data_ptr(), params.data_ptr(), rot.data_ptr(), T, B, C, H, W,
                                                       stream), name)
    return lambda: check(lib().leod_augment_u8(ev.data_ptr(), out.data_ptr(), params.data_ptr(), T, B, C, H, W, stream), name)


launch = {k: launcher(k, st) for k, st in variants.items()}
times = {k: [] for k in variants}
for fn in launch.values():                                      # warm-up: code object load
    for _ in range(5):
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
nbytes = 2 * ev.numel()
print(f'shape {[T, B, C, H, W]}, {N} launches per window, {WINDOWS} windows')
for k, v in times.items():
    v = sorted(v)
    med = v[len(v) // 2]
    print(f'{k:<40} median {med:8.1f} us  (min {v[0]:.1f}, max {v[-1]:.1f})  {nbytes / med / 1e6:7.2f} TB/s read+write')
