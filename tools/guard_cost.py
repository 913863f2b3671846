#!/usr/bin/env python
"""What the non-finite guard costs per optimiser step: ``leod_adamw_clip_step`` (one launch) against ``leod_grad_stats`` +
``leod_adamw_clip_step_guarded`` (two + two launches) over a flat buffer of the size of RVT-S, 9.87 M parameters cut into 400
parameter-like segments (a few large matrices, many short vectors).
Device events around windows of back-to-back optimiser phases on one stream, the two variants alternating window by window; prints the
median, minimum and maximum window per phase, the bytes each moves per second and the difference.  Gradients are finite, so the
guarded step is taken every time (the case a training run pays for).
usage: python tools/guard_cost.py [phases per window] [windows] [parameters]"""
import os, sys
import torch
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
from leod_amd import ops  # noqa: E402

assert torch.cuda.is_available(), 'guard_cost.py measures on the GPU; there is nothing to report without one'
DEV = 'cuda'
N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
WINDOWS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
PARAMS = int(sys.argv[3]) if len(sys.argv) > 3 else 9_870_000
NSEG = 400

# 400 segments: 40 matrices share 98 % of the parameters, 360 vectors of 48 .. 1152 floats the rest (the shape of the RVT-S list)
small = [48 * (1 + (i * 7) % 24) for i in range(NSEG - 40)]
big = (PARAMS - sum(small)) // 40
lengths = small[:180] + [big] * 39 + [PARAMS - sum(small) - 39 * big] + small[180:]
offsets, n = [], 0
for k in lengths:
    offsets.append(n)
    n += (k + 3) // 4 * 4
gen = torch.Generator().manual_seed(7)
p = torch.randn(n, generator=gen).to(DEV)
g0 = (torch.randn(n, generator=gen) * 1e-2).to(DEV)
g, m, v = g0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
plan = ops.GradStatsPlan(offsets, lengths, DEV)
state, scratch = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(8, device=DEV)
HP = dict(weight_decay=0.01, clip_value=1.0, grad_scale=1.0)
step = [0]


def plain():
    step[0] += 1
    ops.adamw_clip_step(p, g, m, v, 2e-4, step[0], **HP)


def guarded():
    _, _, total = ops.grad_stats(g, plan)
    ops.adamw_clip_step_guarded(p, g, m, v, 2e-4, total, state, scratch, **HP)


def stats_only():
    ops.grad_stats(g, plan)


variants = {'adamw_clip_step': (plain, 28), 'grad_stats + adamw_clip_step_guarded': (guarded, 32), 'grad_stats alone': (stats_only, 4)}
times = {k: [] for k in variants}
for fn, _ in variants.values():                               # warm-up: code object load
    for _ in range(5):
        fn()
torch.cuda.synchronize()
assert int(plan.total.cpu()[0]) == 0 and state.cpu().tolist()[1] == 0
for _ in range(WINDOWS):
    for k, (fn, _) in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / N)
print(f'{n} floats in {NSEG} segments ({plan.nchunk} chunks of {ops.GRAD_STATS_CHUNK}), {N} phases per window, {WINDOWS} windows')
med = {}
for k, t in times.items():
    t = sorted(t)
    med[k] = t[len(t) // 2]
    print(f'{k:<40} median {med[k]:8.1f} us  (min {t[0]:.1f}, max {t[-1]:.1f})  {variants[k][1] * n / med[k] / 1e6:6.2f} TB/s at {variants[k][1]} B/param')
a, b = med['adamw_clip_step'], med['grad_stats + adamw_clip_step_guarded']
print(f'guard: +{b - a:.1f} us per step, {100 * (b - a) / a:+.1f} % of the optimiser phase')
