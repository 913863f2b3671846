#!/usr/bin/env python
"""Voxelising a whole recording: ``ops.voxelize_dat_windows`` (one batched call on the raw .dat records) against the only way the package
had before it, ``ops.voxelize_u8`` once per window on int64 fields that are already on the device.

Synthetic Gen1-sized recording (240 x 304, 50 ms windows): ``--windows`` windows of ``--events`` events each, times sorted, pixels uniform
or (``--blobs``) half of them in a few moving clusters, which is closer to a sensor and harder on the atomics.  Both paths are warmed, then
timed alternately ``--reps`` times with a host clock around work that ends in a device synchronise; medians are reported.  The outputs of
the two paths are compared on every window first.  Enqueues and host-to-device bytes are counted from the shapes, not measured.

    python tools/kbench_ingest.py [--windows 1200] [--events 50000] [--sweep 1,2,4,8,16,32,64] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from leod_amd import ops  # noqa: E402
from leod_amd.data.utils import dat_events  # noqa: E402

H, W, BINS, D = 240, 304, 10, 50_000


def synth(n_win: int, per_win: int, blobs: bool, seed: int = 0):
    rng = np.random.RandomState(seed)
    n = n_win * per_win
    t = (np.sort(rng.randint(1, D + 1, (n_win, per_win)), axis=1) + np.arange(n_win)[:, None] * D).reshape(-1).astype(np.int64)
    x, y = rng.randint(0, W, n), rng.randint(0, H, n)
    if blobs:
        half = rng.rand(n) < 0.5
        k = rng.randint(0, 6, n)
        cx = (40 + 40 * k + t / (n_win * D) * 30).astype(np.int64)
        cy = 40 + 30 * k
        x = np.where(half, np.clip(cx + rng.normal(0, 6, n), 0, W - 1).astype(np.int64), x)
        y = np.where(half, np.clip(cy + rng.normal(0, 6, n), 0, H - 1).astype(np.int64), y)
    p = rng.randint(0, 2, n)
    return t, x, y, p, np.arange(n_win + 1, dtype=np.int64) * per_win


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--windows', type=int, default=1200)
    ap.add_argument('--events', type=int, default=50_000, help='events per window')
    ap.add_argument('--blobs', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sweep', default='1,2,4,8,16,32,64', help='ws_windows values to time besides the default')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda', 0)
    t, x, y, p, off = synth(args.windows, args.events, args.blobs)
    n = len(t)
    rec = torch.from_numpy(dat_events.encode(t, x, y, p).view(np.uint8).reshape(-1)).to(dev)
    fields = [torch.from_numpy(a).to(dev) for a in (x, y, p, t)]
    off_dev = torch.from_numpy(off).to(dev)
    bounds = off.tolist()

    def loop():
        return [ops.voxelize_u8(*(a[bounds[w]:bounds[w + 1]] for a in fields), BINS, H, W) for w in range(args.windows)]

    def batched(ws=None):
        return ops.voxelize_dat_windows(rec, off_dev, BINS, H, W, ws_windows=ws)

    # same results first (and the warm-up of both paths)
    out, dropped = batched()
    ref = loop()
    same = all(torch.equal(out[w], ref[w]) for w in range(args.windows)) and int(dropped) == 0
    del ref, out
    default_ws = ops.ingest_ws_windows(BINS, H, W)
    sweep = sorted({int(s) for s in args.sweep.split(',') if s} | {default_ws})
    for ws in sweep:
        batched(ws)
    times = {'loop': [], **{ws: [] for ws in sweep}}
    for _ in range(args.reps):                                   # alternate the candidates within one repetition
        times['loop'].append(timed(loop))
        for ws in sweep:
            times[ws].append(timed(lambda: batched(ws)))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = dict(bench='kbench_ingest', windows=args.windows, events_per_window=args.events, events=n, blobs=args.blobs, reps=args.reps,
               outputs_equal=same, default_ws_windows=default_ws,
               loop_ms=round(med['loop'], 3), loop_ms_min_max=[round(min(times['loop']), 3), round(max(times['loop']), 3)],
               batched_ms={str(ws): round(med[ws], 3) for ws in sweep},
               batched_ms_min_max={str(ws): [round(min(times[ws]), 3), round(max(times[ws]), 3)] for ws in sweep},
               speedup_default=round(med['loop'] / med[default_ws], 2),
               events_per_s_loop=round(n / med['loop'] * 1e3), events_per_s_batched=round(n / med[default_ws] * 1e3),
               enqueues_loop=3 * args.windows, enqueues_batched={str(ws): 3 * -(-args.windows // ws) for ws in sweep},
               h2d_bytes_loop=32 * n, h2d_bytes_batched=8 * n + 8 * (args.windows + 1))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    raise SystemExit(main())
