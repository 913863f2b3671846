#!/usr/bin/env python
"""Sensor fit at ingestion: the SYNTHETIC 60 s recording of ``tools/kbench_ingest.py`` (50 ms windows, ``--windows`` windows of
``--events`` events, uniform pixels) generated for a 640 x 480 sensor, fitted onto Gen1 frames (240 x 304; k = 2, centred: auto), then,
in one run over the same records, already on the device, in chunks of ``--chunk-mib`` with the carried state,

  (i)   ``ops.fit_events`` with reduce ``pick``, ``sum`` and ``fire`` (per chunk: the launches of every piece, the emit launch, the
        workspace, marks, state and record allocations and the one read-back);
  (ii)  ``ops.pixel_filter_events`` (trail filter ``--trail`` us) at the source geometry: like ``fire`` it sorts the records of a piece
        per pixel -- 19 key bits for 480 x 640, where ``fire`` sorts the 17 bits of the Gen1 frame, as the per-pixel filter does on a
        Gen1 recording -- so it is the yardstick of ``fire``;
  (iii) ``ops.filter_events(tau_us=None)``, the bounds-only activity filter (classify, count, scan, emit: no table), the yardstick of
        ``pick`` and ``sum``.

Everything is warmed, then timed ``--reps`` times (the candidates alternately) with a host clock around work that ends in a device
synchronise; medians and ranges are reported.  Two runs of every reduce are compared byte for byte first.

    python tools/kbench_fit.py [--windows 1200] [--events 50000] [--trail 3000] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kbench_ingest  # noqa: E402
from leod_amd import ops  # noqa: E402
from leod_amd.data.utils import dat_events, event_filter  # noqa: E402

SRC_HW, FRAME_HW = (480, 640), (240, 304)
REDUCES = ('pick', 'sum', 'fire')


def stats(ms):
    return dict(ms=round(statistics.median(ms), 3), ms_min_max=[round(min(ms), 3), round(max(ms), 3)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--windows', type=int, default=1200)
    ap.add_argument('--events', type=int, default=50_000, help='events per window')
    ap.add_argument('--trail', type=int, default=3000, help='the trail filter the fire reduce is compared with')
    ap.add_argument('--chunk-mib', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda', 0)
    kbench_ingest.H, kbench_ingest.W = SRC_HW                    # synth draws its pixels from the module's sensor
    t, x, y, p, _ = kbench_ingest.synth(args.windows, args.events, False)
    n = len(t)
    records = dat_events.encode(t, x, y, p)
    del t, x, y, p
    chunk = (args.chunk_mib << 20) // 8
    specs = {r: event_filter.fit_spec(SRC_HW, FRAME_HW, reduce=r) for r in REDUCES}
    kws = {r: dict(src_hw=tuple(s['src_hw']), dst_hw=tuple(s['frame_hw']), orient=s['orient'], mirror=s['mirror'], scale=s['scale'],
                   offset=tuple(s['offset']), reduce=r, threshold=s['threshold']) for r, s in specs.items()}
    tile, per_pass, digit, ws_chunk, marks_chunk = ops.fit_query(min(chunk, n), FRAME_HW, 'fire')
    res = dict(bench='kbench_fit', synthetic=True, windows=args.windows, events_per_window=args.events, events=n, sensor_hw=list(SRC_HW),
               frame_hw=list(FRAME_HW), fit=specs['fire'], trail_us=args.trail, chunk_mib=args.chunk_mib, reps=args.reps,
               tile_events=tile, tiles_per_pass=per_pass, digit_bits=digit, fire_ws_bytes_for_a_whole_chunk=ws_chunk,
               fire_ws_bytes_used_per_chunk=min(ws_chunk, ops.FIT_WS_BYTES), marks_bytes_per_chunk=marks_chunk,
               state_bytes=8 * (ops.FIT_STATE_HEAD + FRAME_HW[0] * FRAME_HW[1]),
               fire_sort_key_bits=int(np.ceil(np.log2(FRAME_HW[0] * FRAME_HW[1]))),
               pixel_filter_sort_key_bits=int(np.ceil(np.log2(SRC_HW[0] * SRC_HW[1]))))
    dev_chunks = [torch.from_numpy(records[a:a + chunk].view(np.uint8).reshape(-1)).to(dev) for a in range(0, n, chunk)]

    def fit_all(reduce, keep=False):
        state, outs = None, []
        for c in dev_chunks:
            rec, state = ops.fit_events(c, state=state, **kws[reduce])
            if keep:
                outs.append(rec)
        torch.cuda.synchronize()
        return state, outs

    def pixel_all():
        state = None
        for c in dev_chunks:
            _, state = ops.pixel_filter_events(c, *SRC_HW, burst_us=args.trail, burst_keep='first', state=state)
        torch.cuda.synchronize()
        return state

    def bounds_all():
        state = None
        for c in dev_chunks:
            _, state = ops.filter_events(c, *SRC_HW, None, state=state)
        torch.cuda.synchronize()
        return state

    ok, counters = True, {}
    for r in REDUCES:                                            # the warm-up of every reduce, and the same bytes from two runs
        sa, a = fit_all(r, keep=True)
        sb, b = fit_all(r, keep=True)
        ok = ok and torch.equal(sa, sb) and all(torch.equal(u, v) for u, v in zip(a, b))
        counters[r] = ops.fit_counters(sa)
        del a, b
    pixel_counters = ops.pixel_filter_counters(pixel_all())
    bounds_counters = ops.event_filter_counters(bounds_all())
    runs = dict({r: (lambda r=r: fit_all(r)) for r in REDUCES}, pixel_filter=pixel_all, bounds_only=bounds_all)
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    st = {k: stats(v) for k, v in times.items()}
    for r in REDUCES:
        res[r] = dict(counters=counters[r], kept_share=round(counters[r]['kept'] / n, 4), events_per_s=round(n / st[r]['ms'] * 1e3), **st[r])
    res.update(pixel_filter=dict(counters=pixel_counters, **st['pixel_filter']), bounds_only=dict(counters=bounds_counters, **st['bounds_only']),
               fire_over_pixel_filter=round(st['fire']['ms'] / st['pixel_filter']['ms'], 2),
               pick_over_bounds_only=round(st['pick']['ms'] / st['bounds_only']['ms'], 2),
               sum_over_bounds_only=round(st['sum']['ms'] / st['bounds_only']['ms'], 2), two_runs_are_byte_identical=bool(ok))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    raise SystemExit(main())
