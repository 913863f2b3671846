#!/usr/bin/env python
"""Per-pixel event filters at ingestion: the SYNTHETIC Gen1-sized recording of ``tools/kbench_ingest.py`` (240 x 304, 50 ms windows,
``--windows`` windows of ``--events`` events, uniform pixels) with 1 % more events ADDED as 100 Hz flicker on 20 pixels (per cycle three
ON events at its start and two OFF events half a cycle later, each jittered by up to 200 us), then, in one run,

  (i)   ``ops.pixel_filter_events`` alone over the records, already on the device, in chunks of ``--chunk-mib`` with the carried state
        (per chunk: the launches of every piece, the emit launch, the workspace, marks, state and record allocations and the one
        read-back): trail filter ``--trail`` us + anti-flicker ``--band`` Hz with the default lock;
  (ii)  ``ops.filter_events`` (the activity filter, ``tau_us = --tau``) alone over the same records, the same way;
  (iii) the same as (i) for every workspace bound of ``--sweep`` (MiB);
  (iv)  ``ingest_recording`` end to end, ``.dat`` -> frame file, with the per-pixel filters off and on, written to ``--tmp``.

Everything is warmed, then timed ``--reps`` times (the candidates alternately) with a host clock around work that ends in a device
synchronise or a closed file; medians and ranges are reported.  The kept records of the default bound are compared with those of every
other bound first.

    python tools/kbench_pixfilter.py [--windows 1200] [--events 50000] [--trail 3000] [--band 80:125] [--out FILE]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kbench_ingest import D, H, W, synth  # noqa: E402
from leod_amd import ops  # noqa: E402
from leod_amd.data import ingest  # noqa: E402
from leod_amd.data.utils import dat_events, event_filter  # noqa: E402

LAMPS, LAMP_SHARE, LAMP_HZ, PER_CYCLE = 20, 0.01, 100, ((0, 1), (40, 1), (80, 1), (5000, 0), (5040, 0))


def stats(ms):
    return dict(ms=round(statistics.median(ms), 3), ms_min_max=[round(min(ms), 3), round(max(ms), 3)])


def with_lamps(t, x, y, p, seed=1):
    """The recording + LAMP_SHARE of its events on LAMPS flickering pixels, sorted in time (stable)."""
    rng = np.random.RandomState(seed)
    period = 1_000_000 // LAMP_HZ
    per_lamp = int(len(t) * LAMP_SHARE) // LAMPS
    cycles = min(per_lamp // len(PER_CYCLE), int(t[-1]) // period - 1)
    lx, ly = rng.randint(0, W, LAMPS), rng.randint(0, H, LAMPS)
    parts = [(t, x, y, p)]
    for k in range(LAMPS):
        start = 300 + rng.randint(0, period) + np.arange(cycles) * period
        for dt, pol in PER_CYCLE:
            tt = start + dt + rng.randint(-200, 201, cycles)
            parts.append((tt, np.full(cycles, lx[k]), np.full(cycles, ly[k]), np.full(cycles, pol)))
    t, x, y, p = (np.concatenate([q[i] for q in parts]).astype(np.int64) for i in range(4))
    order = np.argsort(t, kind='stable')
    return t[order], x[order], y[order], p[order], LAMPS * cycles * len(PER_CYCLE)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--windows', type=int, default=1200)
    ap.add_argument('--events', type=int, default=50_000, help='events per window')
    ap.add_argument('--trail', type=int, default=3000)
    ap.add_argument('--band', default='80:125')
    ap.add_argument('--tau', type=int, default=10_000, help='the activity filter it is compared with')
    ap.add_argument('--chunk-mib', type=int, default=64)
    ap.add_argument('--sweep', default='4,16,64,256', help='workspace bounds in MiB to time besides the default')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--reps-ingest', type=int, default=3)
    ap.add_argument('--tmp', default=None, help='directory for the recording and the trees (default: a temporary one)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda', 0)
    t, x, y, p, _ = synth(args.windows, args.events, False)
    t, x, y, p, n_lamp = with_lamps(t, x, y, p)
    n = len(t)
    records = dat_events.encode(t, x, y, p)
    del t, x, y, p
    flicker = event_filter.flicker_band(args.band) + (event_filter.DEFAULT_FLICKER_LOCK,)
    kw = dict(burst_us=args.trail, burst_keep='first', flicker=flicker)
    chunk = (args.chunk_mib << 20) // 8
    default_ws = ops.PIXFILTER_WS_BYTES
    sweep = sorted({int(s) << 20 for s in args.sweep.split(',') if s} | {default_ws})
    tile, per_pass, digit, ws_chunk, marks_chunk = ops.pixel_filter_query(min(chunk, n), H, W)
    res = dict(bench='kbench_pixfilter', synthetic=True, windows=args.windows, events_per_window=args.events, events=n, lamp_events=n_lamp,
               lamps=LAMPS, lamp_hz=LAMP_HZ, options=dict(trail_us=args.trail, anti_flicker=args.band, flicker=list(flicker)),
               activity_tau_us=args.tau, chunk_mib=args.chunk_mib, reps=args.reps, default_ws_mib=default_ws >> 20,
               tile_events=tile, tiles_per_pass=per_pass, digit_bits=digit, ws_bytes_for_a_whole_chunk=ws_chunk,
               ws_bytes_used_per_chunk=min(ws_chunk, default_ws), marks_bytes_per_chunk=marks_chunk,
               state_bytes=8 * (ops.PIXFILTER_STATE_HEAD + ops.PIXFILTER_PIXEL_LONGS * H * W))
    ok = True
    tmp = tempfile.mkdtemp(prefix='kbench_pixfilter_', dir=args.tmp)
    try:
        dev_chunks = [torch.from_numpy(records[a:a + chunk].view(np.uint8).reshape(-1)).to(dev) for a in range(0, n, chunk)]

        def pixel_all(ws, keep=False):
            state, outs = None, []
            for c in dev_chunks:
                rec, state = ops.pixel_filter_events(c, H, W, state=state, ws_bytes=ws, **kw)
                if keep:
                    outs.append(rec)
            torch.cuda.synchronize()
            return state, outs

        def activity_all():
            state = None
            for c in dev_chunks:
                _, state = ops.filter_events(c, H, W, args.tau, state=state)
            torch.cuda.synchronize()
            return state

        state, want = pixel_all(default_ws, keep=True)
        counters = ops.pixel_filter_counters(state)
        for ws in sweep:                                         # the warm-up of every bound, and the same records from each
            _, got = pixel_all(ws, keep=True)
            ok = ok and all(torch.equal(a, b) for a, b in zip(got, want))
            del got
        del want
        activity_counters = ops.event_filter_counters(activity_all())
        times, act = {ws: [] for ws in sweep}, []
        for _ in range(args.reps):
            for ws in sweep:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pixel_all(ws)
                times[ws].append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            activity_all()
            act.append((time.perf_counter() - t0) * 1e3)
        d, a = stats(times[default_ws]), stats(act)
        res.update(counters=counters, kept_share=round(counters['kept'] / n, 4), pixel_filter_ms=d['ms'], pixel_filter_ms_min_max=d['ms_min_max'],
                   pixel_filter_events_per_s=round(n / d['ms'] * 1e3), activity_filter_counters=activity_counters,
                   activity_filter_ms=a['ms'], activity_filter_ms_min_max=a['ms_min_max'],
                   pixel_over_activity=round(d['ms'] / a['ms'], 2), sweep_ws_mib={str(ws >> 20): stats(times[ws]) for ws in sweep})
        del dev_chunks

        dat_fn = os.path.join(tmp, 'lamps_td.dat')
        dat_events.write_dat(dat_fn, records, H, W)
        kw_on = dict(trail_us=args.trail, anti_flicker=args.band)

        def run(opts, tree):
            out = os.path.join(tmp, tree)
            shutil.rmtree(out, ignore_errors=True)
            t0 = time.perf_counter()
            rep = ingest.ingest_recording(dat_fn, None, out, 'gen1', **opts)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, rep

        _, rep_off = run({}, 'tree_off')
        _, rep_on = run(kw_on, 'tree_on')
        ok = ok and rep_on['frames'] == rep_off['frames'] and rep_on['kept_events'] == counters['kept'] and \
            rep_on['flicker_events'] == counters['flicker'] and rep_on['burst_events'] == counters['burst']
        ms = {'off': [], 'on': []}
        for _ in range(args.reps_ingest):
            ms['off'].append(run({}, 'tree_off')[0])
            ms['on'].append(run(kw_on, 'tree_on')[0])
        off, on = stats(ms['off']), stats(ms['on'])
        res.update(ingest_off_ms=off['ms'], ingest_off_ms_min_max=off['ms_min_max'], ingest_on_ms=on['ms'],
                   ingest_on_ms_min_max=on['ms_min_max'], on_over_off=round(on['ms'] / off['ms'], 3), ingest_on_options=kw_on,
                   frames=rep_on['frames'], window_us=D)
        res['same_records_for_every_bound'] = bool(ok)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    raise SystemExit(main())
