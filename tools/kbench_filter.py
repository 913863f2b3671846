#!/usr/bin/env python
"""Event noise filters at ingestion: the SYNTHETIC Gen1-sized recording of ``tools/kbench_ingest.py`` (240 x 304, 50 ms windows,
``--windows`` windows of ``--events`` events, uniform pixels -- close to the worst case for a neighbourhood filter: two events in three
look all 8 neighbours up before one supports them, one in three finds none) and a variant with 1 % of the events on 20 hot pixels, then

  (i)   ``ops.filter_events`` alone over the records, already on the device, in chunks of ``--chunk-mib`` with the carried state (per
        chunk: the memsets and launches of every piece, the emit launch, the table, marks, state and record allocations and the one
        read-back), ``tau_us = --tau``; the hot variant with the mask that ``ops.event_pixel_counts`` + ``hot_pixel_mask`` give;
  (ii)  the same for every table bound of ``--sweep`` (MiB): the sweep behind ``ops.FILTER_WS_BYTES``;
  (iii) ``ingest_recording`` end to end, ``.dat`` -> frame file, with the filter off and on, written to ``--tmp``.

Everything is warmed, then timed ``--reps`` times (the candidates alternately) with a host clock around work that ends in a device
synchronise or a closed file; medians and ranges are reported.  The kept records of the default bound are compared with those of every
other bound first.

    python tools/kbench_filter.py [--windows 1200] [--events 50000] [--tau 10000] [--sweep 1,4,16,32,64,128,256] [--out FILE]
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

from kbench_ingest import H, W, synth  # noqa: E402
from leod_amd import ops  # noqa: E402
from leod_amd.data import ingest  # noqa: E402
from leod_amd.data.utils import dat_events, event_filter  # noqa: E402

HOT_PIXELS, HOT_SHARE, HOT_RATE_HZ = 20, 0.01, 100


def stats(ms):
    return dict(ms=round(statistics.median(ms), 3), ms_min_max=[round(min(ms), 3), round(max(ms), 3)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--windows', type=int, default=1200)
    ap.add_argument('--events', type=int, default=50_000, help='events per window')
    ap.add_argument('--tau', type=int, default=10_000)
    ap.add_argument('--chunk-mib', type=int, default=64)
    ap.add_argument('--sweep', default='1,4,16,32,64,128,256', help='table bounds in MiB to time besides the default')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--reps-ingest', type=int, default=3)
    ap.add_argument('--tmp', default=None, help='directory for the recordings and the trees (default: a temporary one)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda', 0)
    t, x, y, p, _ = synth(args.windows, args.events, False)
    n = len(t)
    rng = np.random.RandomState(1)
    hot = rng.rand(n) < HOT_SHARE
    which = rng.randint(0, HOT_PIXELS, n)
    hx, hy = rng.randint(0, W, HOT_PIXELS), rng.randint(0, H, HOT_PIXELS)
    variants = {'uniform': dat_events.encode(t, x, y, p), 'hot': dat_events.encode(t, np.where(hot, hx[which], x), np.where(hot, hy[which], y), p)}
    duration = int(t[-1] - t[0])
    del t, x, y, p, hot, which
    chunk = (args.chunk_mib << 20) // 8
    default_ws = ops.FILTER_WS_BYTES
    sweep = sorted({int(s) << 20 for s in args.sweep.split(',') if s} | {default_ws})
    res = dict(bench='kbench_filter', synthetic=True, windows=args.windows, events_per_window=args.events, events=n, tau_us=args.tau,
               chunk_mib=args.chunk_mib, reps=args.reps, default_ws_mib=default_ws >> 20, hot_pixels=HOT_PIXELS, hot_share=HOT_SHARE,
               hot_rate_hz=HOT_RATE_HZ)
    ok = True
    tmp = tempfile.mkdtemp(prefix='kbench_filter_', dir=args.tmp)
    try:
        for name, records in variants.items():
            dev_chunks = [torch.from_numpy(records[a:a + chunk].view(np.uint8).reshape(-1)).to(dev) for a in range(0, n, chunk)]
            mask = None
            if name == 'hot':
                counts = None
                for c in dev_chunks:
                    counts, _ = ops.event_pixel_counts(c, H, W, counts)
                m = event_filter.hot_pixel_mask(counts.cpu().numpy(), duration, HOT_RATE_HZ)
                res['hot_masked_pixels'] = int(m.sum())
                mask = torch.from_numpy(m).to(dev)

            def filter_all(ws, keep=False):
                state, outs = None, []
                for c in dev_chunks:
                    rec, state = ops.filter_events(c, H, W, args.tau, state=state, pixel_mask=mask, ws_bytes=ws)
                    if keep:
                        outs.append(rec)
                torch.cuda.synchronize()
                return state, outs

            state, want = filter_all(default_ws, keep=True)
            counters = ops.event_filter_counters(state)
            for ws in sweep:                                     # the warm-up of every bound, and the same records from each
                _, got = filter_all(ws, keep=True)
                ok = ok and all(torch.equal(a, b) for a, b in zip(got, want))
                del got
            del want
            times = {ws: [] for ws in sweep}
            for _ in range(args.reps):
                for ws in sweep:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    filter_all(ws)
                    times[ws].append((time.perf_counter() - t0) * 1e3)
            d = stats(times[default_ws])
            res[name] = dict(counters=counters, kept_share=round(counters['kept'] / n, 4),
                             filter_ms_per_60M_events=round(d['ms'] * 60e6 / n, 3), filter_ms=d['ms'], filter_ms_min_max=d['ms_min_max'],
                             filter_events_per_s=round(n / d['ms'] * 1e3),
                             sweep_ws_mib={str(ws >> 20): stats(times[ws]) for ws in sweep})
            del dev_chunks

            # (iii) end to end
            dat_fn = os.path.join(tmp, f'{name}_td.dat')
            dat_events.write_dat(dat_fn, records, H, W)
            kw_on = dict(denoise_us=args.tau, **(dict(hot_rate_hz=HOT_RATE_HZ) if name == 'hot' else {}))

            def run(kw, tree):
                out = os.path.join(tmp, tree)
                shutil.rmtree(out, ignore_errors=True)
                t0 = time.perf_counter()
                rep = ingest.ingest_recording(dat_fn, None, out, 'gen1', **kw)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, rep

            _, rep_off = run({}, 'tree_off')
            _, rep_on = run(kw_on, 'tree_on')
            ok = ok and rep_on['frames'] == rep_off['frames'] == args.windows and rep_on['kept_events'] == counters['kept']
            ms = {'off': [], 'on': []}
            for _ in range(args.reps_ingest):
                ms['off'].append(run({}, 'tree_off')[0])
                ms['on'].append(run(kw_on, 'tree_on')[0])
            off, on = stats(ms['off']), stats(ms['on'])
            res[name].update(ingest_off_ms=off['ms'], ingest_off_ms_min_max=off['ms_min_max'], ingest_on_ms=on['ms'],
                             ingest_on_ms_min_max=on['ms_min_max'], on_over_off=round(on['ms'] / off['ms'], 3),
                             ingest_on_options=kw_on, frames=rep_on['frames'])
            shutil.rmtree(os.path.join(tmp, 'tree_off'), ignore_errors=True)
            shutil.rmtree(os.path.join(tmp, 'tree_on'), ignore_errors=True)
            os.remove(dat_fn)
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
