#!/usr/bin/env python
"""Filter survey: the SYNTHETIC Gen1-sized recording of ``tools/kbench_ingest.py`` (240 x 304, ``--windows`` windows of 50 ms with
``--events`` events, uniform pixels) with the flicker addition of ``tools/kbench_pixfilter.py`` (1 % more events as 100 Hz flicker on 20
pixels), then, in one run over the records, already on the device, in chunks of ``--chunk-mib`` with the carried state,

  (i)   ``ops.survey_events`` (the default 16 edges of ``leod_amd.data.survey``, band ``--band``): ONE pass, per chunk the launches of
        every piece, the workspace and state allocations and the one read-back;
  (ii)  what a user has without it: per edge ``ops.filter_events(tau_us = edge)`` plus ``ops.pixel_filter_events(burst_us = edge,
        'first')`` over the same chunks -- 16 times two filter passes.  That is the LEAST such a user runs: the STC curves and the
        flicker locks would take further passes, which are not timed here;
  (iii) the same as (i) for every workspace bound of ``--sweep`` (MiB).

Everything is warmed, then timed ``--reps`` times (the candidates alternately) with a host clock around work that ends in a device
synchronise; medians and ranges are reported.  First the survey's curves are compared with the counters of (ii) at every edge and with
one anti-flicker pass at the default lock, and its state with that of every other workspace bound.

    python tools/kbench_survey.py [--windows 1200] [--events 50000] [--band 80:125] [--out FILE]
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

from kbench_ingest import H, W, synth  # noqa: E402
from kbench_pixfilter import LAMP_HZ, LAMPS, with_lamps  # noqa: E402
from leod_amd import ops  # noqa: E402
from leod_amd.data.survey import DEFAULT_EDGES_US  # noqa: E402
from leod_amd.data.utils import dat_events, event_filter  # noqa: E402


def stats(ms):
    return dict(ms=round(statistics.median(ms), 3), ms_min_max=[round(min(ms), 3), round(max(ms), 3)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--windows', type=int, default=1200)
    ap.add_argument('--events', type=int, default=50_000, help='events per window')
    ap.add_argument('--band', default='80:125')
    ap.add_argument('--chunk-mib', type=int, default=64)
    ap.add_argument('--sweep', default='4,16,64', help='workspace bounds in MiB to time besides the default')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda', 0)
    t, x, y, p, _ = synth(args.windows, args.events, False)
    t, x, y, p, n_lamp = with_lamps(t, x, y, p)
    n = len(t)
    records = dat_events.encode(t, x, y, p)
    del t, x, y, p
    edges = list(DEFAULT_EDGES_US)
    K = len(edges)
    band = event_filter.flicker_band(args.band)
    lock = event_filter.DEFAULT_FLICKER_LOCK
    chunk = (args.chunk_mib << 20) // 8
    default_ws = ops.SURVEY_WS_BYTES
    sweep = sorted({int(s) << 20 for s in args.sweep.split(',') if s} | {default_ws})
    tile, digit, ws_chunk, state_longs = ops.survey_query(min(chunk, n), H, W, K)
    res = dict(bench='kbench_survey', synthetic=True, windows=args.windows, events_per_window=args.events, events=n, lamp_events=n_lamp,
               lamps=LAMPS, lamp_hz=LAMP_HZ, edges_us=edges, band=args.band, band_us=list(band), chunk_mib=args.chunk_mib, reps=args.reps,
               default_ws_mib=default_ws >> 20, tile_events=tile, digit_bits=digit, ws_bytes_for_a_whole_chunk=ws_chunk,
               ws_bytes_used_per_chunk=min(ws_chunk, default_ws), state_bytes=8 * state_longs)
    dev_chunks = [torch.from_numpy(records[a:a + chunk].view(np.uint8).reshape(-1)).to(dev) for a in range(0, n, chunk)]
    del records

    def survey_all(ws):
        state = None
        for c in dev_chunks:
            state = ops.survey_events(c, H, W, edges, flicker=band, state=state, ws_bytes=ws)
        torch.cuda.synchronize()
        return state

    def per_edge_all():
        out = []
        for e in edges:
            fs = ps = None
            for c in dev_chunks:
                _, fs = ops.filter_events(c, H, W, e, state=fs)
                _, ps = ops.pixel_filter_events(c, H, W, burst_us=e, burst_keep='first', state=ps)
            out.append((fs, ps))
        torch.cuda.synchronize()
        return out

    state = survey_all(default_ws)
    counters = ops.survey_counters(state, K)
    resp = event_filter.survey_responses(counters, edges)
    ok = all(torch.equal(survey_all(ws), state) for ws in sweep)              # the warm-up of every bound, and the same state from each
    res['same_state_for_every_bound'] = bool(ok)
    unsupported, burst = [], []
    for fs, ps in per_edge_all():                                            # the warm-up of (ii), and the identities at every edge
        unsupported.append(ops.event_filter_counters(fs)['unsupported'])
        burst.append(ops.pixel_filter_counters(ps)['burst'])
    ps = None
    for c in dev_chunks:
        _, ps = ops.pixel_filter_events(c, H, W, flicker=band + (lock,), state=ps)
    flicker = ops.pixel_filter_counters(ps)['flicker']
    same = unsupported == resp['denoise'].tolist() and burst == resp['trail'].tolist() and flicker == int(resp['flicker'][lock])
    ok = ok and same
    res.update(curves_equal_the_filters_counters=bool(same), candidates=counters['candidates'],
               removed=dict(denoise=resp['denoise'].tolist(), trail=resp['trail'].tolist(), stc=resp['stc'].tolist(),
                            stc_cut_trail=resp['stc_cut_trail'].tolist(), flicker_at_locks_1_2_3_5_10=resp['flicker'][[1, 2, 3, 5, 10]].tolist()))
    times, alt = {ws: [] for ws in sweep}, []
    for _ in range(args.reps):
        for ws in sweep:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            survey_all(ws)
            times[ws].append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per_edge_all()
        alt.append((time.perf_counter() - t0) * 1e3)
    s, a = stats(times[default_ws]), stats(alt)
    res.update(survey_ms=s['ms'], survey_ms_min_max=s['ms_min_max'], survey_events_per_s=round(n / s['ms'] * 1e3),
               per_edge_filters_ms=a['ms'], per_edge_filters_ms_min_max=a['ms_min_max'], per_edge_passes=2 * K,
               per_edge_over_survey=round(a['ms'] / s['ms'], 2), sweep_ws_mib={str(ws >> 20): stats(times[ws]) for ws in sweep})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    raise SystemExit(main())
