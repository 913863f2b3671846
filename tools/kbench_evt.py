#!/usr/bin/env python
"""Metavision RAW ingestion: the synthetic Gen1-sized recording of ``tools/kbench_ingest.py`` (240 x 304, 50 ms windows, ``--windows``
windows of ``--events`` events) encoded as EVT3, then

  (i)  ``ops.decode_evt`` alone over the payload, already on the device, in chunks of ``--chunk-mib`` (per chunk: the reduce, scan and
       emit launches, the workspace and record allocations and the one read-back of the event count);
  (ii) ``ingest_recording`` end to end, ``.raw`` -> frame file against ``.dat`` -> frame file for the same events, written to ``--tmp``.

Both are warmed, then timed ``--reps`` times (alternately in (ii)) with a host clock around work that ends in a device synchronise or a
closed file; medians are reported.  The frame files of the two containers are compared byte for byte first.  Host-to-device bytes per
event are counted from the file sizes, not measured: 8 for ``.dat``, payload bytes / events for ``.raw``.

    python tools/kbench_evt.py [--windows 1200] [--events 50000] [--blobs] [--no-vectors] [--out FILE]
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
from leod_amd.data.utils import dat_events, misc, raw_events  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--windows', type=int, default=1200)
    ap.add_argument('--events', type=int, default=50_000, help='events per window')
    ap.add_argument('--blobs', action='store_true')
    ap.add_argument('--no-vectors', action='store_true', help='ADDR_X words only')
    ap.add_argument('--chunk-mib', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--tmp', default=None, help='directory for the recordings and the trees (default: a temporary one)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda', 0)
    t, x, y, p, _ = synth(args.windows, args.events, args.blobs)
    order = np.lexsort((x, p, y, t))                             # within one microsecond a sensor reads row by row
    t, x, y, p = t[order], x[order], y[order], p[order]
    n = len(t)
    t0 = time.perf_counter()
    words = raw_events.encode_evt3(t, x, y, p, first_time_high=1000, vectors=not args.no_vectors)
    encode_s = time.perf_counter() - t0
    kinds = np.bincount(words >> 12, minlength=16)
    tmp = tempfile.mkdtemp(prefix='kbench_evt_', dir=args.tmp)
    try:
        raw_fn, dat_fn = os.path.join(tmp, 'rec.raw'), os.path.join(tmp, 'rec_td.dat')
        raw_events.write_raw(raw_fn, words, 'evt3', height=H, width=W)
        dat_events.write_dat(dat_fn, dat_events.encode(t, x, y, p), H, W)
        payload = words.nbytes
        del t, x, y, p, order

        # (i) the decoder alone
        chunk = args.chunk_mib << 20
        dev_chunks = [torch.from_numpy(words[a:a + chunk // 2].view(np.uint8)).to(dev) for a in range(0, len(words), chunk // 2)]

        def decode_all():
            state, total = None, 0
            for c in dev_chunks:
                rec, state = ops.decode_evt(c, 'evt3', state)
                total += rec.shape[0]
            torch.cuda.synchronize()
            return total, state

        total, state = decode_all()
        counters = ops.evt_state_counters(state)
        decode_ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            decode_all()
            decode_ms.append((time.perf_counter() - t0) * 1e3)
        del dev_chunks

        # (ii) end to end
        def run(fn, name):
            out = os.path.join(tmp, name)
            shutil.rmtree(out, ignore_errors=True)
            t0 = time.perf_counter()
            rep = ingest.ingest_recording(fn, None, out, 'gen1', raw_chunk_bytes=chunk)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, rep, out

        _, rep_raw, out_raw = run(raw_fn, 'tree_raw')
        _, rep_dat, out_dat = run(dat_fn, 'tree_dat')
        a, b = (np.load(misc.get_ev_raw_fn(o, 'gen1'), mmap_mode='r') for o in (out_raw, out_dat))
        same = a.shape == b.shape and all(np.array_equal(a[k:k + 64], b[k:k + 64]) for k in range(0, len(a), 64))
        del a, b
        ms = {'raw': [], 'dat': []}
        for _ in range(args.reps):
            ms['raw'].append(run(raw_fn, 'tree_raw')[0])
            ms['dat'].append(run(dat_fn, 'tree_dat')[0])
        med = {k: statistics.median(v) for k, v in ms.items()}
        dm = statistics.median(decode_ms)
        res = dict(bench='kbench_evt', windows=args.windows, events_per_window=args.events, events=n, blobs=args.blobs,
                   vectors=not args.no_vectors, reps=args.reps, chunk_mib=args.chunk_mib, words=int(len(words)), payload_bytes=int(payload),
                   words_by_type={hex(k): int(v) for k, v in enumerate(kinds) if v}, encode_s=round(encode_s, 1),
                   decoded_events=int(total), counters=counters, frames_equal=bool(same), frames=rep_raw['frames'],
                   decode_ms=round(dm, 3), decode_ms_min_max=[round(min(decode_ms), 3), round(max(decode_ms), 3)],
                   decode_words_per_s=round(len(words) / dm * 1e3), decode_events_per_s=round(n / dm * 1e3),
                   decode_gb_per_s_in_plus_out=round((payload + 8 * n) / dm / 1e6, 2),
                   ingest_raw_ms=round(med['raw'], 1), ingest_raw_ms_min_max=[round(min(ms['raw']), 1), round(max(ms['raw']), 1)],
                   ingest_dat_ms=round(med['dat'], 1), ingest_dat_ms_min_max=[round(min(ms['dat']), 1), round(max(ms['dat']), 1)],
                   raw_over_dat=round(med['raw'] / med['dat'], 3),
                   h2d_bytes_per_event_raw=round(payload / n, 3), h2d_bytes_per_event_dat=8.0)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if same and total == n else 1


if __name__ == '__main__':
    raise SystemExit(main())
