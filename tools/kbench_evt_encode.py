#!/usr/bin/env python
"""Writing the kept event stream back: the SYNTHETIC 60 s Gen1 recording of ``tools/kbench_ingest.py`` (50 ms windows, ``--windows``
windows of ``--events`` events, uniform pixels -- so vector runs are rare, unlike on a sensor), its records already on the device, in
chunks of ``--chunk-mib`` with the carried state.  In one run:

  (i)   the encode launches alone (``leod_evtenc_scan`` + ``leod_evtenc_emit`` into buffers allocated once, sized by the query's bound, no
        read-back) for evt3 without and with vectors and for evt2;
  (ii)  ``ops.encode_evt`` as the writer calls it (allocations, the read-back of the state that sizes the output);
  (iii) the copy of the words to the host (pageable memory, as ``EventFileWriter`` does it), and bytes per event;
  (iv)  what the parent commit offers for the same events: ``raw_events.encode_evt3`` on the host, the copy of the records to it and
        their unpacking included, on the first 1/``--host-share`` of the recording, SCALED by that share; and ``ops.decode_evt`` of the
        words of (ii), the way in;
  (v)   the ``.dat`` file to the ``.npy`` frame file end to end through ``ingest_recording``, without and with ``--write-events evt3``
        (the first takes the route that knows its frames in advance, the second the streaming route).

Everything but (iv)'s host encoder and (v) is warmed, then timed ``--reps`` times with a host clock around work that ends in a device
synchronise (the device-only sections ``--inner`` calls per window, reported per call); medians and ranges are reported.  The words of
(i) and (ii) are compared first.

    python tools/kbench_evt_encode.py [--windows 1200] [--events 50000] [--no-e2e] [--out FILE]
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

import kbench_ingest  # noqa: E402
from leod_amd import ops  # noqa: E402
from leod_amd.data.utils import dat_events, raw_events  # noqa: E402

MODES = {'evt3': ('evt3', False), 'evt3_vectors': ('evt3', True), 'evt2': ('evt2', False)}


def stats(ms):
    return dict(ms=round(statistics.median(ms), 3), ms_min_max=[round(min(ms), 3), round(max(ms), 3)])


def timed(fn, reps, inner=1):
    """ms per call of ``fn``, ``reps`` windows of ``inner`` calls each: a window of a millisecond would measure the clock."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / inner)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--windows', type=int, default=1200)
    ap.add_argument('--events', type=int, default=50_000, help='events per window')
    ap.add_argument('--chunk-mib', type=int, default=64)
    ap.add_argument('--host-share', type=int, default=60, help='the host encoder runs on the first 1/N of the recording and is scaled by N')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20, help='calls per timed window of the device-only sections')
    ap.add_argument('--no-e2e', action='store_true', help='skip the end-to-end ingestion of (v)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda', 0)
    t, x, y, p, _ = kbench_ingest.synth(args.windows, args.events, False)
    n = len(t)
    records = dat_events.encode(t, x, y, p)
    del t, x, y, p
    chunk = (args.chunk_mib << 20) // 8
    dev_chunks = [torch.from_numpy(records[a:a + chunk].view(np.uint8).reshape(-1)).to(dev) for a in range(0, n, chunk)]
    tile = ops.evt_encode_query(0)[0]
    res = dict(bench='kbench_evt_encode', synthetic=True, windows=args.windows, events_per_window=args.events, events=n,
               chunk_mib=args.chunk_mib, chunks=len(dev_chunks), reps=args.reps, calls_per_window=args.inner, tile_events=tile)
    lib, stream = ops._l(), ops._stream()

    def launches_only(fmt, vectors):
        """The two entry points per chunk on buffers allocated once; -> (the words of every chunk, the last state)."""
        f = ops.EVT_FORMATS[fmt]
        _, ws_bytes, bound = ops.evt_encode_query(chunk, fmt)
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
        out = torch.empty(bound * ops.EVT_WORD_BYTES[f], dtype=torch.uint8, device=dev)
        states = [torch.zeros(ops.EVT_ENC_STATE_LONGS, dtype=torch.int64, device=dev) for _ in range(2)]

        def run():
            states[0].zero_()                                    # a recording starts from zeros
            for i, c in enumerate(dev_chunks):
                a = (ops._p(c), c.numel() // 8, f, int(vectors), int(i == len(dev_chunks) - 1), 64, 0, ops._p(states[i % 2]))
                ops.check(lib.leod_evtenc_scan(*a, ops._p(states[1 - i % 2]), ops._p(ws), ws_bytes, stream), 'scan')
                ops.check(lib.leod_evtenc_emit(*a, ops._p(ws), ws_bytes, ops._p(out), bound, stream), 'emit')
            return states[len(dev_chunks) % 2], out
        return run

    def op_all(fmt, vectors, keep=False):
        state, outs = None, []
        for i, c in enumerate(dev_chunks):
            w, state = ops.encode_evt(c, fmt, state, final=i == len(dev_chunks) - 1, vectors=vectors)
            if keep:
                outs.append(w)
        return state, outs

    ok = True
    for name, (fmt, vectors) in MODES.items():
        state, words = op_all(fmt, vectors, keep=True)           # the warm-up, and the words of the other sections
        c = ops.evt_encode_counters(state)
        run = launches_only(fmt, vectors)
        st, out = run()
        torch.cuda.synchronize()
        last = words[-1]
        ok = ok and ops.evt_encode_counters(st) == c and torch.equal(out[:last.numel()], last)
        wb = ops.EVT_WORD_BYTES[ops.EVT_FORMATS[fmt]]
        r = dict(counters=c, payload_bytes=c['words'] * wb, bytes_per_event=round(c['words'] * wb / n, 3),
                 launches_only=stats(timed(run, args.reps, args.inner)),
                 op_with_read_backs=stats(timed(lambda: op_all(fmt, vectors), args.reps, args.inner)),
                 words_to_host=stats(timed(lambda: [w.cpu() for w in words], args.reps)),
                 decode_evt=stats(timed(lambda: _decode_all(words, fmt), args.reps + 1, args.inner)[1:]))
        r['events_per_s_launches_only'] = round(n / r['launches_only']['ms'] * 1e3)
        r['events_per_s_op_and_copy'] = round(n / (r['op_with_read_backs']['ms'] + r['words_to_host']['ms']) * 1e3)
        res[name] = r
        del words, out
    # (iv) the host encoder on a slice, the copy of the records to the host and their unpacking included
    m = max(n // args.host_share, 1)
    piece = dev_chunks[0][:m * 8]
    for name, vectors in (('host_encode_evt3', False), ('host_encode_evt3_vectors', True)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = piece.cpu().numpy().view('<u4').reshape(-1, 2)
        words = raw_events.encode_evt3(*dat_events.decode(host), vectors=vectors)
        ms = (time.perf_counter() - t0) * 1e3
        res[name] = dict(events=m, ms_slice=round(ms, 3), ms_scaled_to_the_recording=round(ms * n / m, 3), scaled=m != n, words_slice=int(len(words)))
        key = 'evt3_vectors' if vectors else 'evt3'
        res[name]['over_device_op_and_copy'] = round(ms * n / m / (res[key]['op_with_read_backs']['ms'] + res[key]['words_to_host']['ms']), 2)
    del dev_chunks, piece
    # (v) end to end
    if not args.no_e2e:
        from leod_amd.data import ingest
        tmp = tempfile.mkdtemp(prefix='kbench_evt_encode_')
        try:
            os.makedirs(os.path.join(tmp, 'src'))
            fn = os.path.join(tmp, 'src', 'a_td.dat')
            dat_events.write_dat(fn, records, kbench_ingest.H, kbench_ingest.W)
            for name, kw in (('ingest_plain', {}), ('ingest_write_events_evt3', dict(write_events='evt3', events_out=os.path.join(tmp, 'ev'))),
                             ('ingest_write_events_evt3_vectors', dict(write_events='evt3', evt3_vectors=True, events_out=os.path.join(tmp, 'ev')))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rep = ingest.ingest_recording(fn, None, os.path.join(tmp, name, 'a'), 'gen1', **kw)
                torch.cuda.synchronize()
                res[name] = dict(s=round(time.perf_counter() - t0, 3), frames=rep['frames'], events=rep['events'],
                                 written_bytes=rep.get('written_bytes'))
                shutil.rmtree(os.path.join(tmp, name))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    res['launch_words_equal_op_words'] = bool(ok)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


def _decode_all(words, fmt):
    state = None
    for w in words:
        _, state = ops.decode_evt(w, fmt, state)


if __name__ == '__main__':
    raise SystemExit(main())
