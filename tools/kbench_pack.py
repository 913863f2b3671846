#!/usr/bin/env python
"""Packed event frames against dense ones, on the synthetic recording of ``tools/kbench_ingest.py`` (Gen1 sized, 50 ms windows,
``--events`` events per window; ``--gen4``: a 720 x 1280 recording written at half resolution).  One training batch of
``--frames`` frames ([168, 20, 240, 304] for RVT-S Gen1) is timed as

  (a) the pinned-to-device copy of the dense batch,
  (b) the pinned-to-device copy of the packed batch plus ``ops.unpack_frames``,
  (c) ``ops.pack_frames`` of the batch on the device,
  (d) bytes per frame and the ratio to dense,
  (e) ``ingest.voxelize_recording`` of the whole recording (``--windows`` windows) with write='npy' against write='packed', wall time.

(a)-(c): warm-up, then ``--reps`` repetitions between two events on the stream, the candidates alternating; medians with min / max.
(e): host clock around a call that ends synchronised, files in a temporary directory.  The recording is SYNTHETIC (uniform pixels, or
``--blobs``); the density of real Gen1 / Gen4 recordings is not measured here.  The ratio is also printed for the frames of the
tests' synthetic trees.

    python tools/kbench_pack.py [--windows 1200] [--events 50000] [--frames 168] [--blobs] [--gen4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from leod_amd import ops  # noqa: E402
from leod_amd.data import ingest  # noqa: E402
from leod_amd.data.utils import dat_events, packed  # noqa: E402

BINS, D = 10, 50_000


def synth(n_win, per_win, blobs, H, W, seed=0):
    import kbench_ingest
    if (H, W) == (kbench_ingest.H, kbench_ingest.W):
        return kbench_ingest.synth(n_win, per_win, blobs, seed)
    rng = np.random.RandomState(seed)                            # the same recipe at another sensor size
    n = n_win * per_win
    t = (np.sort(rng.randint(1, D + 1, (n_win, per_win)), axis=1) + np.arange(n_win)[:, None] * D).reshape(-1).astype(np.int64)
    return t, rng.randint(0, W, n), rng.randint(0, H, n), rng.randint(0, 2, n), np.arange(n_win + 1, dtype=np.int64) * per_win


def event_ms(fn, reps):
    """Median / min / max of ``reps`` timings of fn() between two events on the current stream."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def test_tree_ratio():
    """Dense / packed bytes of the frames the tests' synthetic trees hold (oracle.synth recordings, thinned as tests/packed_trees.py does)."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import packed_trees
    with tempfile.TemporaryDirectory() as d:
        raw, pk = packed_trees.make_tree_pair(d)
        dense = sum(np.load(f, mmap_mode='r').size for f in packed_trees.frame_files(raw, '.npy'))
        return round(dense / sum(os.path.getsize(f) for f in packed_trees.frame_files(pk, '.evp')), 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--windows', type=int, default=1200)
    ap.add_argument('--events', type=int, default=50_000, help='events per window')
    ap.add_argument('--frames', type=int, default=168, help='frames of the timed batch (L * B)')
    ap.add_argument('--blobs', action='store_true')
    ap.add_argument('--gen4', action='store_true')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--skip-ingest', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda', 0)
    H, W, ds2 = (720, 1280, True) if args.gen4 else (240, 304, False)
    Ho, Wo = (H // 2, W // 2) if ds2 else (H, W)
    t, x, y, p, off = synth(args.windows, args.events, args.blobs, H, W)
    records = dat_events.encode(t, x, y, p)
    n_batch = min(args.frames, args.windows)
    rec_dev = torch.from_numpy(records[:off[n_batch]].view(np.uint8).reshape(-1)).to(dev)
    dense_dev = torch.cat([ops.voxelize_dat_windows(rec_dev[off[a] * 8:off[min(a + 32, n_batch)] * 8],
                                                    off[a:min(a + 32, n_batch) + 1] - off[a], BINS, H, W, ds2=ds2)[0]
                           for a in range(0, n_batch, 32)])
    del rec_dev
    frame_bytes = 2 * BINS * Ho * Wo

    # (c) + the packed batch
    blob_dev, blob_off = ops.pack_frames(dense_dev)
    blob_host = blob_dev.cpu().numpy()
    ref_blob, ref_off = packed.encode_frames(dense_dev[:2].cpu().numpy())
    same = np.array_equal(blob_host[:ref_off[-1]], ref_blob) and np.array_equal(blob_off[:3].numpy(), ref_off)
    host_ms = {}                                                 # per frame, one thread, 16 frames after one warm-up call each
    frame_out = np.empty((2 * BINS, Ho, Wo), dtype=np.uint8)
    nh = min(16, n_batch)
    for name, fn in (('validate_numpy', packed.validate_frame), ('validate_lib', packed.validate_frame_host),
                     ('decode_numpy', lambda b, *chw: packed.decode_frame(b, *chw, out=frame_out)),
                     ('decode_lib', lambda b, *chw: packed.decode_frame_host(b, *chw, out=frame_out))):
        fn(blob_host[:int(blob_off[1])], 2 * BINS, Ho, Wo)
        t0 = time.perf_counter()
        for k in range(nh):
            fn(blob_host[int(blob_off[k]):int(blob_off[k + 1])], 2 * BINS, Ho, Wo)
        host_ms[name] = round((time.perf_counter() - t0) * 1e3 / nh, 3)

    dense_pin = torch.empty(dense_dev.shape, dtype=torch.uint8).pin_memory()
    dense_pin.copy_(dense_dev)
    blob_pin = torch.empty((blob_dev.numel(),), dtype=torch.uint8).pin_memory()
    blob_pin.copy_(blob_dev)
    off_pin = blob_off[:-1].clone().pin_memory()
    flags_pin = torch.zeros((n_batch,), dtype=torch.int32).pin_memory()
    out_dev = torch.empty_like(dense_dev)

    def copy_dense():
        out_dev.copy_(dense_pin, non_blocking=True)

    def copy_packed_unpack():
        b = blob_pin.to(dev, non_blocking=True)
        ops.unpack_frames(b, off_pin.to(dev, non_blocking=True), flags_pin.to(dev, non_blocking=True), 2 * BINS, Ho, Wo, out=out_dev)

    def unpack_only():
        ops.unpack_frames(blob_dev, slot_dev, None, 2 * BINS, Ho, Wo, out=out_dev)

    def pack():
        ops.pack_frames(dense_dev)

    slot_dev = blob_off[:-1].to(dev)
    copy_packed_unpack()
    torch.cuda.synchronize()
    same = same and torch.equal(out_dev, dense_dev)
    cands = dict(dense_copy=copy_dense, packed_copy_unpack=copy_packed_unpack, unpack_only=unpack_only, pack=pack)
    for fn in cands.values():                                    # warm-up
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.reps):                                   # alternate the candidates within one repetition
        for k, fn in cands.items():
            times[k] += event_ms(fn, 1)
    res = dict(bench='kbench_pack', synthetic=True, dataset='gen4_ds2' if args.gen4 else 'gen1', blobs=args.blobs, windows=args.windows,
               events_per_window=args.events, batch=[n_batch, 2 * BINS, Ho, Wo], reps=args.reps, outputs_equal=bool(same),
               dense_bytes_per_frame=frame_bytes, packed_bytes_per_frame=round(blob_dev.numel() / n_batch),
               ratio=round(frame_bytes * n_batch / blob_dev.numel(), 2),
               nonzero_fraction=round(float((dense_dev != 0).float().mean()), 5),
               a_dense_copy_ms=stats(times['dense_copy']), b_packed_copy_unpack_ms=stats(times['packed_copy_unpack']),
               unpack_only_ms=stats(times['unpack_only']), c_pack_ms=stats(times['pack']),
               host_ms_per_frame=host_ms,
               test_tree_ratio=test_tree_ratio())
    del dense_pin, blob_pin, out_dev, dense_dev, blob_dev

    if not args.skip_ingest:                                      # (e)
        with tempfile.TemporaryDirectory() as d:
            shape = (args.windows, 2 * BINS, Ho, Wo)

            def run_npy():
                mm = np.lib.format.open_memmap(os.path.join(d, 'f.npy'), mode='w+', dtype=np.uint8, shape=shape)
                ingest.voxelize_recording(records, off, mm, BINS, H, W, ds2)
                mm.flush()
                del mm

            def run_packed():
                w = packed.PackedWriter(os.path.join(d, 'f.evp'), *shape[1:])
                ingest.voxelize_recording(records, off, None, BINS, H, W, ds2, packed_writer=w)
                w.close()

            wall = {'npy': [], 'packed': []}
            for rep in range(3):                                 # the first pair is the warm-up (page cache, allocator)
                for name, fn in (('npy', run_npy), ('packed', run_packed)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep:
                        wall[name].append(time.perf_counter() - t0)
            st = packed.PackedFrames(os.path.join(d, 'f.evp'))
            k = args.windows // 2
            file_same = np.array_equal(st.read(k, k + 2), np.load(os.path.join(d, 'f.npy'), mmap_mode='r')[k:k + 2])
            st.close()
            res.update(e_voxelize_recording_s=dict(npy=round(statistics.median(wall['npy']), 3), packed=round(statistics.median(wall['packed']), 3)),
                       file_bytes=dict(npy=os.path.getsize(os.path.join(d, 'f.npy')), packed=os.path.getsize(os.path.join(d, 'f.evp'))),
                       files_equal=bool(file_same))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')
    return 0 if res['outputs_equal'] and res.get('files_equal', True) else 1


if __name__ == '__main__':
    raise SystemExit(main())
