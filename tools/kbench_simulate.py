#!/usr/bin/env python
"""Video-to-events simulator on a GENERATED clip -- no real video and no camera is involved: 304 x 240, ``--fps`` 30, ``--seconds`` 10,
made in integers: a textured pattern that pans a pixel every second frame, and three bright rectangles that move over it.  The response
table is ``linlog``, the contrast ``--contrast`` 0.2 on both polarities, no refractory period.  In one run, with the frames on the device:

  (i)   the count + emit launches for the whole clip alone (``leod_simulate_count`` + ``leod_simulate_emit`` on buffers allocated once, the
        event count known, the state reset by a device copy, no read-back);
  (ii)  ``ops.simulate_events`` on the whole clip as a caller uses it (uploads of the table and thresholds, allocations, the read-back);
  (iii) the same rule on the HOST as a per-interval vectorised numpy formulation (no Python loop over pixels or events), on the first
        second of the clip, SCALED to the clip by the number of intervals; its records are compared with the device's first;
  (iv)  ``data.simulate.simulate_video`` from the ``.npy`` file to the ``.dat`` file, end to end;
  (v)   what no uniform-pixel recording could show: the share of non-zero voxels of the stream after ``ops.voxelize_dat_windows`` (50 ms
        windows, 10 bins), and the EVT3 bytes per event with vector words on and off.

Everything but (iii) and (iv) is warmed, then timed ``--reps`` times with a host clock around work that ends in a device synchronise (the
device sections ``--inner`` clips per window); medians and ranges are reported.  Two runs are compared byte for byte first.

    python tools/kbench_simulate.py [--seconds 10] [--fps 30] [--out FILE]
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

from leod_amd import ops  # noqa: E402
from leod_amd.data import simulate  # noqa: E402
from leod_amd.data.utils import dat_events  # noqa: E402

H, W = 240, 304
# x0, y0, vx, vy (pixels per frame), width, height, value
RECTS = ((10, 30, 3, 0, 40, 24, 230), (250, 150, -2, 1, 30, 30, 200), (120, 200, 1, -2, 56, 16, 180))


def tri(v, period):
    return np.abs(v % period - period // 2)


def scene(n):
    """The clip uint8 [n, H, W]: integers only, the same bytes everywhere."""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    frames = np.empty((n, H, W), dtype=np.uint8)
    for i in range(n):
        xs = x + i // 2
        f = 70 + tri(xs, 64) + tri(3 * y + xs, 96) // 2 + ((xs // 8 + y // 8) % 2) * 6
        for x0, y0, vx, vy, rw, rh, val in RECTS:
            rx, ry = (x0 + vx * i) % W, (y0 + vy * i) % H
            f[ry:ry + rh, rx:rx + rw] = val                      # clipped at the border
        frames[i] = f
    return frames


def host_rule(frames, times, lut, th_on, th_off):
    """The rule without a refractory period, an interval at a time, every pixel of it at once -> records [n, 2] u32."""
    lut, th_on, th_off = lut.astype(np.int64), th_on.reshape(-1).astype(np.int64), th_off.reshape(-1).astype(np.int64)
    flat = frames.reshape(len(frames), -1)
    P = flat.shape[1]
    m = lut[flat[0]]
    out = []
    for k in range(1, len(flat)):
        l0, l1, D = lut[flat[k - 1]], lut[flat[k]], int(times[k] - times[k - 1])
        on = l1 > l0
        th, gap, dl = np.where(on, th_on, th_off), np.where(on, l1 - m, m - l1), np.abs(l1 - l0)
        n = np.where((dl > 0) & (gap >= th), gap // th, 0)
        pix = np.repeat(np.arange(P), n)
        j = np.arange(len(pix)) - np.repeat(np.cumsum(n) - n, n) + 1
        a0 = np.where(on, m - l0, l0 - m)
        t = int(times[k - 1]) + np.maximum(1, D * (a0[pix] + j * th[pix]) // np.maximum(dl[pix], 1))
        order = np.lexsort((pix, t))                             # stable: time, then pixel, then j
        rec = np.empty((len(pix), 2), dtype='<u4')
        rec[:, 0] = t[order]
        px = pix[order]
        rec[:, 1] = (px % W) | ((px // W) << 14) | (on[px].astype(np.int64) << 28)
        out.append(rec)
        m = m + np.where(on, n * th, -n * th)
    return np.concatenate(out)


def stats(ms):
    return dict(ms=round(statistics.median(ms), 3), ms_min_max=[round(min(ms), 3), round(max(ms), 3)])


def timed(fn, reps, inner=1):
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
    ap.add_argument('--seconds', type=int, default=10)
    ap.add_argument('--fps', type=int, default=30)
    ap.add_argument('--contrast', type=float, default=0.2)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10, help='clips per timed window of sections (i) and (ii)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda', 0)
    n = args.seconds * args.fps
    frames = scene(n)
    times = simulate.frame_times(n, fps=args.fps)
    lut = simulate.response_table('linlog')
    th_on, th_off = simulate.thresholds(lut, H, W, args.contrast, args.contrast)
    d_frames = torch.from_numpy(frames).to(dev)
    res = dict(bench='kbench_simulate', generated_clip=True, real_video=False, height=H, width=W, fps=args.fps, frames=n,
               duration_us=int(times[-1] - times[0]), lut='linlog', contrast=args.contrast, theta=int(th_on[0, 0]), reps=args.reps,
               clips_per_timed_window=args.inner, frame_bytes=int(frames.nbytes))

    def op_all():
        return ops.simulate_events(d_frames, times, lut, th_on, th_off)
    rec, state = op_all()                                        # the warm-up, and the records of the other sections
    rec2, state2 = op_all()
    ok = torch.equal(rec, rec2) and torch.equal(state, state2)
    del rec2, state2
    c = ops.simulate_counters(state)
    n_ev = c['kept']
    tile, digit, n_state, n_count, ws_bytes = ops.simulate_query(n_ev, H, W)
    span = int(times[-1] - times[0])
    res.update(counters=c, events=n_ev, events_per_pixel_per_s=round(n_ev / (H * W) / (span / 1e6), 3), tile_pixels=tile, digit_bits=digit,
               sort_key_bits=int(np.ceil(np.log2(span))), state_bytes=8 * n_state, count_bytes=8 * (n_count + n), ws_bytes=ws_bytes)

    # (i) the launches alone
    lib, stream = ops._l(), ops._stream()
    d_times, d_lut = torch.from_numpy(times).to(dev), torch.from_numpy(lut).to(dev)
    d_on, d_off = torch.from_numpy(th_on).to(dev), torch.from_numpy(th_off).to(dev)
    fresh = torch.zeros((n_state,), dtype=torch.int64, device=dev)
    fresh[5] = -1
    fresh[ops.SIM_STATE_HEAD + 1:ops.SIM_STATE_HEAD + 2 * H * W:2] = -1
    st = torch.empty_like(fresh)
    counts = torch.empty((n_count + n,), dtype=torch.int64, device=dev)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
    out = torch.empty((n_ev, 8), dtype=torch.uint8, device=dev)
    a = (ops._p(d_frames), n, H, W, ops._p(d_times), ops._p(d_lut), ops._p(d_on), ops._p(d_off), 0, ops._p(st), ops._p(counts))

    def count_only():
        st.copy_(fresh)
        ops.check(lib.leod_simulate_count(*a, stream), 'count')

    def launches():
        count_only()
        ops.check(lib.leod_simulate_emit(*a, int(times[0]), int(times[-1]), n_ev, ops._p(ws), ws_bytes, ops._p(out), n_ev, stream), 'emit')
    launches()
    torch.cuda.synchronize()
    ok = ok and torch.equal(out, rec) and torch.equal(st, state)
    res['launches_only'] = stats(timed(launches, args.reps, args.inner))
    res['count_launch_only'] = stats(timed(count_only, args.reps, args.inner))
    # (ii) the op
    res['op_with_uploads_and_read_back'] = stats(timed(op_all, args.reps, args.inner))
    res['events_per_s_op'] = round(n_ev / res['op_with_uploads_and_read_back']['ms'] * 1e3)
    res['frames_per_s_op'] = round(n / res['op_with_uploads_and_read_back']['ms'] * 1e3)
    res['clip_seconds_per_wall_second_op'] = round(span / 1e3 / res['op_with_uploads_and_read_back']['ms'], 1)

    # (iii) the host formulation on the first second, scaled
    head = args.fps + 1                                          # fps intervals
    t0 = time.perf_counter()
    host_rec = host_rule(frames[:head], times[:head], lut, th_on, th_off)
    host_ms = (time.perf_counter() - t0) * 1e3
    dev_head, _ = ops.simulate_events(d_frames[:head], times[:head], lut, th_on, th_off)
    host_equal = bool(np.array_equal(dev_head.cpu().numpy().reshape(-1).view('<u4').reshape(-1, 2), host_rec))
    scale = (n - 1) / (head - 1)
    res['host_numpy'] = dict(intervals=head - 1, events=int(len(host_rec)), ms_first_second=round(host_ms, 3),
                             ms_scaled_to_the_clip=round(host_ms * scale, 3), scaled=True, scale=round(scale, 3),
                             records_equal_the_device=host_equal,
                             over_device_op=round(host_ms * scale / res['op_with_uploads_and_read_back']['ms'], 2),
                             over_device_launches=round(host_ms * scale / res['launches_only']['ms'], 2))
    ok = ok and host_equal

    # (v) the structured stream: voxel occupancy, EVT3 bytes per event
    t_host = rec.cpu().numpy().reshape(-1).view('<u4').reshape(-1, 2)[:, 0].astype(np.int64)
    win_off = dat_events.window_offsets(t_host, 50_000)
    vox, dropped = ops.voxelize_dat_windows(rec, win_off, 10, H, W)
    res['voxels'] = dict(windows=int(vox.shape[0]), bins=10, non_zero_share=round(float((vox != 0).float().mean()), 6), dropped=int(dropped))
    del vox
    for name, vectors in (('evt3_vectors', True), ('evt3', False)):
        words, es = ops.encode_evt(rec, 'evt3', final=True, vectors=vectors)
        ec = ops.evt_encode_counters(es)
        res[name] = dict(payload_bytes=int(words.numel()), bytes_per_event=round(words.numel() / n_ev, 3), counters=ec)
    res['dat_bytes_per_event'] = 8

    # (iv) end to end
    tmp = tempfile.mkdtemp(prefix='kbench_simulate_')
    try:
        np.save(os.path.join(tmp, 'clip.npy'), frames)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = simulate.simulate_video(os.path.join(tmp, 'clip.npy'), os.path.join(tmp, 'out'), fps=args.fps, contrast=args.contrast)
        torch.cuda.synchronize()
        res['simulate_video_npy_to_dat'] = dict(s=round(time.perf_counter() - t0, 3), events=rep['events'], file_bytes=rep['file_bytes'],
                                                batch_frames=simulate.BATCH_FRAMES)
        ok = ok and rep['events'] == n_ev
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res['two_runs_and_the_launches_are_byte_identical'] = bool(ok)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    raise SystemExit(main())
