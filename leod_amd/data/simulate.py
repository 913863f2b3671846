"""Video-to-events simulator: labelled frame video to an event recording the ingestion takes unchanged.

    python -m leod_amd.data.simulate SRC DST --fps 30 [--contrast 0.2] [--write-events dat|evt2|evt3] [--boxes FILE.npy]

``SRC`` is a ``.npy`` file, uint8 ``[N, H, W]`` (luma) or ``[N, H, W, 3]`` (RGB), memory-mapped and uploaded a batch of frames at a time, or
a directory of images, read in name order with Pillow.  RGB becomes luma by the integer ``(77 R + 150 G + 29 B + 128) >> 8``.  The frames
go through ``ops.simulate_events`` (csrc/k_simulate.hip; the rule, all in integers: DESIGN.md section 1) with the state carried from
batch to batch, and the records through ``EventFileWriter``: ``DST/<name>_td.dat`` or ``DST/<name>.raw``, with ``--boxes`` the box array
beside it as ``DST/<name>_bbox.npy``.  ``DST`` is then a source directory of ``python -m leod_amd.data.ingest``.

The response table is built here, once, with numpy, and handed to the op as 256 integers in Q16: ``linlog`` (default; ``ln v`` above 20,
the line through the origin that meets it there below), ``log`` (``ln (1 + v)``), ``linear`` (``v / 255``).  A contrast ``C`` is the
threshold ``round(C * 65536)`` on that scale; ``--threshold-sigma S`` draws a threshold per pixel and polarity from a normal distribution
around it (``numpy.random.RandomState(seed)``), clamped from below so that the op's limits hold.

What this is not: no noise is injected (no shot noise, no leak events, no hot pixels), no frames are interpolated -- the linear course of
the table's value between two frames is the whole temporal model -- colour is a luma conversion and nothing more, and nothing is claimed
about the accuracy of a detector trained on the result."""
import argparse
import json
import os
from typing import Optional

import numpy as np

from leod_amd.data.genx_utils.labels import BBOX_DTYPE
from leod_amd.data.utils import event_writer as ew

LUTS = ('linlog', 'log', 'linear')
Q = 1 << 16                      # the table and the thresholds are Q16
LINLOG_KNEE = 20
MAX_CANDIDATES = 4096            # ops.SIM_MAX_CANDIDATES, restated: this module is checked without the library
BATCH_FRAMES = 64
IMAGE_SUFFIXES = ('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff', '.pgm', '.ppm')


def response_table(kind: str = 'linlog') -> np.ndarray:
    """The response table int32 [256] in Q16: non-decreasing, from 0."""
    v = np.arange(256, dtype=np.float64)
    if kind == 'linlog':
        f = np.where(v > LINLOG_KNEE, np.log(np.maximum(v, 1.0)), v * (np.log(LINLOG_KNEE) / LINLOG_KNEE))
    elif kind == 'log':
        f = np.log1p(v)
    elif kind == 'linear':
        f = v / 255.0
    else:
        raise ValueError(f'lut={kind!r}: one of {LUTS} expected')
    return np.round(f * Q).astype(np.int32)


def least_threshold(lut) -> int:
    """The least threshold the op takes with this table: (max - min) // theta <= 4096."""
    span = int(np.max(lut)) - int(np.min(lut))
    return span // (MAX_CANDIDATES + 1) + 1


def thresholds(lut, height: int, width: int, contrast_on: float, contrast_off: float, sigma: float = 0.0, seed: int = 0):
    """(theta_on, theta_off) int32 [H, W]: ``round(C * 65536)``, with ``sigma`` > 0 drawn per pixel around it, not below ``least_threshold``."""
    for name, c in (('contrast_on', contrast_on), ('contrast_off', contrast_off)):
        if not isinstance(c, (int, float)) or isinstance(c, bool) or not 0 < c < 1 << 14:
            raise ValueError(f'{name}={c!r}: a positive number expected')
    if not isinstance(sigma, (int, float)) or isinstance(sigma, bool) or not 0 <= sigma < 1 << 14:
        raise ValueError(f'threshold_sigma={sigma!r}: a number >= 0 expected')
    least = least_threshold(lut)
    rng = np.random.RandomState(seed)
    out = []
    for c in (contrast_on, contrast_off):
        th = np.full((height, width), float(c))
        if sigma > 0:
            th = th + sigma * rng.standard_normal((height, width))
        th = np.round(th * Q)
        if sigma == 0 and th[0, 0] < least:
            raise ValueError(f'a contrast of {c} is the threshold {int(th[0, 0])}; the least this table takes is {least} ({least / Q:.6f})')
        out.append(np.maximum(th, least).astype(np.int32))
    return out[0], out[1]


def luma(frames: np.ndarray) -> np.ndarray:
    """uint8 [n, H, W] or [n, H, W, 3] -> uint8 [n, H, W], contiguous."""
    if frames.dtype != np.uint8 or frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] != 3):
        raise ValueError(f'frames: uint8 [N, H, W] or [N, H, W, 3] expected, got {frames.dtype} {frames.shape}')
    if frames.ndim == 3:
        return np.array(frames, order='C')                       # a copy: a memory-mapped file is read-only
    f =frames.astype(np.int32)
    return ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).astype(np.uint8)


def frame_times(n: int, fps=None, times=None) -> np.ndarray:
    """int64 [n]: ``round(i * 10^6 / fps)``, or the array given."""
    if (fps is None) == (times is None):
        raise ValueError('frame times: fps or times expected, one of them')
    if times is not None:
        t = np.asarray(times)
        if t.dtype.kind not in 'iu' or t.shape != (n,):
            raise ValueError(f'times: {n} integers expected, got {t.dtype} {t.shape}')
        return t.astype(np.int64)
    if isinstance(fps, bool) or not isinstance(fps, (int, float)) or not 0 < fps <= 1e6:
        raise ValueError(f'fps={fps!r}: a number in (0, 10^6] expected')
    return np.array([int(round(i * 1e6 / fps)) for i in range(n)], dtype=np.int64)


def boxes_from_frames(frame_idx, xywh, class_id, times_us) -> np.ndarray:
    """Per-frame boxes -> the box array of a recording (``labels.BBOX_DTYPE``, which ``ingest.convert_labels`` reads by field name):
    box i lies on frame ``frame_idx[i]`` and takes its time ``times_us[frame_idx[i]]``; ``xywh`` [n, 4] with (x, y) the top-left corner;
    confidence and objectness are 1.  Sorted by time, boxes of one frame in the order given."""
    frame_idx = np.asarray(frame_idx)
    xywh = np.asarray(xywh, dtype=np.float32).reshape(-1, 4)
    class_id = np.asarray(class_id)
    times_us = np.asarray(times_us)
    n = len(frame_idx)
    if frame_idx.ndim != 1 or frame_idx.dtype.kind not in 'iu' or len(xywh) != n or class_id.shape != (n,) or class_id.dtype.kind not in 'iu':
        raise ValueError('boxes_from_frames: n frame indices, n x 4 numbers and n class ids expected')
    if n and (frame_idx.min() < 0 or frame_idx.max() >= len(times_us)):
        raise ValueError(f'boxes_from_frames: frame indices in [0, {len(times_us)}) expected')
    if n and class_id.min() < 0:
        raise ValueError('boxes_from_frames: class ids >= 0 expected')
    out = np.zeros((n,), dtype=BBOX_DTYPE)
    out['t'] = times_us[frame_idx] if n else 0
    for k, name in enumerate('xywh'):
        out[name] = xywh[:, k]
    out['class_id'] = class_id
    out['class_confidence'] = 1.0
    out['objectness'] = 1.0
    return out[np.argsort(out['t'], kind='stable')]


class _Frames:
    """The frames of ``src`` a batch at a time: ``len``, ``hw``, ``batch(a, b)`` -> luma uint8 [b - a, H, W]."""

    def __init__(self, src: str):
        self.files = None
        if os.path.isdir(src):
            self.files = sorted(f for f in os.listdir(src) if f.lower().endswith(IMAGE_SUFFIXES))
            if not self.files:
                raise FileNotFoundError(f'{src}: no image ({", ".join(IMAGE_SUFFIXES)}) in it')
            try:
                from PIL import Image
            except ImportError:
                raise RuntimeError(f'{src} is a directory of images, which are read with Pillow, and Pillow is not installed; '
                                   'convert the frames to a .npy file, uint8 [N, H, W] or [N, H, W, 3]') from None
            self._open, self.dir = Image.open, src
            first = self._image(0)
            self.n, self.hw = len(self.files), first.shape[1:3]
        else:
            self.arr = np.load(src, mmap_mode='r')
            if self.arr.dtype != np.uint8 or self.arr.ndim not in (3, 4) or (self.arr.ndim == 4 and self.arr.shape[3] != 3):
                raise ValueError(f'{src}: uint8 [N, H, W] or [N, H, W, 3] expected, got {self.arr.dtype} {self.arr.shape}')
            self.n, self.hw = self.arr.shape[0], self.arr.shape[1:3]

    def _image(self, i: int) -> np.ndarray:
        with self._open(os.path.join(self.dir, self.files[i])) as im:
            a = np.asarray(im.convert('RGB') if im.mode not in ('L', 'RGB') else im)
        if a.dtype != np.uint8:
            raise ValueError(f'{self.files[i]}: 8-bit image expected, got {a.dtype}')
        return luma(a[None])

    def batch(self, a: int, b: int) -> np.ndarray:
        if self.files is None:
            return luma(np.asarray(self.arr[a:b]))
        frames = [self._image(i) for i in range(a, b)]
        for i, f in zip(range(a, b), frames):
            if f.shape[1:3] != tuple(self.hw):
                raise ValueError(f'{self.files[i]}: {f.shape[2]}x{f.shape[1]}, the first image is {self.hw[1]}x{self.hw[0]}')
        return np.concatenate(frames)


def simulate_video(src: str, dst: str, fps=None, times=None, contrast: float = 0.2, contrast_on: Optional[float] = None,
                   contrast_off: Optional[float] = None, threshold_sigma: float = 0.0, seed: int = 0, refractory_us: int = 0,
                   lut: str = 'linlog', write_events: str = 'dat', evt3_vectors: bool = False, boxes=None, name: Optional[str] = None,
                   batch_frames: int = BATCH_FRAMES, device=None) -> dict:
    """``src`` -> ``dst/<name>_td.dat`` or ``dst/<name>.raw`` (and ``dst/<name>_bbox.npy`` with ``boxes``: a file name or a structured
    array); -> the report.  Every option is checked before a file is written."""
    fr = _Frames(src)
    (height, width), n = (int(v) for v in fr.hw), fr.n
    if isinstance(times, str):
        times = np.load(times)
    t = frame_times(n, fps, times)
    table = response_table(lut)
    th_on, th_off = thresholds(table, height, width, contrast if contrast_on is None else contrast_on,
                               contrast if contrast_off is None else contrast_off, threshold_sigma, seed)
    ew.check_format(write_events, height, width, evt3_vectors)
    if isinstance(batch_frames, bool) or not isinstance(batch_frames, int) or batch_frames < 1:
        raise ValueError(f'batch_frames={batch_frames!r}: a positive integer expected')
    import torch
    from leod_amd import ops
    ops.simulate_check(height, width, t, table, th_on, th_off, refractory_us)
    if isinstance(boxes, str):
        boxes = np.load(boxes)
    if boxes is not None and (not isinstance(boxes, np.ndarray) or boxes.dtype.names is None or 't' not in boxes.dtype.names):
        raise ValueError('boxes: a structured box array with a field t expected')
    if name is None:
        name = os.path.splitext(os.path.basename(os.path.normpath(src)))[0]
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    os.makedirs(dst, exist_ok=True)
    fn = os.path.join(dst, name + ew.SUFFIX[write_events])
    writer = ew.EventFileWriter(fn, write_events, height, width, evt3_vectors)
    state = None
    try:
        for a in range(0, n, batch_frames):
            b = min(a + batch_frames, n)
            frames = torch.from_numpy(fr.batch(a, b)).to(device)
            rec, state = ops.simulate_events(frames, t[a:b], table, th_on, th_off, refractory_us, state)
            writer.append(rec)
        writer.close()
    except BaseException:
        writer.abort()
        raise
    if boxes is not None:
        np.save(os.path.join(dst, name + '_bbox.npy'), boxes)
    c = ops.simulate_counters(state) if state is not None else dict(frames=0, kept=0, on=0, off=0, dropped=0, t_last=-1)
    duration = int(t[-1] - t[0]) if n else 0
    return dict(name=name, file=fn, format=write_events, frames=n, height=height, width=width, duration_us=duration, lut=lut,
                theta_on=[int(th_on.min()), int(th_on.max())], theta_off=[int(th_off.min()), int(th_off.max())],
                refractory_us=int(refractory_us), events=c['kept'], on=c['on'], off=c['off'], dropped=c['dropped'],
                payload_bytes=writer.payload_bytes, file_bytes=os.path.getsize(fn), boxes=None if boxes is None else int(len(boxes)),
                events_per_pixel_per_s=round(c['kept'] / (height * width) / (duration / 1e6), 6) if duration else None)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog='python -m leod_amd.data.simulate', description=__doc__.split('\n\n')[0])
    ap.add_argument('src', help='frames: a .npy file uint8 [N, H, W] or [N, H, W, 3], or a directory of images (name order)')
    ap.add_argument('dst', help='directory to write <name>_td.dat or <name>.raw (and <name>_bbox.npy) into')
    when = ap.add_mutually_exclusive_group(required=True)
    when.add_argument('--fps', type=float, default=None, help='frame i is at round(i * 10^6 / FPS) microseconds')
    when.add_argument('--times', default=None, metavar='FILE.npy', help='the frame times in microseconds, strictly increasing integers')
    ap.add_argument('--contrast', type=float, default=0.2, help='the contrast threshold, on the scale of the table (default 0.2)')
    ap.add_argument('--contrast-on', type=float, default=None, help='the ON threshold alone')
    ap.add_argument('--contrast-off', type=float, default=None, help='the OFF threshold alone')
    ap.add_argument('--threshold-sigma', type=float, default=0.0, metavar='S', help='draw a threshold per pixel: normal around the contrast')
    ap.add_argument('--seed', type=int, default=0, help='of the threshold draw')
    ap.add_argument('--refractory-us', type=int, default=0, metavar='R', help='drop an event less than R microseconds behind its pixel\'s last')
    ap.add_argument('--lut', default='linlog', choices=list(LUTS), help='the response table (default linlog)')
    ap.add_argument('--write-events', default='dat', choices=list(ew.FORMATS), metavar='FMT', help='dat (default), evt2 or evt3')
    ap.add_argument('--evt3-vectors', action='store_true', help='with --write-events evt3: write runs of events in one row as vector words')
    ap.add_argument('--boxes', default=None, metavar='FILE.npy', help='a Prophesee structured box array, copied as <name>_bbox.npy')
    ap.add_argument('--name', default=None, help='the recording\'s name (default: the name of SRC)')
    ap.add_argument('--batch-frames', type=int, default=BATCH_FRAMES, help='frames per upload and device call')
    args = ap.parse_args(argv)
    try:
        rep = simulate_video(args.src, args.dst, fps=args.fps, times=args.times, contrast=args.contrast, contrast_on=args.contrast_on,
                             contrast_off=args.contrast_off, threshold_sigma=args.threshold_sigma, seed=args.seed,
                             refractory_us=args.refractory_us, lut=args.lut, write_events=args.write_events, evt3_vectors=args.evt3_vectors,
                             boxes=args.boxes, name=args.name, batch_frames=args.batch_frames)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    print(json.dumps(rep), flush=True)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
