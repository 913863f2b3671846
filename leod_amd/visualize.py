"""Prediction videos (what vis_pred.py of the reference does with OpenCV, nerv and an mp4 writer): a detector's boxes, the boxes the
pseudo-label filter would drop, the ground truth and a timestamp drawn over the event frames of whole test recordings.

    module = fetch_model_module(config); module.load_weight(ckpt); module.to('cuda')
    run_visualization(config, module, fetch_data_module(config), 'vis', num_video=5)

    python -m leod_amd.visualize --dataset gen1 --size small --path DATA --checkpoint CKPT --out vis [--num-video 5] [--reverse]
                                 [--video png|avi] [--jpeg-quality 90]

The frames are rendered on the device in one pass (``ops.render_frames``: event image, box outlines and text in the library's own 5 x 7
font).  ``--video png`` (the default) writes them as numbered 8-bit RGB PNG files with the standard library, ``%05d.png`` + ``frames.json``
(fps).  ``--video avi`` writes a video file: the frames stay on the device, ``ops.encode_jpeg`` makes a baseline JPEG file of each, and
one copy per ``RENDER_CHUNK`` frames brings them to the host, where ``utils.mjpeg.AviWriter`` puts them into a Motion-JPEG AVI.  OpenCV's
thick-line and Hershey-font rasterisers are not reproduced: the raster rules of ``leod_render_frames_u8`` are the specification, and
so are the stream rules of the JPEG files."""
import argparse
import contextlib
import copy
import json
import os
import struct
import zlib
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from leod_amd import ops
from leod_amd.data.utils.types import DataType
from leod_amd.modules.utils.detection import DATA_KEY
from leod_amd.modules.utils.ssod import filter_pred_boxes
from leod_amd.utils.mjpeg import AviWriter

UPSAMPLE = 2
SKIP = 2
FPS = 30 // SKIP
FRAME_DT = 0.05                      # seconds between two event frames (the 50 ms windows of the representation)
RENDER_CHUNK = 128                   # frames per ops.render_frames call and per device -> host copy
GREEN, RED, BLACK = (0, 255, 0), (255, 0, 0), (0, 0, 0)
GAP = 5                              # black pixels between the forward and the time-reversed frame
VIDEO_MODES = ('png', 'avi')


def _rgb(c: Tuple[int, int, int]) -> int:
    return int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16


def get_exp_name(config, reverse: bool = False) -> str:
    """<dataset>_<model>_<size>/pred[_reverse] (vis_pred.py:41-59)."""
    dim = config.model.backbone.embed_dim
    size = {64: 'base', 48: 'small', 32: 'tiny'}.get(dim, f'dim{dim}')
    return f'{config.dataset.name}_{config.model.name}_{size}/pred' + ('_reverse' if reverse else '')


def event2rgb(ev_seq: torch.Tensor, upsample: int = UPSAMPLE) -> torch.Tensor:
    """[L, 2*bins, H, W] event representation on the device -> [L, up*H, up*W, 3] uint8 on the device, polarity ignored: a pixel with
    events is 0.25, any other 1.0, upsampled bilinearly (vis_pred.py:74-93; HWC here, the layout the drawing and the files use)."""
    return ops.render_frames(ev_seq if ev_seq.dtype in (torch.uint8, torch.float32) else ev_seq.float(), upsample=upsample)


def filter_boxes_ssod(boxes, dataset_name: str = 'gen1', downsampled_by_2: bool = False):
    """[N, 7] predictions (x1, y1, x2, y2, obj, cls conf, cls) -> (kept, removed) by the box filter of the pseudo-label loop; the
    kept boxes are clamped to the frame (vis_pred.py:62-70).  (None, None) without boxes."""
    if boxes is None or len(boxes) == 0:
        return None, None
    new_xyxy, keep = filter_pred_boxes(boxes[:, :4].clone(), dataset_name, downsampled_by_2)
    boxes = boxes.clone()
    boxes[keep, :4] = new_xyxy[keep]
    return boxes[keep], boxes[~keep]


def video_frame_indices(has_label: Sequence[bool], n_classes: int) -> List[int]:
    """The source frame shown by every frame of the video (vis_pred.py:216-224): a labelled frame is held -- 3 entries with three
    classes (Gen4 labels are dense), FPS // 2 otherwise -- and every SKIP-th entry of the result is kept."""
    hold = 3 if n_classes == 3 else FPS // 2
    shown = []
    for i, lab in enumerate(has_label):
        shown.extend([i] * (hold if lab else 1))
    return shown[::SKIP]


def _rows(x):
    if x is None:
        return np.zeros((0, 7), dtype=np.float32)
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)


def build_items(preds_keep, preds_remove, labels, label_map, times, upsample: int = UPSAMPLE):
    """The overlay of ``len(times)`` frames as ``ops.render_frames`` takes it -> (frame_off int32 [n+1], items int32 [n_items, 8], text
    uint8).  Per frame: kept predictions green, removed predictions red, labels black, the timestamp.  A box is one rectangle with
    corners int(coord * upsample) and thickness ``upsample``, followed by its text lines from the top-left corner downwards (line
    pitch 8 * upsample)."""
    items, text, frame_off = [], bytearray(), [0]
    up = int(upsample)

    def put_text(f, x, y, s, color):
        raw = s.encode('ascii', 'replace')
        items.append((f, ops.RENDER_TEXT, x, y, up, len(text), len(raw), _rgb(color)))
        text.extend(raw)

    def put_box(f, xyxy, lines, color):
        x1, y1, x2, y2 = (int(float(v) * up) for v in xyxy)
        items.append((f, ops.RENDER_RECT, x1, y1, x2, y2, up, _rgb(color)))
        for i, line in enumerate(lines):
            put_text(f, x1, y1 + 8 * up * i, line, color)

    for f, t in enumerate(times):
        for pred, color in ((preds_keep[f], GREEN), (preds_remove[f], RED)):
            for row in _rows(pred):
                obj, conf = float(row[4]), float(row[5])
                put_box(f, row[:4], (label_map[int(row[6])], f'{obj:.3f}x{conf:.3f}', f'{obj * conf:.3f}'), color)
        lbl = labels[f]
        if lbl is not None:
            xyxy, cls = _rows(lbl.get_xyxy()), _rows(lbl.get('class_id'))
            assert len(xyxy) == len(cls)
            for box, c in zip(xyxy, cls):
                put_box(f, box, (label_map[int(c)],), BLACK)
        put_text(f, 10, 10 + 10 * up, f'{t:.2f}s (N={int(t / FRAME_DT):04d})', RED)
        frame_off.append(len(items))
    return (np.asarray(frame_off, dtype=np.int32), np.asarray(items, dtype=np.int32).reshape(-1, 8),
            np.frombuffer(bytes(text), dtype=np.uint8).copy())


class EncodedVideo(NamedTuple):
    """Video frames as JPEG files: ``jpeg[k]`` is frame k (a frame the video holds several times is the same bytes object every time),
    ``hw`` the frame size, ``pixels`` uint8 [T, H', W', 3] on the host, or None where nobody asked for them."""
    jpeg: List[bytes]
    hw: Tuple[int, int]
    pixels: Optional[np.ndarray]


def encode_frames(frames: torch.Tensor, quality: int) -> List[bytes]:
    """uint8 [n, H, W, 3] on the device -> n JPEG files: ``ops.encode_jpeg`` and one device -> host copy of the blob (and one of its offsets)."""
    blob, off = ops.encode_jpeg(frames, quality)
    data, off = memoryview(blob.cpu().numpy()), off.cpu().tolist()
    return [bytes(data[off[i]:off[i + 1]]) for i in range(frames.shape[0])]


def render_sequence(preds, ev_seq: torch.Tensor, labels, filter_fn: Callable, label_map, prev_t: float = 0.,
                    jpeg_quality: Optional[int] = None, pixels: bool = False):
    """One ``predict_one_seq`` result -> (video frames uint8 [T, H', W', 3] on the host, time of the frame after the last).  Frame i
    carries the time prev_t + i * 0.05 s; which frames the video shows, and how often, is ``video_frame_indices``.  Every distinct frame
    is rendered once: one ``ops.render_frames`` call and one device -> host copy per ``RENDER_CHUNK`` frames.
    With ``jpeg_quality`` the frames stay on the device and are encoded there, once each: -> (``EncodedVideo``, time), the pixels in it
    only with ``pixels`` (a second copy per chunk)."""
    L = ev_seq.shape[0]
    assert len(preds) == len(labels) == L
    shown = video_frame_indices([l is not None for l in labels], len(label_map))
    distinct = sorted(set(shown))
    # the predictions of the whole sequence in one device -> host copy
    counts = [0 if p is None else len(p) for p in preds]
    flat = torch.cat([p.reshape(-1, 7).float() for p in preds if p is not None and len(p)]).cpu() if sum(counts) else torch.zeros((0, 7))
    starts = np.concatenate([[0], np.cumsum(counts)])
    up = UPSAMPLE
    hw = (up * ev_seq.shape[2], up * ev_seq.shape[3])
    want_pixels = jpeg_quality is None or pixels
    out = np.empty((len(distinct) if want_pixels else 0,) + hw + (3,), dtype=np.uint8)
    files: List[bytes] = []
    for lo in range(0, len(distinct), RENDER_CHUNK):
        idx = distinct[lo:lo + RENDER_CHUNK]
        keep, remove = [], []
        for i in idx:
            k, r = filter_fn(flat[starts[i]:starts[i + 1]])
            keep.append(k)
            remove.append(r)
        frame_off, items, text = build_items(keep, remove, [labels[i] for i in idx], label_map, [prev_t + i * FRAME_DT for i in idx], up)
        contiguous = idx[-1] - idx[0] + 1 == len(idx)
        ev = ev_seq[idx[0]:idx[-1] + 1] if contiguous else ev_seq[torch.as_tensor(idx, device=ev_seq.device)]
        if ev.dtype not in (torch.uint8, torch.float32):
            ev = ev.float()
        frames = ops.render_frames(ev.contiguous(), frame_off, items, text, upsample=up)
        if jpeg_quality is not None:
            files.extend(encode_frames(frames, jpeg_quality))
        if want_pixels:
            out[lo:lo + len(idx)] = frames.cpu().numpy()
    pos = {i: n for n, i in enumerate(distinct)}
    video = (out[[pos[i] for i in shown]] if shown else out[:0]) if want_pixels else None
    if jpeg_quality is not None:
        video = EncodedVideo([files[pos[i]] for i in shown], hw, video if pixels else None)
    return video, prev_t + L * FRAME_DT


# ---- PNG files with the standard library ---------------------------------------------------------------------------------------------
_PNG_MAGIC = b'\x89PNG\r\n\x1a\n'


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path: str, hwc_u8, level: int = 3) -> None:
    """[H, W, 3] uint8 -> an 8-bit RGB PNG, non-interlaced, every scanline with filter 0."""
    img = np.ascontiguousarray(hwc_u8.cpu().numpy() if isinstance(hwc_u8, torch.Tensor) else hwc_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f'write_png: uint8 [H, W, 3] expected, got {img.dtype} {img.shape}')
    h, w = img.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    raw[:, 1:] = img.reshape(h, 3 * w)
    with open(path, 'wb') as f:
        f.write(_PNG_MAGIC + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
                + _chunk(b'IDAT', zlib.compress(raw.tobytes(), level)) + _chunk(b'IEND', b''))


def read_png(path: str) -> np.ndarray:
    """The inverse of ``write_png`` for the files it writes (8-bit RGB, filter 0 on every line) -> uint8 [H, W, 3]."""
    data = open(path, 'rb').read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f'{path}: not a PNG file')
    pos, idat, w = 8, b'', None
    while pos < len(data):
        n, tag = struct.unpack('>I', data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if tag == b'IHDR':
            w, h, depth, colour, _, _, interlace = struct.unpack('>IIBBBBB', body)
            if (depth, colour, interlace) != (8, 2, 0):
                raise ValueError(f'{path}: only 8-bit RGB, non-interlaced')
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    if raw[:, 0].any():
        raise ValueError(f'{path}: filtered scanlines (not written by write_png)')
    return raw[:, 1:].reshape(h, w, 3).copy()


# ---- the loop over recordings ---------------------------------------------------------------------------------------------------------
def _truncate_padding(batch):
    """Cut the batch (B = 1) at its first padded timestep (vis_pred.py:183-190)."""
    data = batch[DATA_KEY]
    masks = data[DataType.IS_PADDED_MASK]
    pad = torch.stack([torch.as_tensor(m).reshape(-1) for m in masks])[:, 0].cpu() if len(masks) else torch.zeros(0, dtype=torch.bool)
    if bool(pad.any()):
        n = int(pad.nonzero()[0, 0])
        batch = dict(batch)
        batch[DATA_KEY] = {k: v[:n] if isinstance(v, list) and k != DataType.PATH else v for k, v in data.items()}
    return batch


def _write_frames(directory: str, frames: np.ndarray, source: List[int], times: List[float]) -> None:
    os.makedirs(directory, exist_ok=True)
    for k, frame in enumerate(frames):
        write_png(os.path.join(directory, f'{k:05d}.png'), frame)
    with open(os.path.join(directory, 'frames.json'), 'w') as f:
        json.dump({'fps': FPS, 'frames': [{'file': f'{k:05d}.png', 'source_frame': int(s), 't': round(float(t), 6)}
                                          for k, (s, t) in enumerate(zip(source, times))]}, f)


def _write_video(stem: str, jpeg: Sequence[bytes], hw: Tuple[int, int], source: List[int], times: List[float]) -> None:
    """``stem``.avi (Motion-JPEG; ``stem``_001.avi ... where one file would pass 1 GiB) and ``stem``.frames.json: what ``_write_frames`` says
    about a directory of PNG files, with ``frame`` = index in the video in the place of ``file``, and the names of the video files."""
    os.makedirs(os.path.dirname(stem) or '.', exist_ok=True)
    with AviWriter(stem + '.avi', hw[1], hw[0], FPS) as avi:
        for data in jpeg:
            avi.append(data)
    with open(stem + '.frames.json', 'w') as f:
        json.dump({'fps': FPS, 'video': [os.path.basename(p) for p in avi.paths],
                   'frames': [{'frame': k, 'source_frame': int(s), 't': round(float(t), 6)} for k, (s, t) in enumerate(zip(source, times))]}, f)


def _join(parts):
    """The per-sample results of ``render_sequence`` of one recording as one."""
    if isinstance(parts[0], EncodedVideo):
        px = None if parts[0].pixels is None else np.concatenate([p.pixels for p in parts])
        return EncodedVideo([f for p in parts for f in p.jpeg], parts[0].hw, px)
    return np.concatenate(parts)


def _one_pass(config, module, data_module, label_map, filter_fn, num_video: int, device, on_recording: Callable, **render_kw) -> int:
    """Streams the test split one recording at a time through ``predict_one_seq`` + ``render_sequence`` (``render_kw``: its JPEG options);
    ``on_recording(name, frames, source frame indices, times)`` for every finished recording but the first of Gen1 (vis_pred.py:264-281).
    -> recordings handed over."""
    from leod_amd.train import _device_batches
    is_gen1 = config.dataset.name == 'gen1'
    data_module.setup('test')
    parts, source, times, video_cnt, prev_t, frame0, done = [], [], [], 0, 0., 0, 0
    batches = iter(_device_batches(data_module.test_dataloader(), module, device))
    with torch.no_grad(), contextlib.closing(batches):           # (leaving early stops the loader's producer thread)
        for batch in batches:
            data = batch[DATA_KEY]
            eoe = bool(torch.as_tensor(data[DataType.IS_LAST_SAMPLE]).reshape(-1)[0])
            name = os.path.basename(str(data[DataType.PATH][0]).rstrip('/'))
            if video_cnt == 0 and is_gen1:                       # the first Gen1 test recording shows next to nothing
                video_cnt, prev_t = video_cnt + int(eoe), 0.
                continue
            batch = _truncate_padding(batch)
            if len(batch[DATA_KEY][DataType.EV_REPR]):
                preds, ev_seq, labels = module.predict_one_seq(batch)
                video, next_t = render_sequence(preds, ev_seq, labels, filter_fn, label_map, prev_t=prev_t, **render_kw)
                shown = video_frame_indices([l is not None for l in labels], len(label_map))
                parts.append(video)
                ev_idx = batch[DATA_KEY].get(DataType.EV_IDX)   # the frames' positions in the recording (a stream may start after frame 0)
                where = [int(torch.as_tensor(e).reshape(-1)[0]) for e in ev_idx] if ev_idx else [frame0 + i for i in range(len(labels))]
                source.extend(where[i] for i in shown)
                times.extend(prev_t + i * FRAME_DT for i in shown)
                prev_t, frame0 = next_t, frame0 + len(labels)
            if eoe:
                if parts:
                    on_recording(name, _join(parts), source, times)
                    done += 1
                parts, source, times, video_cnt, prev_t, frame0 = [], [], [], video_cnt + 1, 0., 0
            if done >= num_video:
                break
    return done


def run_visualization(config, module, data_module, out_dir: str, num_video: Optional[int] = None, reverse: Optional[bool] = None,
                      sequence_length: Optional[int] = None, video: Optional[str] = None, jpeg_quality: int = 90):
    """The loop of vis_pred.py:229-319.  One recording at a time (batch size 1, one loader worker, samples of 640 frames for Gen1 and
    256 for Gen4 unless ``sequence_length`` says otherwise), ``num_video`` recordings of the test split (``dataset.test_ratio`` = num_video /
    400 for Gen1, / 100 for Gen4; every recording when that would select none), the first Gen1 recording skipped.  Writes
    ``out_dir/<exp_name>/<recording>/%05d.png`` and ``frames.json`` = {fps, frames: [{file, source_frame, t}]}.  ``reverse``: a second
    pass with ``dataset.reverse_event_order``; forward and time-reversed frames side by side (5 black pixels between them, cropped to
    the common length) under ``<recording>_both/``; the forward frames stay where they are (the reference deletes its forward file).
    ``num_video`` counts the recordings written, not the skipped one.  Like the script, the call CHANGES ``config`` (dataset.sequence_length,
    dataset.test_ratio, batch_size.eval, hardware.num_workers.eval) and ``data_module`` (dataset_config, eval batch size and workers) in
    place.  -> {'dir', 'recordings': [names], 'both': [names]}.
    ``video`` = 'avi' (None: ``config.video``, else 'png'): ``out_dir/<exp_name>/<recording>.avi`` and ``<recording>.frames.json`` = {fps, video:
    [file names], frames: [{frame, source_frame, t}]} instead of the directory of PNG files, JPEG frames of ``jpeg_quality`` encoded on the
    device; with ``reverse`` also ``<recording>_both.avi``: the composite is built on the host as above, from the pixels of the forward
    pass, which this mode keeps in host memory until the second pass has used them, and goes to the device to be encoded."""
    video = str(config.get('video', 'png') if video is None else video)
    if video not in VIDEO_MODES:
        raise ValueError(f'video={video!r}: one of {VIDEO_MODES} expected')
    avi = video == 'avi'
    from leod_amd.utils.evaluation.prophesee.evaluator import get_labelmap
    num_video = int(config.get('num_video', 5) if num_video is None else num_video)
    reverse = bool(config.get('reverse', False) if reverse is None else reverse)
    is_gen1 = config.dataset.name == 'gen1'
    ds = config.dataset
    ds.sequence_length = int(sequence_length) if sequence_length else (640 if is_gen1 else 256)
    ratio = num_video / (400 if is_gen1 else 100)
    test_dir = os.path.join(str(ds.path), 'test')
    n_rec = len(os.listdir(test_dir)) if os.path.isdir(test_dir) else 0
    ds.test_ratio = ratio if round(n_rec * ratio) >= 1 else -1
    config.batch_size.eval = 1
    config.hardware.num_workers.eval = 1
    data_module.dataset_config = ds
    data_module.overall_batch_size_eval = data_module.overall_num_workers_eval = 1
    label_map = get_labelmap(dst_name=ds.name)
    filter_fn = lambda b: filter_boxes_ssod(b, ds.name, ds.downsample_by_factor_2)          # noqa: E731
    device = next(module.parameters()).device
    module.eval()
    module.setup('test')
    vis_dir = os.path.join(out_dir, get_exp_name(config, reverse))
    os.makedirs(vis_dir, exist_ok=True)
    summary = {'dir': vis_dir, 'recordings': [], 'both': []}

    kept = {}                                                    # avi + reverse: recording -> (forward pixels, source frames, times)

    def forward(name, frames, source, times):
        if avi:
            _write_video(os.path.join(vis_dir, name), frames.jpeg, frames.hw, source, times)
            if reverse:
                kept[name] = (frames.pixels, list(source), [round(float(t), 6) for t in times])
        else:
            _write_frames(os.path.join(vis_dir, name), frames, source, times)
        summary['recordings'].append(name)
    render_kw = dict(jpeg_quality=int(jpeg_quality), pixels=reverse) if avi else {}
    _one_pass(config, module, data_module, label_map, filter_fn, num_video, device, forward, **render_kw)
    if not reverse:
        return summary
    rev_module = copy.copy(data_module)                          # the same loaders over the recordings read backwards (vis_pred.py:285-290)
    rev_module.dataset_config = copy.deepcopy(ds)
    rev_module.dataset_config.reverse_event_order = True

    def both(name, frames, source, times):
        fwd_dir = os.path.join(vis_dir, name)
        if avi:
            fwd_pixels, fwd_source, fwd_t = kept.pop(name)
            meta = [{'source_frame': s, 't': t} for s, t in zip(fwd_source, fwd_t)]
        else:
            meta = json.load(open(os.path.join(fwd_dir, 'frames.json')))['frames']
        frames = frames[::-1]                                    # back into forward time
        n = min(len(meta), len(frames))
        rows = []
        for k in range(n):
            a, b = fwd_pixels[k] if avi else read_png(os.path.join(fwd_dir, meta[k]['file'])), frames[k]
            h, w = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
            row = np.zeros((h, 2 * w + GAP, 3), dtype=np.uint8)
            row[:, :w], row[:, w + GAP:] = a[:h, :w], b[:h, :w]
            rows.append(row)
        if avi:
            jpeg = []
            for lo in range(0, n, RENDER_CHUNK):
                jpeg.extend(encode_frames(torch.from_numpy(np.stack(rows[lo:lo + RENDER_CHUNK])).to(device), int(jpeg_quality)))
            hw = rows[0].shape[:2] if rows else (1, 1)
            _write_video(os.path.join(vis_dir, name + '_both'), jpeg, hw, [m['source_frame'] for m in meta[:n]], [m['t'] for m in meta[:n]])
        else:
            _write_frames(os.path.join(vis_dir, name + '_both'), rows, [m['source_frame'] for m in meta[:n]], [m['t'] for m in meta[:n]])
        summary['both'].append(name)
    _one_pass(config, module, rev_module, label_map, filter_fn, num_video, device, both)
    return summary


def main(argv=None) -> int:
    from leod_amd.config import vis_config, dynamically_modify_train_config
    from leod_amd.modules.utils.fetch import fetch_data_module, fetch_model_module
    ap = argparse.ArgumentParser(prog='python -m leod_amd.visualize', description=__doc__.split('\n\n')[0])
    ap.add_argument('--dataset', required=True, choices=['gen1', 'gen4'])
    ap.add_argument('--size', default='small', choices=['tiny', 'small', 'base'])
    ap.add_argument('--path', required=True, help='dataset path (holds test/<recording>/...)')
    ap.add_argument('--checkpoint', required=True)
    ap.add_argument('--out', default='vis')
    ap.add_argument('--num-video', type=int, default=5)
    ap.add_argument('--reverse', action='store_true')
    ap.add_argument('--video', default='png', choices=list(VIDEO_MODES), help='png: numbered files (default); avi: one Motion-JPEG file per recording')
    ap.add_argument('--jpeg-quality', type=int, default=90, help='quality 1 .. 100 of the frames of --video avi')
    args = ap.parse_args(argv)
    config = dynamically_modify_train_config(vis_config(args.dataset, args.size, overrides=dict(
        dataset=dict(path=args.path), checkpoint=args.checkpoint, num_video=args.num_video, reverse=args.reverse)))
    module = fetch_model_module(config)
    module.load_weight(config.checkpoint)
    module.to('cuda')
    out = run_visualization(config, module, fetch_data_module(config), args.out, video=args.video, jpeg_quality=args.jpeg_quality)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
