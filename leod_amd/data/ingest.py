"""Recording ingestion: a raw Prophesee recording (``*_td.dat`` or Metavision ``*.raw`` events + ``*_bbox.npy`` boxes) to the dataset tree
the loaders read (layout: ``leod_amd/data/utils/misc.py``).  The reference has no such stage (its docs/install.md points at pre-voxelised
downloads).

The record bytes go to the device as they lie in the file; ``ops.voxelize_dat_windows`` (csrc/k_ingest.hip) decodes them and writes
the stacked histogram of every window.  The host only reads timestamps (sortedness, window offsets), moves bytes and writes labels.

Window rule (the project's own), D = ``duration_us``:
  * frame k holds the events with k*D < t <= (k+1)*D; events at t = 0 belong to frame 0; N = max(ceil(t_last / D), 1) frames;
  * a box with timestamp t_l belongs to frame max(ceil(t_l / D) - 1, 0): a frame's labels sit at its end; boxes beyond frame N - 1 are
    dropped; where boxes of several timestamps fall in one frame, those of the latest timestamp are kept.

``--write packed`` writes the frames as a packed store (``.evp``, data/utils/packed.py) instead of the raw ``.npy`` twin: every chunk
of windows is encoded on the device (``ops.pack_frames``) and only the packed bytes come back.

An unfiltered ``.dat`` file knows its number of frames in advance (``voxelize_recording``, into an ``open_memmap``).  A ``.raw`` file (EVT2 /
EVT3; ``data/utils/raw_events.py``), or either container with a filter, a fit or ``--write-events`` on, streams through ``voxelize_raw_recording``: the chunk reader
(``_RecordChunks``: payload bytes through one pinned buffer, ``ops.decode_evt`` of csrc/k_evt.hip with the carried state), the filter chain
(``_FilterChain``: what reaches the voxeliser, the order check, the filters' part of the report) and one loop body that cuts complete windows
and carries the rest.  ``_TreeWriter`` writes the tree of both.  ``--unlabelled ok`` accepts recordings without a box file (zero labels).

Noise filters (off by default; the rule: DESIGN.md section 1; ``ops.filter_events``, csrc/k_filter.hip): ``--pixel-mask FILE.npy`` removes
the events of the masked pixels, ``--hot-rate HZ`` first counts the recording's events per pixel on the device and masks the pixels that
fire faster (the mask is written beside the frames as ``hot_pixels.npy``), ``--denoise-us N`` keeps an event only if one of its 8
neighbours fired at most N microseconds before it.  With one of them given, both containers take the streaming route, at sensor
resolution; the number of frames, the window edges and the label files are those of the unfiltered recording.

Per-pixel filters (off by default; the rule: DESIGN.md section 1; ``ops.pixel_filter_events``, csrc/k_pixfilter.hip): ``--trail-us N`` keeps
the first event of every burst of same-polarity events of a pixel that follow each other within N microseconds, ``--stc-us N`` keeps a
burst from its second event on (``--stc-cut-trail``: the second alone), ``--anti-flicker FMIN:FMAX`` removes the events of a pixel
whose rising edges have repeated ``--flicker-lock`` times in a row at a frequency in the band.  They run first, on whole per-pixel
sequences, and apply the bounds and the mask; ``--denoise-us`` then sees what they keep.

Sensor fit (off by default; the rule: DESIGN.md section 1; ``ops.fit_events``, csrc/k_fit.hip): ``--fit auto|K`` accepts a recording of
any sensor size or mounting and maps its events onto the frames of ``--dataset`` -- mirror (``--fit-mirror``), quarter turns
(``--fit-orient``), an integer scale K (auto: the largest at which the scaled image still covers the frame), an offset (``--fit-offset``,
default centred; what leaves the frame is cropped) -- and ``--fit-reduce`` says which events of the K x K pixels of a cell survive: those
of the centre pixel (``pick``; for K = 2 what ``ds2`` does for Gen4), all (``sum``), or one per ``--fit-threshold`` of net polarity
(``fire``).  The source size is ``--sensor WxH``, else the header's, else the dataset's.  With a fit both containers take the streaming
route; the filters above, the masks and ``hot_pixels.npy`` stay at the source geometry, the fit is the chain's last stage and the
voxeliser runs at the frame geometry; the boxes take the same map (``event_filter.fit_boxes``).  Without ``--fit`` a recording of any
other size is refused as before.

Event file (off by default; the rule: DESIGN.md section 1; ``ops.encode_evt``, csrc/k_evtenc.hip; ``data/utils/event_writer.py``):
``--write-events dat|evt2|evt3 --events-out DIR`` also writes the events that reach the voxeliser -- after the decoder, the filters and
the fit -- as ``DIR[/<split>]/<name>_td.dat`` or ``DIR[/<split>]/<name>.raw`` (``--evt3-vectors``: EVT3 with vector words), at the fit's
frame geometry where a fit is on, else the source sensor's, and the boxes as they enter ``convert_labels`` as ``<name>_bbox.npy`` beside
it: ``DIR`` is a source directory this tool reads, so a cleaned stream can be looked at, archived, or ingested again with another window
without the filter chain.  EVT words are made on the device, chunk by chunk, and are those of ``raw_events.encode_evt2`` /
``encode_evt3`` on all the events at once.  With the option both containers take the streaming route; the dataset tree is byte for byte
the one written without it.  ``DIR`` must be neither SRC nor DST; EVT holds 11 bits of x and of y, so a geometry beyond 2048 x 2048 is
refused (``dat`` holds 14).  No Metavision tool has read a file written here.

    python -m leod_amd.data.ingest SRC DST --dataset gen1|gen4 [--write npy|packed] [--unlabelled error|ok]
                                   [--denoise-us N] [--pixel-mask FILE.npy] [--hot-rate HZ]
                                   [--trail-us N | --stc-us N [--stc-cut-trail]] [--anti-flicker FMIN:FMAX [--flicker-lock N]]
                                   [--sensor WxH] [--fit auto|K [--fit-offset center|X,Y] [--fit-orient 0|90|180|270] [--fit-mirror]
                                    [--fit-reduce pick|sum|fire [--fit-threshold N]]]
                                   [--write-events dat|evt2|evt3 --events-out DIR [--evt3-vectors]]
"""
import argparse
import contextlib
import glob
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from leod_amd.data.utils import dat_events, event_filter as ef, event_writer as ew
from leod_amd.data.utils.types import DatasetType

# labels.npz 'labels': the tree's 40-byte label record (data/genx_utils/labels.py reads it by field name)
LABEL_DTYPE = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence', 'objectness'],
                        'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<f4', '<f4'],
                        'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})
# older Prophesee annotation files name two fields differently (io/box_loading.py:27-44)
_FIELD_ALIASES = {'ts': 't', 'confidence': 'class_confidence'}
SENSOR_HW = {DatasetType.GEN1: (240, 304), DatasetType.GEN4: (720, 1280)}
DEFAULT_KEEP_CLASSES = {DatasetType.GEN1: None, DatasetType.GEN4: (0, 1, 2)}        # the three classes the Gen4 configs train on
FRAMES_PER_COPY = 32             # windows per device call and per copy through the pinned buffer
RAW_CHUNK_BYTES = 64 << 20       # payload bytes of a .raw file per decode call (a multiple of 4: whole EVT2 and EVT3 words)
FIT_KEYS = ('scale', 'offset', 'orient', 'mirror', 'reduce', 'threshold')           # the options of a sensor fit: event_filter.fit_spec


def _dataset_type(dataset_type) -> DatasetType:
    if isinstance(dataset_type, DatasetType):
        return dataset_type
    try:
        return {'gen1': DatasetType.GEN1, 'gen4': DatasetType.GEN4}[str(dataset_type).lower()]
    except KeyError:
        raise ValueError(f'dataset type {dataset_type!r}: gen1 or gen4 expected') from None


def frame_hw(dataset_type) -> Tuple[int, int]:
    """(Hd, Wd) of the frames of a dataset: the sensor for Gen1, half of it for Gen4."""
    dataset_type = _dataset_type(dataset_type)
    h, w = SENSOR_HW[dataset_type]
    return (h // 2, w // 2) if dataset_type == DatasetType.GEN4 else (h, w)


def parse_sensor(sensor) -> Tuple[int, int]:
    """'WxH' (as a camera's data sheet spells it) or a pair (height, width) -> (height, width), integers in [1, 16384]."""
    if isinstance(sensor, str):
        parts = sensor.lower().split('x')
        if len(parts) != 2 or not all(q.strip().isdigit() for q in parts):
            raise ValueError(f'sensor={sensor!r}: WxH expected, as in 640x480')
        hw = (int(parts[1]), int(parts[0]))
    else:
        try:
            h, w = sensor
        except (TypeError, ValueError):
            raise ValueError(f'sensor_hw={sensor!r}: WxH or a pair (height, width) expected') from None
        if any(isinstance(v, (bool, float)) or not isinstance(v, (int, np.integer)) for v in (h, w)):
            raise ValueError(f'sensor_hw={sensor!r}: integers expected')
        hw = (int(h), int(w))
    if not all(1 <= v <= ef.FIT_MAX_SIDE for v in hw):
        raise ValueError(f'sensor_hw={sensor!r}: height and width in [1, {ef.FIT_MAX_SIDE}] expected')
    return hw


def ev_repr_name(duration_us: int, bins: int) -> str:
    assert duration_us % 1000 == 0, 'the directory name states the window in whole milliseconds'
    return f'stacked_histogram_dt={duration_us // 1000}_nbins={bins}'


def label_frame(t_label, duration_us: int) -> np.ndarray:
    """Frame of a box timestamp: max(ceil(t / D) - 1, 0)."""
    t = np.asarray(t_label, dtype=np.int64)
    return np.maximum(-(-t // int(duration_us)) - 1, 0)


def convert_labels(boxes: np.ndarray, n_frames: int, duration_us: int, keep_classes: Optional[Sequence[int]] = None
                   ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Prophesee boxes (structured array) -> (labels [LABEL_DTYPE], objframe_idx_2_label_idx, objframe_idx_2_repr_idx) by the window rule.
    Fields are copied by name, ``objectness`` = 1, ``track_id`` is dropped; no filtering but ``keep_classes`` (the evaluator applies the
    Prophesee size and time filters itself)."""
    names = {_FIELD_ALIASES.get(n, n): n for n in boxes.dtype.names}
    missing = [n for n in LABEL_DTYPE.names if n != 'objectness' and n not in names]
    if missing:
        raise ValueError(f'box file lacks the fields {missing} (has {boxes.dtype.names})')
    lab = np.zeros((len(boxes),), dtype=LABEL_DTYPE)
    for n in LABEL_DTYPE.names:
        if n != 'objectness':
            lab[n] = boxes[names[n]]
    lab['objectness'] = 1.0
    if keep_classes is not None:
        lab = lab[np.isin(lab['class_id'], np.asarray(list(keep_classes), dtype=np.int64))]
    lab = lab[np.argsort(lab['t'], kind='stable')]
    frame = label_frame(lab['t'], duration_us)
    lab, frame = lab[frame < n_frames], frame[frame < n_frames]
    # per frame only the boxes of its latest timestamp: after the stable sort these are the rows that equal the frame's last row in t
    if len(lab):
        last_row_of_frame = np.searchsorted(frame, frame, side='right') - 1
        keep = lab['t'] == lab['t'][last_row_of_frame]
        lab, frame = lab[keep], frame[keep]
    repr_idx, starts = np.unique(frame, return_index=True)
    return lab, starts.astype(np.int64), repr_idx.astype(np.int64)


def voxelize_recording(records: np.ndarray, offsets: np.ndarray, frames_out: Optional[np.ndarray], bins: int, height: int, width: int,
                       ds2: bool, device=None, frames_per_copy: int = FRAMES_PER_COPY, packed_writer=None) -> int:
    """Memory-mapped records [n, 2] u32 + window offsets -> ``frames_out`` [N, 2*bins, Ho, Wo] uint8 (e.g. an ``open_memmap``),
    ``frames_per_copy`` windows at a time through one pinned record buffer and one pinned frame buffer.  With ``packed_writer`` (a
    ``packed.PackedWriter``; ``frames_out`` None) every chunk is encoded on the device and only its packed bytes are copied back and
    appended.  -> number of dropped events."""
    import torch
    from leod_amd import ops
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    n_frames = len(offsets) - 1
    assert (frames_out is None) != (packed_writer is None), 'either a dense destination or a packed writer'
    spans = [(k, min(k + frames_per_copy, n_frames)) for k in range(0, n_frames, frames_per_copy)]
    most = max([int(offsets[b] - offsets[a]) for a, b in spans] + [1])
    rec_pin = torch.empty((most, 8), dtype=torch.uint8).pin_memory()
    rec_np = rec_pin.numpy().view('<u4')
    if packed_writer is None:
        assert frames_out.shape[0] == n_frames and frames_out.dtype == np.uint8
        out_pin = torch.empty((min(frames_per_copy, n_frames),) + tuple(frames_out.shape[1:]), dtype=torch.uint8).pin_memory()
        out_np = out_pin.numpy()
    dropped = torch.zeros((1,), dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        for a, b in spans:
            lo, hi = int(offsets[a]), int(offsets[b])
            rec_np[:hi - lo] = records[lo:hi]
            rec_dev = rec_pin[:hi - lo].to(device, non_blocking=True)
            out, d = ops.voxelize_dat_windows(rec_dev, offsets[a:b + 1] - lo, bins, height, width, ds2=ds2)
            dropped += d
            if packed_writer is not None:
                blob, blob_off = ops.pack_frames(out)           # one read-back of b - a sizes inside, then the packed bytes
                packed_writer.append(blob.cpu().numpy(), blob_off.numpy())
                continue
            out_pin[:b - a].copy_(out, non_blocking=True)
            torch.cuda.current_stream().synchronize()           # the pinned buffers are reused by the next span
            frames_out[a:b] = out_np[:b - a]
    return int(dropped.item())


def _npy_header(shape) -> bytes:
    """The header ``np.lib.format.open_memmap`` writes for a uint8 array of this shape (format 1.0)."""
    import io
    buf = io.BytesIO()
    np.lib.format.write_array_header_1_0(buf, dict(descr=np.lib.format.dtype_to_descr(np.dtype(np.uint8)), fortran_order=False,
                                                   shape=tuple(int(v) for v in shape)))
    return buf.getvalue()


class _NpyStream:
    """A dense frame file whose number of frames is known only at the end, byte for byte the file ``open_memmap`` would have made: the
    frames are appended to ``fn + '.tmp'`` behind room for the header (``reserve`` bytes; None: the header of an empty file -- NumPy pads
    it to 64 bytes with room for the first axis to grow, so its length rarely depends on N); ``close`` writes the header of the final
    shape in front and renames the file.  Where that header does not have the reserved length the frames are moved once, through
    ``fn + '.body'``."""

    def __init__(self, fn: str, frame_shape, reserve: Optional[int] = None):
        self.fn, self.frame_shape, self.n = fn, tuple(int(s) for s in frame_shape), 0
        self.reserve = len(_npy_header((0,) + self.frame_shape)) if reserve is None else int(reserve)
        self._f = open(fn + '.tmp', 'wb')
        self._f.write(b'\0' * self.reserve)

    def append(self, frames: np.ndarray) -> None:
        assert frames.dtype == np.uint8 and tuple(frames.shape[1:]) == self.frame_shape
        self._f.write(memoryview(np.ascontiguousarray(frames)).cast('B'))
        self.n += len(frames)

    def close(self) -> None:
        header = _npy_header((self.n,) + self.frame_shape)
        if len(header) == self.reserve:
            self._f.seek(0)
            self._f.write(header)
            self._f.close()
        else:
            import shutil
            self._f.close()
            os.replace(self.fn + '.tmp', self.fn + '.body')
            with open(self.fn + '.body', 'rb') as src, open(self.fn + '.tmp', 'wb') as dst:
                dst.write(header)
                src.seek(self.reserve)
                shutil.copyfileobj(src, dst, 1 << 24)
            os.remove(self.fn + '.body')
        os.replace(self.fn + '.tmp', self.fn)

    def abort(self) -> None:
        self._f.close()
        for fn in (self.fn + '.body', self.fn + '.tmp'):
            if os.path.exists(fn):
                os.remove(fn)


class _RecordChunks:
    """The chunk reader: iterating yields the device records (uint8 [n, 8]) of ``raw_chunk_bytes`` of ``payload`` at a time -- the payload
    of a .raw file, decoded with the carried state (``ops.decode_evt``; a time outside [0, 2^32) us raises ``ValueError``), or with
    ``encoding`` 'dat' the bytes of .dat records, cut at whole records.  ``counters()``: the decoder's so far (zeros for 'dat').  ONE pinned
    buffer: it is written again only after the event recorded right behind its non-blocking copy to the device has passed."""

    def __init__(self, payload: np.ndarray, encoding: str, raw_chunk_bytes: int, device, what: str):
        step = int(raw_chunk_bytes)
        if step < 4 or step % 4:
            raise ValueError(f'raw_chunk_bytes={step}: a positive multiple of 4 expected')
        self.step = max(step // 8, 1) * 8 if encoding == 'dat' else step         # whole records
        self.payload, self.encoding, self.device, self.what, self.state = payload, encoding, device, what, None

    def __iter__(self):
        import torch
        from leod_amd import ops
        payload, step, copied = self.payload, self.step, None
        pin = torch.empty((min(step, max(len(payload), 4)),), dtype=torch.uint8).pin_memory()
        for pos in range(0, len(payload), step):
            n = min(step, len(payload) - pos)
            if copied is not None:
                copied.synchronize()                             # the copy of the chunk before has left the pinned buffer
            pin.numpy()[:n] = payload[pos:pos + n]               # the host fills it while the device works on the chunk before
            rec = pin[:n].to(self.device, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record()
            if self.encoding == 'dat':
                rec = rec.view(-1, 8)
            else:
                rec, self.state = ops.decode_evt(rec, self.encoding, self.state)
                if int(self.state[12].item()):
                    raise ValueError(f'{self.what}: an event time lies outside [0, 2^32) microseconds after the shift by the first '
                                     'TIME_HIGH; it does not fit a .dat record')
            yield rec

    def counters(self) -> Dict:
        from leod_amd import ops
        zeros = dict(events=0, early_events=0, ignored_words=0, unknown_words=0, overflow=0, wraps=0)
        return zeros if self.state is None else ops.evt_state_counters(self.state)


def _order_error(what: str, t_before: int, t_at: int) -> ValueError:
    return ValueError(f'{what}: timestamps decrease ({t_before} -> {t_at}); a recording must be sorted in time')


def _report_fragment(frames: int, dropped: int, decoder: Dict, first: Optional[str] = None, tau_on: bool = False,
                     activity: Optional[Dict] = None, pixel: Optional[Dict] = None, fit: Optional[Dict] = None) -> Dict:
    """What ``voxelize_raw_recording`` returns, from plain numbers: the decoder's counters, the voxeliser's ``dropped``, ``first`` the stage
    that saw every event and applied the bounds and the mask (None: no filter; 'activity': ``ops.filter_events``; 'pixel': that op, followed
    by ``ops.filter_events`` iff ``tau_on``), ``activity`` / ``pixel`` the counters of the ops' states (None: no state yet, zeros).
    ``kept_events`` is what reached the voxeliser, ``events`` the first stage's ``seen``, its ``outside`` joins ``dropped_events``.
    ``fit`` (None: no sensor fit): the counters of the state of ``ops.fit_events``, the last stage -- the first one, too, where ``first`` is
    None; ``kept_events`` is then its ``kept``, and ``cropped_events``, ``skipped_events`` and ``merged_events`` are added."""
    rep = dict(frames=frames, dropped_events=dropped, **decoder)
    if fit is not None:
        if first is None:
            rep.update(events=fit['seen'], dropped_events=dropped + fit['outside'])
        else:
            rep.update(_report_fragment(frames, dropped, decoder, first, tau_on, activity, pixel))
        rep.update(kept_events=fit['kept'], cropped_events=fit['cropped'], skipped_events=fit['skipped'], merged_events=fit['merged'])
        return rep
    if first is None:
        return rep
    fc = activity or dict(seen=0, kept=0, outside=0, masked=0, unsupported=0)
    pc = pixel or dict(seen=0, kept=0, outside=0, masked=0, flicker=0, burst=0)
    head = pc if first == 'pixel' else fc
    rep.update(events=head['seen'], dropped_events=dropped + head['outside'], masked_events=head['masked'],
               unsupported_events=fc['unsupported'], kept_events=pc['kept'] if first == 'pixel' and not tau_on else fc['kept'])
    if first == 'pixel':
        rep.update(flicker_events=pc['flicker'], burst_events=pc['burst'])
    return rep


class _FilterChain:
    """The filter chain of one recording, built once from ``event_filter``: None, or dict(tau_us: int or None, mask: uint8 [H, W] or None,
    pixel: None or the dict of ``check_pixel_filter_options``).  Calling it on a chunk's records returns those that reach the voxeliser
    and carries the states.  With ``pixel``: ``ops.pixel_filter_events`` first, which applies the bounds and the mask and needs whole
    per-pixel sequences; ``ops.filter_events`` follows only where ``tau_us`` is set, only on a non-empty result, and without the mask.
    Else ``ops.filter_events`` with the mask.  Times that decrease -- against the chunk before, too -- raise one ``ValueError``.
    ``fit`` (None, or the resolved dict of ``event_filter.fit_spec`` whose source is ``sensor_hw``): the sensor fit, ``ops.fit_events``,
    is the last stage; the stages before it work at the source geometry, and it sees what they keep (where there is none it also checks
    the order)."""

    def __init__(self, event_filter: Optional[Dict], sensor_hw, device, what: str, fit: Optional[Dict] = None):
        import torch
        self.hw, self.what, self.pstate, self.fstate = tuple(sensor_hw), what, None, None
        self.fit, self.tstate = None, None
        if fit is not None:
            assert tuple(fit['src_hw']) == self.hw, 'the fit starts from the geometry the filters work at'
            self.fit = dict(src_hw=tuple(fit['src_hw']), dst_hw=tuple(fit['frame_hw']), orient=fit['orient'], mirror=fit['mirror'],
                            scale=fit['scale'], offset=tuple(fit['offset']), reduce=fit['reduce'], threshold=fit['threshold'])
        self.tau_us, mask, self.pixel = (event_filter[k] for k in ('tau_us', 'mask', 'pixel')) if event_filter else (None, None, None)
        self.first = None if event_filter is None else 'activity' if self.pixel is None else 'pixel'
        self.mask = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(device)
        self.t_seen = torch.full((1,), -1, dtype=torch.int64, device=device) if event_filter is None else None

    def __call__(self, rec):
        import torch
        from leod_amd import ops
        if self.fit is not None:
            try:
                if self.first is not None:
                    rec = self._filters(rec)
                if self.first is None or rec.shape[0]:
                    rec, self.tstate = ops.fit_events(rec, state=self.tstate, **self.fit)
            except ops.EventOrderError as e:
                raise _order_error(self.what, e.t_before, e.t_at) from None
            return rec
        if self.first is None:                                   # no stage: the order check alone, on the device
            t = rec.view(torch.int32)[:, 0].to(torch.int64) & 0xffffffff
            bad = torch.nonzero(torch.cat([t[:1] < self.t_seen, t[1:] < t[:-1]]))
            if bad.numel():                                      # position 0: earlier than the last event of the chunk before
                t, i = torch.cat([self.t_seen, t]), int(bad[0])
                raise _order_error(self.what, int(t[i]), int(t[i + 1]))
            self.t_seen = t[-1:].clone()
            return rec
        try:
            return self._filters(rec)
        except ops.EventOrderError as e:
            raise _order_error(self.what, e.t_before, e.t_at) from None

    def _filters(self, rec):
        from leod_amd import ops
        if self.first == 'pixel':
            rec, self.pstate = ops.pixel_filter_events(rec, *self.hw, state=self.pstate, pixel_mask=self.mask, **self.pixel)
            if self.tau_us is not None and rec.shape[0]:
                rec, self.fstate = ops.filter_events(rec, *self.hw, self.tau_us, state=self.fstate)
        else:
            rec, self.fstate = ops.filter_events(rec, *self.hw, self.tau_us, state=self.fstate, pixel_mask=self.mask)
        return rec

    def report(self, frames: int, dropped: int, decoder: Dict) -> Dict:
        from leod_amd import ops
        fit = None
        if self.fit is not None:
            fit = ops.fit_counters(self.tstate) if self.tstate is not None else dict(seen=0, kept=0, outside=0, cropped=0, skipped=0, merged=0)
        return _report_fragment(frames, dropped, decoder, self.first, self.tau_us is not None,
                                ops.event_filter_counters(self.fstate) if self.fstate is not None else None,
                                ops.pixel_filter_counters(self.pstate) if self.pstate is not None else None, fit)


def voxelize_raw_recording(payload: np.ndarray, encoding: str, sink, packed: bool, duration_us: int, bins: int, height: int, width: int,
                           ds2: bool, what: str, device=None, raw_chunk_bytes: int = RAW_CHUNK_BYTES,
                           frames_per_copy: int = FRAMES_PER_COPY, event_filter: Optional[Dict] = None, fit: Optional[Dict] = None,
                           events_writer=None) -> Dict:
    """Memory-mapped payload bytes of a .raw file -> frames appended to ``sink`` (``_NpyStream`` or, with ``packed``, a ``PackedWriter``).
    ``_RecordChunks`` brings the records of ``raw_chunk_bytes`` of payload at a time; ``_FilterChain`` (from ``event_filter``) checks the
    order of their times and hands on those that reach the voxeliser; every window that is complete -- a later event has been seen -- is
    voxelised by ``ops.voxelize_dat_windows``, the records of the last, incomplete one are carried into the next chunk.  A window that
    loses all its events is a zero frame.  With ``event_filter`` or ``fit`` ``encoding`` may be 'dat' (.dat record bytes).  With ``fit``
    (the resolved dict of ``event_filter.fit_spec``) ``height``, ``width`` are the SOURCE geometry, which the filters work at; the fit
    is the chain's last stage and the voxeliser runs at the fit's frame geometry with ``ds2`` off.  ``events_writer`` (an
    ``event_writer.EventFileWriter``; then an unfiltered 'dat' comes here, too): the records the chain hands on are appended to it, chunk
    by chunk, before the carry joins them.  -> ``_report_fragment``."""
    import torch
    from leod_amd import ops
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    chunks = _RecordChunks(payload, encoding, raw_chunk_bytes, device, what)
    assert encoding != 'dat' or event_filter is not None or fit is not None or events_writer is not None, \
        'unfiltered .dat records take voxelize_recording'
    chain = _FilterChain(event_filter, (height, width), device, what, fit=fit)
    if fit is not None:
        (height, width), ds2 = fit['frame_hw'], False
    D = int(duration_us)
    dropped = torch.zeros((1,), dtype=torch.int64, device=device)
    carry, done, t_last = torch.empty((0, 8), dtype=torch.uint8, device=device), 0, 0

    def emit(rec, off):                                          # windows `done` .. of rec, offsets [k + 1] on the device
        nonlocal done, dropped
        n_win = off.numel() - 1
        for a in range(0, n_win, frames_per_copy):
            b = min(a + frames_per_copy, n_win)
            lo, hi = int(off[a]), int(off[b])
            out, d = ops.voxelize_dat_windows(rec[lo:hi].reshape(-1), off[a:b + 1] - lo, bins, height, width, ds2=ds2)
            dropped += d
            if packed:
                blob, blob_off = ops.pack_frames(out)
                sink.append(blob.cpu().numpy(), blob_off.numpy())
            else:
                sink.append(out.cpu().numpy())
        done += n_win

    with torch.cuda.device(device):
        for rec in chunks:
            if rec.shape[0] == 0:
                continue
            t_last = int(rec.view(torch.int32)[-1, 0]) & 0xffffffff      # of the events SEEN, kept or not: it sets the number of frames
            rec = chain(rec)
            if events_writer is not None:
                events_writer.append(rec)
            rec = torch.cat([carry, rec]) if carry.shape[0] else rec
            k_last = max(-(-t_last // D) - 1, 0)                  # the window of the last event: everything before it is complete
            if k_last > done:
                t = rec.view(torch.int32)[:, 0].to(torch.int64) & 0xffffffff
                edges = torch.arange(done + 1, k_last + 1, dtype=torch.int64, device=device) * D
                off = torch.cat([torch.zeros((1,), dtype=torch.int64, device=device), torch.searchsorted(t, edges, right=True)])
                emit(rec, off)
                carry = rec[int(off[-1]):].clone()
            else:
                carry = rec
        n_frames = dat_events.num_windows(t_last, D)
        assert n_frames == done + 1
        emit(carry, torch.tensor([0, carry.shape[0]], dtype=torch.int64, device=device))
        return chain.report(n_frames, int(dropped.item()), chunks.counters())


def count_pixel_events(payload: np.ndarray, encoding: str, height: int, width: int, what: str, device=None,
                       raw_chunk_bytes: int = RAW_CHUNK_BYTES) -> Dict:
    """The first pass of ``--hot-rate``: events per pixel of a whole recording, counted on the device (``ops.event_pixel_counts``) from the
    chunks of ``_RecordChunks`` (the payload of a .raw file, or the bytes of .dat records with ``encoding`` 'dat').
    -> dict(counts int64 [H, W], outside, events, t_first, t_last): the times of the first and the last event (0 without any)."""
    import torch
    from leod_amd import ops
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    chunks = _RecordChunks(payload, encoding, raw_chunk_bytes, device, what)
    counts = torch.zeros((height, width), dtype=torch.int64, device=device)
    outside = torch.zeros((1,), dtype=torch.int64, device=device)
    first, last, events = None, None, 0
    with torch.cuda.device(device):
        for rec in chunks:
            if rec.shape[0] == 0:
                continue
            events += rec.shape[0]
            if first is None:
                first = rec[0].clone()
            last = rec[-1].clone()
            _, o = ops.event_pixel_counts(rec, height, width, counts)
            outside += o
        t_first = int(first.view(torch.int32)[0]) & 0xffffffff if first is not None else 0
        t_last = int(last.view(torch.int32)[0]) & 0xffffffff if last is not None else 0
        return dict(counts=counts.cpu().numpy(), outside=int(outside.item()), events=events, t_first=t_first, t_last=t_last)


def check_filter_options(dataset_type, denoise_us=None, pixel_mask=None, hot_rate_hz=None) -> Optional[Dict]:
    """The three filter options of a call, checked on the host before anything is opened -> None when all are off, else
    dict(tau_us, mask, hot_rate_hz): ``pixel_mask`` (a ``.npy`` file name or an array) read and checked against the sensor of the
    dataset."""
    return _filter_options(dataset_type, denoise_us, pixel_mask, hot_rate_hz)


def _filter_options(dataset_type, denoise_us=None, pixel_mask=None, hot_rate_hz=None, fito: Optional[Dict] = None) -> Optional[Dict]:
    """``check_filter_options`` for a call whose sensor and fit options are ``fito`` (``check_fit_options``; None: none): the mask is
    checked against its ``sensor_hw`` where that is given; with a fit and no ``sensor_hw`` the recording's header may state the size, so
    any [H, W] is taken here and ``_ingest_streaming`` compares it with the source size once the file is open."""
    if denoise_us is None and pixel_mask is None and hot_rate_hz is None:
        return None
    if denoise_us is not None:
        if isinstance(denoise_us, (bool, float)) or int(denoise_us) != denoise_us or not 0 <= int(denoise_us) < 2 ** 31:
            raise ValueError(f'denoise_us={denoise_us!r}: an integer number of microseconds in [0, 2^31) expected')
        denoise_us = int(denoise_us)
    if hot_rate_hz is not None:
        if isinstance(hot_rate_hz, (bool, float)) or int(hot_rate_hz) != hot_rate_hz or int(hot_rate_hz) < 0:
            raise ValueError(f'hot_rate_hz={hot_rate_hz!r}: a non-negative integer rate in events per second expected')
        hot_rate_hz = int(hot_rate_hz)
    sensor = SENSOR_HW[_dataset_type(dataset_type)]
    if fito is not None and fito['sensor_hw'] is not None:
        sensor = fito['sensor_hw']
    elif fito is not None and fito['fit'] is not None and pixel_mask is not None:
        shape = np.shape(np.load(pixel_mask, allow_pickle=False) if isinstance(pixel_mask, (str, os.PathLike)) and
                         str(pixel_mask).lower().endswith('.npy') else pixel_mask)
        sensor = shape if len(shape) == 2 else sensor
    mask = None
    if pixel_mask is not None:
        mask = ef.read_pixel_mask(pixel_mask, sensor) if isinstance(pixel_mask, (str, os.PathLike)) else ef.check_pixel_mask(pixel_mask, sensor)
    return dict(tau_us=denoise_us, mask=mask, hot_rate_hz=hot_rate_hz)


def check_fit_options(dataset_type, sensor_hw=None, fit=None, fit_offset=None, fit_orient=None, fit_mirror=False, fit_reduce=None,
                      fit_threshold=None) -> Optional[Dict]:
    """The sensor and fit options of a call, checked on the host before anything is opened -> None when all are off, else
    dict(sensor_hw: (height, width) or None, fit: None or dict(scale, offset, orient, mirror, reduce, threshold), the keyword arguments of
    ``event_filter.fit_spec``).  ``sensor_hw``: 'WxH' or (height, width).  ``fit``: 'auto' or the integer scale K -- the fit is on iff it
    is given -- or such a dict (then the other ``fit_*`` stay unset).  ``fit_offset`` 'center' | 'X,Y' | (x, y), ``fit_orient`` 0 | 90 |
    180 | 270, ``fit_mirror``, ``fit_reduce`` 'pick' | 'sum' | 'fire' and ``fit_threshold`` (only with 'fire') need ``fit``.  Without a fit
    a sensor other than the dataset's is refused.  The options are resolved once against ``sensor_hw`` (None: the dataset's sensor) to
    find every misuse here; the recording's own size resolves them again."""
    if fit_mirror not in (False, True):
        raise ValueError(f'fit_mirror={fit_mirror!r}: True or False expected')
    others = dict(offset=fit_offset, orient=fit_orient, reduce=fit_reduce, threshold=fit_threshold)
    given = [f'fit_{k}' for k, v in others.items() if v is not None] + (['fit_mirror'] if fit_mirror else [])
    if sensor_hw is None and fit is None and not given:
        return None
    dataset_type = _dataset_type(dataset_type)
    sensor = None if sensor_hw is None else parse_sensor(sensor_hw)
    if fit is None:
        if given:
            raise ValueError(f'{", ".join(given)}: these need fit (auto or an integer scale)')
        if sensor != tuple(SENSOR_HW[dataset_type]):
            raise ValueError(f'sensor_hw={sensor_hw!r}: a {dataset_type.name} recording has (height, width) = {tuple(SENSOR_HW[dataset_type])}; '
                             'another sensor needs a fit (fit=auto or an integer scale)')
        return dict(sensor_hw=sensor, fit=None)
    if isinstance(fit, dict):
        if given:
            raise ValueError(f'{", ".join(given)}: with fit given as a dict they belong in it')
        unknown = sorted(set(fit) - set(FIT_KEYS))
        if unknown:
            raise ValueError(f'fit: unknown keys {unknown}; {FIT_KEYS} expected')
        kw = dict(fit)
    else:
        kw = dict(scale=fit, mirror=bool(fit_mirror), **{k: v for k, v in others.items() if v is not None})
    if kw.get('threshold') is not None and kw.get('reduce', 'pick') != 'fire':
        raise ValueError("fit_threshold needs fit_reduce 'fire'")
    ef.fit_spec(SENSOR_HW[dataset_type] if sensor is None else sensor, frame_hw(dataset_type), **kw)
    return dict(sensor_hw=sensor, fit=kw)


def check_pixel_filter_options(trail_us=None, stc_us=None, stc_cut_trail=False, anti_flicker=None, flicker_lock=None) -> Optional[Dict]:
    """The per-pixel filter options of a call, checked on the host before anything is opened -> None when all are off, else the keyword
    arguments of ``ops.pixel_filter_events``: dict(burst_us, burst_keep, flicker).  ``trail_us`` keeps the first event of a burst,
    ``stc_us`` a burst from its second event on (``stc_cut_trail``: the second alone); ``anti_flicker``: 'FMIN:FMAX' or (fmin, fmax) in
    Hz, ``flicker_lock`` (None: 3) the in-band periods in a row after which a pixel is removed."""
    if trail_us is not None and stc_us is not None:
        raise ValueError('trail_us and stc_us: one burst rule at a time (a trail filter keeps the first event of a burst, STC drops it)')
    if stc_cut_trail not in (False, True):
        raise ValueError(f'stc_cut_trail={stc_cut_trail!r}: True or False expected')
    if stc_cut_trail and stc_us is None:
        raise ValueError('stc_cut_trail needs stc_us')
    if flicker_lock is not None and anti_flicker is None:
        raise ValueError('flicker_lock needs anti_flicker')
    burst_us, burst_keep = None, 'first'
    for name, v in (('trail_us', trail_us), ('stc_us', stc_us)):
        if v is None:
            continue
        if isinstance(v, (bool, float)) or int(v) != v or not 0 <= int(v) < 2 ** 31:
            raise ValueError(f'{name}={v!r}: an integer number of microseconds in [0, 2^31) expected')
        burst_us = int(v)
        burst_keep = 'first' if name == 'trail_us' else ('second' if stc_cut_trail else 'from_second')
    flicker = None
    if anti_flicker is not None:
        lock = ef.DEFAULT_FLICKER_LOCK if flicker_lock is None else flicker_lock
        if isinstance(lock, (bool, float)) or int(lock) != lock or not 1 <= int(lock) <= 255:
            raise ValueError(f'flicker_lock={flicker_lock!r}: an integer in [1, 255] expected')
        flicker = ef.flicker_band(anti_flicker) + (int(lock),)
    if burst_us is None and flicker is None:
        return None
    return dict(burst_us=burst_us, burst_keep=burst_keep, flicker=flicker)


class _TreeWriter:
    """What every route writes around its frames.  Creating it checks the header's size against the dataset's sensor (the field named as
    the container spells it) and resolves ``keep_classes``; nothing is written yet.  ``sink`` opens the frame file of the streaming
    route, ``labels`` converts the boxes, ``finish`` writes the label files (and ``hot_pixels.npy``) and returns the base report.
    ``fito`` (``check_fit_options``; None: no sensor or fit option): the source size is its ``sensor_hw``, else the header's, else the
    dataset's; a header that contradicts ``sensor_hw`` is refused; with a fit ``height``, ``width`` are that source size (what the
    filters work at), ``fit`` is the resolved ``event_filter.fit_spec`` and ``labels`` maps the boxes through it; without one the source
    must be the dataset's sensor, as ever.  The frame file and its shape are the dataset's either way."""

    def __init__(self, ev_fn, hdr, bbox_fn, out_dir, dataset_type, duration_us, bins, keep_classes, write, fito=None):
        self.height, self.width = SENSOR_HW[dataset_type]
        names = ('height', 'width') if ev_fn.lower().endswith('.raw') else ('Height', 'Width')
        sensor, fit = (fito['sensor_hw'], fito['fit']) if fito is not None else (None, None)
        self.fit, self.boxes_outside, self.boxes_in = None, 0, None
        if fit is not None:                                      # without one ``sensor`` is the dataset's: the check below is the one there was
            for name, got, want in zip(names, (hdr.height, hdr.width), sensor or ()):
                if got is not None and got != want:
                    raise ValueError(f'{ev_fn}: header says {name} {got}, the sensor given has {want}')
            src = sensor if sensor is not None else tuple(want if got is None else int(got)
                                                          for got, want in zip((hdr.height, hdr.width), (self.height, self.width)))
            self.fit = ef.fit_spec(src, frame_hw(dataset_type), **fit)
            self.height, self.width = src
        for name, got, want in zip(names, (hdr.height, hdr.width), (self.height, self.width)):
            if got is not None and got != want:
                raise ValueError(f'{ev_fn}: header says {name} {got}, a {dataset_type.name} recording has {want}')
        self.keep_classes = DEFAULT_KEEP_CLASSES[dataset_type] if keep_classes is None else keep_classes
        self.bbox_fn, self.out_dir, self.duration_us = bbox_fn, out_dir, duration_us
        self.packed, self.ds2 = write == 'packed', dataset_type == DatasetType.GEN4
        self.ev_dir = os.path.join(out_dir, 'event_representations_v2', ev_repr_name(duration_us, bins))
        self.frame_fn = os.path.join(self.ev_dir, 'event_representations' + ('_ds2_nearest' if self.ds2 else '') +
                                     ('.evp' if self.packed else '.npy'))
        self.frame_shape = (2 * bins,) + (tuple(self.fit['frame_hw']) if self.fit is not None else
                                          (self.height // 2, self.width // 2) if self.ds2 else (self.height, self.width))

    def makedirs(self) -> None:
        os.makedirs(self.ev_dir, exist_ok=True)
        os.makedirs(os.path.join(self.out_dir, 'labels_v2'), exist_ok=True)

    @contextlib.contextmanager
    def sink(self):                                              # the frame file of a route that appends: removed if anything raises
        self.makedirs()
        if self.packed:
            from leod_amd.data.utils.packed import PackedWriter
            sink = PackedWriter(self.frame_fn, *self.frame_shape)     # writes frame_fn + '.tmp', renamed on close
        else:
            sink = _NpyStream(self.frame_fn, self.frame_shape)
        try:
            yield sink
        except BaseException:
            sink.abort()
            raise
        sink.close()

    def labels(self, n_frames: int):
        boxes = np.load(self.bbox_fn) if self.bbox_fn is not None else np.zeros((0,), dtype=LABEL_DTYPE)
        if self.fit is not None:
            boxes, self.boxes_outside = ef.fit_boxes(boxes, self.fit)
        self.boxes_in = boxes if self.bbox_fn is not None else None      # what --write-events writes beside the event file
        return convert_labels(boxes, n_frames, self.duration_us, self.keep_classes)

    def finish(self, labels, n_frames: int, events: int, dropped: int, hot_mask=None) -> Dict:
        lab, label_idx, repr_idx = labels
        if hot_mask is not None:
            np.save(os.path.join(self.ev_dir, ef.MASK_FILE), hot_mask)       # the mask that was applied: --pixel-mask with it repeats the run
        np.save(os.path.join(self.ev_dir, 'objframe_idx_2_repr_idx.npy'), repr_idx)
        np.savez(os.path.join(self.out_dir, 'labels_v2', 'labels.npz'), labels=lab, objframe_idx_2_label_idx=label_idx)
        return dict(recording=self.out_dir, frames=n_frames, events=events, dropped_events=dropped, labelled_frames=int(len(repr_idx)),
                    boxes=int(len(lab)))


def check_write_options(write_events=None, events_out=None, evt3_vectors=False) -> Optional[Dict]:
    """The options that write the kept event stream back, checked on the host before anything is opened -> None when off, else
    dict(fmt: 'dat' | 'evt2' | 'evt3', dir, vectors).  ``write_events`` needs ``events_out`` (a directory; it is made), ``events_out``
    and ``evt3_vectors`` need ``write_events``, ``evt3_vectors`` needs 'evt3'."""
    if evt3_vectors not in (False, True):
        raise ValueError(f'evt3_vectors={evt3_vectors!r}: True or False expected')
    if write_events is None:
        if events_out is not None or evt3_vectors:
            raise ValueError('events_out and evt3_vectors need write_events (dat, evt2 or evt3)')
        return None
    if write_events not in ew.FORMATS:
        raise ValueError(f'write_events={write_events!r}: one of {ew.FORMATS} expected')
    if events_out is None or not isinstance(events_out, (str, os.PathLike)) or not str(events_out):
        raise ValueError(f'write_events={write_events!r} needs events_out, the directory the event files are written to')
    if evt3_vectors and write_events != 'evt3':
        raise ValueError(f'evt3_vectors: only EVT3 has vector words, the format written is {write_events}')
    return dict(fmt=write_events, dir=os.fspath(events_out), vectors=bool(evt3_vectors))


def _check_events_dir(wev: Optional[Dict], src_dir: str, *dst_dirs: str) -> None:
    """``ValueError`` where the event files would land among the recordings they are made from, or in a directory of the dataset tree."""
    if wev is None:
        return
    real = os.path.realpath(wev['dir'])
    if real == os.path.realpath(src_dir or '.'):
        raise ValueError(f'events_out={wev["dir"]!r} is the source directory; the written files would join the recordings read')
    for d in dst_dirs:
        if real == os.path.realpath(d or '.'):
            raise ValueError(f'events_out={wev["dir"]!r} is the destination {d!r}; the event files get a directory of their own')


def _events_file(wev: Optional[Dict], ev_fn: str, out_dir: str, tree) -> Optional[str]:
    """The event file of the recording ``ev_fn`` under ``wev`` (None: none), after every refusal that needs the open recording: the
    directory, and the written geometry -- the fit's frame where a fit is on, else the source sensor's -- against the format."""
    if wev is None:
        return None
    _check_events_dir(wev, os.path.dirname(ev_fn), out_dir, os.path.dirname(os.path.abspath(out_dir)))
    ew.check_format(wev['fmt'], *_written_hw(tree), wev['vectors'])
    base = os.path.basename(ev_fn)
    stem = base[:-len('_td.dat')] if base.lower().endswith('_td.dat') else os.path.splitext(base)[0]
    return os.path.join(wev['dir'], stem + ew.SUFFIX[wev['fmt']])


def _written_hw(tree) -> Tuple[int, int]:
    return tuple(int(v) for v in tree.fit['frame_hw']) if tree.fit is not None else (tree.height, tree.width)


@contextlib.contextmanager
def _events_sink(wev: Optional[Dict], events_fn: Optional[str], tree):
    """The event file writer of a recording (None without ``wev``): closed when the body ends, aborted -- no ``.tmp`` left -- if it raises."""
    if wev is None:
        yield None
        return
    os.makedirs(wev['dir'], exist_ok=True)
    writer = ew.EventFileWriter(events_fn, wev['fmt'], *_written_hw(tree), vectors=wev['vectors'])
    try:
        yield writer
    except BaseException:
        writer.abort()
        raise
    writer.close()


def _ingest_streaming(ev_fn, bbox_fn, out_dir, dataset_type, duration_us, bins, keep_classes, write, raw_chunk_bytes, flt, pix,
                      fito=None, wev=None) -> Dict:
    """A ``.raw`` file, or with ``flt`` (``check_filter_options``), ``pix`` (``check_pixel_filter_options``), a fit in ``fito``
    (``check_fit_options``) or ``wev`` (``check_write_options``) either container."""
    is_raw = ev_fn.lower().endswith('.raw')
    if is_raw:
        from leod_amd.data.utils import raw_events
        hdr, payload = raw_events.open_words(ev_fn)
        encoding = hdr.encoding
    else:
        assert flt is not None or pix is not None or (fito is not None and fito['fit'] is not None) or wev is not None, \
            'an unfiltered .dat recording takes voxelize_recording'
        hdr, records = dat_events.open_records(ev_fn)
        payload, encoding = records.view(np.uint8).reshape(-1), 'dat'
    tree = _TreeWriter(ev_fn, hdr, bbox_fn, out_dir, dataset_type, duration_us, bins, keep_classes, write, fito)
    events_fn = _events_file(wev, ev_fn, out_dir, tree)          # refuses before anything is written
    filtered = flt is not None or pix is not None
    tau_us, mask, hot = (flt['tau_us'], flt['mask'], None) if flt is not None else (None, None, None)
    if mask is not None and tree.fit is not None:
        ef.check_pixel_mask(mask, (tree.height, tree.width))     # the source size may have come from the header only now
    if flt is not None and flt['hot_rate_hz'] is not None:
        seen = count_pixel_events(payload, encoding, tree.height, tree.width, ev_fn, raw_chunk_bytes=raw_chunk_bytes)
        hot = ef.hot_pixel_mask(seen['counts'], max(seen['t_last'] - seen['t_first'], 1), flt['hot_rate_hz'])
        mask = hot = hot if mask is None else (mask | hot)       # hot_pixels.npy is the mask that was applied
    event_filter = dict(tau_us=tau_us, mask=mask, pixel=pix) if filtered else None
    with tree.sink() as sink, _events_sink(wev, events_fn, tree) as writer:
        res = voxelize_raw_recording(payload, encoding, sink, tree.packed, duration_us, bins, tree.height, tree.width, tree.ds2, ev_fn,
                                     raw_chunk_bytes=raw_chunk_bytes, event_filter=event_filter, fit=tree.fit, events_writer=writer)
    if not is_raw and not filtered and tree.fit is None:         # here for the event file alone: no stage has counted the events
        res['events'] = int(hdr.n_events)
    rep = tree.finish(tree.labels(res['frames']), res['frames'], res['events'], res['dropped_events'], hot_mask=hot)
    if writer is not None:
        if tree.boxes_in is not None:
            np.save(events_fn[:-len(ew.SUFFIX[wev['fmt']])] + '_bbox.npy', tree.boxes_in)
        rep.update(events_file=events_fn, written_events=writer.events, written_bytes=os.path.getsize(events_fn))
        if wev['fmt'] != 'dat':
            rep.update(written_words=writer.words)
    if is_raw:
        rep.update(early_events=res['early_events'], ignored_words=res['ignored_words'], unknown_words=res['unknown_words'],
                   clock_wraps=res['wraps'])
    if filtered:
        rep.update(kept_events=res['kept_events'], masked_events=res['masked_events'], unsupported_events=res['unsupported_events'],
                   masked_pixels=int(np.count_nonzero(mask)) if mask is not None else 0)
    if pix is not None:
        rep.update(flicker_events=res['flicker_events'], burst_events=res['burst_events'])
    if tree.fit is not None:
        rep.update(fit=tree.fit, kept_events=res['kept_events'], cropped_events=res['cropped_events'], skipped_events=res['skipped_events'],
                   merged_events=res['merged_events'], boxes_outside=tree.boxes_outside)
    return rep


def ingest_recording(dat_fn: str, bbox_fn: Optional[str], out_dir: str, dataset_type, duration_us: int = 50_000, bins: int = 10,
                     keep_classes: Optional[Sequence[int]] = None, write: str = 'npy', raw_chunk_bytes: int = RAW_CHUNK_BYTES,
                     denoise_us: Optional[int] = None, pixel_mask=None, hot_rate_hz: Optional[int] = None,
                     trail_us: Optional[int] = None, stc_us: Optional[int] = None, stc_cut_trail: bool = False, anti_flicker=None,
                     flicker_lock: Optional[int] = None, sensor_hw=None, fit=None, write_events: Optional[str] = None, events_out=None,
                     evt3_vectors: bool = False) -> Dict:
    """One recording -> ``out_dir`` in the dataset layout: frames as the raw ``.npy`` twin (``event_representations.npy`` for Gen1,
    ``event_representations_ds2_nearest.npy`` at half resolution for Gen4) or, with ``write='packed'``, as the packed store of the same
    stem (``.evp``), ``objframe_idx_2_repr_idx.npy``, ``labels_v2/labels.npz``.
    ``keep_classes`` None: every class for Gen1, (0, 1, 2) for Gen4.  -> a small report.
    ``dat_fn`` may be a Metavision ``.raw`` file (EVT2 / EVT3): its payload is decoded on the device, ``raw_chunk_bytes`` at a time, and
    the report also counts ``early_events``, ``ignored_words``, ``unknown_words`` and ``clock_wraps``.  ``bbox_fn`` None: an unlabelled
    recording, the tree is written with zero labels.
    Noise filters (all off by default, and then nothing here differs): ``denoise_us`` keeps an event only if one of its 8 neighbours
    fired at most so many microseconds before it; ``pixel_mask`` (a ``.npy`` file or a uint8 / bool array [H, W] at sensor resolution)
    removes the events of its non-zero pixels; ``hot_rate_hz`` counts the recording's events per pixel in a first pass and masks the pixels
    above that rate (OR-ed with ``pixel_mask``; written beside the frames as ``hot_pixels.npy``).  The frames, the window edges and the
    labels stay those of the unfiltered recording; the report gains ``kept_events``, ``masked_events``, ``unsupported_events`` and
    ``masked_pixels``, and ``dropped_events`` is the filter's count of events outside the sensor.
    Per-pixel filters (``check_pixel_filter_options``; all off by default, and then nothing here differs): ``trail_us`` / ``stc_us`` /
    ``stc_cut_trail`` and ``anti_flicker`` / ``flicker_lock``.  They run first and apply the bounds and the mask, ``denoise_us`` then
    sees what they keep; the report also gains ``flicker_events`` and ``burst_events``, ``kept_events`` is what reaches the voxeliser.
    Sensor fit (``check_fit_options``; off by default, and then nothing here differs): ``fit`` ('auto', an integer scale, or the dict of
    keyword arguments of ``event_filter.fit_spec``) maps a recording of another sensor size or mounting onto the frames of the dataset
    (``ops.fit_events``, the rule: DESIGN.md section 1).  The source size is ``sensor_hw`` ('WxH' or (height, width)), else the size in
    the file's header, else the dataset's; a header that contradicts ``sensor_hw`` is a ``ValueError``, and so is, without ``fit``, any
    size but the dataset's.  The filters above, ``pixel_mask`` and ``hot_pixels.npy`` stay at the source geometry and the fit runs last;
    the boxes take the same map (``event_filter.fit_boxes``); the report gains ``fit`` (the resolved options), ``cropped_events``,
    ``skipped_events``, ``merged_events`` and ``boxes_outside``.
    Event file (``check_write_options``; off by default, and then nothing here differs): ``write_events`` 'dat' | 'evt2' | 'evt3' writes
    the events that reach the voxeliser -- after the filters and the fit -- to ``events_out/<name>_td.dat`` or ``events_out/<name>.raw``
    (``event_writer.EventFileWriter``; EVT words come from ``ops.encode_evt`` on the device, ``evt3_vectors``: with vector words), at the
    fit's frame geometry where a fit is on, else the source sensor's, and the boxes as they enter ``convert_labels`` to
    ``events_out/<name>_bbox.npy``: ``events_out`` is a source directory this function reads.  Both containers then take the streaming
    route; the tree is byte for byte the one written without the option.  ``events_out`` must not be the source directory, ``out_dir`` or
    its parent; a geometry beyond 2048 x 2048 does not fit EVT.  The report gains ``events_file``, ``written_events``, ``written_bytes``
    and, for EVT, ``written_words``."""
    if write not in ('npy', 'packed'):
        raise ValueError(f"write={write!r}: the raw 'npy' frame file or the 'packed' store is written (an HDF5 writer is not part of "
                         'this package)')
    dataset_type = _dataset_type(dataset_type)
    fito = check_fit_options(dataset_type, sensor_hw, fit)
    flt = _filter_options(dataset_type, denoise_us, pixel_mask, hot_rate_hz, fito)
    pix = check_pixel_filter_options(trail_us, stc_us, stc_cut_trail, anti_flicker, flicker_lock)
    wev = check_write_options(write_events, events_out, evt3_vectors)
    if flt is not None or pix is not None or (fito is not None and fito['fit'] is not None) or wev is not None or \
            dat_fn.lower().endswith('.raw'):
        return _ingest_streaming(dat_fn, bbox_fn, out_dir, dataset_type, duration_us, bins, keep_classes, write, raw_chunk_bytes, flt, pix,
                                 fito, wev)
    hdr, records = dat_events.open_records(dat_fn)
    tree = _TreeWriter(dat_fn, hdr, bbox_fn, out_dir, dataset_type, duration_us, bins, keep_classes, write)
    offsets = dat_events.scan_windows(records, duration_us, what=dat_fn)
    n_frames = len(offsets) - 1
    labels = tree.labels(n_frames)
    if tree.packed:
        with tree.sink() as writer:
            dropped = voxelize_recording(records, offsets, None, bins, tree.height, tree.width, tree.ds2, packed_writer=writer)
    else:
        tree.makedirs()
        mm = np.lib.format.open_memmap(tree.frame_fn + '.tmp', mode='w+', dtype=np.uint8, shape=(n_frames,) + tree.frame_shape)
        try:
            dropped = voxelize_recording(records, offsets, mm, bins, tree.height, tree.width, tree.ds2)
            mm.flush()
        finally:
            del mm
        os.replace(tree.frame_fn + '.tmp', tree.frame_fn)
    return tree.finish(labels, n_frames, int(hdr.n_events), dropped)


def ingest_split(src_dir: str, dst_dir: str, dataset_type, duration_us: int = 50_000, bins: int = 10,
                 keep_classes: Optional[Sequence[int]] = None, write: str = 'npy', verbose: bool = False, unlabelled: str = 'error',
                 raw_chunk_bytes: int = RAW_CHUNK_BYTES, denoise_us: Optional[int] = None, pixel_mask=None,
                 hot_rate_hz: Optional[int] = None, trail_us: Optional[int] = None, stc_us: Optional[int] = None,
                 stc_cut_trail: bool = False, anti_flicker=None, flicker_lock: Optional[int] = None, sensor_hw=None, fit=None,
                 write_events: Optional[str] = None, events_out=None, evt3_vectors: bool = False):
    """Every ``<name>_td.dat`` and every ``<name>.raw`` of ``src_dir`` with its ``<name>_bbox.npy`` -> ``dst_dir/<name>/``.  A recording
    without a box file raises ``FileNotFoundError`` (``unlabelled='error'``) or is written with zero labels (``'ok'``); the same name in
    both containers is a ``ValueError``.  ``denoise_us``, ``pixel_mask``, ``hot_rate_hz``: the noise filters of ``ingest_recording``, the same
    for every recording (a mask file is read once); ``trail_us``, ``stc_us``, ``stc_cut_trail``, ``anti_flicker``, ``flicker_lock``: its
    per-pixel filters; ``sensor_hw``, ``fit``: its sensor fit; ``write_events``, ``events_out``, ``evt3_vectors``: its event files, all in
    the one directory ``events_out``, which must be neither ``src_dir`` nor ``dst_dir``.  -> the reports, in file-name order."""
    if unlabelled not in ('error', 'ok'):
        raise ValueError(f"unlabelled={unlabelled!r}: 'error' or 'ok' expected")
    fito = check_fit_options(dataset_type, sensor_hw, fit)
    flt = _filter_options(dataset_type, denoise_us, pixel_mask, hot_rate_hz, fito)
    filter_kw = {} if flt is None else dict(denoise_us=flt['tau_us'], pixel_mask=flt['mask'], hot_rate_hz=flt['hot_rate_hz'])
    if check_pixel_filter_options(trail_us, stc_us, stc_cut_trail, anti_flicker, flicker_lock) is not None:
        filter_kw.update(trail_us=trail_us, stc_us=stc_us, stc_cut_trail=stc_cut_trail, anti_flicker=anti_flicker, flicker_lock=flicker_lock)
    if fito is not None:
        filter_kw.update(sensor_hw=fito['sensor_hw'], fit=fito['fit'])
    wev = check_write_options(write_events, events_out, evt3_vectors)
    if wev is not None:
        _check_events_dir(wev, src_dir, dst_dir)
        filter_kw.update(write_events=wev['fmt'], events_out=wev['dir'], evt3_vectors=wev['vectors'])
    found = {}
    for fn in sorted(glob.glob(os.path.join(src_dir, '*_td.dat')) + glob.glob(os.path.join(src_dir, '*.raw'))):
        base = os.path.basename(fn)
        stem = base[:-len('_td.dat')] if base.endswith('_td.dat') else base[:-len('.raw')]
        if stem in found:
            raise ValueError(f'{src_dir}: the recording {stem!r} is there twice, as {os.path.basename(found[stem])} and as {base}')
        found[stem] = fn
    reports = []
    for stem, ev_fn in found.items():                            # in file-name order, as the .dat files always were
        bbox_fn = os.path.join(src_dir, stem + '_bbox.npy')
        if not os.path.exists(bbox_fn):
            if unlabelled == 'error':
                raise FileNotFoundError(f'{ev_fn} has no box file {bbox_fn}')
            bbox_fn = None
        rep = ingest_recording(ev_fn, bbox_fn, os.path.join(dst_dir, stem), dataset_type, duration_us=duration_us, bins=bins,
                               keep_classes=keep_classes, write=write, raw_chunk_bytes=raw_chunk_bytes, **filter_kw)
        if verbose:
            print(rep, flush=True)
        reports.append(rep)
    return reports


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog='python -m leod_amd.data.ingest', description=__doc__.split('\n\n')[0])
    ap.add_argument('src', help="directory of *_td.dat / *.raw recordings + *_bbox.npy, or one that holds such directories named train / val / test")
    ap.add_argument('dst', help='dataset path to write (dst/<split>/<recording>/...)')
    ap.add_argument('--dataset', required=True, choices=['gen1', 'gen4'])
    ap.add_argument('--duration-us', type=int, default=50_000)
    ap.add_argument('--bins', type=int, default=10)
    ap.add_argument('--keep-classes', type=int, nargs='*', default=None)
    ap.add_argument('--write', choices=['npy', 'packed'], default='npy', help="frame file: the raw .npy twin or the packed .evp store")
    ap.add_argument('--unlabelled', choices=['error', 'ok'], default='error',
                    help="a recording without a box file: an error, or a tree with zero labels (for pseudo-labelling)")
    ap.add_argument('--denoise-us', type=int, default=None, metavar='N',
                    help='keep an event only if one of its 8 neighbour pixels fired at most N microseconds before it')
    ap.add_argument('--pixel-mask', default=None, metavar='FILE.npy',
                    help='uint8 / bool array [H, W] at sensor resolution; the events of its non-zero pixels are removed')
    ap.add_argument('--hot-rate', type=int, default=None, metavar='HZ',
                    help='first count the events per pixel of each recording and mask the pixels that fire faster than HZ events/s '
                         '(the mask is written beside the frames as hot_pixels.npy)')
    burst = ap.add_mutually_exclusive_group()
    burst.add_argument('--trail-us', type=int, default=None, metavar='N',
                       help='per pixel, keep only the first event of a burst of same-polarity events that follow each other within N microseconds')
    burst.add_argument('--stc-us', type=int, default=None, metavar='N',
                       help='per pixel, keep such a burst from its second event on: an event is confirmed by a second one')
    ap.add_argument('--stc-cut-trail', action='store_true', help='with --stc-us: keep the second event of a burst alone')
    ap.add_argument('--anti-flicker', default=None, metavar='FMIN:FMAX',
                    help='remove the events of a pixel whose rising edges repeat at a frequency between FMIN and FMAX Hz (integers)')
    ap.add_argument('--flicker-lock', type=int, default=None, metavar='N',
                    help='in-band periods in a row after which a pixel counts as flickering (default 3)')
    ap.add_argument('--sensor', default=None, metavar='WxH',
                    help="the camera's sensor size, e.g. 640x480, where the file's header does not state it; any size but the dataset's needs --fit")
    ap.add_argument('--fit', default=None, metavar='auto|K',
                    help='fit the recording onto the frames of the dataset: K x K sensor pixels per frame pixel (auto: the largest K at '
                         'which the scaled image still covers the frame)')
    ap.add_argument('--fit-offset', default=None, metavar='center|X,Y', help='with --fit: where the scaled image lies in the frame (default center)')
    ap.add_argument('--fit-orient', type=int, default=None, choices=[0, 90, 180, 270], help='with --fit: turn the image clockwise by so many degrees')
    ap.add_argument('--fit-mirror', action='store_true', help='with --fit: mirror the image left to right first')
    ap.add_argument('--fit-reduce', default=None, choices=list(ef.FIT_REDUCES),
                    help='with --fit: of the events of K x K pixels, pick those of the centre pixel (default), sum them all, or integrate '
                         'and fire per frame pixel')
    ap.add_argument('--fit-threshold', type=int, default=None, metavar='N', help='with --fit-reduce fire: the firing threshold (default K * K)')
    ap.add_argument('--write-events', default=None, choices=list(ew.FORMATS), metavar='FMT',
                    help='also write the events that reach the voxeliser, after the filters and the fit, as a .dat file (dat) or a '
                         'Metavision .raw file (evt2, evt3) per recording; needs --events-out')
    ap.add_argument('--events-out', default=None, metavar='DIR',
                    help='with --write-events: the directory of the event files and their box files (DIR/<split>/ where SRC holds splits); '
                         'neither SRC nor DST; it is itself a source directory this tool reads')
    ap.add_argument('--evt3-vectors', action='store_true', help='with --write-events evt3: write runs of events in one row as vector words')
    args = ap.parse_args(argv)
    pix_kw = dict(trail_us=args.trail_us, stc_us=args.stc_us, stc_cut_trail=args.stc_cut_trail, anti_flicker=args.anti_flicker,
                  flicker_lock=args.flicker_lock)
    fit_kw = {}
    try:
        fito = check_fit_options(args.dataset, args.sensor, args.fit, args.fit_offset, args.fit_orient, args.fit_mirror, args.fit_reduce,
                                 args.fit_threshold)
        if fito is not None:
            fit_kw = dict(sensor_hw=fito['sensor_hw'], fit=fito['fit'])
        _filter_options(args.dataset, args.denoise_us, args.pixel_mask, args.hot_rate, fito)
        check_pixel_filter_options(**pix_kw)
        wev = check_write_options(args.write_events, args.events_out, args.evt3_vectors)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    splits = [s for s in ('train', 'val', 'test') if os.path.isdir(os.path.join(args.src, s))]
    pairs = [(os.path.join(args.src, s), os.path.join(args.dst, s)) for s in splits] or [(args.src, args.dst)]
    n = 0
    for split, (src, dst) in zip(splits or [None], pairs):
        wev_kw = {} if wev is None else dict(write_events=wev['fmt'], evt3_vectors=wev['vectors'],
                                             events_out=os.path.join(wev['dir'], split) if split else wev['dir'])
        n += len(ingest_split(src, dst, args.dataset, duration_us=args.duration_us, bins=args.bins, keep_classes=args.keep_classes,
                              write=args.write, verbose=True, unlabelled=args.unlabelled, denoise_us=args.denoise_us,
                              pixel_mask=args.pixel_mask, hot_rate_hz=args.hot_rate, **pix_kw, **fit_kw, **wev_kw))
    if n == 0:
        ap.error(f'no *_td.dat or *.raw under {args.src}')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
