"""Host side of the event noise filters of the ingestion (``ops.filter_events``, csrc/k_filter.hip; ``ops.pixel_filter_events``,
csrc/k_pixfilter.hip; the rules: DESIGN.md section 1): the hot-pixel threshold, the pixel-mask file, the band of the anti-flicker
filter, the response curves of a filter survey (``ops.survey_events``, csrc/k_survey.hip), and the options and the box map of the
sensor fit (``ops.fit_events``, csrc/k_fit.hip).  NumPy only; nothing here touches the device."""
from typing import Tuple

import numpy as np

MASK_FILE = 'hot_pixels.npy'         # written beside the frames when the mask was derived from the recording (--hot-rate)
DEFAULT_FLICKER_LOCK = 3             # in-band periods in a row after which a pixel is removed; a default with no data behind it
MAX_FLICKER_HZ = 1_000_000


def flicker_band(band) -> Tuple[int, int]:
    """'FMIN:FMAX' or (fmin, fmax), integer Hz with 1 <= FMIN <= FMAX <= 10^6 -> (p_min_us, p_max_us), the periods in whole microseconds
    that lie in the band: p_min = ceil(10^6 / FMAX), p_max = floor(10^6 / FMIN).  ``ValueError`` where no whole period does (3:3)."""
    if isinstance(band, str):
        parts = band.split(':')
        if len(parts) != 2 or not all(q.strip().isdigit() for q in parts):
            raise ValueError(f'anti_flicker={band!r}: FMIN:FMAX in integer Hz expected')
        fmin, fmax = (int(q) for q in parts)
    else:
        try:
            fmin, fmax = band
        except (TypeError, ValueError):
            raise ValueError(f'anti_flicker={band!r}: FMIN:FMAX or a pair (fmin, fmax) in integer Hz expected') from None
        for v in (fmin, fmax):
            if isinstance(v, (bool, float)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f'anti_flicker={band!r}: integer frequencies expected')
        fmin, fmax = int(fmin), int(fmax)
    if not 1 <= fmin <= fmax <= MAX_FLICKER_HZ:
        raise ValueError(f'anti_flicker={band!r}: 1 <= FMIN <= FMAX <= {MAX_FLICKER_HZ} Hz expected')
    p_min, p_max = -(-1_000_000 // fmax), 1_000_000 // fmin
    if p_min > p_max:
        raise ValueError(f'anti_flicker={band!r}: no whole number of microseconds is a period in this band')
    return p_min, p_max


def hot_pixel_mask(counts, duration_us: int, max_rate_hz: int) -> np.ndarray:
    """Events per pixel over ``duration_us`` microseconds -> uint8 mask [H, W], 1 where the pixel fired at MORE than ``max_rate_hz``:
    ``count * 10^6 > max_rate_hz * duration_us``, in integer arithmetic (a pixel exactly at the rate is not hot)."""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.dtype.kind not in 'iu':
        raise ValueError(f'counts: an integer array [H, W] expected, got {counts.dtype} {counts.shape}')
    for name, v in (('duration_us', duration_us), ('max_rate_hz', max_rate_hz)):
        if isinstance(v, (bool, float)) or int(v) != v or int(v) < 0:
            raise ValueError(f'{name}={v!r}: a non-negative integer expected')
    if counts.size and int(counts.min()) < 0:
        raise ValueError('counts: negative entries')
    limit = int(max_rate_hz) * int(duration_us)                  # Python integers: no overflow at any rate or length
    # count * 10^6 > limit  <=>  count > limit // 10^6, for integers
    floor = limit // 1_000_000
    if floor >= np.iinfo(np.int64).max:
        return np.zeros(counts.shape, dtype=np.uint8)
    return (counts.astype(np.int64, copy=False) > floor).astype(np.uint8)


def survey_responses(counters, edges_us) -> dict:
    """The histograms of a filter survey (``ops.survey_counters``) -> the events each filter would REMOVE, applied
    alone to the unfiltered stream: per edge of ``edges_us`` int64 arrays [K] ``denoise`` (``--denoise-us e``: unsupported events),
    ``trail`` (``--trail-us e``), ``stc`` (``--stc-us e``), ``stc_cut_trail`` (``--stc-us e --stc-cut-trail``: burst events each), and
    ``flicker`` int64 [256]: entry L is the number of events ``--flicker-lock L`` removes in the surveyed band (entry 0 is 0: no such
    lock; all zeros where the survey had no band).  The five identities, in integers:
        denoise[b]       = nb[K + 1] + sum(nb[b + 1 .. K])
        trail[b]         = sum(same[.. b])
        stc[b]           = candidates - sum(same[.. b])
        stc_cut_trail[b] = candidates - (sum(sec_on[.. b]) - sum(sec_off[.. b]))
        flicker[L]       = sum(run[L ..])"""
    K = len(list(edges_us))
    arr = {}
    for name, n in (('nb', K + 2), ('same', K + 1), ('sec_on', K + 1), ('sec_off', K + 1), ('run', 256)):
        a = np.asarray(counters[name])
        if a.shape != (n,) or a.dtype.kind not in 'iu':
            raise ValueError(f'counters[{name!r}]: {n} integers expected for {K} edges, got {a.dtype} {a.shape}')
        arr[name] = a.astype(np.int64)
    cand = int(counters['candidates'])
    nb, same = arr['nb'], np.cumsum(arr['same'])[:K]
    above = np.cumsum(nb[::-1])[::-1]                            # above[c] = sum(nb[c ..]), with nb[K + 1]: no earlier neighbour at all
    second = (np.cumsum(arr['sec_on']) - np.cumsum(arr['sec_off']))[:K]
    flicker = np.cumsum(arr['run'][::-1])[::-1].copy()
    flicker[0] = 0
    return dict(denoise=above[1:K + 1].copy(), trail=same.copy(), stc=cand - same, stc_cut_trail=cand - second, flicker=flicker)


FIT_REDUCES = ('pick', 'sum', 'fire')
FIT_MAX_SIDE, FIT_MAX_SCALE, FIT_MAX_OFFSET, FIT_MAX_THRESHOLD = 16384, 64, 16384, 32767      # the limits of include/leod_hip.h


def _fit_int(name, v, lo, hi, what):
    if isinstance(v, str) and v.strip().lstrip('+-').isdigit():
        v = int(v)
    if isinstance(v, (bool, float)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f'{name}={v!r}: {what} expected')
    return int(v)


def fit_oriented_hw(src_hw, orient: int) -> Tuple[int, int]:
    """(H', W') of a sensor (Hs, Ws) turned by ``orient`` degrees clockwise."""
    hs, ws = src_hw
    return (ws, hs) if orient in (90, 270) else (hs, ws)


def fit_spec(src_hw, frame_hw, scale='auto', offset='center', orient=0, mirror=False, reduce='pick', threshold=None) -> dict:
    """The options of a sensor fit (the rule: DESIGN.md section 1), checked and resolved to plain ints -> dict(src_hw [Hs, Ws], frame_hw
    [Hd, Wd], orient, mirror, scale, offset [ox, oy], reduce, threshold).  ``scale`` 'auto': the largest k with W' // k >= Wd and
    H' // k >= Hd, or 1 when there is none ((H', W'): the sensor after ``orient``); else an integer in [1, 64].  ``offset`` 'center':
    ox = (Wd - W' // k) // 2, oy = (Hd - H' // k) // 2, floor division; else 'X,Y' or a pair.  ``threshold`` (only with reduce 'fire';
    None: k * k there, and None in the result for 'pick' / 'sum').  ``ValueError`` for anything else."""
    def hw(name, v):
        try:
            h, w = v
        except (TypeError, ValueError):
            raise ValueError(f'{name}={v!r}: (height, width) expected') from None
        return [_fit_int(name, q, 1, FIT_MAX_SIDE, f'(height, width), integers in [1, {FIT_MAX_SIDE}],') for q in (h, w)]
    src, frame = hw('sensor_hw', src_hw), hw('frame_hw', frame_hw)
    orient = _fit_int('fit_orient', orient, 0, 270, '0, 90, 180 or 270 (degrees clockwise)')
    if orient % 90:
        raise ValueError(f'fit_orient={orient!r}: 0, 90, 180 or 270 (degrees clockwise) expected')
    if mirror not in (False, True):
        raise ValueError(f'fit_mirror={mirror!r}: True or False expected')
    if reduce not in FIT_REDUCES:
        raise ValueError(f"fit_reduce={reduce!r}: 'pick', 'sum' or 'fire' expected")
    if threshold is not None and reduce != 'fire':
        raise ValueError("fit_threshold needs fit_reduce 'fire'")
    ho, wo = fit_oriented_hw(src, orient)
    if isinstance(scale, str) and scale.strip().lower() == 'auto':
        k = max(min(wo // frame[1], ho // frame[0], FIT_MAX_SCALE), 1)       # W' // k >= Wd  <=>  k <= W' // Wd, for positive integers
    else:
        k = _fit_int('fit', scale, 1, FIT_MAX_SCALE, f"'auto' or an integer scale in [1, {FIT_MAX_SCALE}]")
    if isinstance(offset, str) and offset.strip().lower() == 'center':
        off = [(frame[1] - wo // k) // 2, (frame[0] - ho // k) // 2]
    else:
        parts = offset.split(',') if isinstance(offset, str) else offset
        try:
            ox, oy = parts
        except (TypeError, ValueError):
            raise ValueError(f"fit_offset={offset!r}: 'center' or X,Y expected") from None
        off = [_fit_int('fit_offset', q, -FIT_MAX_OFFSET, FIT_MAX_OFFSET, f"'center' or X,Y, integers in [-{FIT_MAX_OFFSET}, {FIT_MAX_OFFSET}],")
               for q in (ox, oy)]
    if reduce == 'fire':
        threshold = _fit_int('fit_threshold', k * k if threshold is None else threshold, 1, FIT_MAX_THRESHOLD,
                             f'an integer in [1, {FIT_MAX_THRESHOLD}]')
    return dict(src_hw=src, frame_hw=frame, orient=orient, mirror=bool(mirror), scale=k, offset=off, reduce=reduce, threshold=threshold)


def fit_boxes(boxes: np.ndarray, spec: dict) -> Tuple[np.ndarray, int]:
    """Boxes (structured array with x, y, w, h: top-left and size, continuous -- a pixel covers [x, x + 1)) of a recording at the source
    geometry of ``spec`` (``fit_spec``) -> (the boxes at the frame geometry, the number dropped).  The same map as the events': mirror,
    orient, divide by the scale, add the offset; then clip to the intersection of the frame and the placed scaled image; a box whose
    clipped width or height is <= 0 is dropped.  No other filtering.  Every other field is copied."""
    hs, ws = spec['src_hw']
    hd, wd = spec['frame_hw']
    k, (ox, oy) = spec['scale'], spec['offset']
    x, y, w, h = (np.asarray(boxes[n], dtype=np.float64) for n in ('x', 'y', 'w', 'h'))
    if spec['mirror']:
        x = ws - (x + w)
    if spec['orient'] == 90:
        x, y, w, h = hs - (y + h), x, h, w
    elif spec['orient'] == 180:
        x, y = ws - (x + w), hs - (y + h)
    elif spec['orient'] == 270:
        x, y, w, h = y, ws - (x + w), h, w
    ho, wo = fit_oriented_hw((hs, ws), spec['orient'])
    x0, y0, x1, y1 = x / k + ox, y / k + oy, (x + w) / k + ox, (y + h) / k + oy
    lo_x, hi_x = max(0, ox), min(wd, ox + wo // k)
    lo_y, hi_y = max(0, oy), min(hd, oy + ho // k)
    x0, x1 = np.clip(x0, lo_x, None), np.clip(x1, None, hi_x)
    y0, y1 = np.clip(y0, lo_y, None), np.clip(y1, None, hi_y)
    keep = (x1 - x0 > 0) & (y1 - y0 > 0)
    out = boxes[keep].copy()
    for name, v in (('x', x0), ('y', y0), ('w', x1 - x0), ('h', y1 - y0)):
        out[name] = v[keep]
    return out, int(len(boxes) - np.count_nonzero(keep))


def check_pixel_mask(mask, sensor_hw: Tuple[int, int], what: str = 'pixel mask') -> np.ndarray:
    """``ValueError`` unless ``mask`` is a uint8 or bool array [H, W] at sensor resolution; -> the mask as uint8 0 / 1."""
    mask = np.asarray(mask)
    if mask.dtype != np.uint8 and mask.dtype != np.bool_:
        raise ValueError(f'{what}: uint8 or bool expected, got {mask.dtype}')
    if tuple(mask.shape) != tuple(int(v) for v in sensor_hw):
        raise ValueError(f'{what}: shape {tuple(mask.shape)}, the sensor is {tuple(int(v) for v in sensor_hw)} (height, width)')
    return np.ascontiguousarray(mask != 0).astype(np.uint8)


def read_pixel_mask(fn: str, sensor_hw: Tuple[int, int]) -> np.ndarray:
    """A mask file (``.npy``; uint8 or bool [H, W] at sensor resolution, non-zero = masked) -> uint8 0 / 1."""
    if not str(fn).lower().endswith('.npy'):
        raise ValueError(f'{fn}: a pixel mask is a .npy file')
    try:
        mask = np.load(fn, allow_pickle=False)
    except ValueError as e:                                      # a missing file stays a FileNotFoundError
        raise ValueError(f'{fn}: no readable .npy array ({e})') from None
    return check_pixel_mask(mask, sensor_hw, what=str(fn))
