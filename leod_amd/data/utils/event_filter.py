"""Host side of the event noise filters of the ingestion (``ops.filter_events``, csrc/k_filter.hip; the rule: DESIGN.md section 1): the
hot-pixel threshold and the pixel-mask file.  NumPy only; nothing here touches the device."""
from typing import Tuple

import numpy as np

MASK_FILE = 'hot_pixels.npy'         # written beside the frames when the mask was derived from the recording (--hot-rate)


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
