"""Writes tests/golden/p01_frames.npy and p01_frames.evp: a few frames and their packed store, from the numpy codec
(leod_amd/data/utils/packed.py).  The pair pins format version 1 of the packed event-frame store.

    python tests/golden/make_golden_packed.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from leod_amd.data.utils.packed import PackedWriter  # noqa: E402


def frames():
    """[6, 20, 24, 19] uint8 (E = 9120: two groups, the last block partial): sparse random counts at three densities, one frame of zeros,
    one with only the first and the last element set, one saturated."""
    rng = np.random.default_rng(20250101)
    shape = (20, 24, 19)
    out = np.zeros((6,) + shape, dtype=np.uint8)
    for k, density in enumerate((0.002, 0.03, 0.3)):
        out[k] = ((rng.random(shape) < density) * rng.integers(1, 256, shape)).astype(np.uint8)
    out[4].reshape(-1)[[0, -1]] = (1, 255)
    out[5] = 255
    return out


def main():
    x = frames()
    np.save(os.path.join(HERE, 'p01_frames.npy'), x)
    w = PackedWriter(os.path.join(HERE, 'p01_frames.evp'), *x.shape[1:])
    w.append_frames(x[:4])
    w.append_frames(x[4:])
    w.close()


if __name__ == '__main__':
    main()
