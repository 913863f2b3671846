#!/usr/bin/env python
"""Record tests/golden/g27_dat_events.npz by running the REFERENCE's own .dat reader (/root/reference,
utils/evaluation/prophesee/io/dat_events_tools.py ``load_td_data``) on CPU, like make_golden.py / make_golden_rotation.py (same
``ref_stubs`` path; runs only in the build container, never on the GPU box).

The fixture holds the BYTES of a small Event2D .dat file (header of a 30 x 24 sensor, 400 events written by the package's own writer,
``leod_amd.data.utils.dat_events.write_dat``: the reference's ``write_header`` cannot run, it names an undefined ``EV_STRINGS``) and
the fields ``t, x, y, p`` the reference decodes from that file, plus the header values its ``parse_header`` returns.  Data only.

Usage:  python tests/golden/make_golden_dat.py        # rewrites tests/golden/g27_dat_events.npz
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, 'ref_stubs'))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.get_device_name = lambda *a, **k: 'none'  # called at import time by the reference's coco_eval

from leod_amd.data.utils import dat_events  # noqa: E402

# ---- reference import ----------------------------------------------------------------------------
from utils.evaluation.prophesee.io import dat_events_tools as ref_dat  # noqa: E402

H, W, N = 24, 30, 400


def main():
    rng = np.random.RandomState(27)
    # sorted times with repeats, t = 0 at the front, exact multiples of 50 ms, and a tail beyond 2^31 us (t is UNSIGNED in the file)
    t = np.sort(np.concatenate([[0, 0, 50_000, 50_000, 100_000], rng.randint(0, 400_000, N - 15),
                                2 ** 31 + rng.randint(0, 1000, 8), [2 ** 32 - 2, 2 ** 32 - 1]]).astype(np.int64))
    x, y, p = rng.randint(0, W, N), rng.randint(0, H, N), rng.randint(0, 2, N)
    x[:4], y[:4], p[:4] = [0, W - 1, 0, W - 1], [0, 0, H - 1, H - 1], [0, 1, 1, 0]
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, 'g27_td.dat')
        dat_events.write_dat(fn, dat_events.encode(t, x, y, p), H, W)
        raw = np.fromfile(fn, dtype=np.uint8)
        ev = ref_dat.load_td_data(fn)
        with open(fn, 'rb') as f:
            bod, ev_type, ev_size, size = ref_dat.parse_header(f)
    out = dict(dat_bytes=raw, t=ev['t'].astype(np.int64), x=ev['x'].astype(np.int64), y=ev['y'].astype(np.int64),
               p=ev['p'].astype(np.int64), header=np.array([bod, ev_type, ev_size, size[0], size[1]], dtype=np.int64))
    assert len(out['t']) == N
    np.savez_compressed(os.path.join(HERE, 'g27_dat_events.npz'), **out)
    print('wrote g27_dat_events.npz', {k: v.shape for k, v in out.items()}, 'header', out['header'])


if __name__ == '__main__':
    main()
