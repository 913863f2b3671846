"""Convert the frame files of an existing dataset tree (raw ``.npy`` twins / HDF5 files; layout: ``leod_amd/data/utils/misc.py``) to
packed stores (``.evp``; format: ``leod_amd/data/utils/packed.py``).

Every ``event_representations*.npy`` / ``.h5`` under TREE gets an ``.evp`` of the same stem beside it.  Chunks of frames are encoded on the
device (``ops.pack_frames``) when one is present and through the numpy codec otherwise; the bytes are the same.  What was written is
then read back through ``PackedFrames``, decoded and compared with the source, frame by frame; only after that comparison does
``--remove-raw`` remove the source files.  While a raw twin exists the loaders keep reading it (.npy, then .evp, then .h5).

    python -m leod_amd.data.pack TREE [--remove-raw]
"""
import argparse
import os
from typing import Dict, List, Optional

import numpy as np

from leod_amd.data.utils import misc
from leod_amd.data.utils.packed import PackedFrames, PackedWriter, encode_frames

FRAMES_PER_CHUNK = 32
_STEMS = ('event_representations', 'event_representations_ds2_nearest')


def _device(device):
    import torch
    if device is None:
        return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
    device = torch.device(device)
    return None if device.type == 'cpu' else device


def find_frame_files(tree: str) -> List[str]:
    """The preferred dense frame file (.npy, else .h5) of every stem under ``tree``, in path order."""
    out = []
    for root, _, files in sorted(os.walk(tree, followlinks=True)):
        for stem in _STEMS:
            for ext in ('.npy', '.h5'):
                if stem + ext in files:
                    out.append(os.path.join(root, stem + ext))
                    break
    return out


def pack_file(src_fn: str, device=None, remove_raw: bool = False, chunk: int = FRAMES_PER_CHUNK) -> Dict:
    """One frame file -> the ``.evp`` of its stem; verified against the source before anything is removed.  -> a small report."""
    import torch
    stem = os.path.splitext(src_fn)[0]
    dst_fn = stem + '.evp'
    device = _device(device)
    src = misc.open_frame_file(misc.resolve_link(src_fn))
    try:
        n, chw = len(src), tuple(int(s) for s in src.shape[1:])
        writer = PackedWriter(dst_fn, *chw)
        try:
            for a in range(0, n, chunk):
                frames = src.read(a, min(a + chunk, n))
                if device is None:
                    writer.append(*encode_frames(frames))
                else:
                    from leod_amd import ops
                    with torch.cuda.device(device):
                        blob, offsets = ops.pack_frames(torch.from_numpy(np.ascontiguousarray(frames)).to(device))
                        writer.append(blob.cpu().numpy(), offsets.numpy())
        except BaseException:
            writer.abort()
            raise
        writer.close()
        got = PackedFrames(dst_fn)
        try:
            if got.shape != (n,) + chw:
                raise IOError(f'{dst_fn}: shape {got.shape} written for a source of {(n,) + chw}')
            for a in range(0, n, chunk):
                b = min(a + chunk, n)
                if not np.array_equal(got.read(a, b), src.read(a, b)):
                    raise IOError(f'{dst_fn}: frames {a}..{b - 1} do not decode to the source; {src_fn} is left as it is')
        finally:
            got.close()
    finally:
        src.close()
    dense, packed_bytes = n * int(np.prod(chw)), os.path.getsize(dst_fn)
    removed = []
    if remove_raw:
        for ext in ('.npy', '.h5'):
            if os.path.lexists(stem + ext):
                os.remove(stem + ext)
                removed.append(stem + ext)
    return dict(source=src_fn, packed=dst_fn, frames=n, dense_bytes=dense, packed_bytes=packed_bytes,
                ratio=round(dense / max(packed_bytes, 1), 2), encoder='numpy' if device is None else 'device', removed=removed)


def pack_tree(tree: str, device=None, remove_raw: bool = False, verbose: bool = False) -> List[Dict]:
    reports = []
    for fn in find_frame_files(tree):
        rep = pack_file(fn, device=device, remove_raw=remove_raw)
        if verbose:
            print(rep, flush=True)
        reports.append(rep)
    return reports


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog='python -m leod_amd.data.pack', description=__doc__.split('\n\n')[0])
    ap.add_argument('tree', help='dataset path, split or recording directory')
    ap.add_argument('--remove-raw', action='store_true', help='remove the .npy / .h5 of a stem once its .evp has been verified')
    ap.add_argument('--device', default=None, help="'cpu' forces the numpy encoder; default: the current GPU when there is one")
    args = ap.parse_args(argv)
    reports = pack_tree(args.tree, device=args.device, remove_raw=args.remove_raw, verbose=True)
    if not reports:
        ap.error(f'no event_representations*.npy / .h5 under {args.tree}')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
