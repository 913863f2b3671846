"""Packed event-frame store (``.evp``, format version 1): the stacked histograms of a recording as sparse blobs that the GPU
expands (``ops.unpack_frames``, csrc/k_pack.hip).  The frames are overwhelmingly zeros; what crosses the disk, the page cache,
pinned memory and PCIe is two levels of bit masks plus the non-zero bytes.  The numpy codec in this module is the statement of the
format: the device encoder and decoder, the host library's validator and decoder (csrc/packed_host.cpp, what the store and the loaders'
host path run, without the GIL) and the committed fixture are tested against it.

File (little endian throughout):

    byte 0    char[8]  magic 'LEODEVP1'
         8    u32      version = 1
        12    u32      N        frames
        16    u32      C, H, W  (three u32: 16, 20, 24)
        28    u32      0
        32    u64      data_pos   = 64: first byte of the data region (64-byte aligned)
        40    u64      table_pos  first byte of ``u64 offsets[N + 1]`` (multiple of 16, behind the data region)
        48    16 bytes 0
        64    frame blobs back to back; blob k is data[offsets[k] : offsets[k + 1]], offsets[0] = 0

The offsets table is a TRAILER that the header points to: a writer appends blobs without knowing N (``PackedWriter`` takes frames
as they come), and the table plus the final header are written on close.

Frame blob: E = C*H*W elements in C order, block = 64 elements, group = 64 blocks (4096 elements), G = ceil(E / 4096):

    16 bytes          u32 n_masks, u32 n_values, 8 zero bytes
    G x 16 bytes      u64 l1 (bit i <=> block 64 g + i has a non-zero element), u32 mask_base, u32 value_base: the number of masks /
                      values that the groups before g hold
    n_masks x u64     one per non-zero block in ascending block order, bit j <=> element j of the block is non-zero (bits >= E are 0)
    n_values x u8     the non-zero elements in ascending element order
    zero padding to a multiple of 16

An all-zero frame takes 16 + 16 G bytes, the worst case 16 + 16 G + 8 ceil(E / 64) + E rounded up to 16.  Exactly one byte string
encodes a given frame, so encoders are compared byte for byte."""
import os
import struct
from typing import List, Optional, Tuple

import numpy as np

MAGIC = b'LEODEVP1'
VERSION = 1
HEADER_BYTES = 64
BLOCK, GROUP = 64, 4096
_HEADER = struct.Struct('<8sIIIIIIQQ16x')
assert _HEADER.size == HEADER_BYTES
SUFFIX = '.evp'


def n_groups(E: int) -> int:
    return -(-int(E) // GROUP)


def zero_frame_bytes(E: int) -> int:
    return 16 + 16 * n_groups(E)


def worst_frame_bytes(E: int) -> int:
    """Upper bound of a blob: every element non-zero."""
    n = 16 + 16 * n_groups(E) + 8 * (-(-int(E) // BLOCK)) + int(E)
    return -(-n // 16) * 16


def _popcount(a: np.ndarray) -> np.ndarray:
    return np.bitwise_count(a) if hasattr(np, 'bitwise_count') else np.unpackbits(a.view(np.uint8).reshape(a.shape + (-1,)), axis=-1).sum(-1)


# ---- numpy codec ---------------------------------------------------------------------------------------------------------------------
def encode_frame(frame: np.ndarray) -> np.ndarray:
    """One uint8 frame (any shape, read in C order) -> its blob (uint8 [nbytes])."""
    x = np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1)
    E, G = x.size, n_groups(x.size)
    assert E > 0 and frame.dtype == np.uint8
    if E != G * GROUP:
        full = np.zeros((G * GROUP,), dtype=np.uint8)
        full[:E] = x
        x = full
    nz = x != 0
    masks_all = np.packbits(nz.reshape(-1, BLOCK), axis=1, bitorder='little').view('<u8').reshape(-1)        # [G * 64]
    blk_nz = masks_all != 0
    l1 = np.packbits(blk_nz.reshape(G, 64), axis=1, bitorder='little').view('<u8').reshape(G)
    per_group_masks = blk_nz.reshape(G, 64).sum(1, dtype=np.int64)
    per_group_values = nz.reshape(G, GROUP).sum(1, dtype=np.int64)
    n_masks, n_values = int(per_group_masks.sum()), int(per_group_values.sum())
    size = 16 + 16 * G + 8 * n_masks + n_values
    blob = np.zeros((-(-size // 16) * 16,), dtype=np.uint8)
    blob[:8].view('<u4')[:] = (n_masks, n_values)
    blob[16:16 + 16 * G].view('<u8').reshape(G, 2)[:, 0] = l1
    bases = blob[16:16 + 16 * G].view('<u4').reshape(G, 4)
    bases[:, 2] = np.cumsum(per_group_masks) - per_group_masks
    bases[:, 3] = np.cumsum(per_group_values) - per_group_values
    m0 = 16 + 16 * G
    blob[m0:m0 + 8 * n_masks].view('<u8')[:] = masks_all[blk_nz]
    blob[m0 + 8 * n_masks:m0 + 8 * n_masks + n_values] = x[nz]
    return blob


def encode_frames(frames: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """uint8 [n, C, H, W] -> (blob uint8 [total], offsets int64 [n + 1]): frame k is blob[offsets[k]:offsets[k + 1]]."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim >= 2, (frames.dtype, frames.shape)
    blobs = [encode_frame(f) for f in frames]
    offsets = np.zeros((len(blobs) + 1,), dtype=np.int64)
    np.cumsum([b.size for b in blobs], out=offsets[1:])
    return (np.concatenate(blobs) if blobs else np.zeros((0,), dtype=np.uint8)), offsets


def _as_u8(blob) -> np.ndarray:
    b = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    assert b.dtype == np.uint8 and b.ndim == 1
    return b


def _parts(b: np.ndarray, E: int):
    """(n_masks, n_values, l1 [G], mask_base [G], value_base [G]) of a blob whose length covers the header and the group entries."""
    G = n_groups(E)
    n_masks, n_values = (int(v) for v in np.frombuffer(b[:8].tobytes(), dtype='<u4'))
    raw = b[16:16 + 16 * G].tobytes()
    bases = np.frombuffer(raw, dtype='<u4').reshape(G, 4)
    return n_masks, n_values, np.frombuffer(raw, dtype='<u8').reshape(G, 2)[:, 0].copy(), bases[:, 2], bases[:, 3]


def decode_frame(blob, C: int, H: int, W: int, flip_channels: bool = False, out: Optional[np.ndarray] = None) -> np.ndarray:
    """A VALID blob (``validate_frame``) -> uint8 [C, H, W] (into ``out`` if given, any writable array of that shape).
    ``flip_channels``: the channel axis reversed, as the time-flipped view reads a frame."""
    b = _as_u8(blob)
    E = C * H * W
    G = n_groups(E)
    n_masks, n_values, l1, _, _ = _parts(b, E)
    m0 = 16 + 16 * G
    blk_nz = np.unpackbits(l1.view(np.uint8), bitorder='little').view(np.bool_)                               # [G * 64]
    masks_all = np.zeros((G * 64,), dtype='<u8')
    masks_all[blk_nz] = np.frombuffer(b[m0:m0 + 8 * n_masks].tobytes(), dtype='<u8')
    nz = np.unpackbits(masks_all.view(np.uint8), bitorder='little', count=E).view(np.bool_)
    flat = np.zeros((E,), dtype=np.uint8)
    flat[nz] = b[m0 + 8 * n_masks:m0 + 8 * n_masks + n_values]
    frame = flat.reshape(C, H, W)
    if flip_channels:
        frame = frame[::-1]
    if out is None:
        return np.ascontiguousarray(frame)
    assert out.shape == (C, H, W) and out.dtype == np.uint8, (out.shape, out.dtype)
    np.copyto(out, frame)
    return out


def validate_frame(blob, C: int, H: int, W: int) -> None:
    """Raises ``ValueError`` unless ``blob`` is THE encoding of some [C, H, W] frame: everything a decoder indexes with is checked
    here, once, so that the decoders (numpy, host library, device kernel) need not trust file contents."""
    b = _as_u8(blob)
    E = C * H * W
    G = n_groups(E)
    if E <= 0:
        raise ValueError(f'frame shape {(C, H, W)}')
    if b.size < 16 + 16 * G or b.size % 16:
        raise ValueError(f'blob of {b.size} bytes: at least {16 + 16 * G} (header + {G} group entries) in multiples of 16 expected')
    if b[8:16].any():
        raise ValueError('non-zero padding in the blob header')
    n_masks, n_values, l1, mask_base, value_base = _parts(b, E)
    size = 16 + 16 * G + 8 * n_masks + n_values
    if b.size != -(-size // 16) * 16:
        raise ValueError(f'blob of {b.size} bytes, but n_masks={n_masks} and n_values={n_values} make {-(-size // 16) * 16}')
    if b[size:].any():
        raise ValueError('non-zero padding behind the values')
    per_group_masks = _popcount(l1).astype(np.int64)
    if int(per_group_masks.sum()) != n_masks:
        raise ValueError(f'the group entries mark {int(per_group_masks.sum())} non-zero blocks, the header says n_masks={n_masks}')
    if not np.array_equal(mask_base.astype(np.int64), np.cumsum(per_group_masks) - per_group_masks):
        raise ValueError('mask_base is not the running sum of the blocks marked before each group')
    blk_nz = np.unpackbits(l1.view(np.uint8), bitorder='little').view(np.bool_)
    n_blocks = -(-E // BLOCK)
    if blk_nz[n_blocks:].any():
        raise ValueError('a block at or beyond the end of the frame is marked non-zero')
    m0 = 16 + 16 * G
    masks = np.frombuffer(b[m0:m0 + 8 * n_masks].tobytes(), dtype='<u8')
    if (masks == 0).any():
        raise ValueError('an empty mask is stored for a block marked non-zero')
    if E % BLOCK and blk_nz[n_blocks - 1] and int(masks[-1]) >> (E % BLOCK):
        raise ValueError('mask bits at or beyond the end of the frame')
    pc = _popcount(masks).astype(np.int64)
    if int(pc.sum()) != n_values:
        raise ValueError(f'the masks mark {int(pc.sum())} non-zero elements, the header says n_values={n_values}')
    pc_all = np.zeros((G * 64,), dtype=np.int64)
    pc_all[blk_nz] = pc
    per_group_values = pc_all.reshape(G, 64).sum(1)
    if not np.array_equal(value_base.astype(np.int64), np.cumsum(per_group_values) - per_group_values):
        raise ValueError('value_base is not the running sum of the elements marked before each group')
    if (b[m0 + 8 * n_masks:size] == 0).any():
        raise ValueError('a zero is stored among the non-zero elements')


def validate_frames(blob, offsets, C: int, H: int, W: int) -> None:
    b = _as_u8(blob)
    for k in range(len(offsets) - 1):
        validate_frame(b[int(offsets[k]):int(offsets[k + 1])], C, H, W)


# ---- the same two operations in the host library (csrc/packed_host.cpp): what the store and the loaders' host path run -----------------
_HOST_CHECKS = ('', 'size', 'header padding', 'size against n_masks / n_values', 'padding behind the values', 'n_masks', 'mask_base',
                'a block beyond the frame', 'an empty mask', 'mask bits beyond the frame', 'n_values', 'value_base', 'a stored zero')


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def validate_frame_host(blob: np.ndarray, C: int, H: int, W: int) -> None:
    """``validate_frame`` in the host library (GIL released): the same blobs pass; a refusal is then explained by the numpy version."""
    from leod_amd._lib import lib
    b = np.ascontiguousarray(_as_u8(blob))
    rc = lib().leod_evp_validate(_ptr(b), b.size, C * H * W)
    if rc:
        validate_frame(b, C, H, W)
        raise ValueError(f'malformed blob: {_HOST_CHECKS[rc] if 0 < rc < len(_HOST_CHECKS) else rc}')


def decode_frame_host(blob: np.ndarray, C: int, H: int, W: int, flip_channels: bool = False, out: Optional[np.ndarray] = None) -> np.ndarray:
    """``decode_frame`` in the host library (GIL released) when ``out`` is C-contiguous, else the numpy decoder."""
    if out is None:
        out = np.empty((C, H, W), dtype=np.uint8)
    if not out.flags['C_CONTIGUOUS']:
        return decode_frame(blob, C, H, W, flip_channels, out)
    from leod_amd._lib import lib
    assert out.shape == (C, H, W) and out.dtype == np.uint8 and out.flags['WRITEABLE'], (out.shape, out.dtype)
    b = np.ascontiguousarray(_as_u8(blob))
    if lib().leod_evp_decode(_ptr(b), b.size, C, H * W, 1 if flip_channels else 0, _ptr(out)):
        raise ValueError('decode_frame_host: the blob is shorter than its counts say')
    return out


# ---- store ---------------------------------------------------------------------------------------------------------------------------
def read_header(fn: str) -> Tuple[int, Tuple[int, int, int], int, int]:
    """-> (N, (C, H, W), data_pos, table_pos)"""
    with open(fn, 'rb') as f:
        raw = f.read(HEADER_BYTES)
    if len(raw) != HEADER_BYTES:
        raise ValueError(f'{fn}: {len(raw)} bytes are no .evp header')
    magic, version, N, C, H, W, zero, data_pos, table_pos = _HEADER.unpack(raw)
    if magic != MAGIC or version != VERSION:
        raise ValueError(f'{fn}: magic {magic!r} version {version}: no version-{VERSION} packed frame file')
    if zero or any(raw[48:]) or data_pos != HEADER_BYTES or table_pos % 16 or table_pos < data_pos or min(C, H, W) < 1:
        raise ValueError(f'{fn}: malformed .evp header')
    return N, (C, H, W), data_pos, table_pos


class PackedFrames:
    """[N,C,H,W] uint8 frames of one recording in a ``.evp`` file, behind the interface of ``misc.RawFrames``: ``read`` decodes on
    the host; ``read_packed`` hands out the blobs as they lie in the file (one ``preadv`` from the page cache) for the device decoder.
    Every frame is validated the first time it is read through this store, on the reading thread."""

    def __init__(self, fn: str):
        self.fn = fn
        N, chw, self._data_pos, table_pos = read_header(fn)
        self._shape = (N,) + chw
        self._fd = os.open(fn, os.O_RDONLY)
        try:
            size = os.fstat(self._fd).st_size
            table = np.empty((N + 1,), dtype='<u8')
            self._pread(memoryview(table.view(np.uint8)), table_pos)
            self.offsets = table.astype(np.int64)
            ok = self.offsets[0] == 0 and (np.diff(self.offsets) >= zero_frame_bytes(int(np.prod(chw)))).all() and \
                (self.offsets % 16 == 0).all() and self._data_pos + int(self.offsets[-1]) <= table_pos and table_pos + 8 * (N + 1) <= size
            if not ok:
                raise ValueError(f'{fn}: the offsets table does not describe the data region')
        except Exception:
            os.close(self._fd)
            self._fd = None
            raise
        self._valid = np.zeros((N,), dtype=np.bool_)

    @property
    def shape(self):
        return self._shape

    def __len__(self):
        return self._shape[0]

    def _pread(self, mv, offset: int) -> None:
        done, total = 0, len(mv)
        while done < total:
            n = os.preadv(self._fd, [mv[done:]], offset + done)
            if n <= 0:
                raise IOError(f'{self.fn}: short read at byte {offset + done}')
            done += n

    def read_packed(self, start: int, end: int) -> Tuple[np.ndarray, np.ndarray]:
        """Frames [start, end) -> (uint8 [nbytes] holding their blobs, int64 offsets [end - start + 1] into it); validated."""
        assert 0 <= start < end <= len(self)
        lo, hi = int(self.offsets[start]), int(self.offsets[end])
        buf = np.empty((hi - lo,), dtype=np.uint8)
        self._pread(memoryview(buf), self._data_pos + lo)
        offs = self.offsets[start:end + 1] - lo
        todo = np.flatnonzero(~self._valid[start:end])
        for k in todo:
            try:
                validate_frame_host(buf[int(offs[k]):int(offs[k + 1])], *self._shape[1:])
            except ValueError as e:
                raise ValueError(f'{self.fn}: frame {start + int(k)}: {e}') from None
        self._valid[start:end] = True
        return buf, offs

    def read(self, start: int, end: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Frames [start, end) decoded -> ``out`` [n,C,H,W] (any strides) or a new array."""
        buf, offs = self.read_packed(start, end)
        if out is None:
            out = np.empty((end - start,) + self._shape[1:], dtype=np.uint8)
        assert out.shape == (end - start,) + self._shape[1:] and out.dtype == np.uint8
        for k in range(end - start):
            decode_frame_host(buf[int(offs[k]):int(offs[k + 1])], *self._shape[1:], out=out[k])
        return out

    def close(self):
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PackedWriter:
    """Writes ``fn + '.tmp'`` and renames it on ``close``: blobs are appended behind a placeholder header; the offsets table goes
    behind the data and the header that points to it is written last (see the module docstring)."""

    def __init__(self, fn: str, C: int, H: int, W: int):
        self.fn, self.chw = fn, (int(C), int(H), int(W))
        self._f = open(fn + '.tmp', 'wb')
        self._f.write(b'\0' * HEADER_BYTES)
        self._sizes: List[np.ndarray] = []
        self._min = zero_frame_bytes(C * H * W)

    def append(self, blob, offsets) -> None:
        b = _as_u8(blob)
        offsets = np.asarray(offsets, dtype=np.int64)
        sizes = np.diff(offsets)
        if offsets[0] != 0 or offsets[-1] != b.size or (sizes < self._min).any() or (sizes % 16).any():
            raise ValueError('append: offsets do not tile the blob with whole frames')
        self._f.write(memoryview(np.ascontiguousarray(b)))
        self._sizes.append(sizes)

    def append_frames(self, frames: np.ndarray) -> None:
        assert tuple(frames.shape[1:]) == self.chw, (frames.shape, self.chw)
        self.append(*encode_frames(frames))

    def close(self) -> None:
        if self._f is None:
            return
        sizes = np.concatenate(self._sizes) if self._sizes else np.zeros((0,), dtype=np.int64)
        table = np.zeros((len(sizes) + 1,), dtype='<u8')
        np.cumsum(sizes, out=table[1:])
        table_pos = HEADER_BYTES + int(table[-1])
        assert self._f.tell() == table_pos and table_pos % 16 == 0
        self._f.write(table.tobytes())
        self._f.seek(0)
        self._f.write(_HEADER.pack(MAGIC, VERSION, len(sizes), *self.chw, 0, HEADER_BYTES, table_pos))
        self._f.close()
        self._f = None
        os.replace(self.fn + '.tmp', self.fn)

    def abort(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None
            if os.path.exists(self.fn + '.tmp'):
                os.remove(self.fn + '.tmp')


# ---- loader batches ------------------------------------------------------------------------------------------------------------------
FLAG_FLIP_CHANNELS = 1


class PackedSlot:
    """What a sequence leaves in place of dense frames when the batch assembler asks for packed ones (``out=PackedSlot()``): the
    blobs of its real frames, their position among the L timesteps and the direction they are read in.  A slot that is left
    untouched (a sample that loads labels only) stands for L zero frames."""

    def __init__(self):
        self.blob = self.offsets = None
        self.pad_front = self.n = 0
        self.reverse = False

    def set_packed(self, blob, offsets, pad_front: int, reverse: bool) -> None:
        self.blob, self.offsets = blob, offsets
        self.pad_front, self.n, self.reverse = pad_front, len(offsets) - 1, reverse


class PackedBatch:
    """The frames of a loader batch before decoding: ``buf`` one (pinned) uint8 tensor of blobs, each at a 16-byte-aligned offset;
    ``slot_off`` int64 / ``slot_flags`` int32 [L * B] in (t, b) order: the blob of timestep t of sample b, -1 for a zero frame (front and
    back padding, exhausted slots); flag bit 0 = channels reversed (time-flipped sample).  ``shape`` = (L, B, C, H, W)."""

    def __init__(self, buf, slot_off, slot_flags, shape):
        self.buf, self.slot_off, self.slot_flags, self.shape = buf, slot_off, slot_flags, tuple(int(s) for s in shape)

    def __len__(self):
        return self.shape[0]

    def decode_host(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        L, B, C, H, W = self.shape
        if out is None:
            out = np.empty(self.shape, dtype=np.uint8)
        buf, off, flags = self.buf.numpy(), self.slot_off.numpy(), self.slot_flags.numpy()
        flat = out.reshape((L * B, C, H, W))
        for i in range(L * B):
            if off[i] < 0:
                flat[i] = 0
            else:
                size = _blob_size(buf, int(off[i]), C * H * W)
                decode_frame_host(buf[int(off[i]):int(off[i]) + size], C, H, W, flip_channels=bool(flags[i] & FLAG_FLIP_CHANNELS), out=flat[i])
        return out


def _blob_size(buf: np.ndarray, off: int, E: int) -> int:
    n_masks, n_values = (int(v) for v in np.frombuffer(buf[off:off + 8].tobytes(), dtype='<u4'))
    return -(-(16 + 16 * n_groups(E) + 8 * n_masks + n_values) // 16) * 16


def assemble_packed(slots, L: int, frame_shape, pin_memory: bool = False) -> PackedBatch:
    """B ``PackedSlot`` (None: exhausted slot) -> the batch's byte buffer and slot table."""
    import torch
    B = len(slots)
    slots = [s if s is not None and s.blob is not None else None for s in slots]
    total = sum(s.blob.size for s in slots if s is not None)
    buf = torch.empty((max(total, 16),), dtype=torch.uint8, pin_memory=pin_memory)
    view = buf.numpy()
    slot_off = np.full((L, B), -1, dtype=np.int64)
    slot_flags = np.zeros((L, B), dtype=np.int32)
    pos = 0
    for b, s in enumerate(slots):
        if s is None:
            continue
        view[pos:pos + s.blob.size] = s.blob
        starts = s.offsets[:-1] + pos
        slot_off[s.pad_front:s.pad_front + s.n, b] = starts[::-1] if s.reverse else starts
        if s.reverse:
            slot_flags[s.pad_front:s.pad_front + s.n, b] = FLAG_FLIP_CHANNELS
        pos += s.blob.size
    if total < 16:
        view[:] = 0
    table = [torch.from_numpy(slot_off.reshape(-1)), torch.from_numpy(slot_flags.reshape(-1))]
    if pin_memory:                                              # the table goes up with the buffer, asynchronously
        table = [t.pin_memory() for t in table]
    return PackedBatch(buf, table[0], table[1], (L, B) + tuple(frame_shape))


def batch_to_device(packed_batch: PackedBatch, device):
    """-> the list of L [B,C,H,W] uint8 tensors on ``device`` that a dense batch gives: one upload of the byte buffer and the slot
    table, one ``ops.unpack_frames`` on the current stream; decoded on the host for a CPU target."""
    import torch
    device = torch.device(device)
    if device.type == 'cpu':
        ev = torch.from_numpy(packed_batch.decode_host())
    else:
        from leod_amd import ops
        L, B, C, H, W = packed_batch.shape
        buf = packed_batch.buf.to(device, non_blocking=True)
        off = packed_batch.slot_off.to(device, non_blocking=True)
        flags = packed_batch.slot_flags.to(device, non_blocking=True)
        ev = ops.unpack_frames(buf, off, flags, C, H, W, out=torch.empty(packed_batch.shape, dtype=torch.uint8, device=device))
    return [ev[t] for t in range(ev.shape[0])]
