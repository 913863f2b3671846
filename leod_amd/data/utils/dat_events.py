"""Raw Prophesee ``.dat`` event recordings (Event2D) as they come from the sensor toolchain: the text header, the 8-byte records and
the cut into windows of fixed duration (record layout: the reference's utils/evaluation/prophesee/io/dat_events_tools.py:18-50,120-175).

    % <comment lines, among them "% Height H" and "% Width W">
    <u8 event type = 0> <u8 event size = 8>
    n x { u32 t [microseconds], i32: x in bits 0-13, y in bits 14-27, p in bit 28 }        little endian

The records are never decoded on the host on the ingestion path: they are memory-mapped and go to the device as bytes
(``ops.voxelize_dat_windows``).  ``decode`` exists for tests and small tools."""
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np

EVENT_TYPE_2D = 0
EVENT_SIZE = 8


class DatHeader(NamedTuple):
    data_offset: int                 # byte offset of the first record
    height: Optional[int]
    width: Optional[int]
    n_events: int


def parse_header(fn: str) -> DatHeader:
    """Header of a .dat file.  Only Event2D records of 8 bytes are accepted; anything else raises ``ValueError`` naming the file."""
    size = os.path.getsize(fn)
    height = width = None
    with open(fn, 'rb') as f:
        n_comment = 0
        while True:
            pos = f.tell()
            line = f.readline()
            if line[:2] != b'% ':
                break
            n_comment += 1
            words = line.split()
            if len(words) > 2 and words[1] in (b'Height', b'Width'):
                try:
                    value = int(words[2])
                except ValueError:
                    raise ValueError(f'{fn}: header line {line!r} holds no integer') from None
                if words[1] == b'Height':
                    height = value
                else:
                    width = value
        f.seek(pos)
        if n_comment > 0:
            tb = f.read(2)
            if len(tb) != 2:
                raise ValueError(f'{fn}: the file ends inside its header')
            ev_type, ev_size = tb[0], tb[1]
            if ev_type != EVENT_TYPE_2D or ev_size != EVENT_SIZE:
                raise ValueError(f'{fn}: event type {ev_type} with {ev_size}-byte records; only Event2D (type {EVENT_TYPE_2D}, '
                                 f'{EVENT_SIZE} bytes) is supported')
        data_offset = f.tell()               # a file without comment lines is bare records (dat_events_tools.py:165-172)
    if (size - data_offset) % EVENT_SIZE:
        raise ValueError(f'{fn}: {size - data_offset} bytes of records are no whole number of {EVENT_SIZE}-byte events')
    return DatHeader(data_offset, height, width, (size - data_offset) // EVENT_SIZE)


def open_records(fn: str) -> Tuple[DatHeader, np.ndarray]:
    """(header, records): the records as a read-only memory map [n, 2] of little-endian u32 -- column 0 is t, column 1 the packed x / y / p."""
    hdr = parse_header(fn)
    if hdr.n_events == 0:
        return hdr, np.zeros((0, 2), dtype='<u4')
    return hdr, np.memmap(fn, dtype='<u4', mode='r', offset=hdr.data_offset, shape=(hdr.n_events, 2))


def decode(records: np.ndarray):
    """records [n, 2] u32 -> (t, x, y, p) as int64 arrays."""
    t = records[:, 0].astype(np.int64)
    w = records[:, 1].astype(np.int64)
    return t, w & 16383, (w >> 14) & 16383, (w >> 28) & 1


def encode(t, x, y, p) -> np.ndarray:
    """(t, x, y, p) -> records [n, 2] u32, the inverse of ``decode`` (writers of test recordings)."""
    t, x, y, p = (np.asarray(a, dtype=np.int64) for a in (t, x, y, p))
    assert t.min(initial=0) >= 0 and t.max(initial=0) < 2 ** 32 and x.min(initial=0) >= 0 and x.max(initial=0) < 2 ** 14
    assert y.min(initial=0) >= 0 and y.max(initial=0) < 2 ** 14 and p.min(initial=0) >= 0 and p.max(initial=0) <= 1
    return np.stack([t, x | (y << 14) | (p << 28)], axis=1).astype('<u4')


def write_dat(fn: str, records: np.ndarray, height: int, width: int) -> None:
    with open(fn, 'wb') as f:
        f.write(b'% Data file containing Event2D events.\n% Version 2\n')
        f.write(f'% Height {height}\n% Width {width}\n'.encode('ascii'))
        f.write(bytes([EVENT_TYPE_2D, EVENT_SIZE]))
        f.write(np.ascontiguousarray(records, dtype='<u4').tobytes())


def check_sorted(t: np.ndarray, what: str = 'events') -> None:
    """``ValueError`` unless t is non-decreasing."""
    t = np.asarray(t)
    if len(t) > 1:
        bad = np.flatnonzero(t[1:] < t[:-1])
        if len(bad):
            i = int(bad[0])
            raise ValueError(f'{what}: timestamps decrease at event {i + 1} ({int(t[i])} -> {int(t[i + 1])}); a recording must be sorted in time')


def num_windows(t_last: int, duration_us: int) -> int:
    """N = max(ceil(t_last / D), 1): the frame that holds the last event is the last frame."""
    return max(-(-int(t_last) // int(duration_us)), 1)


def window_offsets(t: np.ndarray, duration_us: int, n_windows: Optional[int] = None) -> np.ndarray:
    """Event offsets [N + 1] of the windows of a time-sorted recording: frame k holds the events with k*D < t <= (k+1)*D, events at t = 0
    belong to frame 0.  ``n_windows`` None: ``num_windows(t[-1], D)`` (1 for an empty recording)."""
    t = np.asarray(t)
    if n_windows is None:
        n_windows = num_windows(t[-1] if len(t) else 0, duration_us)
    edges = (np.arange(1, n_windows + 1, dtype=np.int64) * int(duration_us))
    off = np.zeros(n_windows + 1, dtype=np.int64)
    off[1:] = np.searchsorted(t.astype(np.int64, copy=False), edges, side='right')
    return off


def scan_windows(records: np.ndarray, duration_us: int, what: str = 'events', block: int = 1 << 22) -> np.ndarray:
    """``check_sorted`` + ``window_offsets`` over the t column of memory-mapped records, ``block`` events at a time (nothing of the size of the
    recording is materialised)."""
    n = len(records)
    n_windows = num_windows(records[n - 1, 0] if n else 0, duration_us)
    off = np.zeros(n_windows + 1, dtype=np.int64)
    prev = None
    for a in range(0, n, block):
        t = np.ascontiguousarray(records[a:a + block, 0])
        if prev is not None and int(t[0]) < prev:
            raise ValueError(f'{what}: timestamps decrease at event {a} ({prev} -> {int(t[0])}); a recording must be sorted in time')
        try:
            check_sorted(t, what)
        except ValueError as e:
            raise ValueError(f'{e} [block starting at event {a}]') from None
        prev = int(t[-1])
        off += window_offsets(t, duration_us, n_windows)
    return off
