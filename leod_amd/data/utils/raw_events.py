"""Metavision ``.raw`` recordings (EVT2 / EVT3), the counterpart of ``dat_events.py``: the text header, the payload as a memory map, a
plain sequential decoder for tools, and encoders that write test recordings.  No reader or sample file of these formats ships with the
reference; the layout below is the published Prophesee one as this project reads it (DESIGN.md section 1 lists it with the project's
own rules where the format leaves room), and the decoders are pinned against this project's own sequential restatement only.

    % <ASCII lines "% key value">, among them "% evt 3.0" or "% format EVT3;height=H;width=W", "% geometry WxH", then "% end"
      (older files have no "% end": the header ends before the first byte that does not begin such a line)
    EVT2: little-endian u32 words, type in bits 31:28         EVT3: little-endian u16 words, type in bits 15:12

On the ingestion path the payload is never decoded on the host: it goes to the device as bytes (``ops.decode_evt``)."""
import os
import re
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np

WORD_BYTES = {'evt2': 4, 'evt3': 2}
WORD_DTYPE = {'evt2': '<u4', 'evt3': '<u2'}
TIME_SHIFT = {'evt2': 6, 'evt3': 12}                             # the time base of a file is its first TIME_HIGH << this
WRAP_DROP = 2048                                                 # an EVT3 TIME_HIGH lower than the previous one by this much is a clock wrap
HIGH_STEP = 1024                                                 # the encoder lets TIME_HIGH rise by at most this much per word


class RawHeader(NamedTuple):
    encoding: str                    # 'evt2' | 'evt3'
    data_offset: int
    height: Optional[int]
    width: Optional[int]


def parse_header(fn: str) -> RawHeader:
    """Header of a .raw file -> (encoding, data offset, height, width).  ``ValueError`` naming the file for: no recognisable encoding, any
    encoding but EVT2 / EVT3 (``evt 2.1`` among them), a payload that is no whole number of words."""
    size = os.path.getsize(fn)
    found, height, width = [], None, None
    with open(fn, 'rb') as f:
        while True:
            pos = f.tell()
            line = f.readline()
            if line[:2] != b'% ':
                f.seek(pos)
                break
            words = line[2:].decode('ascii', 'replace').split()
            if not words:
                continue
            if words[0] == 'end':
                break
            if words[0] == 'evt' and len(words) > 1:
                found.append('evt' + {'2.0': '2', '3.0': '3'}.get(words[1], ' ' + words[1]))
            elif words[0] == 'format' and len(words) > 1:
                parts = words[1].split(';')
                found.append(parts[0].lower() if parts[0] in ('EVT2', 'EVT3') else 'format ' + parts[0])
                for part in parts[1:]:
                    m = re.fullmatch(r'(height|width)=(\d+)', part)
                    if m and m.group(1) == 'height':
                        height = int(m.group(2))
                    elif m:
                        width = int(m.group(2))
            elif words[0] == 'geometry' and len(words) > 1:
                m = re.fullmatch(r'(\d+)x(\d+)', words[1])
                if not m:
                    raise ValueError(f'{fn}: header line {line!r} holds no geometry WxH')
                width, height = int(m.group(1)), int(m.group(2))
        data_offset = f.tell()
    if not found:
        raise ValueError(f'{fn}: the header names no encoding ("% evt 2.0", "% evt 3.0", "% format EVT2" or "% format EVT3")')
    if len(set(found)) > 1 or found[0] not in WORD_BYTES:
        raise ValueError(f'{fn}: encoding {" / ".join(sorted(set(found)))}; only EVT2 (evt 2.0) and EVT3 (evt 3.0) are supported')
    enc = found[0]
    if (size - data_offset) % WORD_BYTES[enc]:
        raise ValueError(f'{fn}: {size - data_offset} bytes of payload are no whole number of {WORD_BYTES[enc]}-byte {enc.upper()} words')
    return RawHeader(enc, data_offset, height, width)


def open_words(fn: str) -> Tuple[RawHeader, np.ndarray]:
    """(header, payload): the payload as a read-only memory map of bytes."""
    hdr = parse_header(fn)
    if os.path.getsize(fn) == hdr.data_offset:
        return hdr, np.zeros((0,), dtype=np.uint8)
    return hdr, np.memmap(fn, dtype=np.uint8, mode='r', offset=hdr.data_offset)


def write_raw(fn: str, words: np.ndarray, encoding: str, height: Optional[int] = None, width: Optional[int] = None, style: str = 'format',
              end: bool = True) -> None:
    """Writes a .raw file.  ``style`` 'format': "% format EVT3;height=H;width=W"; 'evt': "% evt 3.0" and "% geometry WxH"."""
    n = encoding[-1]
    with open(fn, 'wb') as f:
        f.write(b'% date 2024-01-01 00:00:00\n')
        geometry = height is not None and width is not None
        if style == 'format':
            f.write(f'% format EVT{n}{f";height={height};width={width}" if geometry else ""}\n'.encode('ascii'))
        else:
            f.write(f'% evt {n}.0\n'.encode('ascii'))
            if geometry:
                f.write(f'% geometry {width}x{height}\n'.encode('ascii'))
        if end:
            f.write(b'% end\n')
        f.write(np.ascontiguousarray(words, dtype=WORD_DTYPE[encoding]).tobytes())


def _events(t, x, y, p, shift, first_time_high):
    t, x, y, p = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (t, x, y, p))
    assert len(t) == len(x) == len(y) == len(p)
    assert t.min(initial=0) >= 0 and (np.diff(t) >= 0).all(), 'the encoders take events sorted in time'
    assert x.min(initial=0) >= 0 and x.max(initial=0) < 2048 and y.min(initial=0) >= 0 and y.max(initial=0) < 2048
    assert p.min(initial=0) >= 0 and p.max(initial=0) <= 1 and first_time_high >= 0
    return t + (int(first_time_high) << shift), x, y, p


def _excl(a):
    return np.cumsum(a) - a


def encode_evt2(t, x, y, p, first_time_high: int = 0, high_period: int = 64) -> np.ndarray:
    """(t, x, y, p), sorted in time -> EVT2 words (u32).  The stream opens with EVT_TIME_HIGH = ``first_time_high`` (so the decoded,
    shifted times are ``t`` again); TIME_HIGH is written where it changes and again before every ``high_period``-th event."""
    a, x, y, p = _events(t, x, y, p, 6, first_time_high)
    n = len(a)
    hi = a >> 6
    assert hi.max(initial=0) < 1 << 28, 'the time does not fit 28 + 6 bits'
    prev = np.concatenate([[first_time_high], hi[:-1]])
    th = (hi != prev) | (np.arange(n) % max(int(high_period), 1) == 0)
    pos = 1 + _excl(th + 1)
    out = np.zeros(1 + int((th + 1).sum()), dtype=np.int64)
    out[0] = (0x8 << 28) | first_time_high
    out[pos[th]] = (0x8 << 28) | hi[th]
    out[pos + th] = (p << 28) | ((a & 63) << 22) | (x << 11) | y
    return out.astype('<u4')


def encode_evt3(t, x, y, p, first_time_high: int = 0, vectors: bool = False, high_period: int = 64) -> np.ndarray:
    """(t, x, y, p), sorted in time -> EVT3 words (u16).  The stream opens with EVT_TIME_HIGH = ``first_time_high`` (< 4096; the decoded,
    shifted times are ``t`` again).  TIME_HIGH is written where it changes -- in steps of at most 1024, so that a pause never looks like a
    wrap of the 24-bit clock -- and again before every ``high_period``-th group of events, as cameras repeat it; TIME_LOW and ADDR_Y where
    they change.  ``vectors``: wherever two or more consecutive events share t, y and p with ascending x inside 12 columns they are written
    as VECT_BASE_X + VECT_12 (VECT_8 where 8 columns do); every other event is an ADDR_X."""
    a, x, y, p = _events(t, x, y, p, 12, first_time_high)
    assert first_time_high < 4096
    n = len(a)
    if n == 0:
        return np.array([0x8000 | first_time_high], dtype='<u2')
    start = np.ones(n, dtype=bool)
    if vectors and n > 1:
        same = (a[1:] == a[:-1]) & (y[1:] == y[:-1]) & (p[1:] == p[:-1]) & (x[1:] > x[:-1])
        start[1:] = ~same
        b = 0
        for i in np.flatnonzero(same) + 1:                       # greedy cut where a run leaves the 12 columns of its first event
            if start[i - 1]:
                b = i - 1
            if x[i] - x[b] >= 12:
                start[i] = True
    gs = np.flatnonzero(start)
    G = len(gs)
    size = np.diff(np.concatenate([gs, [n]]))
    gid = np.repeat(np.arange(G), size)
    mask = np.bitwise_or.reduceat(np.int64(1) << (x - x[gs][gid]), gs)
    vect = size > 1
    hi, lo, gy = a[gs] >> 12, a[gs] & 4095, y[gs]
    hi_prev = np.concatenate([[first_time_high], hi[:-1]])
    gap = hi - hi_prev
    k = np.where(gap > 0, -(-gap // HIGH_STEP), (np.arange(G) % max(int(high_period), 1) == 0).astype(np.int64))
    first = np.arange(G) == 0
    tl = first | (lo != np.concatenate([[0], lo[:-1]])) | (gap > 0)
    wy = first | (gy != np.concatenate([[0], gy[:-1]]))
    cnt = k + tl + wy + 1 + vect
    pos = 1 + _excl(cnt)
    out = np.zeros(1 + int(cnt.sum()), dtype=np.int64)
    out[0] = 0x8000 | first_time_high
    rep = np.repeat(np.arange(G), k)
    j = np.arange(len(rep)) - np.repeat(_excl(k), k)
    out[pos[rep] + j] = 0x8000 | (np.where(j == k[rep] - 1, hi[rep], hi_prev[rep] + HIGH_STEP * (j + 1)) & 4095)
    out[(pos + k)[tl]] = 0x6000 | lo[tl]
    out[(pos + k + tl)[wy]] = gy[wy]
    last = pos + k + tl + wy
    single = ~vect
    out[last[single]] = 0x2000 | (p[gs][single] << 11) | x[gs][single]
    out[last[vect]] = 0x3000 | (p[gs][vect] << 11) | x[gs][vect]
    wide = mask >= 256
    out[last[vect & wide] + 1] = 0x4000 | mask[vect & wide]
    out[last[vect & ~wide] + 1] = 0x5000 | mask[vect & ~wide]
    return out.astype('<u2')


# ---- the decoder as a scan: the algebra of csrc/k_evt.hip restated on the host (tests combine it in random order) ------------------------
# A transform is what a run of words does to the decoder state: dict(set = bits of the fields it writes (1 time high, 2 time low, 4 row,
# 8 vector base), low, y, vpol = their last values, first / last / wraps = its first and last TIME_HIGH and the clock wraps between them,
# base = the vector base after the run if it sets one, else the columns it adds).  A state is the transform of everything read so far.
F_HIGH, F_LOW, F_Y, F_BASE = 1, 2, 4, 8
IDENTITY = dict(set=0, low=0, y=0, vpol=0, first=0, last=0, wraps=0, base=0)


def word_transform(w: int, encoding: str) -> dict:
    o = dict(IDENTITY)
    if encoding == 'evt2':
        if w >> 28 == 0x8:
            o.update(set=F_HIGH, first=w & 0x0fffffff, last=w & 0x0fffffff)
        return o
    ty, v = w >> 12, w & 4095
    if ty == 0x8:
        o.update(set=F_HIGH, first=v, last=v)
    elif ty == 0x6:
        o.update(set=F_LOW, low=v)
    elif ty == 0x0:
        o.update(set=F_Y, y=v & 2047)
    elif ty == 0x3:
        o.update(set=F_BASE, base=v & 2047, vpol=v >> 11)
    elif ty in (0x4, 0x5):
        o.update(base=12 if ty == 0x4 else 8)
    return o


def compose(l: dict, r: dict, encoding: str) -> dict:
    """``l`` then ``r``.  Associative."""
    o = dict(set=l['set'] | r['set'])
    o['low'] = r['low'] if r['set'] & F_LOW else l['low']
    o['y'] = r['y'] if r['set'] & F_Y else l['y']
    o['vpol'] = r['vpol'] if r['set'] & F_BASE else l['vpol']
    o['base'] = r['base'] if r['set'] & F_BASE else l['base'] + r['base']
    if not r['set'] & F_HIGH:
        o.update(first=l['first'], last=l['last'], wraps=l['wraps'])
    elif not l['set'] & F_HIGH:
        o.update(first=r['first'], last=r['last'], wraps=r['wraps'])
    else:
        wrap = encoding == 'evt3' and l['last'] - r['first'] >= WRAP_DROP
        o.update(first=l['first'], last=r['last'], wraps=l['wraps'] + r['wraps'] + int(wrap))
    return o


def decode(words: np.ndarray, encoding: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, Dict[str, int]]:
    """Plain sequential host decoder (tools and small files; one Python step per word): words -> (t, x, y, p, counters) by the rules of
    DESIGN.md section 1.  t is shifted by the file's first TIME_HIGH and not reduced to 32 bits; ``overflow`` counts as on the device."""
    words = np.asarray(words)
    words = (words.view(WORD_DTYPE[encoding]) if words.dtype == np.uint8 else words).reshape(-1).astype(np.int64)      # payload bytes or words
    evt3 = encoding == 'evt3'
    high = low = row = base = vpol = None
    wraps = time_base = 0
    c = dict(events=0, early_events=0, ignored_words=0, unknown_words=0, overflow=0, wraps=0)
    ev = []

    def emit(tt, xs, yy, pol, ready):
        if not ready:
            c['early_events'] += len(xs)
            return
        tt -= time_base
        if not 0 <= tt < 1 << 32:
            c['overflow'] = 1
        ev.extend((tt, xx & 16383, yy, pol) for xx in xs)

    for w in words.tolist():
        ty = w >> (12 if evt3 else 28)
        if ty == 0x8:
            v = w & (4095 if evt3 else (1 << 28) - 1)
            if high is None:
                time_base = v << TIME_SHIFT[encoding]
            elif evt3 and high - v >= WRAP_DROP:
                wraps += 1
            high = v
        elif ty in (0xA, 0xE, 0xF) or (evt3 and ty == 0x7):
            c['ignored_words'] += 1
        elif not evt3:
            if ty <= 1:
                emit(((high or 0) << 6) | ((w >> 22) & 63), [(w >> 11) & 2047], w & 2047, ty, high is not None)
            else:
                c['unknown_words'] += 1
        elif ty == 0x6:
            low = w & 4095
        elif ty == 0x0:
            row = w & 2047
        elif ty == 0x3:
            base, vpol = w & 2047, (w >> 11) & 1
        elif ty in (0x2, 0x4, 0x5):
            ready = None not in (high, low, row)
            tt = (((wraps * 4096 + high) << 12) | low) if ready else 0
            if ty == 0x2:
                emit(tt, [w & 2047], row, (w >> 11) & 1, ready)
            else:
                bits = [i for i in range(12 if ty == 0x4 else 8) if (w >> i) & 1]
                emit(tt, [(base or 0) + i for i in bits], row, vpol, ready and base is not None)
                if base is not None:
                    base += 12 if ty == 0x4 else 8
        else:
            c['unknown_words'] += 1
    c['events'], c['wraps'] = len(ev), wraps
    cols = np.array(ev, dtype=np.int64).reshape(-1, 4)
    return cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3], c
