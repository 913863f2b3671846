"""Motion-JPEG in an AVI container with the standard library: every frame is a complete JPEG file in a chunk of its own, the container a
few fixed headers and an index (the reference writes its prediction videos with an mp4 encoder on the host, vis_pred.py:216-227).

    with AviWriter('out.avi', width, height, fps) as avi:
        avi.append(jpeg_bytes)

    RIFF 'AVI '
      LIST 'hdrl'   avih (main header)   LIST 'strl'   strh (vids / MJPG)   strf (BITMAPINFOHEADER, compression MJPG, 24 bits)
      LIST 'movi'   00dc <jpeg> ...                  odd sizes padded to even; the chunk header keeps the true size
      idx1          one entry per frame: '00dc', AVIIF_KEYFRAME, offset from the 'movi' tag, size

Sizes and frame counts are patched on ``close``.  RIFF sizes are 32-bit: a file stays below ``limit`` bytes (1 GiB) and the writer goes on
in ``<stem>_001.avi``, ``<stem>_002.avi`` ...; ``paths`` lists what was written.  No OpenDML index, no audio."""
import os
import struct
from typing import List

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
_HEADERS = 12 + (12 + (8 + 56) + (12 + (8 + 56) + (8 + 40))) + 12         # bytes in front of the first frame chunk
_MOVI_TAG = _HEADERS - 4                                                  # position of the 'movi' tag: idx1 offsets count from here


class AviWriter:
    def __init__(self, path: str, width: int, height: int, fps: float, limit: int = 1 << 30):
        if not (0 < int(width) <= 65535 and 0 < int(height) <= 65535) or fps <= 0:
            raise ValueError(f'AviWriter: width {width}, height {height}, fps {fps}')
        self.path, self.width, self.height, self.fps, self.limit = str(path), int(width), int(height), fps, int(limit)
        # the frame rate as rate / scale: whole rates exactly, others to a thousandth
        self.scale, self.rate = (1, int(fps)) if float(fps).is_integer() else (1000, int(round(fps * 1000)))
        self.paths: List[str] = []
        self.frames = 0                                                   # over all files
        self._file = None
        self._open(self.path)

    def _open(self, path):
        self._file = open(path, 'wb')
        self.paths.append(path)
        self._index, self._pos, self._largest = [], _HEADERS, 0
        self._file.write(self._headers(0, 0, 0))

    def _headers(self, n, movi_bytes, idx_bytes):
        usec = int(round(1e6 * self.scale / self.rate))
        avih = struct.pack('<14I', usec, 0, 0, AVIF_HASINDEX, n, 0, 1, self._largest, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack('<4s4sIHHIIIIIIIIhhhh', b'vids', b'MJPG', 0, 0, 0, 0, self.scale, self.rate, 0, n, self._largest, 0xFFFFFFFF, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack('<IiiHH4sIiiII', 40, self.width, self.height, 1, 24, b'MJPG', self.width * self.height * 3, 0, 0, 0, 0)
        strl = b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh + b'strf' + struct.pack('<I', len(strf)) + strf
        hdrl = b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + b'LIST' + struct.pack('<I', len(strl)) + strl
        riff = 4 + (8 + len(hdrl)) + (8 + 4 + movi_bytes) + idx_bytes
        out = b'RIFF' + struct.pack('<I', riff) + b'AVI ' + b'LIST' + struct.pack('<I', len(hdrl)) + hdrl
        out += b'LIST' + struct.pack('<I', 4 + movi_bytes) + b'movi'
        assert len(out) == _HEADERS
        return out

    def append(self, jpeg: bytes) -> None:
        if self._file is None:
            raise ValueError('AviWriter: closed')
        data = bytes(jpeg)
        chunk = 8 + len(data) + (len(data) & 1)
        if _HEADERS + chunk + 8 + 16 > self.limit:
            raise ValueError(f'AviWriter: a frame of {len(data)} bytes does not fit a file of {self.limit}')
        if self._index and self._pos + chunk + 8 + 16 * (len(self._index) + 1) > self.limit:
            self._finish()
            stem, ext = os.path.splitext(self.path)
            self._open(f'{stem}_{len(self.paths):03d}{ext}')
        self._file.write(b'00dc' + struct.pack('<I', len(data)) + data + (b'\x00' if len(data) & 1 else b''))
        self._index.append((self._pos - _MOVI_TAG, len(data)))
        self._pos += chunk
        self._largest = max(self._largest, len(data))
        self.frames += 1

    def _finish(self):
        idx = b''.join(struct.pack('<4sIII', b'00dc', AVIIF_KEYFRAME, off, size) for off, size in self._index)
        self._file.write(b'idx1' + struct.pack('<I', len(idx)) + idx)
        self._file.seek(0)
        self._file.write(self._headers(len(self._index), self._pos - _HEADERS, 8 + len(idx)))
        self._file.close()
        self._file = None

    def close(self) -> None:
        if self._file is not None:
            self._finish()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def read_avi_frames(path: str) -> List[bytes]:
    """The inverse of ``AviWriter`` for one file it wrote: the frames in index order."""
    data = open(path, 'rb').read()
    if data[:4] != b'RIFF' or data[8:12] != b'AVI ' or data[_MOVI_TAG:_MOVI_TAG + 4] != b'movi':
        raise ValueError(f'{path}: not an AVI file of AviWriter')
    movi_bytes = struct.unpack('<I', data[_MOVI_TAG - 4:_MOVI_TAG])[0] - 4
    pos = _HEADERS + movi_bytes
    if data[pos:pos + 4] != b'idx1':
        raise ValueError(f'{path}: no index behind the frames')
    n = struct.unpack('<I', data[pos + 4:pos + 8])[0] // 16
    frames = []
    for k in range(n):
        tag, flags, off, size = struct.unpack('<4sIII', data[pos + 8 + 16 * k:pos + 24 + 16 * k])
        at = _MOVI_TAG + off
        if tag != b'00dc' or data[at:at + 4] != b'00dc' or struct.unpack('<I', data[at + 4:at + 8])[0] != size:
            raise ValueError(f'{path}: index entry {k} does not point at its frame')
        frames.append(data[at + 8:at + 8 + size])
    return frames
