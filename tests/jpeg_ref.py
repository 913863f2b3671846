"""Sequential restatement of the baseline JPEG stream of ``ops.encode_jpeg`` ("JPEG frames") in numpy and plain
Python, and a small baseline decoder for the streams it describes (Huffman decode, dequantisation, float IDCT), so that a machine without
an image library can still look into a frame.  Nothing here shares code with the library: the tables are written out again."""
import math
import struct

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# Annex K.1, natural (row-major) order
Q_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
Q_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# Annex K.3: (codes per length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

DCT = np.array([[int(round(8192 * (math.sqrt(1 / 8) if k == 0 else 0.5) * math.cos((2 * n + 1) * k * math.pi / 16))) for n in range(8)]
                for k in range(8)], dtype=np.int64)


def quant_tables(quality):
    """(luma, chroma) in natural order under the IJG quality rule."""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (Q_LUMA, Q_CHROMA))


def huff_codes(table):
    """symbol -> (code, length): codes of one length count upwards, the first code of the next length is twice the successor of the last."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack('>H', len(body) + 2) + bytes(body)


def header(H, W, quality):
    ql, qc = quant_tables(quality)
    out = b'\xFF\xD8' + _segment(0xE0, b'JFIF\x00\x01\x01\x00' + struct.pack('>HH', 1, 1) + b'\x00\x00')
    out += _segment(0xDB, [0] + [ql[z] for z in ZIGZAG]) + _segment(0xDB, [1] + [qc[z] for z in ZIGZAG])
    out += _segment(0xC0, struct.pack('>BHHB', 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, [tc_th] + bits + vals)
    out += _segment(0xDD, struct.pack('>H', (W + 7) // 8))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def ycc(rgb):
    """uint8 [H, W, 3] -> int64 [3, H, W]: the fixed-point conversion, clipped to 0 .. 255."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.clip(np.stack([y, cb, cr]), 0, 255)


def coefficients(rgb, quality):
    """uint8 [H, W, 3] -> quantised coefficients int64 [rows of blocks, blocks per row, 3, 64] in zigzag order."""
    H, W = rgb.shape[:2]
    by, bx = (H + 7) // 8, (W + 7) // 8
    planes = np.pad(ycc(rgb), ((0, 0), (0, 8 * by - H), (0, 8 * bx - W)), mode='edge') - 128
    x = planes.reshape(3, by, 8, bx, 8).transpose(1, 3, 0, 2, 4)             # [by, bx, 3, r, n]
    t = (np.einsum('kn,...rn->...rk', DCT, x) + 512) >> 10                   # rows: t[r][k]
    y = (np.einsum('kr,...rc->...kc', DCT, t) + 32768) >> 16                 # columns: y[k][c]
    q = np.array(quant_tables(quality), dtype=np.int64)[[0, 1, 1]].reshape(3, 8, 8)
    c = np.sign(y) * ((np.abs(y) + q // 2) // q)
    return c.reshape(by, bx, 3, 64)[..., ZIGZAG]


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(v):
    """(category, extra bits) of a non-zero-or-zero value: a negative one sends v - 1 in ``category`` bits."""
    cat = int(abs(v)).bit_length()
    return cat, (v if v >= 0 else v - 1) & ((1 << cat) - 1)


def encode(rgb, quality=90):
    """uint8 [H, W, 3] -> the bytes of one JFIF file."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W = rgb.shape[:2]
    coef = coefficients(rgb, quality)
    dc_t = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA), huff_codes(DC_CHROMA)]
    ac_t = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA), huff_codes(AC_CHROMA)]
    out = bytearray(header(H, W, quality))
    for row in range(coef.shape[0]):
        bits, pred = _Bits(), [0, 0, 0]
        for col in range(coef.shape[1]):
            for c in range(3):
                blk = coef[row, col, c]
                cat, extra = _magnitude(int(blk[0]) - pred[c])
                pred[c] = int(blk[0])
                bits.put(*dc_t[c][cat])
                bits.put(extra, cat)
                last = 0
                for k in np.flatnonzero(blk[1:]) + 1:
                    run = int(k) - last - 1
                    while run > 15:
                        bits.put(*ac_t[c][0xF0])
                        run -= 16
                    cat, extra = _magnitude(int(blk[k]))
                    bits.put(*ac_t[c][run << 4 | cat])
                    bits.put(extra, cat)
                    last = int(k)
                if last != 63:
                    bits.put(*ac_t[c][0x00])
        bits.pad()
        out += bits.out
        if row + 1 < coef.shape[0]:
            out += bytes([0xFF, 0xD0 + row % 8])
    return bytes(out + b'\xFF\xD9')


def encode_many(frames, quality=90):
    """uint8 [N, H, W, 3] -> (blob uint8, offsets int64 [N + 1]) as ``ops.encode_jpeg`` returns them."""
    files = [encode(f, quality) for f in np.asarray(frames)]
    return np.frombuffer(b''.join(files), dtype=np.uint8), np.cumsum([0] + [len(f) for f in files]).astype(np.int64)


# ---- a baseline decoder for such streams ----------------------------------------------------------------------------------------------
def _idct_basis():
    k, n = np.arange(8).reshape(8, 1), np.arange(8).reshape(1, 8)
    return np.where(k == 0, math.sqrt(1 / 8), 0.5) * np.cos((2 * n + 1) * k * math.pi / 16)


def decode(data):
    """One baseline JFIF file, three components 1x1 (any tables, restart intervals of whole rows or none) -> uint8 [H, W, 3] RGB.
    Float IDCT, values rounded half up and clipped; the colour conversion is JFIF's, in floats."""
    data = bytes(data)
    assert data[:2] == b'\xFF\xD8', 'no SOI'
    pos, qt, ht, dri = 2, {}, {}, 0
    while True:
        assert data[pos] == 0xFF, f'marker expected at {pos}'
        marker, n = data[pos + 1], struct.unpack('>H', data[pos + 2:pos + 4])[0]
        seg = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if marker == 0xDB:
            while seg:
                assert seg[0] >> 4 == 0, '8-bit tables only'
                qt[seg[0] & 15], seg = np.array(list(seg[1:65]), dtype=np.float64), seg[65:]
        elif marker == 0xC0:
            depth, H, W, nc = struct.unpack('>BHHB', seg[:6])
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i], seg[8 + 3 * i]) for i in range(nc)]
            assert depth == 8 and nc == 3 and all(c[1] == 0x11 for c in comps), 'three 8-bit components, 1x1 each'
        elif marker == 0xC4:
            while seg:
                bits, k = list(seg[1:17]), sum(seg[1:17])
                ht[seg[0]] = {(length, code): sym for sym, (code, length) in huff_codes((bits, list(seg[17:17 + k]))).items()}
                seg = seg[17 + k:]
        elif marker == 0xDD:
            dri = struct.unpack('>H', seg)[0]
        elif marker == 0xDA:
            scan = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])]
            break
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, f'marker {marker:#x}'
    by, bx = (H + 7) // 8, (W + 7) // 8
    assert dri in (0, bx), 'restart interval of one row of blocks'
    coef = np.zeros((by, bx, 3, 64), dtype=np.float64)
    state = {'pos': pos, 'acc': 0, 'n': 0}

    def bit():
        if state['n'] == 0:
            b = data[state['pos']]
            state['pos'] += 1
            if b == 0xFF:
                assert data[state['pos']] == 0, 'marker inside an interval'
                state['pos'] += 1
            state['acc'], state['n'] = b, 8
        state['n'] -= 1
        return (state['acc'] >> state['n']) & 1

    def symbol(table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | bit()
            if (length, code) in table:
                return table[(length, code)]
        raise AssertionError('no such code')

    def value(cat):
        v = 0
        for _ in range(cat):
            v = v << 1 | bit()
        return v if cat == 0 or v >> (cat - 1) else v - (1 << cat) + 1

    pred = [0, 0, 0]
    for row in range(by):
        for col in range(bx):
            for c, (_, td, ta) in enumerate(scan):
                pred[c] += value(symbol(ht[td]))
                coef[row, col, c, 0] = pred[c]
                k = 1
                while k < 64:
                    rs = symbol(ht[0x10 | ta])
                    if rs == 0:
                        break
                    k += rs >> 4
                    if rs & 15:
                        coef[row, col, c, k] = value(rs & 15)
                    k += 1
        if dri and row + 1 < by:
            state['n'], pred = 0, [0, 0, 0]
            assert data[state['pos']:state['pos'] + 2] == bytes([0xFF, 0xD0 + row % 8]), f'RST{row % 8} expected after row {row}'
            state['pos'] += 2
    assert data[state['pos']:state['pos'] + 2] == b'\xFF\xD9' and state['pos'] + 2 == len(data), 'EOI expected at the end'
    tq = np.stack([qt[comps[c][2]] for c in range(3)])
    nat = np.zeros_like(coef)
    nat[..., ZIGZAG] = coef * tq
    B = _idct_basis()
    pix = np.einsum('ky,...kl,lx->...yx', B, nat.reshape(by, bx, 3, 8, 8), B) + 128.0
    planes = pix.transpose(2, 0, 3, 1, 4).reshape(3, 8 * by, 8 * bx)[:, :H, :W]
    planes = np.clip(np.floor(planes + 0.5), 0, 255)
    y, cb, cr = planes[0], planes[1] - 128.0, planes[2] - 128.0
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)
