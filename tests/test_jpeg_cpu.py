"""The JPEG stream of ``ops.encode_jpeg`` as tests/jpeg_ref.py restates it, judged without a GPU: libjpeg (through Pillow) opens every
restated stream and is no better an encoder at the same tables; the small decoder of jpeg_ref.py agrees with libjpeg's; and the
Motion-JPEG container of leod_amd/utils/mjpeg.py is what its structure says it is."""
import io
import os
import struct

import numpy as np
import pytest

import jpeg_ref as jr
from leod_amd.utils.mjpeg import AviWriter, read_avi_frames

SIZES = [(8, 8), (16, 21), (24, 37), (64, 77)]
QUALITIES = [50, 90, 100]


def speckle(h, w, seed):
    """What the renderer's frames look like: white, 10 % dark speckle, a green and a red one-pixel line."""
    rng = np.random.RandomState(seed)
    a = np.full((h, w, 3), 255, dtype=np.uint8)
    a[rng.rand(h, w) < 0.1] = 64
    a[h // 3, :] = (0, 255, 0)
    a[:, w // 2] = (255, 0, 0)
    return a


def psnr(a, b):
    mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.fixture(scope='module')
def streams():
    """(h, w, quality) -> (image, restated stream), encoded once."""
    out = {}
    for q in QUALITIES:
        for h, w in SIZES:
            img = speckle(h, w, 1000 * q + h * w)
            out[h, w, q] = (img, jr.encode(img, q))
    return out


def test_fidelity_against_libjpeg(streams):
    Image = pytest.importorskip('PIL.Image')
    worst, ratios = 0.0, []
    for (h, w, q), (img, data) in streams.items():
        opened = Image.open(io.BytesIO(data))
        assert opened.size == (w, h) and opened.mode == 'RGB' and opened.format == 'JPEG'
        ours = psnr(img, np.asarray(opened.convert('RGB')))
        ql, qc = jr.quant_tables(q)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', qtables=[[ql[z] for z in jr.ZIGZAG], [qc[z] for z in jr.ZIGZAG]], subsampling=0)
        theirs = psnr(img, np.asarray(Image.open(buf).convert('RGB')))
        ratios.append(len(data) / len(buf.getvalue()))
        print(f'{h}x{w} q{q}: {len(data)} bytes, {ours:.2f} dB; libjpeg {len(buf.getvalue())} bytes, {theirs:.2f} dB')
        worst = max(worst, theirs - ours)
        # Measured on these inputs: the worst deficit is 1.58 dB (8 x 8 at quality 100: 53.26 dB against libjpeg's 54.84 dB; every
        # quantiser is 1 there and the rounding of the fixed-point DCT is all that is left), the best lead 0.40 dB.  The margin is the
        # worst deficit plus 0.5 dB.  A deficit above 3 dB would mean a wrong transform, not a margin to widen.
        assert ours >= theirs - (1.58 + 0.5), (h, w, q, ours, theirs)
    print(f'worst deficit {worst:.3f} dB')
    assert worst < 3.0
    assert 0.95 < min(ratios) and max(ratios) < 1.05                       # the same tables and no optimised codes on either side


def test_own_decoder_agrees_with_libjpeg(streams):
    Image = pytest.importorskip('PIL.Image')
    cases = dict(streams)
    noise = np.random.RandomState(7).randint(0, 256, size=(40, 50, 3)).astype(np.uint8)
    for q in (1, 100):
        cases[40, 50, q] = (noise, jr.encode(noise, q))
    worst = 0
    for (h, w, q), (img, data) in cases.items():
        mine = jr.decode(data)
        theirs = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
        assert mine.shape == theirs.shape == (h, w, 3)
        worst = max(worst, int(np.abs(mine.astype(np.int64) - theirs).max()))
    # libjpeg's integer IDCT and colour conversion against floats: 2 levels at the most were observed on these streams
    assert worst <= 2, worst


def test_own_decoder_returns_the_picture():
    """Without Pillow: the restated stream decodes, at quality 100, to within the rounding of transform and colour conversion."""
    img = speckle(24, 37, 5)
    back = jr.decode(jr.encode(img, 100))
    assert back.shape == img.shape and psnr(img, back) > 45 and int(np.abs(back.astype(np.int64) - img).max()) <= 6
    flat = np.full((9, 20, 3), 255, dtype=np.uint8)
    assert np.array_equal(jr.decode(jr.encode(flat, 90)), flat)


def test_stream_layout():
    data = jr.encode(speckle(20, 21, 3), 90)
    markers, pos = [], 2
    assert data[:2] == b'\xFF\xD8'
    while data[pos + 1] != 0xDA:
        markers.append(data[pos + 1])
        pos += 2 + struct.unpack('>H', data[pos + 2:pos + 4])[0]
    assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD]
    assert data[6:11] == b'JFIF\x00' and data[11:13] == b'\x01\x01' and data[13:18] == b'\x00\x00\x01\x00\x01'
    scan = data[pos + 2 + struct.unpack('>H', data[pos + 2:pos + 4])[0]:]
    rst = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert rst == [0xD0, 0xD1] and scan[-2:] == b'\xFF\xD9'                # three rows of blocks: RST0, RST1, none behind the last
    ql, qc = jr.quant_tables(90)
    assert (ql[0], ql[63], qc[0]) == (3, 20, 3) and jr.quant_tables(100) == ([1] * 64, [1] * 64) and max(jr.quant_tables(1)[0]) == 255


def chunks(data, pos, end):
    """(tag, body position, size) of the RIFF chunks in data[pos:end]"""
    out = []
    while pos < end:
        tag, size = data[pos:pos + 4], struct.unpack('<I', data[pos + 4:pos + 8])[0]
        out.append((tag, pos + 8, size))
        pos += 8 + size + (size & 1)
    assert pos == end, 'chunks do not fill their list'
    return out


def check_avi(path, frames, width, height, fps):
    data = open(path, 'rb').read()
    assert data[:4] == b'RIFF' and struct.unpack('<I', data[4:8])[0] == len(data) - 8 and data[8:12] == b'AVI '
    top = chunks(data, 12, len(data))
    assert [(t, data[p:p + 4]) if t == b'LIST' else (t, None) for t, p, _ in top] == [(b'LIST', b'hdrl'), (b'LIST', b'movi'), (b'idx1', None)]
    (_, hdrl, hdrl_size), (_, movi, movi_size), (_, idx, idx_size) = top
    h = chunks(data, hdrl + 4, hdrl + hdrl_size)
    assert [t for t, _, _ in h] == [b'avih', b'LIST'] and h[0][2] == 56 and data[h[1][1]:h[1][1] + 4] == b'strl'
    avih = struct.unpack('<14I', data[h[0][1]:h[0][1] + 56])
    assert avih[0] == round(1e6 / fps) and avih[3] & 0x10 and avih[4] == len(frames) and avih[6] == 1 and avih[8:10] == (width, height)
    s = chunks(data, h[1][1] + 4, h[1][1] + h[1][2])
    assert [(t, n) for t, _, n in s] == [(b'strh', 56), (b'strf', 40)]
    strh = struct.unpack('<4s4sIHHIIIIIIIIhhhh', data[s[0][1]:s[0][1] + 56])
    assert strh[:2] == (b'vids', b'MJPG') and strh[7] / strh[6] == fps and strh[9] == len(frames) and strh[-2:] == (width, height)
    strf = struct.unpack('<IiiHH4sIiiII', data[s[1][1]:s[1][1] + 40])
    assert strf[:6] == (40, width, height, 1, 24, b'MJPG')
    m = chunks(data, movi + 4, movi + movi_size)
    assert [t for t, _, _ in m] == [b'00dc'] * len(frames) and [n for _, _, n in m] == [len(f) for f in frames]
    assert idx_size == 16 * len(frames)
    for k, f in enumerate(frames):
        tag, flags, off, size = struct.unpack('<4sIII', data[idx + 16 * k:idx + 16 * k + 16])
        at = movi + off                                                   # offsets count from the 'movi' tag
        assert (tag, flags, size) == (b'00dc', 0x10, len(f)) and data[at:at + 4] == b'00dc'
        assert struct.unpack('<I', data[at + 4:at + 8])[0] == size and data[at + 8:at + 8 + size] == f
        if size & 1:
            assert data[at + 8 + size] == 0
    assert max(avih[7], strh[10]) == max(len(f) for f in frames)


def test_avi_round_trip_and_structure(tmp_path):
    rng = np.random.RandomState(0)
    frames = [jr.encode(speckle(16, 21, k), 90) for k in range(3)]
    frames += [bytes(rng.randint(0, 256, size=n).astype(np.uint8)) for n in (1, 2, 333, 1000)]      # the writer does not look inside
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)
    path = str(tmp_path / 'a.avi')
    with AviWriter(path, 21, 16, 15) as avi:
        for f in frames:
            avi.append(f)
    assert avi.paths == [path] and avi.frames == len(frames)
    assert read_avi_frames(path) == frames
    check_avi(path, frames, 21, 16, 15)
    with pytest.raises(ValueError):
        avi.append(frames[0])                                             # closed
    w = AviWriter(str(tmp_path / 'b.avi'), 8, 8, 29.97)
    w.append(frames[0])
    w.close()
    w.close()
    check_avi(str(tmp_path / 'b.avi'), frames[:1], 8, 8, 29.97)
    with pytest.raises(ValueError):
        AviWriter(str(tmp_path / 'c.avi'), 0, 8, 15)
    with pytest.raises(ValueError):
        read_avi_frames(__file__)


def test_avi_split_at_the_size_limit(tmp_path):
    rng = np.random.RandomState(1)
    frames = [bytes(rng.randint(0, 256, size=int(n)).astype(np.uint8)) for n in rng.randint(200, 400, size=12)]
    limit = 2000
    path = str(tmp_path / 'rec.avi')
    with AviWriter(path, 32, 24, 15, limit=limit) as avi:
        for f in frames:
            avi.append(f)
    assert len(avi.paths) >= 3 and avi.paths[:3] == [path, str(tmp_path / 'rec_001.avi'), str(tmp_path / 'rec_002.avi')]
    back, at = [], 0
    for p in avi.paths:
        assert os.path.getsize(p) <= limit
        part = read_avi_frames(p)
        assert part
        check_avi(p, frames[at:at + len(part)], 32, 24, 15)
        back, at = back + part, at + len(part)
    assert back == frames
    with pytest.raises(ValueError):
        AviWriter(str(tmp_path / 'big.avi'), 32, 24, 15, limit=500).append(bytes(600))
