"""Independent restatement of the frame renderer (``leod_render_frames_u8``) for tests/test_render_*.py.

Base image: the reference's ``event2rgb`` (vis_pred.py:74-93) with torch on the CPU -- channel sums, ``> 0`` mask, fp32 canvas of
1.0 / 0.25, ``F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)``, ``round(img * 255)`` -- permuted to HWC.
Overlay: a plain loop over the items in order, each WRITING its pixels (rectangles as slice fills, glyph bits block by block; a later
item overwrites an earlier one) -- the kernel does the opposite, every pixel asking the items --, with the raster rules of the header and
the glyph table the library itself hands out (``leod_render_font``)."""
import numpy as np
import torch
import torch.nn.functional as F

RECT, TEXT = 0, 1


def rgb(r, g, b):
    return r | g << 8 | b << 16


def base_image(ev: torch.Tensor, up: int = 2) -> np.ndarray:
    """[L, C2, H, W] (any dtype, counts >= 0) -> uint8 [L, up*H, up*W, 3]."""
    ev = ev.cpu()
    L, C2, H, W = ev.shape
    e = ev.reshape(L, 2, C2 // 2, H, W).to(torch.float32)
    pos, neg = e[:, 0].sum(1, keepdim=True), e[:, 1].sum(1, keepdim=True)
    img = torch.ones((L, 3, H, W), dtype=torch.float32)
    img[((pos > 0) | (neg > 0)).repeat(1, 3, 1, 1)] = 0.25
    if up != 1:
        img = F.interpolate(img, scale_factor=up, mode='bilinear', align_corners=False)
    img = torch.round(img * 255.).to(torch.uint8)
    return img.permute(0, 2, 3, 1).contiguous().numpy()


def font() -> np.ndarray:
    from leod_amd import ops
    return ops.render_font()


def draw_items(frames: np.ndarray, frame_off, items, text, table: np.ndarray) -> np.ndarray:
    """frames uint8 [L, Ho, Wo, 3] -> a copy with the items drawn."""
    out = frames.copy()
    L, Ho, Wo, _ = out.shape
    text = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, dtype=np.uint8)
    for f in range(L):
        for i in range(int(frame_off[f]), int(frame_off[f + 1])):
            _, kind, x, y, a, b, c, col = (int(v) for v in items[i])
            colour = (col & 255, (col >> 8) & 255, (col >> 16) & 255)
            if kind == RECT:
                x0, x1, y0, y1 = min(x, a), max(x, a), min(y, b), max(y, b)
                p, q = c // 2, (c - 1) // 2
                def span(lo, hi, n):                                     # [lo, hi] clipped to [0, n - 1] as a slice (empty if nothing is left)
                    lo, hi = max(lo, 0), min(hi, n - 1)
                    return slice(lo, max(hi + 1, lo))
                oy_, ox_ = span(y0 - p, y1 + q, Ho), span(x0 - p, x1 + q, Wo)
                iy_, ix_ = span(y0 + q + 1, y1 - p - 1, Ho), span(x0 + q + 1, x1 - p - 1, Wo)
                inside = out[f, iy_, ix_].copy()                          # the outer box filled, the inner box put back
                out[f, oy_, ox_] = colour
                out[f, iy_, ix_] = inside
            else:
                for j in range(c):
                    ch = int(text[b + j])
                    glyph = table[ch - 0x20] if 0x20 <= ch <= 0x7E else np.full(7, 0x1F, dtype=np.uint8)
                    for r in range(7):
                        for k in range(5):
                            if (int(glyph[r]) >> (4 - k)) & 1:
                                bx, by = x + (6 * j + k) * a, y - 7 * a + r * a
                                ys, xs = slice(max(by, 0), max(min(by + a, Ho), 0)), slice(max(bx, 0), max(min(bx + a, Wo), 0))
                                out[f, ys, xs] = colour
    return out
