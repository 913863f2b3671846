"""Torch-only restatement of torchvision's tensor ``rotate`` (transforms/functional.py + _functional_tensor.py) for
``interpolation=NEAREST, expand=False, center=None, fill=None`` -- what the reference's augmentor calls on the event frames
(data/utils/augmentor.py:364-369).  torchvision is not installed where this project is built and tested, so the pixel rule is
pinned from ATen primitives, the way the zooms' nearest-exact rule is (oracle/augment.py).  Helper of the rotation tests, not a test.

Steps of torchvision's code path, all in fp32:
  * inverse matrix of ``_get_inverse_affine_matrix([0, 0], -angle, [0, 0], 1.0, [0, 0])`` = [cos r, sin r, 0, -sin r, cos r, 0]
    with r = radians(-angle), built from Python floats;
  * ``_gen_affine_grid``: base grid linspace(-W/2 + 0.5, W/2 - 0.5, W) x linspace(-H/2 + 0.5, H/2 - 0.5, H) x 1, ``bmm`` with
    theta^T / [W/2, H/2];
  * ``grid_sample(mode='nearest', padding_mode='zeros', align_corners=False)`` on the float image, cast back to uint8.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def _theta(angle: float) -> torch.Tensor:
    r = math.radians(-angle)
    return torch.tensor([math.cos(r), math.sin(r), 0.0, -math.sin(r), math.cos(r), 0.0], dtype=torch.float32).reshape(1, 2, 3)


def _gen_affine_grid(theta: torch.Tensor, w: int, h: int, ow: int, oh: int) -> torch.Tensor:
    d = 0.5
    base_grid = torch.empty(1, oh, ow, 3, dtype=theta.dtype)
    x_grid = torch.linspace(-ow * 0.5 + d, ow * 0.5 + d - 1, steps=ow)
    base_grid[..., 0].copy_(x_grid)
    y_grid = torch.linspace(-oh * 0.5 + d, oh * 0.5 + d - 1, steps=oh).unsqueeze_(-1)
    base_grid[..., 1].copy_(y_grid)
    base_grid[..., 2].fill_(1)
    rescaled_theta = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=theta.dtype)
    return base_grid.view(1, oh * ow, 3).bmm(rescaled_theta).view(1, oh, ow, 2)


def rotate(img: torch.Tensor, angle: float, interpolation=None, **_ignored) -> torch.Tensor:
    """img [..., H, W] (uint8 or float, CPU) rotated counter-clockwise by ``angle`` degrees about the image centre; same
    signature start as torchvision's so that it can stand in for the name ``rotate`` of the reference's augmentor module."""
    H, W = img.shape[-2:]
    flat = img.reshape((1, -1, H, W))
    grid = _gen_affine_grid(_theta(float(angle)), W, H, W, H)
    out = F.grid_sample(flat.to(torch.float32), grid, mode='nearest', padding_mode='zeros', align_corners=False)
    if not img.is_floating_point():
        out = torch.round(out)
    return out.to(img.dtype).reshape(img.shape)


def source_coords(H: int, W: int, angle: float):
    """float64 source pixel coordinates (sy, sx), each [H, W], of every output pixel: the exact values that the fp32 chain above
    approximates before it rounds to the nearest pixel."""
    a = math.radians(angle)
    c, s = math.cos(a), math.sin(a)
    cx, cy = 0.5 * W - 0.5, 0.5 * H - 0.5
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    sx = c * (x - cx) - s * (y - cy) + cx
    sy = s * (x - cx) + c * (y - cy) + cy
    return sy, sx


def near_tie_mask(H: int, W: int, angle: float, band: float = 1e-3) -> np.ndarray:
    """bool [H, W]: True where either source coordinate lies within ``band`` of a half-integer, i.e. where the order of the fp32
    operations may legitimately decide which of two neighbouring source pixels is the nearest one."""
    sy, sx = source_coords(H, W, angle)

    def near_half(v):
        return np.abs((v - 0.5) - np.round(v - 0.5)) < band
    return near_half(sy) | near_half(sx)
