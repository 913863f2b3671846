"""The attention half of a block in one launch (csrc/k_attn_block.hip, ``ops.attn_block_fwd``): LayerNorm -> qkv -> partition attention ->
proj -> LayerScale -> residual for RVT stages 1-2 in the 16-bit precision modes.

* the kernel against fp32 CPU arithmetic (``F.layer_norm`` -> ``F.linear`` -> ``_attn_ref`` -> ``x + gamma * F.linear``), every stage of
  the reference fed the rounded 16-bit qkv / O rows the kernel stored, as the 16-bit tests of tests/test_bf16_gpu.py do: window and grid
  partitions, both modes, tensors saved and not saved, norm1 a LayerNorm or the identity (the first block of a stage); four partitions per
  frame, an odd frame count;
* ``AttnBlockFn`` forward and backward with ``ops.ATTN_BLOCK_FUSED`` on and off on maps large enough for the block to take the fused
  route: y, the input gradient and every parameter gradient agree within the modes' bounds (forward bound for y, bf16 bound for gradients).
``pytest -m gpu``."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import test_kernels_gpu as tk  # noqa: E402
from test_bf16_gpu import bf16_ops  # noqa: E402,F401  (fixture: runs a test in modes 'bf16' and '16f')

PART = (8, 10)
SHAPES = [(2, 16, 20, 48, 2), (3, 16, 20, 48, 2), (2, 16, 20, 96, 4)]


def _inputs(B, H, W, C):
    x = tk.rnd((B, H, W, C), 1)
    lw, lb = 1 + 0.2 * tk.rnd((C,), 2), 0.1 * tk.rnd((C,), 3)
    Wq, bq = tk.rnd((3 * C, C), 4, 0.2), tk.rnd((3 * C,), 5, 0.2)
    Wp, bp, g = tk.rnd((C, C), 6, 0.2), tk.rnd((C,), 7, 0.2), 0.5 + 0.1 * tk.rnd((C,), 8)
    return x, lw, lb, Wq, bq, Wp, bp, g


def _dev(t):
    return None if t is None else t.to(tk.DEV)


@functools.lru_cache(maxsize=None)
def _saved_run(mode, B, H, W, C, heads, window, ln):
    """One fused call that keeps its tensors, and the fp32 CPU reference of every stage on the rounded rows it stored (computed once per
    geometry and mode, shared by the saved and the not-saved case, never modified)."""
    from leod_amd import ops
    assert ops.get_precision() == mode
    cpu = _inputs(B, H, W, C)
    if not ln:
        cpu = (cpu[0], None, None) + cpu[3:]
    x, lw, lb, Wq, bq, Wp, bp, g = cpu
    y, qkv, st, o, lse = ops.attn_block_fwd(*[_dev(t) for t in cpu], heads, PART, window, want_saved=True)
    qkv_s, o_s = qkv.float().cpu(), o.float().cpu()
    ref = dict(qkv=F.linear(F.layer_norm(x, (C,), lw, lb, 1e-5) if ln else x, Wq, bq),
               o=tk._attn_ref(qkv_s, heads, PART, window),
               y=x + g * F.linear(o_s, Wp, bp))
    d = C // heads
    p = tk.ob.window_partition(qkv_s, PART) if window else tk.ob.grid_partition(qkv_s, PART)
    q, k, _ = p.reshape(p.shape[0], -1, heads, 3 * d).transpose(1, 2).chunk(3, dim=3)
    l = torch.logsumexp((q @ k.transpose(-2, -1)) * d ** -0.5, -1).transpose(1, 2).reshape(p.shape[0], PART[0], PART[1], heads)
    ref['lse'] = tk.ob.window_reverse(l, PART, (H, W)) if window else tk.ob.grid_reverse(l, PART, (H, W))
    return cpu, (y, qkv, st, o, lse), ref


@pytest.mark.parametrize('saved', [True, False], ids=['saved', 'notsaved'])
@pytest.mark.parametrize('ln', [True, False], ids=['norm1', 'nonorm'])
@pytest.mark.parametrize('window', [True, False], ids=['window', 'grid'])
@pytest.mark.parametrize('B,H,W,C,heads', SHAPES)
def test_attn_block_fwd_against_cpu(bf16_ops, B, H, W, C, heads, window, ln, saved):
    ops = bf16_ops
    mode = ops.get_precision()
    cpu, (y, qkv, st, o, lse), ref = _saved_run(mode, B, H, W, C, heads, window, ln)
    x = cpu[0]
    if saved:
        assert qkv.dtype is ops.act16_dtype() and o.dtype is ops.act16_dtype()
        tk.close(qkv.float(), ref['qkv'], what='qkv rows', fwd=True)
        tk.close(o.float(), ref['o'], what='attention output O on the stored qkv', fwd=True)
        tk.close(y, ref['y'], what='y on the stored O', fwd=True)
        tk.close(lse, ref['lse'], what='lse on the stored qkv')
        if not ln:
            assert st is None
            return
        tk.close(st[:, 0], x.reshape(-1, C).mean(1), rtol=1e-4, atol=1e-5, what='LayerNorm mean')
        tk.close(st[:, 1], (x.reshape(-1, C).var(1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-4, atol=1e-5, what='LayerNorm rstd')
    else:
        y2, qkv2, st2, o2, lse2 = ops.attn_block_fwd(*[_dev(t) for t in cpu], heads, PART, window, want_saved=False)
        assert qkv2 is None and st2 is None and o2 is None and lse2 is None
        tk.close(y2, ref['y'], what='y, nothing saved', fwd=True)
        assert torch.equal(y2, y), 'the stores that are skipped do not change y'


def _block(C, window, skip_first_norm, seed):
    from leod_amd.config import create
    from leod_amd.models.layers.maxvit.maxvit import PartitionAttentionCl, PartitionType
    cfg = create(dict(use_torch_mha=False, partition_size=PART, dim_head=24, attention_bias=True, mlp_activation='gelu', mlp_gated=False,
                      mlp_bias=True, mlp_ratio=4, drop_mlp=0, drop_path=0, ls_init_value=1e-5))
    m = PartitionAttentionCl(C, PartitionType.WINDOW if window else PartitionType.GRID, cfg, skip_first_norm=skip_first_norm)
    assert not m.generic
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('gamma'):
                p.copy_(0.5 + 0.1 * torch.randn(p.shape, generator=gen))
            elif n.startswith('norm') and n.endswith('weight'):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=gen))
            else:
                p.copy_(0.2 * torch.randn(p.shape, generator=gen))
    return m.to(tk.DEV)


# the smallest maps of 8 x 10 partitions on which the block keeps O as 16-bit rows (leod_attn_block_o16_ok) and so takes the fused route
@pytest.mark.parametrize('window,skip', [(True, False), (False, False), (True, True)], ids=['window', 'grid', 'window-nonorm'])
@pytest.mark.parametrize('B,H,W,C,heads', [(52, 16, 20, 48, 2), (26, 16, 20, 96, 4)])
def test_block_fused_against_composed(bf16_ops, B, H, W, C, heads, window, skip):
    ops = bf16_ops
    assert ops.attn_block_fwd_route(B, H, W, C, heads, PART, flags=ops.ABF_NO_NORM if skip else ops.ABF_LN_AFFINE) > 0
    m = _block(C, window, skip, 11)
    x0, r = tk.rnd((B, H, W, C), 12).to(tk.DEV), tk.rnd((B, H, W, C), 13).to(tk.DEV)
    out = {}
    prev = ops.ATTN_BLOCK_FUSED
    try:
        for fused in (True, False):
            ops.ATTN_BLOCK_FUSED = fused
            m.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            y = m(x)
            (y * r).sum().backward()
            torch.cuda.synchronize()
            out[fused] = (y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
    finally:
        ops.ATTN_BLOCK_FUSED = prev
    (yf, dxf, gf), (yc, dxc, gc) = out[True], out[False]
    print(f'fused vs composed {ops.get_precision()} C={C} {"window" if window else "grid"}: max |dy| {float((yf - yc).abs().max()):.3e}, '
          f'max |ddx| {float((dxf - dxc).abs().max()):.3e}')
    tk.close(yf, yc, what='block output', fwd=True)
    tk.close(dxf, dxc, what='input gradient')
    for n in gc:
        tk.close(gf[n], gc[n], what='gradient of ' + n)
