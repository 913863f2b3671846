"""What a MaxViT block launches (``functions.AttnBlockFn`` following ``ops.attn_block_routes``): forward and backward of one block with a
recording stand-in for the library handle, on three geometries that between them take every branch of the route record.

* no ``leod_*`` call returns a negative code: nothing is called in order to be refused;
* the sequence of entry points equals the literal list below.  The lists were RECORDED with this recorder on the commit before the
  route record existed (the block then found its routes by trial) and the calls that returned -3 deleted -- 1 / 3 / 3 of them in G1 /
  G2 / G3 in mode f32, 1 / 4 / 5 in the 16-bit modes (leod_mlp_fwd_fused, leod_mlp_bwd_dgrad_fused, leod_linear_wgrad_group,
  leod_linear_dgrad_lnbwd, leod_ln_linear_bf16_fwd, leod_ln_linear_gelu16_fwd); the calls that ran are unchanged, in number and order;
* the sequence is the one the route record predicts, field by field.
``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_kernels_gpu as tk  # noqa: E402

PART = (8, 10)
# (B, H, W, C, heads): rows M = B H W
GEOMS = {'G1': (52, 16, 20, 48, 2),      # M = 16640: one-launch attention half, one-launch MLP, single weight gradients
         'G2': (26, 16, 20, 96, 4),      # M = 8320: one-launch attention half, fp16 pre-activation pair, grouped weight gradients
         'G3': (2, 16, 20, 192, 6)}      # M = 640: three-launch attention, small-row kernels, two-call LayerNorm backward
CASES = [(g, mode, True) for g in GEOMS for mode in ('f32', 'bf16', '16f')] + [('G1', mode, False) for mode in ('f32', 'bf16', '16f')]

# queries and registrations: they launch nothing, and whether a workspace is registered depends on what ran before on the stream
_NOT_LAUNCHES = ('_ok', '_mode', '_bytes', '_floats', '_route', 'get_precision', 'set_precision', 'set_workspace')

SINGLE_WGRADS = ['linear_wgrad', 'layerscale_finalize', 'linear_wgrad', 'linear_wgrad', 'layerscale_finalize', 'linear_wgrad']
GROUPED_WGRADS = ['linear_wgrad_group', 'layerscale_finalize', 'layerscale_finalize']
F32_FWD = ['ln_linear_fwd', 'partition_attn_fwd', 'linear_lsres_fwd', 'ln_linear_fwd', 'linear_lsres_fwd']
# (geometry, norm1 present) -> {mode: entry points without their ``leod_`` prefix}; bf16 and 16f recorded equal
RECORDED = {
    ('G1', True): {
        'f32': F32_FWD + ['linear_dgrad', 'linear_dgrad_lnbwd', 'linear_dgrad', 'partition_attn_bwd'] + SINGLE_WGRADS + ['linear_dgrad_lnbwd'],
        '16bit': ['attn_block_fwd', 'mlp_fwd_fused', 'mlp_bwd_dgrad_fused', 'linear_dgrad', 'partition_attn_bwd'] + SINGLE_WGRADS
                 + ['linear_dgrad_lnbwd']},
    ('G1', False): {
        'f32': F32_FWD + ['linear_dgrad', 'linear_dgrad_lnbwd', 'linear_dgrad', 'partition_attn_bwd'] + SINGLE_WGRADS + ['linear_dgrad'],
        '16bit': ['attn_block_fwd', 'mlp_fwd_fused', 'mlp_bwd_dgrad_fused', 'linear_dgrad', 'partition_attn_bwd'] + SINGLE_WGRADS
                 + ['linear_dgrad']},
    ('G2', True): {
        'f32': F32_FWD + ['linear_dgrad', 'linear_dgrad', 'layernorm_bwd', 'linear_dgrad', 'partition_attn_bwd'] + SINGLE_WGRADS
               + ['linear_dgrad', 'layernorm_bwd'],
        '16bit': ['attn_block_fwd', 'ln_linear_gelu16_fwd', 'linear_lsres_gelu16_fwd', 'linear_dgrad_gelu16', 'linear_dgrad', 'layernorm_bwd',
                  'linear_dgrad', 'partition_attn_bwd'] + GROUPED_WGRADS + ['linear_dgrad', 'layernorm_bwd']},
    ('G3', True): {
        'f32': F32_FWD + ['linear_dgrad', 'linear_dgrad', 'layernorm_bwd', 'linear_dgrad', 'partition_attn_bwd'] + SINGLE_WGRADS
               + ['linear_dgrad', 'layernorm_bwd'],
        '16bit': F32_FWD + ['linear_dgrad', 'linear_dgrad', 'layernorm_bwd', 'linear_dgrad', 'partition_attn_bwd'] + SINGLE_WGRADS
                 + ['linear_dgrad', 'layernorm_bwd']},
}


class _RecordingLib:
    """Stand-in for the CDLL (as ``ops._ProbedLib``): notes (entry point, return code) of every ``leod_*`` launch call."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        real = getattr(self._lib, name)
        if not name.startswith('leod_') or name.endswith(_NOT_LAUNCHES):
            return real

        def fn(*a):
            rc = real(*a)
            self.calls.append((name[len('leod_'):], rc))
            return rc
        return fn


def _block(C, heads, norm1, seed=11):
    from leod_amd.config import create
    from leod_amd.models.layers.maxvit.maxvit import PartitionAttentionCl, PartitionType
    cfg = create(dict(use_torch_mha=False, partition_size=PART, dim_head=C // heads, attention_bias=True, mlp_activation='gelu', mlp_gated=False,
                      mlp_bias=True, mlp_ratio=4, drop_mlp=0, drop_path=0, ls_init_value=1e-5))
    m = PartitionAttentionCl(C, PartitionType.WINDOW, cfg, skip_first_norm=not norm1)
    assert not m.generic
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((1 if n.startswith('norm') and n.endswith('weight') else 0) + 0.2 * torch.randn(p.shape, generator=gen))
    return m.to(tk.DEV)


def record_block(geom, mode, norm1):
    """-> [(entry point, return code)] of one forward + backward of a block of GEOMS[geom] in precision mode ``mode``."""
    from leod_amd import ops
    B, H, W, C, heads = GEOMS[geom]
    prev = ops.set_precision(mode)
    real = ops._l()
    rec = _RecordingLib(real)
    try:
        m = _block(C, heads, norm1)
        x = tk.rnd((B, H, W, C), 12).to(tk.DEV).requires_grad_(True)
        ops._LIB = rec
        m(x).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops._LIB = real
        ops.set_precision(prev)
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    return rec.calls


def _predicted(r, norm1):
    """the entry points the fields of an ``ops.BlockRoutes`` stand for, in the order of AttnBlockFn"""
    from leod_amd import ops
    two_call = ['linear_dgrad', 'layernorm_bwd']
    seq = ['attn_block_fwd'] if r.attn > 0 else ['ln_linear_bf16_fwd' if r.q16 else 'ln_linear_fwd', 'partition_attn_fwd',
                                                  'linear_lsres_bf16_fwd' if r.o16 else 'linear_lsres_fwd']
    seq += {ops.MLP_FUSED: ['mlp_fwd_fused'], ops.MLP_PAIR16: ['ln_linear_gelu16_fwd', 'linear_lsres_gelu16_fwd'],
            ops.MLP_PAIR32: ['ln_linear_fwd', 'linear_lsres_fwd']}[r.mlp_fwd]
    if r.mlp_bwd_fused:
        seq += ['mlp_bwd_dgrad_fused']
    else:
        seq += ['linear_dgrad_gelu16' if r.u16 else 'linear_dgrad'] + (['linear_dgrad_lnbwd'] if r.ln2_fused else two_call)
    seq += ['linear_dgrad', 'partition_attn_bwd'] + (GROUPED_WGRADS if r.wgrads_grouped else SINGLE_WGRADS)
    return seq + ((['linear_dgrad_lnbwd'] if r.ln1_fused else two_call) if norm1 else ['linear_dgrad'])


@pytest.mark.parametrize('geom,mode,norm1', CASES, ids=[f'{g}-{m}-{"norm1" if n else "nonorm"}' for g, m, n in CASES])
def test_block_launches_what_its_routes_say(geom, mode, norm1):
    from leod_amd import ops
    calls = record_block(geom, mode, norm1)
    print(geom, mode, norm1, calls)
    refused = [c for c in calls if c[1] < 0]
    assert not refused, f'calls that returned an error code: {refused}'
    names = [n for n, _ in calls]
    assert names == RECORDED[(geom, norm1)]['f32' if mode == 'f32' else '16bit']
    prev = ops.set_precision(mode)
    try:
        B, H, W, C, heads = GEOMS[geom]
        r = ops.attn_block_routes(B, H, W, C, heads, PART, 4 * C, ops.ABF_LN_AFFINE if norm1 else ops.ABF_NO_NORM)
    finally:
        ops.set_precision(prev)
    assert names == _predicted(r, norm1), r
