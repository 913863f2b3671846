"""Route table of the one-launch attention sub-block (``leod_attn_block_fwd_route``, csrc/attn_route.hpp): the decision
``functions.AttnBlockFn.forward`` asks for on every block.  It launches nothing and reads no device memory, so it is checked without a GPU,
beside tests/test_attn_lstm_routes_cpu.py."""
import pytest

FUSED = 40000 + 100 * 5 + 24          # family 4, five 16-token tiles, head dimension 24 (include/leod_hip.h)
UNSUPPORTED = -3
# (B, H, W) of the headline workload's stages: T = 21 frames x 8 sequences of a 256 x 320 map, downsampled by 4 / 8 / 16 / 32
STAGES = {1: (168, 64, 80, 48, 2), 2: (168, 32, 40, 96, 4), 3: (168, 16, 20, 192, 8), 4: (168, 8, 10, 384, 16)}


@pytest.fixture(scope='module')
def ops():
    import __graft_entry__ as g
    g.build()
    from leod_amd import ops
    prev = ops.get_precision()
    yield ops
    ops.set_precision(prev)


@pytest.mark.parametrize('mode', ['bf16', '16f'])
@pytest.mark.parametrize('stage', [1, 2])
def test_stages_1_and_2_take_the_fused_route_in_the_16bit_modes(ops, mode, stage):
    ops.set_precision(mode)
    B, H, W, C, heads = STAGES[stage]
    assert ops.attn_block_fwd_route(B, H, W, C, heads, (8, 10)) == FUSED
    assert ops.attn_block_fwd_route(B, H, W, C, heads, (8, 10), flags=ops.ABF_NO_NORM) == FUSED      # norm1 = identity: first block of a stage
    assert ops.attn_block_o16_ok(B, H, W, C, heads, (8, 10)), 'the fused route implies 16-bit O rows'


@pytest.mark.parametrize('stage', [1, 2, 3, 4])
def test_mode_f32_is_unsupported(ops, stage):
    ops.set_precision('f32')
    B, H, W, C, heads = STAGES[stage]
    assert ops.attn_block_fwd_route(B, H, W, C, heads, (8, 10)) == UNSUPPORTED


@pytest.mark.parametrize('mode', ['bf16', '16f'])
def test_everything_else_is_unsupported(ops, mode):
    ops.set_precision(mode)
    for stage in (3, 4):                                      # qkv tile + weights do not fit a CU's LDS; not bandwidth-bound
        B, H, W, C, heads = STAGES[stage]
        assert ops.attn_block_fwd_route(B, H, W, C, heads, (8, 10)) == UNSUPPORTED
    B, H, W, C, heads = STAGES[1]
    assert ops.attn_block_fwd_route(B, 56, 80, C, heads, (7, 8)) == UNSUPPORTED          # padded partitions: 56 of 64 tokens
    assert ops.attn_block_fwd_route(B, H, W, C, heads, (8, 10), flags=0) == UNSUPPORTED  # a norm1 without weight and bias
    assert ops.attn_block_fwd_route(B, H, W, 64, 2, (8, 10)) == UNSUPPORTED              # d = 32 is not instantiated
    # a map too small for the block's 16-bit O consumers (leod_attn_block_o16_ok): the block keeps its three launches
    assert not ops.attn_block_o16_ok(2, 16, 20, C, heads, (8, 10))
    assert ops.attn_block_fwd_route(2, 16, 20, C, heads, (8, 10)) == UNSUPPORTED
