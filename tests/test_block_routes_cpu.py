"""Route tables of the MaxViT block: ``leod_mlp_fused_route``, ``leod_linear_wgrad_group_route`` and the record ``ops.attn_block_routes``
builds from the library's queries.  They launch nothing and read host state only, so they are checked without a GPU, beside
tests/test_linear_routes_cpu.py and tests/test_attn_block_route_cpu.py.

The expected values are written down from the conditions the entry points had BEFORE the queries existed (csrc/k_mlp.hip: 16-bit mode,
(K, H) = (48, 192) | (64, 256), M >= 16384; csrc/k_linear_wgrad.hip: the checks of leod_linear_wgrad_group in their order) and, for the
record, from the call table of an eager benchmark step of that commit (profiles/r14_a_calls_parent.txt: which calls of a stage ran and
which returned at once)."""
import pytest

MODES = ('f32', 'bf16', '16f')
MODES16 = ('bf16', '16f')


@pytest.fixture(scope='module')
def ops():
    import __graft_entry__ as g
    g.build()
    from leod_amd import ops
    prev = ops.get_precision()
    yield ops
    ops.set_precision(prev)


# ---- leod_mlp_fused_route -------------------------------------------------------------------------------------------------------------
MLP_ROWS = (16383, 16384, 860160, 61440)
MLP_TABLE = {(48, 192): (-3, 7312, 7312, 7312), (64, 256): (-3, 7416, 7416, 7416), (96, 384): (-3, -3, -3, -3), (48, 144): (-3, -3, -3, -3)}


@pytest.mark.parametrize('mode', MODES)
def test_mlp_fused_route(ops, mode):
    ops.set_precision(mode)
    for (K, H), want in MLP_TABLE.items():
        for M, w in zip(MLP_ROWS, want):
            for entry in (0, 1):
                assert ops.mlp_fused_route(entry, M, H, K) == (-3 if mode == 'f32' else w), (mode, entry, M, H, K)
            assert ops.mlp_fused_route(2, M, H, K) == -1


# ---- leod_linear_wgrad_group_route ----------------------------------------------------------------------------------------------------
def _block_problems(ops, C):
    """fc2, fc1, proj, qkv of a block of width C as attn_block_wgrads hands them over: dz fp32 x fp16 pre-activation, bf16 du x LN(y),
    fp32 dy x 16-bit O rows, bf16 dqkv x LN(x)"""
    return (C, 4 * C, C, 3 * C), (4 * C, C, C, C), (0, 1, 0, 1), (2, 1, 4 if ops.get_precision() == '16f' else 3, 1)


@pytest.mark.parametrize('mode', MODES)
def test_group_route_of_the_blocks(ops, mode):
    ops.set_precision(mode)
    # RVT-S at the benchmark's row counts: no tile class for 48 | 215040 rows above the 60 000 of tile 6 | tile 6 | tile 6
    for C, M, want in ((48, 860160, -3), (96, 215040, -3), (192, 53760, 106), (384, 13440, 106)):
        assert ops.linear_wgrad_group_route(M, *_block_problems(ops, C)) == (-3 if mode == 'f32' else want), (mode, C)
    # RVT-B widths: 64 is of the 64-class only (tile 4), 128 / 256 / 512 of the 128-class (tile 8); 61440 rows are inside 8192 .. 400 000
    for C, want in ((64, 104), (128, 108), (256, 108), (512, 108)):
        assert ops.linear_wgrad_group_route(61440, *_block_problems(ops, C)) == (-3 if mode == 'f32' else want), (mode, C)


@pytest.mark.parametrize('mode', MODES16)
def test_group_route_bounds(ops, mode):
    ops.set_precision(mode)

    def one(M, N, K, dy_fmt=1, x_fmt=3):              # bf16 operands: nothing to copy, the operand bound stays out of the way
        return ops.linear_wgrad_group_route(M, (N,), (K,), (dy_fmt,), (x_fmt,))
    assert one(8128, 96, 96) == -3 and one(8192, 96, 96) == 106
    assert one(8200, 96, 96) == -3                    # not a multiple of 64
    assert one(59968, 96, 96) == 106 and one(60032, 96, 96) == -3
    assert one(400000, 64, 64) == 104 and one(400064, 64, 64) == -3
    assert one(400000, 128, 128) == 108 and one(400064, 128, 128) == -3
    assert one(8192, 48, 48) == -3                    # no tile class
    assert ops.linear_wgrad_group_route(8192, (96, 128), (96, 128), (1, 1), (3, 3)) == -3       # a 96-class problem with a 128-class one
    # the operand bound: 400 000 rows x 4 x (128 + 128) columns x 2 bytes = 819 MB of 16-bit copies against 600 MiB; none with 16-bit operands
    assert ops.linear_wgrad_group_route(400000, (128,) * 4, (128,) * 4, (0,) * 4, (0,) * 4) == -3
    assert ops.linear_wgrad_group_route(400000, (128,) * 4, (128,) * 4, (1,) * 4, (3,) * 4) == 108


@pytest.mark.parametrize('mode', MODES)
def test_group_route_argument_errors_and_their_order(ops, mode):
    ops.set_precision(mode)
    assert ops.linear_wgrad_group_route(8192, (), (), (), ()) == -1
    assert ops.linear_wgrad_group_route(8192, (96,) * 5, (96,) * 5, (1,) * 5, (3,) * 5) == -1
    assert ops.linear_wgrad_group_route(8192, (96,), (96,), (1,), (5,)) == -1                   # x_fmt is checked before the mode
    # problem 0 is refused (no tile class; mode f32) before problem 1 is looked at
    assert ops.linear_wgrad_group_route(8192, (48, 96), (48, 96), (1, 1), (3, 5)) == -3
    # ... and a valid problem 0 lets the x_fmt of problem 1 through to its check
    assert ops.linear_wgrad_group_route(8192, (96, 96), (96, 96), (1, 1), (3, 5)) == (-3 if mode == 'f32' else -1)
    lib = ops._l()
    assert lib.leod_linear_wgrad_group_route(1, 8192, None, None, None, None) == -1


# ---- ops.attn_block_routes ------------------------------------------------------------------------------------------------------------
FUSED = 40524
# the four stages of RVT-S on the benchmark's maps (168 frames of 64 x 80 ... 8 x 10 tokens, partitions of 8 x 10, hidden 4 C)
STAGES = ((168, 64, 80, 48, 2), (168, 32, 40, 96, 4), (168, 16, 20, 192, 8), (168, 8, 10, 384, 16))
# fields: attn, q16, o16, mlp_fwd, mlp_bwd_fused, ln2_fused, ln1_fused, wgrads_grouped -- with norm1; without it ln1_fused is False.
# mode f32: three launches on fp32 rows, the fp32 pair, singles; the dgrad + LayerNorm-backward kernel covers K = 48 (stage 1) only.
# 16-bit modes: stages 1-2 one-launch attention (the same 16-bit qkv / O as the three launches), stages 3-4 three launches on 16-bit rows;
# the one-launch MLP on stage 1 alone, the fp16 pre-activation pair on 2-4; dgrad + LayerNorm backward fused on stages 1-2 (bf16 dy:
# K = 96 as well), two calls on 3-4; the weight gradients grouped on stages 3-4 (stage 1: no tile class, stage 2: 215040 rows).
RECORDS = {
    'f32': ((-3, False, False, 'pair32', False, True, True, False),
            (-3, False, False, 'pair32', False, False, False, False),
            (-3, False, False, 'pair32', False, False, False, False),
            (-3, False, False, 'pair32', False, False, False, False)),
    '16bit': ((FUSED, True, True, 'fused', True, True, True, False),
              (FUSED, True, True, 'pair16', False, True, True, False),
              (-3, True, True, 'pair16', False, False, False, True),
              (-3, True, True, 'pair16', False, False, False, True)),
}


@pytest.mark.parametrize('norm1', [True, False], ids=['norm1', 'nonorm'])
@pytest.mark.parametrize('mode', MODES)
def test_block_records_of_the_four_stages(ops, mode, norm1):
    ops.set_precision(mode)
    for (B, H, W, C, heads), want in zip(STAGES, RECORDS['f32' if mode == 'f32' else '16bit']):
        r = ops.attn_block_routes(B, H, W, C, heads, (8, 10), 4 * C, ops.ABF_LN_AFFINE if norm1 else ops.ABF_NO_NORM)
        assert tuple(r) == want[:6] + (want[6] and norm1,) + want[7:], (mode, C, r)
        assert r.u16 == (want[3] != 'pair32')
        assert not r.attn > 0 or (r.q16 and r.o16), 'a one-launch attention half leaves 16-bit qkv and O rows behind'


def test_block_record_is_per_precision_mode(ops):
    B, H, W, C, heads = STAGES[0]
    ops.set_precision('bf16')
    r16 = ops.attn_block_routes(B, H, W, C, heads, (8, 10), 4 * C)
    ops.set_precision('f32')
    r32 = ops.attn_block_routes(B, H, W, C, heads, (8, 10), 4 * C)
    assert r16.attn == FUSED and r32.attn == -3 and r32.mlp_fwd == ops.MLP_PAIR32
    ops.set_precision('bf16')
    assert ops.attn_block_routes(B, H, W, C, heads, (8, 10), 4 * C) is r16
