"""The routing tables of the partition attention core and of the ConvLSTM sequence kernels, pinned without a GPU:
``leod_partition_attn_route`` and ``leod_convlstm_seq_route`` (the decisions the entry points themselves switch on; they launch nothing
and read only host state) against literal tables, one per precision mode.

The expected values were written down BEFORE the routers existed.  The kernel families come from the hand-written cascades of the entry
points as they stood then (k_attn.hip: ``dispatch_attn``'s shape rule, ``run_attn_lds``'s cascade over the precision mode and the format
bits, the ``ATTL`` / ``ATT`` instantiation ladders; k_lstm.hip: ``leod_convlstm_seq_mode``, the ``LSTM_FWD_CASE`` / ``LSTM_BWD_CASE``
ladders, the two chains of the streamed kernels and the register budget of the backward).  The values of the five host-only predicates
(``leod_partition_attn_16bit_ok`` / ``_o16_ok``, ``leod_convlstm_seq_mode`` / ``_gates16_ok`` / ``_pack_bytes``) were recorded from a
build of that state.  tools/attn_lstm_route_sweep.py runs every launching row on a GPU, so that two builds can be compared output for
output.

Attention codes: 10000 F + 100 PT + D -- F = 1 register-direct fp32 kernels (D = 16 ceil(d / 16)), 2 LDS kernels on fp32 tiles, 3 LDS
kernels on 16-bit tiles (D = d); flags 1 qkv rows 16-bit, 2 O / dO rows 16-bit, 4 dqkv written as bf16 (backward only).  ConvLSTM codes:
forward 1000 + C fused, 2000 + C hoisted, 3000 + C streamed, backward 3000 + C streamed, 4000 + C register-resident; flags 1 xin is the
projection, 2 gates16, 4 a wpack is given.  0 nothing to do, -1 bad argument, -3 unsupported."""
import pytest

MODES = ('f32', 'bf16', '16f')
FWD, BWD = 0, 1
QKV16, O16, DQKV16 = 1, 2, 4
PROJ, GATES16, PACK = 1, 2, 4

# ---------------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------------
# real (ph, pw) pairs per tile count PT = ceil(ph pw / 16): the first fills its tiles, the others are padded (7 x 8, 6 x 10, 5 x 7 and 6 x 6
# also run in the GPU tests)
PARTS = {1: ((4, 4), (3, 5)), 2: ((4, 8), (5, 6)), 3: ((6, 8), (5, 7), (6, 6)), 4: ((8, 8), (7, 8), (6, 10)), 5: ((8, 10), (7, 11)),
         6: ((8, 12), (9, 10)), 7: ((8, 14), (10, 10)), 8: ((8, 16), (11, 11)), 9: ((12, 12), (10, 14)), 10: ((10, 16), (12, 13)),
         11: ((11, 16), (13, 13)), 12: ((12, 16), (13, 14)), 13: ((13, 16), (14, 14)), 14: ((14, 16), (14, 15)), 15: ((12, 20), (15, 15)),
         16: ((16, 16), (15, 17))}
HEADS = (1, 2, 3)

# Family per head dimension (row) and tile count PT = 1 .. 16 (column): a digit is F, '.' is -3 (no kernel: PT 6, 7, 9, 11 .. 14, 16
# everywhere, PT 3 / 8 / 10 / 15 below d = 20).  Neither the head count nor padding moves a cell.
#            PT  1234567890123456
REG = {4:       '11.11...........', 8:  '11.11...........', 12: '11.11...........', 16: '11.11...........',
       20:      '11111..1.1....1.', 28: '11111..1.1....1.'}
NONE = '................'
LDS32 = '22222..2.2....2.'
LDS16 = '33333..3.3....3.'
PLAIN = {**REG, 24: LDS32, 32: LDS32}                 # fp32 tensors, any mode, either entry


def _lds_only(row):                                          # any 16-bit flag: the register-direct kernels refuse; d = 24 / 32 as given
    return {**{d: NONE for d in REG}, 24: row, 32: row}


# (entry, flags) -> grid, per mode.  The combinations the wrappers produce are 0; 1; 1|2; backward 1|4; 1|2|4.  The others are the
# refusals and oddities of the cascades: 16-bit O / dO without the 16-bit tiles (-3), 16-bit rows on an F = 1 shape (-3), fp16 rows off
# the 16-bit tiles (mode 16f: -3), the dqkv flag on the forward (not looked at), bf16 rows read or written by the fp32-tile kernels
# (format bits 1 / 2 of the kernels, modes f32 and bf16).
ATTN = {
    'f32': {
        (FWD, 0): PLAIN, (FWD, DQKV16): PLAIN, (FWD, QKV16): _lds_only(LDS32), (FWD, QKV16 | DQKV16): _lds_only(LDS32),
        (FWD, O16): _lds_only(NONE), (FWD, QKV16 | O16): _lds_only(NONE), (FWD, QKV16 | O16 | DQKV16): _lds_only(NONE),
        (BWD, 0): PLAIN, (BWD, QKV16): _lds_only(LDS32), (BWD, DQKV16): _lds_only(LDS32), (BWD, QKV16 | DQKV16): _lds_only(LDS32),
        (BWD, O16): _lds_only(NONE), (BWD, QKV16 | O16): _lds_only(NONE), (BWD, QKV16 | O16 | DQKV16): _lds_only(NONE),
    },
    'bf16': {
        (FWD, 0): PLAIN, (FWD, DQKV16): PLAIN, (FWD, QKV16): _lds_only(LDS16), (FWD, QKV16 | DQKV16): _lds_only(LDS16),
        (FWD, O16): _lds_only(NONE), (FWD, QKV16 | O16): _lds_only(LDS16), (FWD, QKV16 | O16 | DQKV16): _lds_only(LDS16),
        (BWD, 0): PLAIN, (BWD, QKV16): _lds_only(LDS32), (BWD, DQKV16): _lds_only(LDS32), (BWD, QKV16 | DQKV16): _lds_only(LDS16),
        (BWD, O16): _lds_only(NONE), (BWD, QKV16 | O16): _lds_only(NONE), (BWD, QKV16 | O16 | DQKV16): _lds_only(LDS16),
    },
    '16f': {
        (FWD, 0): PLAIN, (FWD, DQKV16): PLAIN, (FWD, QKV16): _lds_only(LDS16), (FWD, QKV16 | DQKV16): _lds_only(LDS16),
        (FWD, O16): _lds_only(NONE), (FWD, QKV16 | O16): _lds_only(LDS16), (FWD, QKV16 | O16 | DQKV16): _lds_only(LDS16),
        (BWD, 0): PLAIN, (BWD, QKV16): _lds_only(NONE), (BWD, DQKV16): _lds_only(NONE), (BWD, QKV16 | DQKV16): _lds_only(LDS16),
        (BWD, O16): _lds_only(NONE), (BWD, QKV16 | O16): _lds_only(NONE), (BWD, QKV16 | O16 | DQKV16): _lds_only(LDS16),
    },
}

# leod_partition_attn_16bit_ok = leod_partition_attn_o16_ok per head dimension and PT, as recorded (heads 1 .. 3, B 1 and 2, every pair
# of PARTS gave the same answer); mode f32: 0 everywhere
OK16_ROW = '1111100101000010'
OK16 = {'f32': {}, 'bf16': {24: OK16_ROW, 32: OK16_ROW}, '16f': {24: OK16_ROW, 32: OK16_ROW}}


def attn_code(cell, PT, d):
    return -3 if cell == '.' else int(cell) * 10000 + 100 * PT + (d if cell != '1' else 16 * ((d + 15) // 16))


def attn_rows():
    """(mode, entry, B, H, W, C, heads, (ph, pw), flags, expected): four partitions per image, so that window and grid addressing differ"""
    for mode in MODES:
        for (entry, flags), grid in ATTN[mode].items():
            for d, row in grid.items():
                for PT, cell in enumerate(row, 1):
                    for ph, pw in PARTS[PT]:
                        for heads in HEADS:
                            yield (mode, entry, 1, 2 * ph, 2 * pw, heads * d, heads, (ph, pw), flags, attn_code(cell, PT, d))


# rows outside the grid: (mode, entry, B, H, W, C, heads, (ph, pw), flags, expected)
ATTN_EXTRA = tuple(r for mode in MODES for r in (
    # every -1 cause: no heads, C no multiple of heads, d no multiple of 4, d > 32, H / W no multiple of the partition, an unknown entry,
    # an empty partition
    (mode, FWD, 2, 16, 20, 64, 0, (8, 10), 0, -1), (mode, BWD, 2, 16, 20, 64, -2, (8, 10), 0, -1),
    (mode, FWD, 2, 16, 20, 50, 3, (8, 10), 0, -1), (mode, BWD, 2, 16, 20, 50, 3, (8, 10), QKV16 | DQKV16, -1),
    (mode, FWD, 2, 16, 20, 12, 2, (8, 10), 0, -1), (mode, BWD, 2, 16, 20, 44, 2, (8, 10), 0, -1),
    (mode, FWD, 2, 16, 20, 72, 2, (8, 10), 0, -1), (mode, BWD, 2, 16, 20, 36, 1, (8, 10), 0, -1),
    (mode, FWD, 2, 15, 20, 64, 2, (8, 10), 0, -1), (mode, BWD, 2, 16, 21, 64, 2, (8, 10), QKV16, -1),
    (mode, 2, 2, 16, 20, 64, 2, (8, 10), 0, -1), (mode, -1, 2, 16, 20, 64, 2, (8, 10), 0, -1),
    (mode, FWD, 2, 16, 20, 64, 2, (0, 10), 0, -1), (mode, BWD, 2, 16, 20, 64, 2, (8, 0), 0, -1),
    # no partitions: nothing to launch.  On the LDS shapes that is answered before the formats are looked at, on the others after
    (mode, FWD, 0, 16, 20, 64, 2, (8, 10), 0, 0), (mode, BWD, 0, 16, 20, 64, 2, (8, 10), 0, 0), (mode, FWD, 0, 16, 20, 64, 2, (8, 10), O16, 0),
    (mode, BWD, 0, 16, 20, 64, 2, (8, 10), QKV16 | O16, 0), (mode, FWD, 2, 0, 20, 64, 2, (8, 10), QKV16, 0),
    (mode, FWD, 0, 16, 20, 32, 2, (8, 10), 0, 0), (mode, BWD, 2, 16, 0, 40, 2, (8, 10), 0, 0), (mode, FWD, 0, 16, 20, 32, 2, (8, 10), QKV16, -3),
    (mode, BWD, 0, 16, 20, 40, 2, (8, 10), DQKV16, -3), (mode, FWD, 0, 24, 24, 64, 2, (12, 12), 0, -3), (mode, BWD, 0, 12, 16, 32, 2, (6, 8), 0, -3),
    # a head dimension of 0 has no kernel
    (mode, FWD, 2, 16, 20, 0, 2, (8, 10), 0, -3),
    # the RVT-S stages of the benchmarked step (window partitions of 8 x 10 on Gen1): B = T * batch frames
    (mode, FWD, 168, 64, 80, 48, 2, (8, 10), 0, 20524), (mode, BWD, 168, 32, 40, 96, 4, (8, 10), 0, 20524),
    (mode, FWD, 168, 16, 20, 192, 8, (8, 10), 0, 20524), (mode, BWD, 168, 8, 10, 384, 16, (8, 10), 0, 20524),
)) + tuple(
    (mode, entry, 168, H, W, C, heads, (8, 10), flags, 30524)
    for mode in ('bf16', '16f') for H, W, C, heads in ((64, 80, 48, 2), (32, 40, 96, 4), (16, 20, 192, 8), (8, 10, 384, 16))
    for entry, flags in ((FWD, QKV16), (FWD, QKV16 | O16), (BWD, QKV16 | DQKV16), (BWD, QKV16 | O16 | DQKV16)))

# ---------------------------------------------------------------------------------------------------------------------------------------
# ConvLSTM sequence
# ---------------------------------------------------------------------------------------------------------------------------------------
LSTM_CS = tuple(sorted(set(range(16, 529, 16)) | set(range(48, 529, 48))))

# leod_convlstm_seq_mode (0 where not listed), leod_convlstm_seq_gates16_ok (1 for the listed) and leod_convlstm_seq_pack_bytes (0 where
# not listed) over LSTM_CS, as recorded
SEQ_MODE = {'f32': {32: 1, 48: 1, 64: 2, 96: 2, 128: 2},
            'bf16': {32: 1, 48: 1, 64: 1, 96: 1, 128: 2, 192: 3, 256: 3, 384: 3, 512: 3},
            '16f': {32: 1, 48: 1, 64: 1, 96: 1, 128: 2, 192: 3, 256: 3, 384: 3, 512: 3}}
GATES16_OK = {'f32': (), 'bf16': (32, 48, 64, 96, 128, 192, 256, 384, 512), '16f': (32, 48, 64, 96, 128, 192, 256, 384, 512)}
PACK_BYTES = {'f32': {}, 'bf16': {192: 589824, 256: 1048576, 384: 2359296, 512: 4194304}, '16f': {192: 589824, 256: 1048576, 384: 2359296, 512: 4194304}}

# (entry, flags) -> ({C: code}, the answer for every other C of LSTM_CS), per mode.  Forward: gates16 without the 16-bit mode or without a
# sequence kernel is -1, before anything else; a projection flag that contradicts the mode (or no kernel at all) -3; a streamed route
# without its pack -1.  Backward: the projection flag is not looked at; -3 where no backward sequence kernel exists -- precision mode f32
# at C = 192 among them, which the autograd function answers with the per-timestep kernels.
_F32_FUSED, _F32_HOIST = {32: 1032, 48: 1048}, {64: 2064, 96: 2096, 128: 2128}
_F32_BWD = {32: 4032, 48: 4048, 64: 4064, 96: 4096, 128: 4128}
_B16_FUSED, _B16_HOIST = {32: 1032, 48: 1048, 64: 1064, 96: 1096}, {128: 2128}
_B16_STREAM = {192: 3192, 256: 3256, 384: 3384, 512: 3512}
_B16_NOPACK = {192: -1, 256: -1, 384: -1, 512: -1}
_B16_BWD = {32: 4032, 48: 4048, 64: 4064, 96: 4096, 128: 4128}
_B16_NOT_FUSED = {128: -3, 192: -3, 256: -3, 384: -3, 512: -3}      # gates16 is known there, the fused call is not
_B16 = {
    (FWD, 0): (_B16_FUSED, -3), (FWD, PACK): (_B16_FUSED, -3),
    (FWD, PROJ): ({**_B16_HOIST, **_B16_NOPACK}, -3), (FWD, PROJ | PACK): ({**_B16_HOIST, **_B16_STREAM}, -3),
    (FWD, GATES16): ({**_B16_FUSED, **_B16_NOT_FUSED}, -1), (FWD, GATES16 | PACK): ({**_B16_FUSED, **_B16_NOT_FUSED}, -1),
    (FWD, GATES16 | PROJ): ({32: -3, 48: -3, 64: -3, 96: -3, 128: 2128, 192: -1, 256: -1, 384: -1, 512: -1}, -1),
    (FWD, GATES16 | PROJ | PACK): ({32: -3, 48: -3, 64: -3, 96: -3, 128: 2128, **_B16_STREAM}, -1),
    (BWD, 0): ({**_B16_BWD, **_B16_NOPACK}, -3), (BWD, PROJ): ({**_B16_BWD, **_B16_NOPACK}, -3),
    (BWD, PACK): ({**_B16_BWD, **_B16_STREAM}, -3), (BWD, PROJ | PACK): ({**_B16_BWD, **_B16_STREAM}, -3),
    (BWD, GATES16): ({**_B16_BWD, **_B16_NOPACK}, -1), (BWD, GATES16 | PROJ): ({**_B16_BWD, **_B16_NOPACK}, -1),
    (BWD, GATES16 | PACK): ({**_B16_BWD, **_B16_STREAM}, -1), (BWD, GATES16 | PROJ | PACK): ({**_B16_BWD, **_B16_STREAM}, -1),
}
# (in a fused mode the hoisted call is refused with -3 and vice versa: 128 under (FWD, 0) and 32 .. 96 under (FWD, PROJ) are the default)
LSTM = {
    'f32': {
        (FWD, 0): (_F32_FUSED, -3), (FWD, PACK): (_F32_FUSED, -3), (FWD, PROJ): (_F32_HOIST, -3), (FWD, PROJ | PACK): (_F32_HOIST, -3),
        (FWD, GATES16): ({}, -1), (FWD, GATES16 | PACK): ({}, -1), (FWD, GATES16 | PROJ): ({}, -1), (FWD, GATES16 | PROJ | PACK): ({}, -1),
        (BWD, 0): (_F32_BWD, -3), (BWD, PACK): (_F32_BWD, -3), (BWD, PROJ): (_F32_BWD, -3), (BWD, PROJ | PACK): (_F32_BWD, -3),
        (BWD, GATES16): ({}, -1), (BWD, GATES16 | PACK): ({}, -1), (BWD, GATES16 | PROJ): ({}, -1), (BWD, GATES16 | PROJ | PACK): ({}, -1),
    },
    'bf16': _B16,
    '16f': _B16,
}


def lstm_rows():
    """(mode, entry, C, flags, expected)"""
    for mode in MODES:
        for (entry, flags), (codes, other) in LSTM[mode].items():
            for C in LSTM_CS:
                yield (mode, entry, C, flags, codes.get(C, other))


# channel counts outside the sweep, and an unknown entry
LSTM_EXTRA = tuple(r for mode in MODES for r in (
    (mode, FWD, 0, 0, -3), (mode, FWD, -32, PROJ | PACK, -3), (mode, BWD, 0, PACK, -3), (mode, BWD, 40, PACK, -3), (mode, FWD, 1024, PROJ | PACK, -3),
    (mode, BWD, 1024, PACK, -3), (mode, FWD, 40, GATES16, -1), (mode, 2, 48, 0, -1), (mode, -1, 48, 0, -1)))


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ops():
    import __graft_entry__ as g
    g.build()
    from leod_amd import ops as o
    prev = o.get_precision()
    yield o
    o.set_precision(prev)


def test_attn_route_table(ops):
    rows = list(attn_rows()) + list(ATTN_EXTRA)
    assert len(set(rows)) == len(rows) and len({r[:-1] for r in rows}) == len(rows)
    bad = []
    for r in rows:
        mode, entry, B, H, W, C, heads, part, flags, want = r
        ops.set_precision(mode)
        got = ops.partition_attn_route(entry, B, H, W, C, heads, part, flags)
        if got != want:
            bad.append((r, got))
    assert not bad, f'{len(bad)} of {len(rows)} rows differ, first (row, got): {bad[:5]}'


def test_attn_predicates_are_the_recorded_ones(ops):
    """leod_partition_attn_16bit_ok / _o16_ok on every geometry of the table: the recorded values, and "both directions route to F = 3"."""
    lib, n = ops._l(), 0
    for mode in MODES:
        ops.set_precision(mode)
        for _, _, B, H, W, C, heads, (ph, pw), _, _ in (r for r in list(attn_rows()) + list(ATTN_EXTRA) if r[0] == mode and r[1] in (FWD, BWD)):
            if ph <= 0 or pw <= 0:
                continue                                     # (asked with an empty partition the predicates used to divide by zero)
            ok = heads > 0 and C % heads == 0 and H % ph == 0 and W % pw == 0
            d, PT = (C // heads, (ph * pw + 15) // 16) if ok else (0, 1)
            want = int(ok and OK16[mode].get(d, '0' * 16)[PT - 1] == '1')
            assert lib.leod_partition_attn_16bit_ok(B, H, W, C, heads, ph, pw) == want, (mode, B, H, W, C, heads, ph, pw)
            assert lib.leod_partition_attn_o16_ok(B, H, W, C, heads, ph, pw) == want, (mode, B, H, W, C, heads, ph, pw)
            assert ops.partition_attn_16bit_ok(B, H, W, C, heads, (ph, pw)) == bool(want)
            if B * H * W > 0:
                both = all(ops.partition_attn_route(e, B, H, W, C, heads, (ph, pw), f) // 10000 == 3 for e, f in ((FWD, QKV16), (BWD, QKV16 | DQKV16)))
                assert both == bool(want), (mode, B, H, W, C, heads, ph, pw)
            n += 1
    assert n > 5000


def test_lstm_route_table(ops):
    rows = list(lstm_rows()) + list(LSTM_EXTRA)
    assert len({r[:-1] for r in rows}) == len(rows)
    bad = []
    for r in rows:
        mode, entry, C, flags, want = r
        ops.set_precision(mode)
        got = ops.convlstm_seq_route(entry, C, flags)
        if got != want:
            bad.append((r, got))
    assert not bad, f'{len(bad)} of {len(rows)} rows differ, first (row, got): {bad[:5]}'


def test_lstm_predicates_are_the_recorded_ones(ops):
    lib = ops._l()
    for mode in MODES:
        ops.set_precision(mode)
        for C in LSTM_CS + (0, 40, 1024):
            assert ops.convlstm_seq_mode(C) == SEQ_MODE[mode].get(C, 0), (mode, C)
            assert ops.convlstm_gates16_ok(C) == (C in GATES16_OK[mode]), (mode, C)
            assert lib.leod_convlstm_seq_pack_bytes(C) == PACK_BYTES[mode].get(C, 0), (mode, C)
            # ... and they are what the route says: the forward family; a backward kernel with gates16; a streamed backward
            fwd = [ops.convlstm_seq_route(FWD, C, PACK | p) for p in (0, PROJ)]
            assert ops.convlstm_seq_mode(C) == max([c // 1000 for c in fwd if c > 0], default=0)
            assert ops.convlstm_gates16_ok(C) == (ops.convlstm_seq_route(BWD, C, GATES16 | PACK) > 0)
            assert (lib.leod_convlstm_seq_pack_bytes(C) != 0) == (ops.convlstm_seq_route(BWD, C, PACK) // 1000 == 3)
            # the pack call refuses a channel count without a streamed route before it looks at anything else (NULL pointers: -1 either way)
            assert lib.leod_convlstm_seq_pack(None, None, C, None) == -1


def _attn_possible_codes():
    """every code attn_route can return: F = 1 on the twelve (PT, 16 DCH) instantiations, F = 2 / 3 on the sixteen (PT, d)"""
    reg = {10000 + 100 * PT + 16 for PT in (1, 2, 4, 5)} | {10000 + 100 * PT + 32 for PT in (1, 2, 3, 4, 5, 8, 10, 15)}
    lds = {F * 10000 + 100 * PT + d for F in (2, 3) for PT in (1, 2, 3, 4, 5, 8, 10, 15) for d in (24, 32)}
    return reg | lds | {0, -1, -3}


def test_every_code_has_a_row_and_every_launching_triple_a_gpu_case():
    """The per-route GPU tests (test_attn_every_route / test_convlstm_seq_every_route in tests/test_kernels_gpu.py, mode f32; their
    16-bit twins in tests/test_bf16_gpu.py, modes bf16 and 16f) run exactly the (entry, code) pairs that launch in these tables."""
    arows, lrows = list(attn_rows()) + list(ATTN_EXTRA), list(lstm_rows()) + list(LSTM_EXTRA)
    assert {r[-1] for r in arows} == _attn_possible_codes()
    lstm_codes = {f * 1000 + C for f, Cs in ((1, (32, 48, 64, 96)), (2, (64, 96, 128)), (3, (192, 256, 384, 512)), (4, (32, 48, 64, 96, 128))) for C in Cs}
    assert {r[-1] for r in lrows} == lstm_codes | {-1, -3}
    import test_kernels_gpu as tk
    import test_bf16_gpu as tb
    for modes, acases, lcases in ((('f32',), tk.ATTN_ROUTE_CASES_F32, tk.LSTM_SEQ_ROUTE_CASES_F32), (('bf16', '16f'), tb.ATTN_ROUTE_CASES_16, tb.LSTM_SEQ_ROUTE_CASES_16)):
        for mode in modes:
            ran = {(e, c) for case in acases for e, c in enumerate(case[-1])}
            table = {(r[1], r[-1]) for r in arows if r[0] == mode and r[-1] > 0}
            assert ran == table, (mode, 'in the table, never run:', sorted(table - ran), 'run, not in the table:', sorted(ran - table))
            # ... and the codes the cases name are the table's for exactly those arguments (B = 1, H = 2 ph, W = 2 pw, two heads)
            have = {r[:-1]: r[-1] for r in arows}
            for (ph, pw), d, t16, want in acases:
                flags = ((QKV16, QKV16 | DQKV16) if t16 else (0, 0))
                assert tuple(have[(mode, e, 1, 2 * ph, 2 * pw, 2 * d, 2, (ph, pw), flags[e])] for e in (FWD, BWD)) == tuple(want)
            ran = {(e, c) for case in lcases for e, c in enumerate(case[-1])}
            table = {(r[1], r[-1]) for r in lrows if r[0] == mode and r[-1] > 0}
            assert ran == table, (mode, 'in the table, never run:', sorted(table - ran), 'run, not in the table:', sorted(ran - table))
            have = {r[:-1]: r[-1] for r in lrows}
            for C, want in lcases:
                fl = (PROJ if want[0] >= 2000 else 0) | (PACK if want[0] >= 3000 else 0)
                for g16 in ((0, GATES16) if mode != 'f32' else (0,)):
                    assert (have[(mode, FWD, C, fl | g16)], have[(mode, BWD, C, (fl & PACK) | g16)]) == tuple(want)
