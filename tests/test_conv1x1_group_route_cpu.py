"""The routing of the grouped 1x1 / stride-1 convolutions, pinned without a GPU: ``leod_conv1x1_group_route`` -- the decision
``leod_conv1x1_group_fwd`` / ``_dgrad`` switch on; it launches nothing and reads only host state -- against a literal table.

A code is 1 followed by one digit per member: the member's 16-row fragments per workgroup (2: 32-row tiles, 4: 64-row tiles, taken by maps of
8192 rows and more while the contraction length is 48, 96 or 192).  -1: bad arguments, -3: not covered (run the members singly).  Members of 8192
rows or more are no faster here than alone (profiles/r18_a_kbench_conv1x1_16f.txt) and gain only by the launch they share: a group of such
members alone is refused, unless it is a forward group of two or more.  A member
whose single call runs on the wide-tile kernel (leod_conv_route 3000 + ..: 32 k per MFMA, sums the grouped kernel cannot reproduce bit for
bit) refuses the group; one whose single call splits K over four waves (6000 + 10 NT + 4) keeps 32-row tiles."""
import pytest

MODES = ('f32', 'bf16', '16f')
FWD, DGRAD = 0, 1
COLSTATS, ACCUMULATE = 2, 64

# the 1x1 / stride-1 convolutions of the benchmarked step (PAFPN and head stems on the 32 labelled frames): (rows, Cin, N)
STEP = ((2560, 384, 192), (2560, 192, 192), (2560, 384, 384), (2560, 384, 96),
        (10240, 384, 96), (10240, 96, 96), (10240, 192, 192), (10240, 192, 96),
        (40960, 192, 48), (40960, 48, 48), (40960, 96, 96))
# entry -> the code of each of them as a one-member group in the 16-bit modes
SINGLE = {FWD: (12, 12, 12, 12, -3, -3, -3, -3, -3, -3, -3),              # a lone long map: its single call
          DGRAD: (12, 12, 12, 12, -3, -3, -3, -3, -3, -3, -3)}
# the groups of the step: conv1 | conv2 of the four CSP layers, the three head stems (forward; their input gradients leave in two rounds)
GROUPS = (
    (FWD, ((2560, 384, 192), (2560, 384, 192)), 122),
    (FWD, ((10240, 384, 96), (10240, 384, 96)), 122),
    (FWD, ((10240, 192, 96), (10240, 192, 96)), 144),
    (FWD, ((40960, 192, 48), (40960, 192, 48)), 144),
    (FWD, ((40960, 96, 96), (10240, 192, 96), (2560, 384, 96)), 1442),
    (DGRAD, ((40960, 96, 96), (10240, 192, 96), (2560, 384, 96)), 1442),
    (FWD, ((2560, 384, 192), (10240, 96, 96), (40960, 48, 48), (33, 16, 16)), 12442),
    (DGRAD, ((40960, 96, 96), (10240, 192, 96)), -3),               # no short member: the single calls
    (DGRAD, ((10240, 192, 96), (33, 16, 16)), 142),
    (FWD, ((10240, 192, 192), (33, 16, 16)), -3),                   # a wide-tile member refuses the group
    (DGRAD, ((10240, 192, 192), (33, 16, 16)), -3),
    (FWD, ((8200, 192, 48), (33, 16, 16)), 122),                    # single call 6034 (K split over four waves): 32-row tiles
    (FWD, ((8200, 96, 48), (33, 16, 16)), 142),
)


@pytest.fixture(scope='module')
def ops():
    import __graft_entry__ as g
    g.build()
    from leod_amd import ops as o
    prev = o.get_precision()
    yield o
    o.set_precision(prev)


def _gemm(entry, shape):             # (rows, Cin, N) of the conv -> (rows, contraction length, output columns) of the entry's GEMM
    M, cin, n = shape
    return (M, cin, n) if entry == FWD else (M, n, cin)


def _ask(ops, entry, n, M, K, N, flags=0):
    import ctypes
    arr = lambda v: (ctypes.c_int * max(len(v), 1))(*v)  # noqa: E731
    from leod_amd import _lib
    return int(_lib.lib().leod_conv1x1_group_route(entry, n, arr(M), arr(K), arr(N), flags))


@pytest.mark.parametrize('mode', MODES)
def test_step_shapes(ops, mode):
    ops.set_precision(mode)
    for entry in (FWD, DGRAD):
        got = tuple(ops.conv1x1_group_route(entry, [_gemm(entry, s)]) for s in STEP)
        assert got == (SINGLE[entry] if mode != 'f32' else (-3,) * len(STEP)), (mode, entry, got)
    for entry, members, want in GROUPS:
        got = ops.conv1x1_group_route(entry, [_gemm(entry, s) for s in members])
        assert got == (want if mode != 'f32' else -3), (mode, entry, members, got)


def test_flags_do_not_move_the_route(ops):
    ops.set_precision('16f')
    for entry, flag in ((FWD, COLSTATS), (DGRAD, ACCUMULATE)):
        for s in STEP:
            assert ops.conv1x1_group_route(entry, [_gemm(entry, s)], flag) == ops.conv1x1_group_route(entry, [_gemm(entry, s)])
    assert _ask(ops, FWD, 1, [64], [32], [32], 1) == -1             # a flag the calls do not have


@pytest.mark.parametrize('mode', ('bf16', '16f'))
def test_coverage_edges(ops, mode):
    ops.set_precision(mode)
    for entry in (FWD, DGRAD):
        for K, want in ((0, -3), (8, -3), (16, 12), (24, -3), (384, 12), (400, -3)):
            assert _ask(ops, entry, 1, [64], [K], [32]) == want, (entry, 'K', K)
        for N, want in ((0, -3), (8, -3), (16, 12), (40, -3), (384, 12), (400, -3)):
            assert _ask(ops, entry, 1, [64], [32], [N]) == want, (entry, 'N', N)
        long = -3                                                    # a lone member of 8192 rows or more
        for M, want in ((0, -3), (1, 12), (8191, 12), (8192, long), (65536, long), (65537, -3)):
            assert _ask(ops, entry, 1, [M], [48], [32]) == want, (entry, 'M', M)
        assert _ask(ops, entry, 2, [65536, 64], [384, 32], [32, 32]) == 122    # 64-row tiles stop at K = 192 (LDS bound)
        assert _ask(ops, entry, 2, [65536, 64], [64, 32], [32, 32]) == 122     # ... and take the contraction lengths the kernel has a body for
        assert _ask(ops, entry, 2, [65536, 64], [96, 32], [32, 32]) == 142
        assert _ask(ops, entry, 2, [65536, 8192], [96, 48], [32, 32]) == (144 if entry == FWD else -3)   # long members only
        for n, want in ((0, -1), (1, 12), (4, 12222), (5, -1), (-1, -1)):
            m = max(n, 1)
            assert _ask(ops, entry, n, [64] * m, [32] * m, [32] * m) == want, (entry, 'n', n)
        # one member outside the coverage refuses the group
        assert _ask(ops, entry, 3, [64, 64, 64], [32, 400, 32], [32, 32, 32]) == -3
    assert _ask(ops, 2, 1, [64], [32], [32]) == -1                  # no such entry
    from leod_amd import _lib
    assert int(_lib.lib().leod_conv1x1_group_route(FWD, 1, None, None, None, 0)) == -1


def test_single_call_routes_are_untouched(ops):
    """The single-call entry points keep their routes for exactly these shapes: read from the existing table, not copied."""
    import test_conv_routes_cpu as tr
    have = {r[:-1]: r[-1] for r in tr.ROWS}
    asked = 0
    for mode in MODES:
        ops.set_precision(mode)
        for M, cin, n in STEP:
            B, H, W = 32, {2560: 8, 10240: 16, 40960: 32}[M], {2560: 10, 10240: 20, 40960: 40}[M]
            for entry, flags in ((0, 10), (1, 8), (0, 2), (1, 0)):
                key = (entry, mode, B, H, W, cin, n, 1, 1, 0, flags, None)
                if key in have:
                    assert ops.conv_route(entry, B, H, W, cin, n, 1, 1, 0, flags) == have[key], key
                    asked += 1
    assert asked >= 2 * 3 * 5, asked                                 # the table holds at least the named 1x1 convs of the step per mode
