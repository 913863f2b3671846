"""Every route of the five dense-convolution entry points (csrc/conv_route.hpp: conv_route / launch_conv) on operands for which the result is
EXACT (tests/conv_exact.py): ``torch.equal`` against a float64 CPU reference -- forward with bias and BatchNorm column statistics, input
gradient (written, then accumulated twice onto a non-zero start), weight gradient and bias gradient (called twice on a non-zero start).

Rows.  The shapes of the per-route lists of the tolerance tests (test_kernels_gpu.CONV_ROUTE_CASES_F32 / STEM_ROUTE_CASES_F32 in mode f32,
test_bf16_gpu.CONV_ROUTE_CASES_16 / STEM_ROUTE_CASES_16 in modes bf16 and 16f; the rows with pack = False go through the raw C ABI), plus
geometry rows at the smallest shape that reaches the route while showing the feature -- the places where the index arithmetic changes:

  implicit GEMM, register-direct (19xxx) and LDS-staged (17xxx / 18xxx, from 2048 rows and 256 workgroups): B >= 2 with H W no multiple of
      the 16- / 64-row tile, so that a tile spans two images and the last one is ragged (5 x 7, 15 x 17; stride 2 on 15 x 31 and 15 x 17);
      odd H and W at stride 2 (1 x 7 x 9); Cin and N no multiple of 16 (36 -> 100)
  parity-class dgrad: the register form (Q = B (H / 2) (W / 2): 48 and 32, multiples of 16 but not of 128) with B >= 2; its LDS form
      (Q % 128 == 0) is in the lists
  direct 3x3 (110 / 120 / 220 / 500; 16-bit modes), shapes of test_conv3x3_direct_bf16 / test_conv3x3_strided_sliced_direct_bf16 at the
      smallest B that keeps the feature: B >= 2; ragged last row block (H = 9, H = 5); W no multiple of 16 (7, 12, 20); two column segments
      (W = 160 at 128 channels); output-channel slices (96 -> 192, 192 -> 384 at 16 x 20); many regions per worker (B = 70 at 8 x 12); both
      strides of 192 -> 192; ragged stride-2 regions (10 x 12, 6 x 8)
  stem: stored frame smaller than the padded one in H only, in W only, in both; W % 4 != 0 (60 x 90 in 64 x 96) as uint8 and as fp32; an
      address that is no multiple of 4; 24 channels; ks = 5; N = 16 / 32 / 48 / 64.  Every frame lies inside a buffer of sentinels
      (conv_exact.frame_buffer)
  1x1 weight gradients of the 16-bit modes: wgradw configurations 301 - 305 are rows of the lists (305 from 65 537 rows on)

Conv rows: (B, H, W, Cin, N, ks, stride, bias, pack offered, (forward, dgrad, wgrad) codes); stem rows: (B, H, W, Cin, N, ks, stride, pad,
uint8, aligned, padded frame | None, (forward, wgrad) codes); eval-BatchNorm rows: (B, H, W, Cin, N, ks, stride, pack offered, code).
Every test first asserts that the router still sends the row there; tests/test_conv_exact_cpu.py asserts the same without a GPU, and that
every (entry, code) pair that launches in the table of tests/test_conv_routes_cpu.py has a row here.  The column statistics are taken in 1,
8 or 32 replicas by row; the sum over the replicas is compared, in float64.

Comparisons: equality everywhere, except the eval-mode BatchNorm + SiLU rows (fast_exp / fast_rcp / rsqrtf): the fp32 bound
``linear_exact.close_fp32`` in every precision mode.  ``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_exact as ce  # noqa: E402
import linear_exact as le  # noqa: E402
import test_bf16_gpu as tb  # noqa: E402
import test_kernels_gpu as tk  # noqa: E402

DEV = 'cuda'
MODES_16 = ('bf16', '16f')
STAT_REPLICAS = (1, 8, 32)

# the implicit GEMMs and the parity-class dgrad route alike in every mode
GEOM_GEMM = [
    (3, 5, 7, 16, 32, 3, 1, True, True, (19024, 19014, 724)), (2, 5, 7, 36, 100, 3, 1, False, True, (19014, 19034, 714)),
    (1, 7, 9, 64, 48, 3, 2, False, True, (19034, 19044, 734)), (3, 7, 9, 36, 100, 3, 2, True, False, (19014, 19034, 714)),
    (70, 15, 31, 48, 96, 3, 2, False, True, (17348, 17348, 734)), (70, 15, 31, 48, 96, 3, 2, False, False, (18348, 18348, 734)),
    (35, 15, 17, 36, 100, 3, 1, True, True, (17164, 19034, 714)), (33, 15, 17, 36, 100, 3, 2, False, False, (18164, 19034, 714)),
    (3, 8, 8, 32, 32, 3, 2, False, True, (19024, 29024, 724)), (2, 8, 8, 48, 16, 3, 2, False, True, (19014, 29031, 714)),
    (3, 5, 7, 36, 100, 1, 1, True, True, (6011, 6031, 414)),
]
GEOM_F32 = GEOM_GEMM + [
    (35, 15, 17, 48, 96, 3, 1, False, True, (17348, 19034, 734)), (40, 15, 17, 96, 96, 1, 1, True, True, (4348, 4348, 434)),
]
GEOM_16 = GEOM_GEMM + [
    (35, 15, 17, 48, 96, 3, 1, True, True, (17348, 110, 734)), (40, 15, 17, 96, 96, 1, 1, True, True, (4348, 4348, 304)),
    # direct 3x3
    (2, 5, 7, 96, 48, 3, 1, False, True, (110, 110, 734)), (2, 9, 12, 48, 96, 3, 1, False, True, (110, 110, 734)),
    (2, 5, 7, 96, 96, 3, 1, False, True, (110, 110, 500)), (2, 9, 20, 96, 96, 3, 1, False, True, (110, 110, 500)),
    (2, 16, 20, 192, 192, 3, 1, False, True, (110, 110, 500)), (1, 12, 160, 128, 128, 3, 1, False, True, (110, 110, 500)),
    (2, 13, 160, 64, 64, 3, 1, False, True, (110, 110, 500)), (2, 7, 12, 128, 128, 3, 1, False, True, (110, 110, 500)),
    (2, 18, 28, 96, 192, 3, 1, False, True, (110, 110, 500)), (70, 9, 12, 96, 96, 3, 1, False, True, (110, 110, 500)),
    (2, 16, 20, 192, 384, 3, 2, False, True, (120, 220, 500)), (70, 8, 12, 96, 96, 3, 2, False, True, (120, 220, 500)),
    (2, 16, 20, 192, 192, 3, 2, False, True, (120, 220, 500)), (2, 10, 12, 48, 96, 3, 2, False, True, (120, 220, 500)),
    (2, 6, 8, 96, 96, 3, 2, False, True, (120, 220, 500)), (2, 32, 40, 96, 192, 3, 2, False, True, (120, 220, 500)),
]
GEOM_STEM_F32 = [
    (2, 60, 96, 20, 48, 7, 4, 3, True, True, (64, 96), (613, 633)), (2, 64, 92, 20, 48, 7, 4, 3, True, True, (64, 96), (613, 633)),
    (2, 64, 96, 20, 48, 7, 4, 3, True, True, None, (613, 633)), (3, 36, 52, 20, 32, 7, 4, 3, True, True, (40, 64), (612, 632)),
    (2, 60, 90, 20, 48, 7, 4, 3, True, True, (64, 96), (39034, 834)), (2, 60, 90, 20, 48, 7, 4, 3, False, True, (64, 96), (49034, 934)),
    (2, 60, 92, 20, 32, 7, 4, 3, True, False, (64, 96), (39024, 824)), (2, 61, 92, 24, 48, 7, 4, 3, True, True, (64, 96), (613, 834)),
]
GEOM_STEM_16 = [
    (2, 60, 96, 20, 48, 7, 4, 3, True, True, (64, 96), (603, 623)), (2, 64, 92, 20, 48, 7, 4, 3, True, True, (64, 96), (603, 623)),
    (2, 64, 96, 20, 48, 7, 4, 3, True, True, None, (603, 623)), (3, 36, 52, 20, 32, 7, 4, 3, True, True, (40, 64), (602, 622)),
    (2, 60, 90, 20, 48, 7, 4, 3, True, True, (64, 96), (39034, 834)), (2, 60, 90, 20, 48, 7, 4, 3, False, True, (64, 96), (49034, 934)),
    (2, 60, 92, 20, 32, 7, 4, 3, True, False, (64, 96), (39024, 824)),
]
CONV_ROWS = {'f32': tk.CONV_ROUTE_CASES_F32 + GEOM_F32, '16': tb.CONV_ROUTE_CASES_16 + GEOM_16}
STEM_ROWS = {'f32': tk.STEM_ROUTE_CASES_F32 + GEOM_STEM_F32, '16': tb.STEM_ROUTE_CASES_16 + GEOM_STEM_16}

# eval-mode BatchNorm + SiLU: one row per forward code of CONV_ROWS, at the smallest shape of those lists that the router sends there when it
# is asked with CF_BN, no statistics and no bias (tests/test_conv_exact_cpu.py: test_every_forward_code_has_an_eval_bn_row)
BN_ROWS = {
    'f32': [
        (2, 64, 64, 48, 96, 1, 1, True, 4348), (32, 32, 40, 20, 40, 1, 1, True, 4364), (2, 64, 64, 96, 192, 1, 1, True, 4448),
        (17, 32, 32, 32, 64, 1, 1, True, 4464), (68, 5, 7, 36, 100, 1, 1, True, 5164), (3, 32, 40, 16, 160, 1, 1, True, 5264),
        (1, 4, 4, 32, 16, 1, 1, True, 6011), (1, 4, 4, 16, 32, 1, 1, True, 6021), (68, 5, 7, 100, 36, 1, 1, True, 6031),
        (9, 2, 324, 192, 48, 1, 1, True, 6034), (1, 4, 4, 64, 128, 1, 1, True, 6041), (2, 32, 32, 512, 256, 1, 1, True, 6044),
        (17, 32, 32, 16, 16, 3, 1, True, 17148), (33, 15, 17, 36, 100, 3, 2, True, 17164), (17, 32, 32, 64, 32, 3, 1, True, 17248),
        (17, 64, 64, 20, 32, 3, 2, True, 17264), (2, 64, 64, 48, 96, 3, 1, True, 17348), (32, 32, 40, 20, 40, 3, 1, True, 17364),
        (17, 32, 32, 32, 64, 3, 1, True, 17448), (33, 15, 17, 36, 100, 3, 2, False, 18164), (2, 64, 64, 48, 96, 3, 1, False, 18348),
        (1, 8, 8, 48, 16, 3, 2, True, 19014), (1, 4, 4, 16, 32, 3, 1, True, 19024), (1, 4, 4, 192, 48, 3, 1, True, 19034),
        (1, 4, 4, 32, 64, 3, 2, True, 19044),
    ],
    '16': [
        (1, 4, 4, 48, 48, 3, 1, True, 110), (1, 8, 8, 48, 96, 3, 2, True, 120), (2, 64, 64, 96, 192, 1, 1, True, 3043),
        (1, 64, 64, 32, 256, 1, 1, True, 3044), (40, 15, 17, 96, 96, 1, 1, True, 4348), (32, 32, 40, 20, 40, 1, 1, True, 4364),
        (1, 32, 64, 96, 512, 1, 1, True, 4448), (68, 16, 16, 32, 64, 1, 1, True, 4464), (68, 16, 16, 16, 16, 1, 1, True, 5164),
        (2, 64, 64, 16, 160, 1, 1, True, 5264), (3, 5, 7, 36, 100, 1, 1, True, 6011), (1, 4, 4, 16, 32, 1, 1, True, 6021),
        (2, 5, 7, 20, 40, 1, 1, True, 6031), (9, 2, 324, 192, 48, 1, 1, True, 6034), (1, 4, 4, 64, 128, 1, 1, True, 6041),
        (1, 4, 4, 128, 128, 1, 1, True, 6044), (17, 64, 64, 16, 16, 3, 2, True, 17148), (33, 15, 17, 36, 100, 3, 2, True, 17164),
        (17, 32, 32, 16, 32, 3, 1, True, 17248), (17, 64, 64, 20, 32, 3, 2, True, 17264), (70, 15, 31, 48, 96, 3, 2, True, 17348),
        (32, 32, 40, 20, 40, 3, 1, True, 17364), (17, 32, 32, 32, 64, 3, 1, True, 17448), (33, 15, 17, 36, 100, 3, 2, False, 18164),
        (2, 64, 64, 48, 96, 3, 1, False, 18348), (1, 4, 4, 32, 16, 3, 1, True, 19014), (1, 4, 4, 16, 32, 3, 1, True, 19024),
        (1, 4, 4, 48, 48, 3, 1, False, 19034), (1, 8, 8, 96, 192, 3, 2, False, 19044),
        # the direct kernel's epilogue at a geometry with a ragged row block, two images and W no multiple of 16, and with channel slices
        (2, 9, 12, 48, 96, 3, 1, True, 110), (2, 10, 12, 48, 96, 3, 2, True, 120), (2, 16, 20, 192, 384, 3, 2, True, 120),
    ],
}


def klass(mode):
    return 'f32' if mode == 'f32' else '16'


def _cases(rows, nshape):
    """(mode, index in the row list, row), the modes of one shape side by side: the cached reference of a shape is computed once"""
    modes = ('f32',) + MODES_16
    cases = [(m, i, r) for m in modes for i, r in enumerate(rows[klass(m)])]
    return sorted(cases, key=lambda c: (str(c[2][:nshape]), modes.index(c[0]), c[1]))


def conv_cases():
    return _cases(CONV_ROWS, 8)


def stem_cases():
    return _cases(STEM_ROWS, 9)


def bn_cases():
    return _cases(BN_ROWS, 7)


def conv_routes_of(ops, row):
    B, H, W, Cin, N, ks, st, bias, pack = row[:9]
    pad, pk = (ks - 1) // 2, ce.PACK if pack else 0
    return (ops.conv_route(0, B, H, W, Cin, N, ks, st, pad, ce.COLSTATS | pk | (ce.BIAS if bias else 0)), ops.conv_route(1, B, H, W, Cin, N, ks, st, pad, pk),
            ops.conv_route(2, B, H, W, Cin, N, ks, st, pad, ce.WS | (ce.DBIAS if bias else 0)))


def stem_routes_of(ops, row):
    B, H, W, Cin, N, ks, st, pad, u8, aligned, padded = row[:11]
    fl = (ce.U8 if u8 else 0) | (ce.ALIGN4 if aligned else 0)
    return ops.conv_route(3, B, H, W, Cin, N, ks, st, pad, fl, padded), ops.conv_route(4, B, H, W, Cin, N, ks, st, pad, fl, padded)


def bn_route_of(ops, row):
    B, H, W, Cin, N, ks, st, pack = row[:8]
    return ops.conv_route(0, B, H, W, Cin, N, ks, st, (ks - 1) // 2, ce.BN | (ce.PACK if pack else 0))


def _id(case):
    mode, i, row = case
    return mode + '-' + '-'.join(str(v) for v in (row[-1] if isinstance(row[-1], tuple) else (row[-1],))) + '@' + 'x'.join(str(v) for v in row[:5]) + f'#{i}'


@pytest.fixture
def ops_in():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops
    prev = ops.get_precision()

    def enter(mode):
        ops.set_precision(mode)
        return ops
    yield enter
    ops.set_precision(prev)


def same(got, ref, what):
    got, ref = got.cpu(), ref.to(got.dtype)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: {len(bad)} of {ref.numel()} elements differ, first at {first}: got {got[first].item()}, exact {ref[first].item()}')


def bounded(p):
    b = ce.bounds(p)
    assert all(v < ce.LIMIT for v in b.values()), b


@pytest.mark.parametrize('case', conv_cases(), ids=_id)
def test_conv_exact(ops_in, case):
    mode, idx, row = case
    ops = ops_in(mode)
    B, H, W, Cin, N, ks, stride, bias, pack, want = row
    assert conv_routes_of(ops, row) == tuple(want), 'the shape no longer reaches the routes this row is here for'
    p = ce.problem(B, H, W, Cin, N, ks, stride, bias)
    bounded(p)
    ref, pad = p['ref'], p['pad']
    x, w, dy = p['x'].to(DEV), p['w'].to(DEV), p['dy'].to(DEV)
    b = p['bias'].to(DEV) if bias else None
    R = STAT_REPLICAS[idx % 3]
    cs = torch.zeros((2, N) if R == 1 else (R, 2, N), dtype=torch.float64, device=DEV)
    dx1 = dx2 = None
    if pack:
        y = ops.conv_nhwc_fwd(x, w, b, stride=stride, colstats=cs)
        dx = ops.conv_nhwc_dgrad(dy, w, x.shape, stride=stride)
        acc = p['dx0'].to(DEV)
        dx1 = ops.conv_nhwc_dgrad(dy, w, x.shape, stride=stride, out=acc, accumulate=True).clone()
        dx2 = ops.conv_nhwc_dgrad(dy, w, x.shape, stride=stride, out=acc, accumulate=True)
    else:
        lib, ptr, st = ops._l(), ops._p, ops._stream()
        y, dx, acc = torch.empty(tuple(ref['y'].shape), device=DEV), torch.empty_like(x), p['dx0'].to(DEV)
        assert lib.leod_conv_nhwc_fwd(ptr(x), ptr(w), ptr(b), ptr(y), ptr(cs), R, None, None, None, None, 1e-5, B, H, W, Cin, N, ks, stride, pad, None, 0, st) == 0
        assert lib.leod_conv_nhwc_dgrad(ptr(dy), ptr(w), ptr(dx), 0, B, H, W, Cin, N, ks, stride, pad, None, 0, st) == 0
        assert lib.leod_conv_nhwc_dgrad(ptr(dy), ptr(w), ptr(acc), 1, B, H, W, Cin, N, ks, stride, pad, None, 0, st) == 0
        dx1 = acc.clone()
        assert lib.leod_conv_nhwc_dgrad(ptr(dy), ptr(w), ptr(acc), 1, B, H, W, Cin, N, ks, stride, pad, None, 0, st) == 0
        dx2 = acc
    same(y, ref['y'], 'forward')
    tot = cs if R == 1 else cs.sum(0)
    same(tot[0], ref['s1'], f'column sums ({R} replicas)')
    same(tot[1], ref['s2'], f'column sums of squares ({R} replicas)')
    same(dx, ref['dx'], 'dgrad')
    same(dx1, ref['dx_acc'][0], 'dgrad accumulating, first call')
    same(dx2, ref['dx_acc'][1], 'dgrad accumulating, second call')
    dw, db = p['dw0'].to(DEV), (p['db0'].to(DEV) if bias else None)
    for n in (0, 1):
        ops.conv_nhwc_wgrad(dy, x, dw, db, stride=stride)
        same(dw, ref['dw'][n], f'wgrad, call {n + 1}')
        if bias:
            same(db, ref['db'][n], f'dbias, call {n + 1}')


@pytest.mark.parametrize('case', stem_cases(), ids=_id)
def test_stem_exact(ops_in, case):
    mode, idx, row = case
    ops = ops_in(mode)
    B, H, W, Cin, N, ks, stride, pad, u8, aligned, padded, want = row
    assert stem_routes_of(ops, row) == tuple(want), 'the shape no longer reaches the routes this row is here for'
    p = ce.stem_problem(B, H, W, Cin, N, ks, stride, pad, u8, padded)
    bounded(p)
    buf, xd = ce.frame_buffer(p['x'], aligned, DEV)
    assert (xd.data_ptr() % 4 == 0) == aligned
    w, dy = p['w'].to(DEV), p['dy'].to(DEV)
    same(ops.stem_conv_fwd(xd, w, p['padded'], stride, pad), p['ref']['y'], 'stem forward')
    dw = p['dw0'].to(DEV)
    for n in (0, 1):
        ops.stem_conv_wgrad(dy, xd, dw, p['padded'], stride, pad)
        same(dw, p['ref']['dw'][n], f'stem wgrad, call {n + 1}')
    same(xd, p['x'], 'the frame itself')


@pytest.mark.parametrize('case', bn_cases(), ids=_id)
def test_conv_eval_bn_exact_underneath(ops_in, case):
    mode, idx, row = case
    ops = ops_in(mode)
    B, H, W, Cin, N, ks, stride, pack, want = row
    assert bn_route_of(ops, row) == want, 'the shape no longer reaches the route this row is here for'
    q = ce.bn_problem(B, H, W, Cin, N, ks, stride)
    p = q['p']
    bounded(p)
    x, w = p['x'].to(DEV), p['w'].to(DEV)
    bn = tuple(t.to(DEV) for t in q['bn'])
    if pack:
        y = ops.conv_nhwc_fwd(x, w, None, stride=stride, bn=bn, bn_eps=ce.BN_EPS)
    else:
        lib, ptr = ops._l(), ops._p
        y = torch.empty(tuple(p['ref']['y'].shape), device=DEV)
        assert lib.leod_conv_nhwc_fwd(ptr(x), ptr(w), None, ptr(y), None, 1, ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), ce.BN_EPS, B, H, W, Cin, N, ks, stride,
                                      p['pad'], None, 0, ops._stream()) == 0
    le.close_fp32(y, q['ref'], what='silu(bn(conv)), eval mode')
