"""Every route of the Linear weight gradients (leod_linear_wgrad, leod_linear_wgrad_group) on operands for which the result is EXACT
(tests/wgrad_exact.py): ``torch.equal`` against a float64 CPU reference, on a dW / dbias that do not start at zero, twice.

Each row of ROUTES names the kernel it is there for as a route code (leod_linear_wgrad_route: 100 + tile LDS-DMA, 200 + combination wide
kernel, 300 + configuration wgradw, 400 + 10 TN + TK wgrad16).  The test first asserts that the router still sends the row there -- a
moved threshold fails loudly instead of retargeting the case -- and test_route_table_is_complete keeps every instantiation in the table.

The predicates the shapes are derived from (16-bit modes unless stated; csrc/k_linear_wgrad.hip wgrad_route):
  DMA   M >= 8192, M % 64 == 0, N, K multiples of 96 (tile 6, M <= 60000) / 128 (tile 8) / 64 (tile 4), strides and K1 % 8 == 0; NOT for
        fp32 dy with fp32 / LayerNorm / fp16 rows when N K < 200000
  wide  M >= 8192, N % 8 (bf16 dy) or % 4, K % 8 (16-bit x) or % 4, and a combination: fp32 dy x {rows, gelu16, bf16 rows, fp16 rows},
        bf16 dy x {rows, ln}; concat counts as rows.  N, K <= 48: rows 1, bf16 rows 8, fp16 rows 14.  K <= 48: ln 2.  N <= 48: gelu16 3.
        N % 192 == 0 and K >= 96: ln 10, bf16-dy rows 11.  K % 192 == 0 and N >= 96: gelu16 12, bf16 rows 13, fp16 rows 16.  Else rows 4, ln 5,
        gelu16 6, bf16-dy rows 7, bf16 rows 9, fp16 rows 15.  Rows per chunk RC: 64 for 1, 6, 8, 12, 14, else 32.
  wgradw  M >= 8192 and none of the above: N, K <= 48: 1; K <= 48: 2; N <= 48: 3; else 4 (16-bit mode, M <= 65536, no LayerNorm) or 5
  wgrad16 M < 8192: N, K % 48 == 0: 33; gelu16: 44; N, K % 32 == 0 but not both % 64: 22; N, K >= 64: 44; K >= 64: 14; N >= 64: 41; else 11
``pytest -m gpu``."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_exact as we  # noqa: E402

DEV = 'cuda'
ERR_ARG, ERR_UNSUPPORTED = -1, -3
B, H, F = 'bf16', '16f', 'f32'

# (precision mode, dy bf16, x mode, M, N, K, route code[, K1 of concat])
ROUTES = []


def _rows(*rows):
    ROUTES.extend(rows)


# ---- wide kernel: per combination its smallest shapes; M = 8192, 8193, 8192 + RC - 1, 8192 + RC + 1 and a ragged ~20 k ------------------
# (M = 8192 is a multiple of 64: there the shape must be one the DMA kernel refuses -- a width below 64, a width that is no multiple
# of 64 (80, 104), or fp32 dy with fp32 / fp16 rows below N K = 200000)
_rows(  # 1: fp32 dy, fp32 rows (also [x | x2]), 48 x 48 tile, RC 64
    (B, 0, 'rows', 8192, 48, 48, 201), (H, 0, 'rows', 8193, 48, 48, 201), (B, 0, 'concat', 8255, 48, 48, 201, 16),
    (H, 0, 'rows', 8257, 20, 36, 201), (B, 0, 'rows', 20011, 48, 48, 201),
    # 2: bf16 dy, LayerNorm, K <= 48 < N, 192 x 48 tile, RC 32
    (B, 1, 'ln', 8192, 144, 48, 202), (H, 1, 'ln', 8193, 192, 48, 202), (B, 1, 'ln', 8223, 144, 40, 202), (H, 1, 'ln', 8225, 192, 48, 202),
    (B, 1, 'ln', 20011, 144, 48, 202),
    # 3: fp32 dy, gelu16, N <= 48 < K, 48 x 192 tile, RC 32
    (B, 0, 'gelu16', 8192, 48, 192, 203), (H, 0, 'gelu16', 8193, 32, 160, 203), (B, 0, 'gelu16', 8223, 48, 192, 203),
    (H, 0, 'gelu16', 8225, 32, 160, 203), (B, 0, 'gelu16', 20011, 48, 192, 203),
    # 4: fp32 dy, fp32 rows, 96 x 96 tile, RC 32 (96 x 96 at M = 8192: 9216 < 200000 keeps it off the DMA kernel)
    (B, 0, 'rows', 8192, 96, 96, 204), (H, 0, 'rows', 8193, 100, 68, 204), (B, 0, 'concat', 8223, 96, 96, 204, 32),
    (H, 0, 'rows', 8225, 96, 96, 204), (B, 0, 'rows', 20011, 96, 96, 204),
    # 5: bf16 dy, LayerNorm, 96 x 96 tile, RC 32 (M = 8192: K = 80 is no tile of the DMA kernel)
    (B, 1, 'ln', 8192, 96, 80, 205), (H, 1, 'ln', 8193, 96, 96, 205), (B, 1, 'ln', 8223, 96, 96, 205), (H, 1, 'ln', 8225, 104, 68, 205),
    (B, 1, 'ln', 20011, 96, 96, 205),
    # 6: fp32 dy, gelu16, 96 x 96 tile, RC 64
    (B, 0, 'gelu16', 8192, 96, 80, 206), (H, 0, 'gelu16', 8193, 96, 96, 206), (B, 0, 'gelu16', 8255, 96, 96, 206),
    (H, 0, 'gelu16', 8257, 100, 72, 206), (B, 0, 'gelu16', 20011, 96, 96, 206),
    # 7: bf16 dy, fp32 rows (also [x | x2]), 96 x 96 tile, RC 32
    (B, 1, 'rows', 8192, 96, 80, 207), (H, 1, 'concat', 8193, 96, 96, 207, 32), (B, 1, 'rows', 8223, 96, 96, 207),
    (H, 1, 'rows', 8225, 104, 68, 207), (B, 1, 'concat', 20011, 96, 96, 207, 64),
    # 8: fp32 dy, bf16 rows, 48 x 48 tile, RC 64
    (B, 0, 'bf16rows', 8192, 48, 48, 208), (B, 0, 'bf16rows', 8193, 20, 40, 208), (B, 0, 'bf16rows', 8255, 48, 48, 208),
    (B, 0, 'bf16rows', 8257, 48, 48, 208), (B, 0, 'bf16rows', 20011, 48, 48, 208),
    # 9: fp32 dy, bf16 rows, 96 x 96 tile, RC 32
    (B, 0, 'bf16rows', 8192, 96, 80, 209), (B, 0, 'bf16rows', 8193, 96, 96, 209), (B, 0, 'bf16rows', 8223, 96, 96, 209),
    (B, 0, 'bf16rows', 8225, 100, 72, 209), (B, 0, 'bf16rows', 20011, 96, 96, 209),
    # 10: bf16 dy, LayerNorm, N % 192 == 0, K >= 96: 192 x 96 tile, RC 32 (M = 8192: K = 104)
    (B, 1, 'ln', 8192, 192, 104, 210), (H, 1, 'ln', 8193, 192, 96, 210), (B, 1, 'ln', 8223, 192, 96, 210), (H, 1, 'ln', 8225, 192, 100, 210),
    (B, 1, 'ln', 20011, 192, 96, 210),
    # 11: bf16 dy, fp32 rows, 192 x 96 tile, RC 32
    (B, 1, 'rows', 8192, 192, 104, 211), (H, 1, 'rows', 8193, 192, 96, 211), (B, 1, 'concat', 8223, 192, 96, 211, 48),
    (H, 1, 'rows', 8225, 192, 96, 211), (B, 1, 'concat', 20011, 384, 192, 211, 96),
    # 12: fp32 dy, gelu16, K % 192 == 0, N >= 96: 96 x 192 tile, RC 64 (M = 8192: N = 104)
    (B, 0, 'gelu16', 8192, 104, 192, 212), (H, 0, 'gelu16', 8193, 96, 192, 212), (B, 0, 'gelu16', 8255, 96, 192, 212),
    (H, 0, 'gelu16', 8257, 100, 192, 212), (B, 0, 'gelu16', 20011, 96, 192, 212),
    # 13: fp32 dy, bf16 rows, 96 x 192 tile, RC 32
    (B, 0, 'bf16rows', 8192, 104, 192, 213), (B, 0, 'bf16rows', 8193, 96, 192, 213), (B, 0, 'bf16rows', 8223, 96, 192, 213),
    (B, 0, 'bf16rows', 8225, 100, 192, 213), (B, 0, 'bf16rows', 20011, 96, 192, 213),
    # 14 - 16: fp32 dy, fp16 rows (the attention output of mode 16f): the tilings of 8 / 9 / 13, RC 64 / 32 / 32.  fp16 rows are prepared
    # like fp32 rows, so N K < 200000 keeps 96 x 96 and 96 x 192 off the DMA kernel at M = 8192
    (H, 0, 'f16rows', 8192, 48, 48, 214), (H, 0, 'f16rows', 8193, 20, 40, 214), (H, 0, 'f16rows', 8255, 48, 48, 214),
    (H, 0, 'f16rows', 8257, 48, 48, 214), (H, 0, 'f16rows', 20011, 48, 48, 214),
    (H, 0, 'f16rows', 8192, 96, 96, 215), (H, 0, 'f16rows', 8193, 100, 72, 215), (H, 0, 'f16rows', 8223, 96, 96, 215),
    (H, 0, 'f16rows', 8225, 96, 96, 215), (H, 0, 'f16rows', 20011, 96, 96, 215),
    (H, 0, 'f16rows', 8192, 96, 192, 216), (H, 0, 'f16rows', 8193, 100, 192, 216), (H, 0, 'f16rows', 8223, 96, 192, 216),
    (H, 0, 'f16rows', 8225, 96, 192, 216), (H, 0, 'f16rows', 20011, 384, 192, 216))

# ---- LDS-DMA kernel: M in {8192, 8256, 13440}; per tile the smallest square and one rectangle; every preparation mode ------------------
_rows(  # tile 6 (multiples of 96)
    (B, 1, 'ln', 8192, 96, 96, 106), (H, 1, 'rows', 8256, 288, 96, 106), (B, 1, 'concat', 13440, 96, 96, 106, 32),
    (H, 0, 'gelu16', 8192, 96, 96, 106), (B, 0, 'bf16rows', 8256, 96, 96, 106), (B, 1, 'bf16rows', 13440, 288, 96, 106),   # bf16 rows in place
    # fp32 dy with rows that need preparing: DMA from N K >= 200000 on.  480 x 480 = 230400 is above the line, 384 x 480 = 184320 below
    (B, 0, 'rows', 8256, 480, 480, 106), (B, 0, 'rows', 8256, 384, 480, 204), (H, 0, 'f16rows', 8192, 480, 480, 106),
    (H, 0, 'ln', 13440, 480, 480, 106), (B, 0, 'concat', 8192, 480, 480, 106, 96),
    # tile 6 ends at 60000 rows: 60032 = 938 * 64 goes to the wide kernel
    (B, 1, 'ln', 60032, 96, 96, 205), (H, 0, 'gelu16', 60032, 96, 192, 212),
    # tile 8 (multiples of 128)
    (B, 1, 'ln', 8192, 128, 128, 108), (H, 1, 'rows', 8256, 256, 128, 108), (B, 0, 'gelu16', 13440, 128, 128, 108),
    (B, 0, 'bf16rows', 8192, 256, 128, 108), (H, 1, 'concat', 8256, 128, 128, 108, 64), (H, 0, 'f16rows', 8192, 512, 512, 108),
    # tile 4 (multiples of 64 that are neither); 448 x 448 = 200704 is the smallest such square above the line
    (B, 1, 'ln', 8192, 64, 64, 104), (H, 1, 'rows', 13440, 192, 64, 104), (B, 0, 'gelu16', 8256, 64, 64, 104),
    (B, 0, 'bf16rows', 13440, 192, 64, 104), (H, 1, 'concat', 8192, 192, 64, 104, 24), (H, 0, 'ln', 8256, 448, 448, 104))

# ---- wgradw: mode f32 (everything with M >= 8192; 32-row chunks are a 16-bit configuration, so 96 x 96 is cfg 5 there) -----------------
_rows((F, 0, 'rows', 8192, 48, 48, 301), (F, 0, 'ln', 8201, 48, 48, 301), (F, 0, 'ln', 8192, 144, 48, 302), (F, 0, 'rows', 8201, 144, 48, 302),
      (F, 0, 'rows', 8192, 48, 192, 303), (F, 0, 'concat', 8201, 48, 192, 303, 64), (F, 0, 'ln', 8192, 96, 96, 305), (F, 0, 'rows', 8201, 96, 96, 305),
      (F, 0, 'concat', 8192, 100, 68, 305, 20), (F, 0, 'ln', 8201, 100, 68, 305),
      # 16-bit modes: what the wide kernel has no combination for -- fp32 dy with LayerNorm (N K < 200000: not DMA either) ...
      (H, 0, 'ln', 8192, 48, 48, 301), (H, 0, 'ln', 8201, 144, 48, 302), (B, 0, 'ln', 8201, 48, 192, 303), (H, 0, 'ln', 8192, 96, 96, 305),
      (B, 0, 'ln', 20011, 100, 68, 305),
      # ... bf16 dy with [x | x2] at K <= 48, bf16 dy with fp32 rows at N <= 48 ...
      (B, 1, 'concat', 8192, 48, 48, 301, 16), (B, 1, 'concat', 8201, 144, 48, 302, 32), (B, 1, 'rows', 8192, 48, 192, 303),
      (H, 1, 'rows', 20011, 48, 192, 303),
      # ... and widths the wide kernel cannot load in 16-byte pieces (bf16 dy with N % 8 != 0, gelu16 with K % 8 != 0): 96 x 96 tile with
      # 32-row chunks up to 65536 rows and without LayerNorm (cfg 4), 16-row chunks beyond (cfg 5)
      (B, 1, 'rows', 8192, 100, 68, 304), (H, 0, 'gelu16', 8201, 100, 68, 304), (B, 1, 'concat', 20011, 100, 68, 304, 20),
      (H, 1, 'rows', 65536, 100, 68, 304), (B, 1, 'rows', 65600, 100, 68, 305), (B, 1, 'ln', 8201, 100, 68, 305))

# ---- wgrad16 ladder (M < 8192), all three modes: M in {1, 31, 33, 127, 129, 300, 8191}; bf16 dy in the 16-bit modes only -------------
_rows(  # <3,3>: N and K multiples of 48
    (F, 0, 'rows', 1, 48, 48, 433), (B, 1, 'ln', 31, 48, 48, 433), (H, 0, 'gelu16', 33, 48, 48, 433), (F, 0, 'ln', 127, 144, 96, 433),
    (B, 1, 'concat', 129, 144, 96, 433, 48), (H, 0, 'concat', 300, 144, 96, 433, 32), (F, 0, 'concat', 8191, 48, 48, 433, 16),
    (B, 0, 'rows', 8191, 144, 96, 433),
    # <2,2>: multiples of 32, not both of 64
    (B, 0, 'rows', 1, 32, 32, 422), (F, 0, 'ln', 31, 32, 32, 422), (H, 1, 'rows', 33, 96, 160, 422), (B, 0, 'ln', 127, 96, 160, 422),
    (F, 0, 'concat', 129, 32, 32, 422, 12), (H, 1, 'ln', 300, 32, 32, 422), (F, 0, 'rows', 8191, 96, 160, 422), (B, 1, 'concat', 8191, 32, 32, 422, 16),
    # <4,4>: N, K >= 64 otherwise
    (H, 0, 'rows', 1, 64, 64, 444), (B, 1, 'rows', 31, 100, 68, 444), (F, 0, 'rows', 33, 64, 64, 444), (H, 1, 'ln', 127, 64, 64, 444),
    (F, 0, 'ln', 129, 100, 68, 444), (B, 0, 'concat', 300, 100, 68, 444, 20), (F, 0, 'concat', 8191, 64, 64, 444, 32), (H, 1, 'concat', 8191, 100, 68, 444, 36),
    # <4,4>, the gelu16 branch: every width that is no multiple of 48, also where the rows modes take <2,2> or <1,4>
    (B, 0, 'gelu16', 127, 80, 112, 444), (F, 0, 'gelu16', 300, 64, 256, 444), (H, 0, 'gelu16', 129, 32, 32, 444), (F, 0, 'gelu16', 8191, 20, 68, 444),
    # <1,4>: N < 64 <= K
    (F, 0, 'rows', 1, 20, 68, 414), (H, 1, 'ln', 31, 20, 68, 414), (B, 0, 'concat', 33, 20, 68, 414, 24), (F, 0, 'ln', 127, 20, 68, 414),
    (B, 1, 'rows', 129, 20, 68, 414), (H, 0, 'ln', 300, 20, 68, 414), (F, 0, 'concat', 8191, 20, 68, 414, 8),
    # <4,1>: K < 64 <= N
    (B, 0, 'ln', 1, 68, 20, 441), (F, 0, 'rows', 31, 68, 20, 441), (H, 1, 'rows', 33, 68, 20, 441), (B, 1, 'concat', 127, 68, 20, 441, 8),
    (F, 0, 'ln', 129, 68, 20, 441), (H, 0, 'gelu16', 300, 96, 48, 433), (F, 0, 'concat', 300, 68, 20, 441, 12), (B, 1, 'ln', 8191, 68, 20, 441),
    # <1,1>: both below 64
    (H, 0, 'rows', 1, 4, 4, 411), (F, 0, 'ln', 31, 20, 36, 411), (B, 1, 'rows', 33, 4, 4, 411), (F, 0, 'concat', 127, 20, 36, 411, 16),
    (H, 1, 'ln', 129, 20, 36, 411), (B, 0, 'ln', 300, 4, 4, 411), (F, 0, 'rows', 8191, 4, 4, 411), (H, 1, 'concat', 8191, 20, 36, 411, 4))

# written out, not computed from the code under test: every instantiation the router can reach
REQUIRED = {F: {301, 302, 303, 305, 433, 422, 444, 414, 441, 411},
            B: {104, 106, 108} | set(range(201, 214)) | {301, 302, 303, 304, 305, 433, 422, 444, 414, 441, 411},
            H: {104, 106, 108} | {201, 202, 203, 204, 205, 206, 207, 210, 211, 212, 214, 215, 216} | {301, 302, 303, 304, 305, 433, 422, 444, 414, 441, 411}}
ALL_CODES = {104, 106, 108} | set(range(201, 217)) | set(range(301, 306)) | {433, 422, 444, 414, 441, 411}


def _id(r):
    return '-'.join(str(v) for v in (r[0], 'dy16' if r[1] else 'dy32', r[2], r[3], f'{r[4]}x{r[5]}', r[6]))


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as o
    prev = o.set_precision(F)
    try:
        yield o
    finally:
        o.set_precision(prev)


@functools.lru_cache(maxsize=6)
def _problem(dy16, xmode, M, N, K, K1):
    """CPU operands + float64 reference of one (formats, shape): computed once, shared by every test and mode that uses it, never modified"""
    dy = we.make_dy(M, N, bool(dy16), seed=M + N)
    o = we.make_x(xmode, M, K, seed=M + K, K1=K1)
    ref_w, ref_b = we.reference(dy, o['X'])
    return dy, o, ref_w, ref_b


def _dev(t, pad=0):
    buf, ld = we.padded(t, pad)
    return buf.to(DEV), ld


def run_exact(ops, dy16, xmode, M, N, K, code, K1=None, pad=0, with_bias=True, raw=False):
    """route assertion, then two accumulating calls on non-zero dW / dbias compared for equality"""
    from leod_amd import _lib
    dy, o, ref_w, ref_b = _problem(dy16, xmode, M, N, K, K1)
    K1 = o.get('K1', K)
    x_fmt, dy_fmt = we.X_FMT[xmode], 1 if dy16 else 0
    got = ops.linear_wgrad_route(M, N, K, dy_fmt, x_fmt, K1=K1, lddy=N + pad, ldx=K1 + pad, ldx2=(K - K1 + pad) if K1 < K else None)
    assert got == code, f'route {got}, this row is here for {code}: re-derive its shape from the predicates'
    dyd, lddy = _dev(dy, pad)
    xd, ldx = _dev(o['x'], pad)
    x2d, ldx2 = _dev(o['x2'], pad) if 'x2' in o else (None, 0)
    st, lw, lb = (o[k].to(DEV) for k in ('stats', 'ln_w', 'ln_b')) if xmode == 'ln' else (None, None, None)
    W0, b0 = we.start_values(N, K)
    dW, db = W0.to(DEV), (b0.to(DEV) if with_bias else None)
    if raw or pad:
        if M >= 8192 and ops.is_16bit() and ops._stream() not in ops._WORKSPACES:
            ops._wgrad_workspace(dW.device)          # a 100 + T route is final only with a registered workspace

        def call():
            _lib.check(_lib.lib().leod_linear_wgrad(ops._p(dyd), lddy, ops._p(xd), ldx, ops._p(st), ops._p(lw), ops._p(lb), ops._p(x2d), ldx2, K1,
                                                    ops._p(dW), ops._p(db), M, N, K, dy_fmt, x_fmt, ops._stream()), 'leod_linear_wgrad')
    else:
        def call():
            ops.linear_wgrad(dyd, xd, dW, db, stats=st, ln_w=lw, ln_b=lb, x2=x2d, x_gelu=None if xmode == 'gelu16' else False)
    for n in (1, 2):
        call()
        assert torch.equal(dW.cpu(), W0 + n * ref_w), f'dW after call {n}: {int((dW.cpu() != W0 + n * ref_w).sum())} of {N * K} elements differ'
        if with_bias:
            assert torch.equal(db.cpu(), b0 + n * ref_b), f'dbias after call {n}'
    if pad:                                          # the padding itself was only read
        assert bool((dyd[:, N:] == we.PAD_VALUE).all()) and bool((xd[:, K1:] == we.PAD_VALUE).all())


@pytest.mark.parametrize('row', ROUTES, ids=_id)
def test_route_exact(ops, row):
    mode, dy16, xmode, M, N, K, code = row[:7]
    assert M <= we.M_MAX
    ops.set_precision(mode)
    run_exact(ops, dy16, xmode, M, N, K, code, K1=row[7] if len(row) > 7 else None)


def test_route_table_is_complete(ops):
    """every instantiation of the four kernel families has a row, in every precision mode that reaches it, and meets every class of M"""
    for mode, need in REQUIRED.items():
        have = {r[6] for r in ROUTES if r[0] == mode}
        assert need <= have, f'mode {mode}: no row for {sorted(need - have)}'
    assert {r[6] for r in ROUTES} == ALL_CODES
    by_code = {}
    for r in ROUTES:
        by_code.setdefault(r[6], set()).add(r[3])
    rc = {c: 64 if c in (201, 206, 208, 212, 214) else 32 for c in range(201, 217)}
    for c in range(201, 217):
        assert {8192, 8193, 8192 + rc[c] - 1, 8192 + rc[c] + 1} <= by_code[c] and any(m > 16384 and m % 64 for m in by_code[c]), c
    for c in (104, 106, 108):
        assert {8192, 8256, 13440} <= by_code[c], c
    for c in (433, 422, 444, 414, 441, 411):
        assert {1, 31, 33, 127, 129, 300, 8191} <= by_code[c], c
    for c in range(301, 306):
        assert len(by_code[c]) >= 2, c
    # every (dy format, x mode) pair meets every family that takes it
    fam = {(r[6] // 100, r[1], r[2]) for r in ROUTES}
    x16 = ('bf16rows', 'f16rows')
    for f_, dys, xms in ((1, (0, 1), ('rows', 'ln', 'concat', 'bf16rows')), (1, (0,), ('gelu16', 'f16rows')),
                         (2, (0,), ('rows', 'concat', 'gelu16') + x16), (2, (1,), ('rows', 'concat', 'ln')),
                         (3, (0, 1), ('rows', 'ln', 'concat')), (3, (0,), ('gelu16',)),
                         (4, (0, 1), ('rows', 'ln', 'concat')), (4, (0,), ('gelu16',))):
        for d_ in dys:
            for xm in xms:
                assert (f_, d_, xm) in fam, (f_, d_, xm)
    assert 150 <= len(ROUTES) <= 250


@pytest.mark.parametrize('mode', [F, B, H])
def test_no_rows_is_ok_and_touches_nothing(ops, mode):
    ops.set_precision(mode)
    from leod_amd import _lib
    assert ops.linear_wgrad_route(0, 48, 48) == 0
    W0, b0 = we.start_values(48, 48)
    dW, db, z = W0.to(DEV), b0.to(DEV), torch.zeros(4, 48, device=DEV)
    rc = _lib.lib().leod_linear_wgrad(ops._p(z), 48, ops._p(z), 48, None, None, None, None, 0, 48, ops._p(dW), ops._p(db), 0, 48, 48, 0, 0, ops._stream())
    assert rc == 0 and torch.equal(dW.cpu(), W0) and torch.equal(db.cpu(), b0)


# ---- non-dense strides through the raw entry point: lddy = N + 8, ldx = K1 + 8, ldx2 = K2 + 8, padding = 64 ------------------------------
# (multiples of 8 keep every alignment predicate: the routes are those of the dense shapes; K1 != K - K1 in the concat rows)
STRIDED = [(B, 1, 'ln', 8192, 96, 96, 106), (H, 0, 'gelu16', 8256, 128, 128, 108), (B, 1, 'concat', 8192, 192, 64, 104, 24),
           (B, 0, 'bf16rows', 8193, 96, 96, 209), (H, 0, 'f16rows', 8225, 96, 192, 216), (B, 1, 'concat', 8223, 192, 96, 211, 32),
           (B, 0, 'gelu16', 8257, 96, 192, 212), (H, 0, 'ln', 8201, 100, 68, 305), (F, 0, 'concat', 8192, 48, 192, 303, 64),
           (B, 1, 'rows', 8201, 100, 68, 304), (F, 0, 'ln', 129, 20, 68, 414), (B, 1, 'concat', 300, 144, 96, 433, 32), (H, 0, 'gelu16', 33, 80, 112, 444)]


@pytest.mark.parametrize('row', STRIDED, ids=_id)
def test_route_exact_strided(ops, row):
    mode, dy16, xmode, M, N, K, code = row[:7]
    ops.set_precision(mode)
    run_exact(ops, dy16, xmode, M, N, K, code, K1=row[7] if len(row) > 7 else None, pad=8)


@pytest.mark.parametrize('row', [(B, 1, 'ln', 8192, 96, 96, 106), (H, 0, 'f16rows', 8193, 96, 96, 215), (F, 0, 'rows', 8201, 100, 68, 305),
                                 (B, 0, 'bf16rows', 8192, 48, 48, 208), (H, 1, 'concat', 129, 144, 96, 433, 48), (F, 0, 'ln', 31, 20, 36, 411)], ids=_id)
def test_route_exact_without_dbias(ops, row):
    mode, dy16, xmode, M, N, K, code = row[:7]
    ops.set_precision(mode)
    run_exact(ops, dy16, xmode, M, N, K, code, K1=row[7] if len(row) > 7 else None, with_bias=False)


# ---- the grouped launch against the same independent reference ----------------------------------------------------------------------------
def _group_problems(ops, M, C, widths, n, no_bias=None):
    """the attention-block quadruple on exact operands: fc2 (gelu16, fp32 dy), fc1 (ln, bf16 dy), proj (16-bit rows, fp32 dy), qkv (ln, bf16 dy)"""
    rows16 = 'f16rows' if ops.get_precision() == H else 'bf16rows'
    spec = [(0, 'gelu16', C, widths[0]), (1, 'ln', widths[1], C), (0, rows16, C, C), (1, 'ln', widths[2], C)][:n]
    probs, checks = [], []
    for i, (dy16, xmode, N, K) in enumerate(spec):
        dy, o, ref_w, ref_b = _problem(dy16, xmode, M, N, K, None)
        W0, b0 = we.start_values(N, K)
        p = dict(dy=dy.to(DEV), x=o['x'].to(DEV), dW=W0.to(DEV), dbias=None if i == no_bias else b0.to(DEV), gelu=xmode == 'gelu16')
        if xmode == 'ln':
            p.update(stats=o['stats'].to(DEV), ln_w=o['ln_w'].to(DEV), ln_b=o['ln_b'].to(DEV))
        probs.append(p)
        checks.append((W0, b0, ref_w, ref_b))
    return probs, checks


def _group_state(probs):
    return [t.clone() for p in probs for t in (p['dW'], p['dbias']) if t is not None]


# one geometry per tile: C = 96 (tile 6), C = 128 (tile 8), C = 64 with widths that are multiples of 64 only (tile 4)
@pytest.mark.parametrize('n', [1, 2, 3, 4])
@pytest.mark.parametrize('mode,M,C,widths', [(B, 8192, 96, (384, 384, 288)), (H, 8256, 96, (384, 384, 288)), (B, 8256, 128, (512, 512, 384)),
                                             (H, 8192, 128, (512, 512, 384)), (B, 8192, 64, (192, 192, 320)), (H, 8256, 64, (192, 192, 320))])
def test_group_exact(ops, mode, M, C, widths, n):
    ops.set_precision(mode)
    no_bias = n - 1 if n > 1 else None
    probs, checks = _group_problems(ops, M, C, widths, n, no_bias=no_bias)
    for k in (1, 2):
        assert ops.linear_wgrad_group(probs)
        for i, (p, (W0, b0, ref_w, ref_b)) in enumerate(zip(probs, checks)):
            assert torch.equal(p['dW'].cpu(), W0 + k * ref_w), f'problem {i}, call {k}: dW'
            if p['dbias'] is not None:
                assert torch.equal(p['dbias'].cpu(), b0 + k * ref_b), f'problem {i}, call {k}: dbias'


@pytest.mark.parametrize('what', ['ragged M', 'mixed tiles', 'mode f32', 'width % 8'])
def test_group_refusals_touch_nothing(ops, what):
    ops.set_precision(F if what == 'mode f32' else B)
    if what == 'mode f32':
        probs, _ = _group_problems_f32(ops, 8192, 96)
    elif what == 'ragged M':
        probs, _ = _group_problems(ops, 8200, 96, (384, 384, 288), 2)
    elif what == 'mixed tiles':
        a, _ = _group_problems(ops, 8192, 96, (384, 384, 288), 1)
        b, _ = _group_problems(ops, 8192, 128, (512, 512, 384), 1)
        probs = a + b
    else:                                            # 100 = 96 + 4: a multiple of 4, not of 8, and of no tile
        dy, o, _, _ = _problem(1, 'ln', 8192, 100, 96, None)
        W0, b0 = we.start_values(100, 96)
        probs = [dict(dy=dy.to(DEV), x=o['x'].to(DEV), dW=W0.to(DEV), dbias=b0.to(DEV), stats=o['stats'].to(DEV), ln_w=o['ln_w'].to(DEV),
                      ln_b=o['ln_b'].to(DEV))]
    before = _group_state(probs)
    assert ops.linear_wgrad_group(probs) is False
    torch.cuda.synchronize()
    for a_, b_ in zip(_group_state(probs), before):
        assert torch.equal(a_, b_)


def _group_problems_f32(ops, M, C):
    dy, o, _, _ = _problem(0, 'ln', M, C, C, None)
    W0, b0 = we.start_values(C, C)
    return [dict(dy=dy.to(DEV), x=o['x'].to(DEV), dW=W0.to(DEV), dbias=b0.to(DEV), stats=o['stats'].to(DEV), ln_w=o['ln_w'].to(DEV),
                 ln_b=o['ln_b'].to(DEV))], None


# ---- the rejection contract: return code, untouched outputs, the same answer from the route query ---------------------------------------
def test_rejections(ops):
    from leod_amd import _lib
    from leod_amd._lib import LeodHipError
    lib = _lib.lib()
    M, N, K = 8191, 48, 48
    f32 = torch.ones(M, 64, device=DEV)
    b16, h16 = f32.to(torch.bfloat16), f32.to(torch.float16)
    st, vec = torch.ones(M, 2, device=DEV), torch.ones(64, device=DEV)
    W0, b0 = we.start_values(64, 64)
    dW, db = W0.to(DEV), b0.to(DEV)

    def raw(dy=f32, x=f32, stats=None, ln_w=None, ln_b=None, x2=None, M=M, N=N, K=K, K1=None, lddy=64, dy_fmt=0, x_fmt=0):
        K1 = K if K1 is None else K1
        rc = lib.leod_linear_wgrad(ops._p(dy), lddy, ops._p(x), 64, ops._p(stats), ops._p(ln_w), ops._p(ln_b), ops._p(x2), 64, K1, ops._p(dW), ops._p(db),
                                   M, N, K, dy_fmt, x_fmt, ops._stream())
        torch.cuda.synchronize()
        assert torch.equal(dW.cpu(), W0) and torch.equal(db.cpu(), b0), 'a refused call wrote to dW / dbias'
        return rc

    def query(M=M, N=N, K=K, K1=None, lddy=64, dy_fmt=0, x_fmt=0, stats=False):
        return ops.linear_wgrad_route(M, N, K, dy_fmt, x_fmt, K1=K1, lddy=lddy, ldx=64, ldx2=64, has_stats=stats)

    for mode in (F, B, H):
        ops.set_precision(mode)
        assert raw(x_fmt=1) == ERR_ARG == query(x_fmt=1, stats=False)                                   # LayerNorm without stats
        for xf, x in ((0, f32), (2, h16), (3, b16), (4, h16)):                                           # stats without LayerNorm
            assert raw(x=x, stats=st, ln_w=vec, ln_b=vec, x_fmt=xf) == ERR_ARG == query(x_fmt=xf, stats=True)
        assert raw(stats=st, ln_b=vec, x_fmt=1) == ERR_ARG and raw(stats=st, ln_w=vec, x_fmt=1) == ERR_ARG   # (the query takes ln_w / ln_b as given with stats)
        assert raw(x=h16, x2=f32, K1=16, x_fmt=2) == ERR_ARG == query(K1=16, x_fmt=2)                    # gelu16 with x2
        assert raw(dy=b16, x=h16, dy_fmt=1, x_fmt=2) == ERR_ARG == query(dy_fmt=1, x_fmt=2)              # gelu16 with bf16 dy
        for xf in (-1, 5):
            assert raw(x_fmt=xf) == ERR_ARG == query(x_fmt=xf)
        for df in (-1, 2):
            assert raw(dy_fmt=df) == ERR_ARG == query(dy_fmt=df)
        for xf, x in ((3, b16), (4, h16)):
            assert raw(x=x, x2=f32, K1=16, x_fmt=xf) == ERR_ARG == query(K1=16, x_fmt=xf)               # 16-bit rows with x2
            assert raw(x=x, x_fmt=xf) == ERR_UNSUPPORTED == query(x_fmt=xf)                              # 16-bit rows at M = 8191
        assert raw(N=50) == ERR_ARG == query(N=50)                                                       # 16-byte row loads on the ladder
        assert raw(lddy=50) == ERR_ARG == query(lddy=50)
        assert raw(K=50) == ERR_ARG == query(K=50)
    ops.set_precision(F)
    assert raw(dy=b16, dy_fmt=1) == ERR_ARG == query(dy_fmt=1)                                           # 16-bit tensors in mode f32
    assert raw(dy=b16, dy_fmt=1, M=8192) == ERR_ARG == query(dy_fmt=1, M=8192)
    # ops.linear_wgrad raises for what it can express
    for mode in (F, B):
        ops.set_precision(mode)
        with pytest.raises(LeodHipError):
            ops.linear_wgrad(f32[:, :N].contiguous(), h16[:, :K].contiguous(), dW[:N, :K].contiguous(), x2=f32[:, :16].contiguous())   # gelu16 with x2
        with pytest.raises(LeodHipError):
            ops.linear_wgrad(b16[:, :N].contiguous(), h16[:, :K].contiguous(), dW[:N, :K].contiguous())                                # gelu16 with bf16 dy
        with pytest.raises(LeodHipError):
            ops.linear_wgrad(f32[:, :N].contiguous(), b16[:, :K].contiguous(), dW[:N, :K].contiguous(), x_gelu=False)                  # 16-bit rows at M = 8191
        with pytest.raises(LeodHipError):
            ops.linear_wgrad(f32[:, :N].contiguous(), f32[:, :K].contiguous(), dW[:N, :K].contiguous(), stats=st, ln_b=vec[:K].contiguous())  # LayerNorm without ln_w
        with pytest.raises(LeodHipError):
            ops.linear_wgrad(f32[:, :50].contiguous(), f32[:, :K].contiguous(), torch.zeros(50, K, device=DEV))                        # N = 50
    ops.set_precision(F)
    with pytest.raises(LeodHipError):
        ops.linear_wgrad(b16[:, :N].contiguous(), f32[:, :K].contiguous(), dW[:N, :K].contiguous())                                    # bf16 dy in mode f32
    assert torch.equal(dW.cpu(), W0) and torch.equal(db.cpu(), b0)
