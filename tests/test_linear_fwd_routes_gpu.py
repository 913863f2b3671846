"""Every route of the nine Linear forward / input-gradient entry points (csrc/linear_common.hpp: linear_route / launch_linear) on operands for
which the result is EXACT (tests/linear_exact.py): ``torch.equal`` against a float64 CPU reference.

Each row names the kernel it is there for as a route code (leod_linear_route: 1000 + 100 KC + NTT row-streaming, 2000 + KC narrow
row-streaming, 3000 + NTW wide tile, 4000 / 5000 + 100 NT + KCH LDS-staged with the two-phase / plain loader, 6000 + 10 NT + KS
register-direct).  The test first asserts that the router still sends the row there; tests/test_linear_exact_cpu.py asserts the same without
a GPU, and that every (entry, mode, code) of the route table of tests/test_linear_routes_cpu.py has a row here.

Rows: (entry, mode, M, N, K, a16, out16, flags, nsplit, pad, code).  M, N, K as the entry takes them (W is [N, K]; the dgrads 6 - 8 contract
over N); a16 / out16 / flags / nsplit as leod_linear_route, plus the test-only flag 1024 (linear_exact.MASKED: the GELU operand takes both
signs); pad: extra columns of every strided buffer, through the raw C ABI.

Comparisons.  Equality: every output of every row except the following.  fp32 bound of test_kernels_gpu.close (rtol 2e-5, floor 2e-6 +
5e-6 max|ref|): out / out_act of LayerNorm rows in mode f32 (nothing absorbs the rounding of mean, rstd and eps there; out_act == out is
still asserted bit for bit).  stats_out as test_ln_linear_fwd: atol 1e-6 on the mean, rtol 1e-5 on rstd.  Entry 7: the fp32 bounds of
test_linear_dgrad_ln_bwd (1e-4 / 1e-5 on dx, 3e-4 / 1e-4 on dgamma, dbeta) in every mode.  Masked GELU rows: equal where u > 0, at most 1e-9
where u < 0 (entries 6, 8), |got - ref| <= 1e-9 (entry 5).  The masked rows of entry 5 run in mode 16f only: there gelu(u <= -8), about -4e-15,
is an MFMA OPERAND, and only fp16 rounds it to an exact zero (test_linear_exact_cpu checks both).  As a bf16 operand it survives, and what
a sum of integers plus 1e-14 comes to is up to the rounding inside the bf16 MFMA: measured once on an MI355X, mode bf16, 99335 x 384 -> 96
(route 2024), the outputs were off by up to 3.8e-6 = one fp32 ulp of a value near 40, against the 1e-9 of this test.  In entries 6 and 8
gelu' multiplies the finished sum in the epilogue, so their masked rows run in every mode.

Where the row counts come from (linear_common.hpp, gemm16.hpp, gemm_bf16.hpp):
  register-direct  below the LDS threshold; M in {1, 15, 17, 63, 65, 300}; KS = 4 from a contraction of 128 on (always < 512 workgroups here)
  LDS-staged       cdiv(M, 64) * cdiv(nout, 16 NT) >= 256 and M >= 2048: the smallest such M of the row's width (8129 for 96 / 128 columns,
                   3265 for 80 / 160), + 1, + 63, a ragged one beside it and 10007; contractions 96 (K % 48 == 0) and 80 / 64; NT 1 - 4 =
                   80 / 160 / 96 / 128 columns
  wide tile        M >= 4096, N >= 144, K >= 32, on the LDS side of the threshold: 384 / 256 columns at M in {4096, 4097, 4223, 4225}, 192 /
                   256 at 32897 (257 tiles of 128 rows on 256 persistent workgroups); 192 x 192 on both sides of M <= 60000
  row-streaming    M >= 16384; rows per pass P = grid.x * 4 waves * 16 (rowstream48_grid: 49152 for 1309, 32768 for 1312 / 1412, 16384
                   for 1609 / 1408, 10752 for 1608; rowstream_narrow_grid: 32768): 16384 and 16391, then k P + 1024 (+ 7) for k = 1, 2, 3, so
                   that waves run 1 - 2, 2 - 3 and 3 - 4 tiles with full and ragged last tiles; entry 7 under linear_exact.reduction_bound
``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import linear_exact as le  # noqa: E402
from linear_exact import LN, STATS, KSCALE, AUX, TOUT, DX2, COLSUM, ACCUMULATE, DRES, MASKED  # noqa: E402

DEV = 'cuda'
B, H, F = 'bf16', '16f', 'f32'
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# ---- register-direct kernel: per code every class of M; the last five rows: LayerNorm without a statistics buffer (whatever M) -----------
G16 = [
    (0, F, 1, 80, 96, 0, 0, 3, 0, 0, 6011), (0, B, 15, 80, 96, 0, 0, 11, 0, 0, 6011), (0, H, 17, 80, 96, 0, 0, 0, 0, 0, 6011),
    (1, F, 63, 80, 96, 0, 0, 0, 0, 0, 6011), (1, B, 65, 80, 96, 0, 0, 16, 0, 0, 6011), (1, H, 300, 80, 96, 0, 0, 0, 0, 0, 6011),
    (5, B, 1, 80, 96, 0, 0, 0, 0, 0, 6011), (5, H, 15, 80, 96, 0, 0, 1024, 0, 0, 6011), (0, F, 1, 80, 320, 0, 0, 8, 0, 0, 6014),
    (0, B, 15, 80, 320, 0, 0, 3, 0, 0, 6014), (0, H, 17, 80, 320, 0, 0, 11, 0, 0, 6014), (1, F, 63, 80, 320, 0, 0, 16, 0, 0, 6014),
    (1, B, 65, 80, 320, 0, 0, 0, 0, 0, 6014), (1, H, 300, 80, 320, 0, 0, 16, 0, 0, 6014), (5, B, 1, 80, 320, 0, 0, 0, 0, 0, 6014),
    (5, H, 15, 80, 320, 0, 0, 1024, 0, 0, 6014), (0, F, 1, 160, 96, 0, 0, 0, 0, 0, 6021), (0, B, 15, 160, 96, 0, 0, 8, 0, 0, 6021),
    (0, H, 17, 160, 96, 0, 0, 3, 0, 0, 6021), (1, F, 63, 160, 96, 0, 0, 0, 0, 0, 6021), (1, B, 65, 160, 96, 0, 0, 16, 0, 0, 6021),
    (1, H, 300, 160, 96, 0, 0, 0, 0, 0, 6021), (5, B, 1, 160, 96, 0, 0, 0, 0, 0, 6021), (5, H, 15, 160, 96, 0, 0, 1024, 0, 0, 6021),
    (0, F, 1, 160, 320, 0, 0, 11, 0, 0, 6024), (0, B, 15, 160, 320, 0, 0, 0, 0, 0, 6024), (0, H, 17, 160, 320, 0, 0, 8, 0, 0, 6024),
    (1, F, 63, 160, 320, 0, 0, 16, 0, 0, 6024), (1, B, 65, 160, 320, 0, 0, 0, 0, 0, 6024), (1, H, 300, 160, 320, 0, 0, 16, 0, 0, 6024),
    (5, B, 1, 160, 320, 0, 0, 0, 0, 0, 6024), (5, H, 15, 160, 320, 0, 0, 1024, 0, 0, 6024), (0, F, 1, 96, 96, 0, 0, 3, 0, 0, 6031),
    (0, B, 15, 96, 96, 0, 0, 11, 0, 0, 6031), (0, H, 17, 96, 96, 0, 0, 0, 0, 0, 6031), (1, F, 63, 96, 96, 0, 0, 0, 0, 0, 6031),
    (1, B, 65, 96, 96, 0, 0, 16, 0, 0, 6031), (1, H, 300, 96, 96, 0, 0, 0, 0, 0, 6031), (5, B, 1, 96, 96, 0, 0, 0, 0, 0, 6031),
    (5, H, 15, 96, 96, 0, 0, 1024, 0, 0, 6031), (6, F, 17, 96, 96, 0, 0, 0, 0, 0, 6031), (6, B, 63, 96, 96, 0, 0, 4, 0, 0, 6031),
    (6, H, 65, 96, 96, 0, 0, 8, 0, 0, 6031), (0, F, 1, 48, 192, 0, 0, 8, 0, 0, 6034), (0, B, 15, 48, 192, 0, 0, 3, 0, 0, 6034),
    (0, H, 17, 48, 192, 0, 0, 11, 0, 0, 6034), (1, F, 63, 48, 192, 0, 0, 16, 0, 0, 6034), (1, B, 65, 48, 192, 0, 0, 0, 0, 0, 6034),
    (1, H, 300, 48, 192, 0, 0, 16, 0, 0, 6034), (5, B, 1, 48, 192, 0, 0, 0, 0, 0, 6034), (5, H, 15, 48, 192, 0, 0, 1024, 0, 0, 6034),
    (6, F, 17, 192, 48, 1, 0, 0, 0, 0, 6034), (6, B, 63, 192, 48, 0, 0, 12, 0, 0, 6034), (6, H, 65, 192, 48, 0, 0, 1032, 0, 0, 6034),
    (0, F, 1, 64, 48, 0, 0, 0, 0, 0, 6041), (0, B, 15, 64, 48, 0, 0, 8, 0, 0, 6041), (0, H, 17, 64, 48, 0, 0, 3, 0, 0, 6041),
    (6, F, 63, 48, 64, 1, 0, 4, 0, 0, 6041), (6, B, 65, 48, 64, 0, 0, 1036, 0, 0, 6041), (6, H, 300, 48, 64, 0, 0, 0, 0, 0, 6041),
    (0, F, 1, 64, 128, 0, 0, 11, 0, 0, 6044), (0, B, 15, 64, 128, 0, 0, 0, 0, 0, 6044), (0, H, 17, 64, 128, 0, 0, 8, 0, 0, 6044),
    (1, F, 63, 64, 128, 0, 0, 0, 0, 0, 6044), (1, B, 65, 64, 128, 0, 0, 16, 0, 0, 6044), (1, H, 300, 64, 128, 0, 0, 0, 0, 0, 6044),
    (5, B, 1, 64, 128, 0, 0, 0, 0, 0, 6044), (5, H, 15, 64, 128, 0, 0, 1024, 0, 0, 6044), (6, F, 17, 128, 64, 0, 0, 4, 0, 0, 6044),
    (6, B, 63, 128, 64, 0, 0, 8, 0, 0, 6044), (6, H, 65, 128, 64, 1, 0, 0, 0, 0, 6044),
    (0, F, 300, 192, 48, 0, 0, 9, 0, 0, 6041), (0, B, 2049, 192, 48, 0, 0, 1, 0, 0, 6041), (0, F, 16384, 192, 48, 0, 0, 1, 0, 0, 6041),
    (0, B, 16391, 192, 48, 0, 0, 9, 0, 0, 6041), (0, H, 20000, 192, 48, 0, 0, 1, 0, 0, 6041),
]
# ---- LDS-staged kernel ------------------------------------------------------------------------------------------------------------------
LDS = [
    (0, F, 8129, 96, 96, 0, 0, 3, 0, 0, 4348), (0, B, 8130, 96, 96, 0, 0, 11, 0, 0, 4348), (0, H, 8192, 96, 96, 0, 0, 0, 0, 0, 4348),
    (1, H, 8129, 96, 96, 0, 0, 0, 0, 0, 4348), (1, B, 8326, 96, 96, 0, 0, 16, 0, 0, 4348), (1, F, 10007, 96, 96, 0, 0, 0, 0, 0, 4348),
    (2, B, 8130, 96, 96, 0, 0, 3, 0, 0, 4348), (2, H, 8192, 96, 96, 0, 0, 3, 0, 0, 4348), (3, H, 8326, 96, 96, 0, 0, 0, 0, 0, 4348),
    (3, B, 10007, 96, 96, 0, 0, 3, 0, 0, 4348), (4, B, 8129, 96, 96, 0, 0, 0, 0, 0, 4348), (4, H, 8130, 96, 96, 0, 0, 0, 0, 0, 4348),
    (5, B, 8192, 96, 96, 0, 0, 0, 0, 0, 4348), (5, H, 10007, 96, 96, 0, 0, 1024, 0, 0, 4348), (6, B, 8129, 96, 96, 0, 0, 4, 0, 0, 4348),
    (6, H, 8130, 96, 96, 0, 0, 8, 0, 0, 4348), (6, F, 8326, 96, 96, 0, 0, 0, 0, 0, 4348), (8, B, 8192, 96, 96, 0, 1, 8, 0, 0, 4348),
    (8, H, 10007, 96, 96, 0, 0, 12, 0, 0, 4348), (0, F, 8129, 96, 80, 0, 0, 8, 0, 0, 4364), (0, B, 8130, 96, 80, 0, 0, 3, 0, 0, 4364),
    (0, H, 8192, 96, 80, 0, 0, 11, 0, 0, 4364), (1, H, 8129, 96, 80, 0, 0, 16, 0, 0, 4364), (1, B, 8326, 96, 80, 0, 0, 0, 0, 0, 4364),
    (1, F, 10007, 96, 80, 0, 0, 16, 0, 0, 4364), (2, B, 8130, 96, 80, 0, 0, 3, 0, 0, 4364), (2, H, 8192, 96, 80, 0, 0, 3, 0, 0, 4364),
    (3, H, 8326, 96, 80, 0, 0, 0, 0, 0, 4364), (3, B, 10007, 96, 80, 0, 0, 3, 0, 0, 4364), (4, B, 8129, 96, 80, 0, 0, 0, 0, 0, 4364),
    (4, H, 8130, 96, 80, 0, 0, 0, 0, 0, 4364), (5, B, 8192, 96, 80, 0, 0, 0, 0, 0, 4364), (5, H, 10007, 96, 80, 0, 0, 1024, 0, 0, 4364),
    (6, B, 8129, 80, 96, 0, 0, 12, 0, 0, 4364), (6, H, 8130, 80, 96, 0, 0, 1032, 0, 0, 4364), (6, F, 8326, 80, 96, 1, 0, 0, 0, 0, 4364),
    (8, B, 8192, 80, 96, 0, 1, 1032, 0, 0, 4364), (8, H, 10007, 80, 96, 0, 0, 8, 0, 0, 4364), (0, F, 8129, 128, 96, 0, 0, 0, 0, 0, 4448),
    (0, B, 8130, 128, 96, 0, 0, 8, 0, 0, 4448), (0, H, 8192, 128, 96, 0, 0, 3, 0, 0, 4448), (1, H, 8129, 128, 96, 0, 0, 0, 0, 0, 4448),
    (1, B, 8326, 128, 96, 0, 0, 16, 0, 0, 4448), (1, F, 10007, 128, 96, 0, 0, 0, 0, 0, 4448), (2, B, 8130, 128, 96, 0, 0, 3, 0, 0, 4448),
    (2, H, 8192, 128, 96, 0, 0, 3, 0, 0, 4448), (3, H, 8326, 128, 96, 0, 0, 0, 0, 0, 4448), (3, B, 10007, 128, 96, 0, 0, 3, 0, 0, 4448),
    (4, B, 8129, 128, 96, 0, 0, 0, 0, 0, 4448), (4, H, 8130, 128, 96, 0, 0, 0, 0, 0, 4448), (5, B, 8192, 128, 96, 0, 0, 0, 0, 0, 4448),
    (5, H, 10007, 128, 96, 0, 0, 1024, 0, 0, 4448), (6, B, 8129, 96, 128, 0, 0, 1036, 0, 0, 4448), (6, H, 8130, 96, 128, 0, 0, 0, 0, 0, 4448),
    (6, F, 8326, 96, 128, 1, 0, 4, 0, 0, 4448), (8, B, 8192, 96, 128, 0, 0, 1036, 0, 0, 4448), (8, H, 10007, 96, 128, 0, 1, 8, 0, 0, 4448),
    (0, F, 8129, 128, 64, 0, 0, 11, 0, 0, 4464), (0, B, 8130, 128, 64, 0, 0, 0, 0, 0, 4464), (0, H, 8192, 128, 64, 0, 0, 8, 0, 0, 4464),
    (1, H, 8129, 128, 64, 0, 0, 16, 0, 0, 4464), (1, B, 8326, 128, 64, 0, 0, 0, 0, 0, 4464), (1, F, 10007, 128, 64, 0, 0, 16, 0, 0, 4464),
    (2, B, 8130, 128, 64, 0, 0, 3, 0, 0, 4464), (2, H, 8192, 128, 64, 0, 0, 3, 0, 0, 4464), (3, H, 8326, 128, 64, 0, 0, 0, 0, 0, 4464),
    (3, B, 10007, 128, 64, 0, 0, 3, 0, 0, 4464), (4, B, 8129, 128, 64, 0, 0, 0, 0, 0, 4464), (4, H, 8130, 128, 64, 0, 0, 0, 0, 0, 4464),
    (5, B, 8192, 128, 64, 0, 0, 0, 0, 0, 4464), (5, H, 10007, 128, 64, 0, 0, 1024, 0, 0, 4464), (6, B, 8129, 64, 128, 0, 0, 8, 0, 0, 4464),
    (6, H, 8130, 64, 128, 1, 0, 0, 0, 0, 4464), (6, F, 8326, 64, 128, 0, 0, 4, 0, 0, 4464), (8, B, 8192, 64, 128, 0, 0, 12, 0, 0, 4464),
    (8, H, 10007, 64, 128, 0, 1, 1032, 0, 0, 4464), (0, F, 3265, 80, 96, 0, 0, 3, 0, 0, 5148), (0, B, 3266, 80, 96, 0, 0, 11, 0, 0, 5148),
    (0, H, 3328, 80, 96, 0, 0, 0, 0, 0, 5148), (1, H, 3265, 80, 96, 0, 0, 0, 0, 0, 5148), (1, B, 3462, 80, 96, 0, 0, 16, 0, 0, 5148),
    (1, F, 10007, 80, 96, 0, 0, 0, 0, 0, 5148), (2, B, 3266, 80, 96, 0, 0, 3, 0, 0, 5148), (2, H, 3328, 80, 96, 0, 0, 3, 0, 0, 5148),
    (3, H, 3462, 80, 96, 0, 0, 0, 0, 0, 5148), (3, B, 10007, 80, 96, 0, 0, 3, 0, 0, 5148), (4, B, 3265, 80, 96, 0, 0, 0, 0, 0, 5148),
    (4, H, 3266, 80, 96, 0, 0, 0, 0, 0, 5148), (5, B, 3328, 80, 96, 0, 0, 0, 0, 0, 5148), (5, H, 10007, 80, 96, 0, 0, 1024, 0, 0, 5148),
    (0, F, 3265, 80, 64, 0, 0, 8, 0, 0, 5164), (0, B, 3266, 80, 64, 0, 0, 3, 0, 0, 5164), (0, H, 3328, 80, 64, 0, 0, 11, 0, 0, 5164),
    (1, H, 3265, 80, 64, 0, 0, 16, 0, 0, 5164), (1, B, 3462, 80, 64, 0, 0, 0, 0, 0, 5164), (1, F, 10007, 80, 64, 0, 0, 16, 0, 0, 5164),
    (2, B, 3266, 80, 64, 0, 0, 3, 0, 0, 5164), (2, H, 3328, 80, 64, 0, 0, 3, 0, 0, 5164), (3, H, 3462, 80, 64, 0, 0, 0, 0, 0, 5164),
    (3, B, 10007, 80, 64, 0, 0, 3, 0, 0, 5164), (4, B, 3265, 80, 64, 0, 0, 0, 0, 0, 5164), (4, H, 3266, 80, 64, 0, 0, 0, 0, 0, 5164),
    (5, B, 3328, 80, 64, 0, 0, 0, 0, 0, 5164), (5, H, 10007, 80, 64, 0, 0, 1024, 0, 0, 5164), (6, B, 3265, 64, 80, 0, 0, 1032, 0, 0, 5164),
    (6, H, 3266, 64, 80, 1, 0, 4, 0, 0, 5164), (6, F, 3462, 64, 80, 0, 0, 12, 0, 0, 5164), (8, B, 3328, 64, 80, 0, 0, 8, 0, 0, 5164),
    (8, H, 10007, 64, 80, 0, 1, 12, 0, 0, 5164), (0, F, 3265, 160, 96, 0, 0, 0, 0, 0, 5248), (1, F, 3266, 160, 96, 0, 0, 0, 0, 0, 5248),
    (1, B, 3328, 160, 96, 0, 0, 16, 0, 0, 5248), (1, H, 10007, 160, 96, 0, 0, 0, 0, 0, 5248), (4, H, 3265, 160, 96, 0, 0, 0, 0, 0, 5248),
    (4, B, 3462, 160, 96, 0, 0, 0, 0, 0, 5248), (5, B, 3266, 160, 96, 0, 0, 0, 0, 0, 5248), (5, H, 3328, 160, 96, 0, 0, 1024, 0, 0, 5248),
    (0, F, 3265, 160, 64, 0, 0, 8, 0, 0, 5264), (1, F, 3266, 160, 64, 0, 0, 16, 0, 0, 5264), (1, B, 3328, 160, 64, 0, 0, 0, 0, 0, 5264),
    (1, H, 10007, 160, 64, 0, 0, 16, 0, 0, 5264), (4, H, 3265, 160, 64, 0, 0, 0, 0, 0, 5264), (4, B, 3462, 160, 64, 0, 0, 0, 0, 0, 5264),
    (5, B, 3266, 160, 64, 0, 0, 0, 0, 0, 5264), (5, H, 3328, 160, 64, 0, 0, 1024, 0, 0, 5264), (8, B, 3266, 64, 80, 0, 0, 1032, 0, 0, 5164),
]
# ---- persistent wide tile (16-bit modes); the last eight rows: both sides of M <= 60000 ------------------------------------------------
WIDE = [
    (0, B, 4096, 384, 32, 0, 0, 3, 0, 0, 3003), (0, H, 4097, 384, 32, 0, 0, 11, 0, 0, 3003), (1, B, 4223, 384, 384, 0, 0, 0, 0, 0, 3003),
    (1, H, 4225, 384, 384, 0, 0, 16, 0, 0, 3003), (2, H, 4096, 384, 32, 0, 0, 3, 0, 0, 3003), (2, B, 32897, 192, 32, 0, 0, 3, 0, 0, 3003),
    (3, B, 4097, 384, 32, 0, 0, 3, 0, 0, 3003), (3, H, 4223, 384, 32, 0, 0, 0, 0, 0, 3003), (4, H, 4225, 384, 384, 0, 0, 0, 0, 0, 3003),
    (5, H, 4096, 384, 384, 0, 0, 1024, 0, 0, 3003), (5, B, 32897, 192, 192, 0, 0, 0, 0, 0, 3003), (6, B, 4097, 384, 384, 0, 0, 0, 0, 0, 3003),
    (6, H, 4223, 384, 384, 0, 0, 4, 0, 0, 3003), (8, B, 4225, 768, 384, 0, 0, 12, 0, 0, 3003), (8, H, 32897, 384, 192, 0, 1, 1032, 0, 0, 3003),
    (0, B, 4096, 256, 32, 0, 0, 0, 0, 0, 3004), (0, H, 4097, 256, 32, 0, 0, 3, 0, 0, 3004), (1, B, 4223, 256, 256, 0, 0, 0, 0, 0, 3004),
    (1, H, 4225, 256, 256, 0, 0, 16, 0, 0, 3004), (2, H, 4096, 256, 32, 0, 0, 3, 0, 0, 3004), (2, B, 32897, 256, 32, 0, 0, 3, 0, 0, 3004),
    (3, B, 4097, 256, 32, 0, 0, 3, 0, 0, 3004), (3, H, 4223, 256, 32, 0, 0, 0, 0, 0, 3004), (4, H, 4225, 256, 256, 0, 0, 0, 0, 0, 3004),
    (5, H, 4096, 256, 256, 0, 0, 1024, 0, 0, 3004), (5, B, 32897, 256, 256, 0, 0, 0, 0, 0, 3004), (6, B, 4097, 256, 256, 1, 0, 0, 0, 0, 3004),
    (6, H, 4223, 256, 256, 0, 0, 0, 0, 0, 3004), (8, B, 4225, 512, 256, 0, 0, 8, 0, 0, 3004), (8, H, 32897, 512, 256, 0, 0, 1036, 0, 0, 3004),
    (0, H, 60000, 192, 192, 0, 0, 0, 0, 0, 3003), (0, B, 60000, 192, 192, 0, 0, 0, 0, 0, 3003), (1, B, 60000, 192, 192, 0, 0, 0, 0, 0, 3003),
    (6, B, 60000, 192, 192, 0, 0, 0, 0, 0, 3003), (0, H, 60001, 192, 192, 0, 0, 0, 0, 0, 4448), (0, B, 60001, 192, 192, 0, 0, 0, 0, 0, 4448),
    (1, H, 60001, 192, 192, 0, 0, 0, 0, 0, 4448), (6, H, 60001, 192, 192, 1, 0, 0, 0, 0, 4448),
    (6, B, 5505, 384, 192, 0, 0, 8, 0, 0, 3003),   # dgrad through GELU' reaches the wide tile only with a contraction of twice the width
]
# ---- row-streaming (1000 +) and narrow row-streaming (2000 +) kernels ------------------------------------------------------------------
RS = [
    (0, F, 16384, 144, 48, 0, 0, 3, 0, 0, 1309), (0, B, 16391, 144, 48, 0, 0, 11, 0, 0, 1309), (0, H, 50176, 144, 48, 0, 0, 0, 0, 0, 1309),
    (0, F, 149504, 144, 48, 0, 0, 8, 0, 0, 1309), (3, B, 99335, 144, 48, 0, 0, 3, 0, 0, 1309), (3, H, 148487, 144, 48, 0, 0, 3, 0, 0, 1309),
    (0, F, 16384, 192, 48, 0, 0, 3, 0, 0, 1312), (0, B, 16391, 192, 48, 0, 0, 11, 0, 0, 1312), (0, H, 33792, 192, 48, 0, 0, 0, 0, 0, 1312),
    (2, B, 66567, 192, 48, 0, 0, 3, 0, 0, 1312), (2, H, 99335, 192, 48, 0, 0, 3, 0, 0, 1312), (6, B, 16384, 48, 192, 0, 0, 4, 0, 0, 1312),
    (6, H, 16391, 48, 192, 0, 0, 8, 0, 0, 1312), (6, F, 100352, 48, 192, 0, 0, 0, 0, 0, 1312), (8, B, 33792, 48, 192, 0, 1, 8, 0, 0, 1312),
    (8, H, 66567, 48, 192, 0, 0, 12, 0, 0, 1312), (0, F, 16384, 256, 64, 0, 0, 0, 0, 0, 1408), (0, B, 16391, 256, 64, 0, 0, 8, 0, 0, 1408),
    (0, H, 17408, 256, 64, 0, 0, 3, 0, 0, 1408), (2, B, 33799, 256, 64, 0, 0, 3, 0, 0, 1408), (2, H, 50183, 256, 64, 0, 0, 3, 0, 0, 1408),
    (6, B, 16384, 64, 256, 0, 0, 4, 0, 0, 1408), (6, H, 16391, 64, 256, 0, 0, 8, 0, 0, 1408), (6, F, 51200, 64, 256, 0, 0, 0, 0, 0, 1408),
    (8, B, 17408, 64, 256, 0, 1, 12, 0, 0, 1408), (8, H, 33799, 64, 256, 0, 0, 1036, 0, 0, 1408), (0, F, 16384, 192, 64, 0, 0, 0, 0, 0, 1412),
    (0, B, 16391, 192, 64, 0, 0, 8, 0, 0, 1412), (0, H, 33792, 192, 64, 0, 0, 3, 0, 0, 1412), (0, F, 100352, 192, 64, 0, 0, 11, 0, 0, 1412),
    (3, B, 66567, 192, 64, 0, 0, 3, 0, 0, 1412), (3, H, 99335, 192, 64, 0, 0, 3, 0, 0, 1412), (0, F, 16384, 384, 96, 0, 0, 8, 0, 0, 1608),
    (0, B, 16391, 384, 96, 0, 0, 3, 0, 0, 1608), (0, H, 22535, 384, 96, 0, 0, 11, 0, 0, 1608), (2, B, 33287, 384, 96, 0, 0, 3, 0, 0, 1608),
    (2, H, 34304, 384, 96, 0, 0, 3, 0, 0, 1608), (6, F, 16384, 96, 384, 0, 0, 12, 0, 0, 1608), (6, B, 16391, 96, 384, 0, 0, 1032, 0, 0, 1608),
    (6, H, 22535, 96, 384, 0, 0, 1036, 0, 0, 1608), (8, B, 33287, 96, 384, 0, 1, 1032, 0, 0, 1608), (8, H, 34304, 96, 384, 0, 0, 8, 0, 0, 1608),
    (0, F, 16384, 288, 96, 0, 0, 8, 0, 0, 1609), (0, B, 16391, 288, 96, 0, 0, 3, 0, 0, 1609), (0, H, 17408, 288, 96, 0, 0, 11, 0, 0, 1609),
    (0, F, 51200, 288, 96, 0, 0, 0, 0, 0, 1609), (3, B, 33799, 288, 96, 0, 0, 3, 0, 0, 1609), (3, H, 50183, 288, 96, 0, 0, 3, 0, 0, 1609),
    (1, F, 16384, 48, 144, 0, 0, 0, 0, 0, 2009), (1, B, 16391, 48, 144, 0, 0, 0, 0, 0, 2009), (1, H, 33792, 48, 144, 0, 0, 0, 0, 0, 2009),
    (6, F, 66567, 144, 48, 0, 0, 0, 0, 0, 2009), (6, B, 99335, 144, 48, 0, 0, 0, 0, 0, 2009), (6, H, 100352, 144, 48, 0, 0, 0, 0, 0, 2009),
    (7, F, 16384, 144, 48, 0, 0, 2, 0, 0, 2009), (7, B, 16391, 144, 48, 0, 0, 258, 0, 0, 2009), (7, H, 33792, 144, 48, 1, 0, 258, 0, 0, 2009),
    (1, F, 16384, 48, 192, 0, 0, 0, 0, 0, 2012), (1, B, 16391, 48, 192, 0, 0, 0, 0, 0, 2012), (1, H, 33792, 48, 192, 0, 0, 0, 0, 0, 2012),
    (5, B, 66567, 48, 192, 0, 0, 0, 0, 0, 2012), (5, H, 99335, 48, 192, 0, 0, 1024, 0, 0, 2012), (6, B, 16384, 192, 48, 0, 0, 0, 0, 0, 2012),
    (6, H, 16391, 192, 48, 0, 0, 0, 0, 0, 2012), (6, F, 100352, 192, 48, 0, 0, 0, 0, 0, 2012), (7, F, 16384, 192, 48, 0, 0, 2, 0, 0, 2012),
    (7, B, 16391, 192, 48, 0, 0, 258, 0, 0, 2012), (7, H, 33792, 192, 48, 1, 0, 258, 0, 0, 2012), (7, B, 16384, 288, 96, 1, 0, 2, 0, 0, 2018),
    (7, H, 16391, 288, 96, 1, 0, 258, 0, 0, 2018), (7, B, 33792, 288, 96, 1, 0, 2, 0, 0, 2018), (5, B, 16384, 96, 384, 0, 0, 0, 0, 0, 2024),
    (5, H, 16391, 96, 384, 0, 0, 1024, 0, 0, 2024), (5, B, 66567, 96, 384, 0, 0, 0, 0, 0, 2024), (5, H, 99335, 96, 384, 0, 0, 1024, 0, 0, 2024),
    (5, B, 100352, 96, 384, 0, 0, 0, 0, 0, 2024), (7, H, 16384, 384, 96, 1, 0, 2, 0, 0, 2024), (7, B, 33792, 384, 96, 1, 0, 258, 0, 0, 2024),
    # entry 7: both dy formats, with and without dres, every class of M under its cap
    (7, B, 16384, 144, 48, 0, 0, 258, 0, 0, 2009), (7, F, 16384, 144, 48, 0, 0, 258, 0, 0, 2009), (7, F, 16391, 144, 48, 0, 0, 2, 0, 0, 2009),
    (7, B, 16391, 144, 48, 1, 0, 258, 0, 0, 2009), (7, F, 33792, 144, 48, 0, 0, 258, 0, 0, 2009), (7, B, 33792, 144, 48, 1, 0, 2, 0, 0, 2009),
    (7, B, 66567, 144, 48, 0, 0, 2, 0, 0, 2009), (7, F, 66567, 144, 48, 0, 0, 2, 0, 0, 2009), (7, B, 99335, 144, 48, 0, 0, 258, 0, 0, 2009),
    (7, F, 99335, 144, 48, 0, 0, 258, 0, 0, 2009), (7, F, 100352, 144, 48, 0, 0, 2, 0, 0, 2009), (7, B, 100352, 144, 48, 1, 0, 258, 0, 0, 2009),
    (7, B, 16384, 192, 48, 0, 0, 258, 0, 0, 2012), (7, F, 16384, 192, 48, 0, 0, 258, 0, 0, 2012), (7, F, 16391, 192, 48, 0, 0, 2, 0, 0, 2012),
    (7, B, 16391, 192, 48, 1, 0, 258, 0, 0, 2012), (7, F, 33792, 192, 48, 0, 0, 258, 0, 0, 2012), (7, B, 33792, 192, 48, 1, 0, 2, 0, 0, 2012),
    (7, B, 66567, 192, 48, 0, 0, 2, 0, 0, 2012), (7, F, 66567, 192, 48, 0, 0, 2, 0, 0, 2012), (7, H, 16384, 288, 96, 1, 0, 258, 0, 0, 2018),
    (7, H, 16391, 288, 96, 1, 0, 2, 0, 0, 2018), (7, H, 33792, 288, 96, 1, 0, 258, 0, 0, 2018), (7, H, 16384, 384, 96, 1, 0, 258, 0, 0, 2024),
    (7, H, 16391, 384, 96, 1, 0, 2, 0, 0, 2024), (7, H, 33792, 384, 96, 1, 0, 258, 0, 0, 2024),
    # entry 0: LayerNorm x GELU output, all four combinations in every mode
    (0, H, 50183, 144, 48, 0, 0, 11, 0, 0, 1309), (0, B, 50183, 144, 48, 0, 0, 11, 0, 0, 1309), (0, F, 50183, 144, 48, 0, 0, 11, 0, 0, 1309),
    (0, H, 33799, 192, 48, 0, 0, 3, 0, 0, 1312), (0, B, 33799, 192, 48, 0, 0, 3, 0, 0, 1312), (0, F, 33799, 192, 48, 0, 0, 3, 0, 0, 1312),
    (0, H, 33799, 256, 64, 0, 0, 0, 0, 0, 1408), (0, B, 33799, 256, 64, 0, 0, 0, 0, 0, 1408), (0, F, 33799, 256, 64, 0, 0, 0, 0, 0, 1408),
    (0, H, 33799, 288, 96, 0, 0, 8, 0, 0, 1609), (0, B, 33799, 288, 96, 0, 0, 8, 0, 0, 1609), (0, F, 33799, 288, 96, 0, 0, 8, 0, 0, 1609),
    # combinations the rows above leave out: plain dgrad in mode 16f, fp32 dy into the LayerNorm backward in mode 16f
    (6, H, 33792, 48, 192, 0, 0, 4, 0, 0, 1312), (7, H, 16391, 144, 48, 0, 0, 2, 0, 0, 2009),
]
# ---- strided rows through the raw C ABI: ldx of entry 0, lddy / lddx / lddx2 of entry 6 (pad a multiple of 4 elements, 8 for bf16 rows) ----
STRIDED = [
    (0, F, 8130, 96, 96, 0, 0, 3, 0, 4, 4348), (0, B, 4097, 384, 32, 0, 0, 3, 0, 4, 3003), (0, H, 3266, 80, 64, 0, 0, 0, 0, 4, 5164),
    (0, F, 65, 96, 96, 0, 0, 11, 0, 4, 6031), (0, B, 16391, 192, 48, 0, 0, 11, 0, 4, 3003), (0, H, 300, 64, 128, 0, 0, 8, 0, 8, 6044),
    (0, F, 16391, 192, 48, 0, 0, 3, 0, 8, 4448), (6, F, 5449, 48, 192, 0, 0, 0, 0, 4, 4448), (6, B, 5449, 48, 192, 1, 0, 0, 0, 8, 4448),
    (6, B, 5505, 192, 192, 0, 0, 0, 0, 4, 3003), (6, F, 3266, 64, 80, 0, 0, 0, 0, 4, 5164), (6, B, 300, 48, 192, 0, 0, 4, 0, 4, 6041),
    (6, H, 65, 128, 64, 0, 0, 0, 0, 4, 6044), (6, F, 5449, 48, 192, 0, 0, 32, 64, 4, 4448), (6, B, 300, 48, 192, 0, 0, 32, 100, 4, 6041),
    (6, B, 5449, 48, 192, 1, 1, 0, 0, 8, 4448), (6, H, 5505, 192, 192, 1, 0, 0, 0, 8, 3003), (6, B, 5505, 192, 192, 0, 0, 160, 64, 4, 3003),
]
# ---- every extra of leod_linear_dgrad, in f32 and bf16, on both sides of the LDS threshold (and on the wide tile): accumulate 128, dres 256,
# dx2 32 with nsplit, colsum 64, aux_u 8 without / with kscale 4, their combinations; the last four rows: dx_fmt = 1 -------------------------
EXTRAS = [
    (6, F, 5449, 48, 192, 0, 0, 128, 0, 0, 4448), (6, F, 5449, 48, 192, 0, 0, 256, 0, 0, 4448), (6, F, 5449, 48, 192, 0, 0, 32, 64, 0, 4448),
    (6, F, 5449, 48, 192, 0, 0, 64, 0, 0, 4448), (6, F, 5449, 48, 192, 0, 0, 8, 0, 0, 4448), (6, F, 5449, 48, 192, 0, 0, 12, 0, 0, 4448),
    (6, F, 5449, 48, 192, 0, 0, 192, 0, 0, 4448), (6, F, 5449, 48, 192, 0, 0, 68, 0, 0, 4448), (6, F, 5449, 48, 192, 0, 0, 1032, 0, 0, 4448),
    (6, F, 5449, 48, 192, 0, 0, 96, 160, 0, 4448), (6, F, 300, 48, 192, 0, 0, 128, 0, 0, 6041), (6, F, 300, 48, 192, 0, 0, 256, 0, 0, 6041),
    (6, F, 300, 48, 192, 0, 0, 32, 64, 0, 6041), (6, F, 300, 48, 192, 0, 0, 64, 0, 0, 6041), (6, F, 300, 48, 192, 0, 0, 8, 0, 0, 6041),
    (6, F, 300, 48, 192, 0, 0, 12, 0, 0, 6041), (6, F, 300, 48, 192, 0, 0, 192, 0, 0, 6041), (6, F, 300, 48, 192, 0, 0, 68, 0, 0, 6041),
    (6, F, 300, 48, 192, 0, 0, 1032, 0, 0, 6041), (6, F, 300, 48, 192, 0, 0, 96, 160, 0, 6041), (6, F, 8193, 96, 96, 0, 0, 128, 0, 0, 4348),
    (6, F, 8193, 96, 96, 0, 0, 256, 0, 0, 4348), (6, F, 8193, 96, 96, 0, 0, 32, 64, 0, 4348), (6, F, 8193, 96, 96, 0, 0, 64, 0, 0, 4348),
    (6, F, 8193, 96, 96, 0, 0, 8, 0, 0, 4348), (6, F, 8193, 96, 96, 0, 0, 12, 0, 0, 4348), (6, F, 8193, 96, 96, 0, 0, 192, 0, 0, 4348),
    (6, F, 8193, 96, 96, 0, 0, 68, 0, 0, 4348), (6, F, 8193, 96, 96, 0, 0, 1032, 0, 0, 4348), (6, F, 8193, 96, 96, 0, 0, 96, 64, 0, 4348),
    (6, B, 5449, 48, 192, 0, 0, 128, 0, 0, 4448), (6, B, 5449, 48, 192, 0, 0, 256, 0, 0, 4448), (6, B, 5449, 48, 192, 0, 0, 32, 64, 0, 4448),
    (6, B, 5449, 48, 192, 0, 0, 64, 0, 0, 4448), (6, B, 5449, 48, 192, 0, 0, 8, 0, 0, 4448), (6, B, 5449, 48, 192, 0, 0, 12, 0, 0, 4448),
    (6, B, 5449, 48, 192, 0, 0, 192, 0, 0, 4448), (6, B, 5449, 48, 192, 0, 0, 68, 0, 0, 4448), (6, B, 5449, 48, 192, 0, 0, 1032, 0, 0, 4448),
    (6, B, 5449, 48, 192, 0, 0, 96, 160, 0, 4448), (6, B, 300, 48, 192, 0, 0, 128, 0, 0, 6041), (6, B, 300, 48, 192, 0, 0, 256, 0, 0, 6041),
    (6, B, 300, 48, 192, 0, 0, 32, 64, 0, 6041), (6, B, 300, 48, 192, 0, 0, 64, 0, 0, 6041), (6, B, 300, 48, 192, 0, 0, 8, 0, 0, 6041),
    (6, B, 300, 48, 192, 0, 0, 12, 0, 0, 6041), (6, B, 300, 48, 192, 0, 0, 192, 0, 0, 6041), (6, B, 300, 48, 192, 0, 0, 68, 0, 0, 6041),
    (6, B, 300, 48, 192, 0, 0, 1032, 0, 0, 6041), (6, B, 300, 48, 192, 0, 0, 96, 160, 0, 6041), (6, B, 5505, 192, 192, 0, 0, 128, 0, 0, 3003),
    (6, B, 5505, 192, 192, 0, 0, 256, 0, 0, 3003), (6, B, 5505, 192, 192, 0, 0, 32, 64, 0, 3003), (6, B, 5505, 192, 192, 0, 0, 64, 0, 0, 3003),
    (6, B, 5505, 192, 192, 0, 0, 8, 0, 0, 4448), (6, B, 5505, 192, 192, 0, 0, 12, 0, 0, 4448), (6, B, 5505, 192, 192, 0, 0, 192, 0, 0, 3003),
    (6, B, 5505, 192, 192, 0, 0, 68, 0, 0, 3003), (6, B, 5505, 192, 192, 0, 0, 1032, 0, 0, 4448), (6, B, 5505, 192, 192, 0, 0, 96, 160, 0, 3003),
    (6, B, 5449, 48, 192, 0, 1, 0, 0, 0, 4448), (6, H, 5449, 48, 192, 1, 1, 0, 0, 0, 4448), (6, H, 8193, 96, 96, 0, 1, 0, 0, 0, 4348),
    (6, B, 5505, 192, 192, 1, 1, 0, 0, 0, 3003),
]
# ---- what leod_linear_dgrad refuses: dres + accumulate and dres + nsplit (-1); dx_fmt = 1 off the LDS path, in mode f32, with an extra (-3) --
REFUSALS = [
    (6, F, 5449, 48, 192, 0, 0, 384, 0, 0, -1), (6, F, 5449, 48, 192, 0, 0, 288, 64, 0, -1), (6, F, 300, 48, 192, 0, 0, 384, 0, 0, -1),
    (6, F, 300, 48, 192, 0, 0, 288, 64, 0, -1), (6, F, 300, 48, 192, 0, 1, 0, 0, 0, -3), (6, B, 5449, 48, 192, 0, 0, 384, 0, 0, -1),
    (6, B, 5449, 48, 192, 0, 0, 288, 64, 0, -1), (6, B, 300, 48, 192, 0, 0, 384, 0, 0, -1), (6, B, 300, 48, 192, 0, 0, 288, 64, 0, -1),
    (6, B, 300, 48, 192, 0, 1, 0, 0, 0, -3), (6, H, 5449, 48, 192, 0, 0, 384, 0, 0, -1), (6, H, 5449, 48, 192, 0, 0, 288, 64, 0, -1),
    (6, H, 300, 48, 192, 0, 0, 384, 0, 0, -1), (6, H, 300, 48, 192, 0, 0, 288, 64, 0, -1), (6, H, 300, 48, 192, 0, 1, 0, 0, 0, -3),
    (6, F, 5449, 48, 192, 0, 1, 0, 0, 0, -3), (6, B, 5449, 48, 192, 0, 1, 128, 0, 0, -3), (6, B, 5449, 48, 192, 0, 1, 256, 0, 0, -3),
    (6, B, 5449, 48, 192, 0, 1, 32, 64, 0, -3), (6, B, 5449, 48, 192, 0, 1, 64, 0, 0, -3), (6, B, 5449, 48, 192, 0, 1, 8, 0, 0, -3),
]
ROUTES = G16 + LDS + WIDE + RS
ALL_ROWS = ROUTES + STRIDED + EXTRAS           # every row that launches
MODES = (F, B, H)
ENTRY_MODES = {e: MODES if e in (0, 1, 6, 7) else (B, H) for e in range(9)}       # entries 2 - 5 and 8 take 16-bit tensors: no mode f32


def _id(r):
    return '-'.join(str(v) for v in (f'e{r[0]}', r[1], r[2], f'{r[3]}x{r[4]}', f'a{r[5]}o{r[6]}', f'f{r[7]}', f'n{r[8]}', f'p{r[9]}', r[10]))


def route_of(ops, row):
    """the routing query with the row's strides and flags (no launch; the caller has set the row's precision mode)"""
    e, _, M, N, K, a16, out16, flags, nsplit, pad = row[:10]
    lda = ((N if e >= 6 else K) + pad) if pad else None
    ldo = ((nsplit if nsplit else K) + pad) if pad and e == 6 else None
    return ops.linear_route(e, M, N, K, lda=lda, ldo=ldo, a16=a16, out16=out16, flags=flags & le.ABI_FLAGS, nsplit=nsplit)


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


def _dev(t, dtype=F32, pad=0):
    if t is None:
        return None, 0
    if t.dim() == 1:
        return t.to(dtype).to(DEV), 0
    buf, ld = le.padded(t.to(dtype), pad)
    return buf.to(DEV), ld


def _same(got, want, what):
    want = want.to(DEV)
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} for {tuple(want.shape)}'
    assert torch.equal(got.float(), want), f'{what}: {int((got.float() != want).sum())} of {want.numel()} elements differ'


def _same_masked(got, want, live, what):
    """equal where the GELU operand is positive, at most MASK_TOL in magnitude where it is below -8 (``want`` is 0 there)"""
    err = (got.double() - want.to(DEV).double()).abs()
    bound = torch.where(live.to(DEV), 0.0, le.MASK_TOL)
    assert bool((err <= bound).all()), f'{what}: {int((err > bound).sum())} of {err.numel()} elements differ'


def _poison(M, *specs):
    """the wrappers allocate their outputs with torch.empty, and the caching allocator hands a block that an earlier, identical row freed
    straight back -- with that row's correct values in it.  NaN blocks of the outputs' sizes, freed just before the call, take their place:
    an element the kernel does not write never compares equal."""
    junk = [torch.full((M, cols), float('nan'), dtype=dtype, device=DEV) for cols, dtype in specs]
    del junk


def _pad_intact(buf, width, what):
    assert bool((buf[:, width:].float() == le.PAD_VALUE).all()), f'{what}: padding columns were written'


def _forward_ln(ops, lib, p, mode, flags, pad, entry):
    """entries 0, 2, 3 -> (out, out_act, stats)"""
    M, N, K = p['M'], p['N'], p['K']
    ln, act = bool(flags & LN), bool(flags & AUX)
    x, ldx = _dev(p['x'], pad=pad)
    lw, lb = (p['ln_w'].to(DEV), p['ln_b'].to(DEV)) if ln else (None, None)
    W, bias = p['W'].to(DEV), p['bias'].to(DEV)
    if entry == 2:
        out, a, st = ops.ln_linear_fwd(x, lw, lb, W, bias, want_act=True, want_stats=True)
        assert out.dtype is F16 and a is None, 'leod_ln_linear_gelu16_fwd refused the row'
    elif entry == 3:
        out, a, st = ops.ln_linear_fwd(x, lw, lb, W, bias, out_bf16=True)
        assert out.dtype is ops.act16_dtype() and a is None, 'leod_ln_linear_bf16_fwd refused the row'
    elif pad == 0 and bool(flags & STATS) == ln:
        out, a, st = ops.ln_linear_fwd(x, lw, lb, W, bias, want_act=act)
    else:                                            # a padded ldx, LayerNorm without a statistics buffer: the raw entry point
        from leod_amd import _lib
        out, a = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV) if act else None
        st = torch.empty(M, 2, device=DEV) if flags & STATS else None
        _lib.check(lib.leod_ln_linear_fwd(ops._p(x), ldx, ops._p(lw), ops._p(lb), le.EPS, ops._p(W), ops._p(bias), ops._p(out), ops._p(a), ops._p(st),
                                          M, N, K, ops._stream()), 'leod_ln_linear_fwd')
    if pad:
        _pad_intact(x, K, 'x')
    return out, a, st


def _check_forward_ln(p, mode, flags, entry, out, a, st):
    ln, ref = bool(flags & LN), p['ref']
    kind = le.out16_kind(entry, 0)
    if kind is not None:
        dtype = F16 if kind == 'f16' or mode == H else BF16
        assert out.dtype is dtype and le.representable(ref['out'], dtype), 'the reference does not fit the stored format'
    if flags & AUX:
        assert float(ref['out'].min()) >= 8 and torch.equal(ref['out'], ref['out'].round())
    if ln and mode == F:                             # nothing rounds the error of mean, rstd and eps away: the fp32 bound
        le.close_fp32(out, p['true']['out'], what='out (LayerNorm, mode f32)')
    else:
        _same(out, ref['out'], 'out')
    if flags & AUX and entry == 0:
        assert torch.equal(a, out), 'out_act: gelu(out) != out on pre-activations >= 8'
    if ln and st is not None:
        le.close_fp32(st[:, 0], p['true']['mean'], atol=1e-6, what='stats_out: mean')
        le.close_fp32(st[:, 1], p['true']['rstd'], rtol=1e-5, what='stats_out: rstd')


def _lsres(ops, p, mode, flags, entry):
    """entries 1, 4, 5"""
    a = p['a'].to({1: F32, 4: ops.act16_dtype(), 5: F16}[entry]).to(DEV)
    out, t = ops.linear_lsres_fwd(a, p['W'].to(DEV), p['bias'].to(DEV), p['gamma'].to(DEV), p['res'].to(DEV), want_t=bool(flags & TOUT),
                                  a_gelu=False if entry == 4 else None)
    if flags & MASKED:
        err = float((out.double() - p['ref']['out'].to(DEV).double()).abs().max())
        assert err <= le.MASK_TOL, f'out: max error {err:.3e}'
    else:
        _same(out, p['ref']['out'], 'out')
    if flags & TOUT:
        _same(t, p['ref']['tout'], 'tout')


def dgrad_buffers(p, a16, out16, flags, nsplit, pad):
    """device buffers of one leod_linear_dgrad call: every strided one padded, every output on its start values"""
    M, N, K = p['M'], p['N'], p['K']
    k1 = nsplit if nsplit else K
    b = dict(dy=_dev(p['dy'], BF16 if a16 else F32, pad), W=p['W'].to(DEV), ks=_dev(p.get('kscale'))[0], aux=_dev(p.get('aux_u'))[0],
             dres=_dev(p.get('dres'), pad=pad)[0], colsum=_dev(p.get('colsum0'))[0])
    dx0 = p['dx0'] if flags & ACCUMULATE else torch.full((M, K), le.PAD_VALUE)
    b['dx'] = _dev(dx0[:, :k1], BF16 if out16 else F32, pad)
    b['dx2'] = _dev(dx0[:, k1:], pad=pad) if flags & DX2 else (None, 0)
    return b


def dgrad_raw(ops, lib, b, M, N, K, a16, out16, flags, nsplit):
    return lib.leod_linear_dgrad(ops._p(b['dy'][0]), b['dy'][1], ops._p(b['ks']), ops._p(b['W']), ops._p(b['dx'][0]), b['dx'][1], ops._p(b['dx2'][0]),
                                 b['dx2'][1], nsplit, ops._p(b['aux']), ops._p(b['colsum']), 1 if flags & ACCUMULATE else 0, ops._p(b['dres']),
                                 M, N, K, a16, out16, ops._stream())


def _dgrad(ops, lib, p, a16, out16, flags, nsplit, pad):
    """entry 6: through ops.linear_dgrad with dense rows, else the raw entry point; twice where an output accumulates"""
    from leod_amd import _lib
    M, N, K = p['M'], p['N'], p['K']
    k1 = nsplit if nsplit else K
    b = dgrad_buffers(p, a16, out16, flags, nsplit, pad)
    live = (p['aux_u'] > 0) if flags & MASKED else None
    for n in range(p['calls']):
        if pad:
            _lib.check(dgrad_raw(ops, lib, b, M, N, K, a16, out16, flags, nsplit), 'leod_linear_dgrad')
            dx, dx2 = b['dx'][0], b['dx2'][0]
        else:
            acc = bool(flags & ACCUMULATE)
            got = ops.linear_dgrad(b['dy'][0], b['W'], kscale=b['ks'], aux_u=b['aux'], colsum=b['colsum'], out=b['dx'][0] if acc else None, accumulate=acc,
                                   split=nsplit, out2=b['dx2'][0] if acc else None, dres=b['dres'], out_bf16=bool(out16))
            dx, dx2 = got if nsplit else (got, None)
        ref = p['ref']['dx'][n]
        if out16:
            assert dx.dtype is BF16 and le.representable(ref, BF16), 'the reference does not fit bf16'
        if live is not None:
            _same_masked(dx[:, :k1], ref[:, :k1], live[:, :k1], f'dx, call {n + 1}')
        else:
            _same(dx[:, :k1], ref[:, :k1], f'dx, call {n + 1}')
        if nsplit:
            _same(dx2[:, :K - k1], ref[:, k1:], f'dx2, call {n + 1}')
        if flags & COLSUM:
            _same(b['colsum'], p['ref_colsum'][n], f'colsum, call {n + 1}')
    if pad:
        _pad_intact(b['dy'][0], N, 'dy')
        _pad_intact(dx, k1, 'dx')
        if nsplit:
            _pad_intact(dx2, K - k1, 'dx2')


def _dgrad_lnbwd(ops, p, a16):
    """entry 7, at the fp32 bounds of test_linear_dgrad_ln_bwd in every mode"""
    dres = p['dres'].to(DEV) if p['dres'] is not None else None
    dw, db = p['dgamma0'].to(DEV), p['dbeta0'].to(DEV)
    dx = ops.linear_dgrad_ln_bwd(p['dy'].to(BF16 if a16 else F32).to(DEV), p['W'].to(DEV), p['x'].to(DEV), p['stats'].to(DEV), p['ln_w'].to(DEV), dres, dw, db)
    le.close_fp32(dx, p['true']['dx'], rtol=1e-4, atol=1e-5, what='dx')
    le.close_fp32(dw, p['true']['dgamma'], rtol=3e-4, atol=1e-4, what='dgamma')
    le.close_fp32(db, p['true']['dbeta'], rtol=3e-4, atol=1e-4, what='dbeta')


def _dgrad_gelu16(ops, lib, p, out16, flags):
    """entry 8: ops.linear_dgrad stores du in the build's format (ops.BF16_GRADS); the other one through the raw entry point"""
    from leod_amd import _lib
    M, N, K = p['M'], p['N'], p['K']
    dy, W, ks, u = p['dy'].to(DEV), p['W'].to(DEV), _dev(p.get('kscale'))[0], p['aux_u'].to(F16).to(DEV)
    if bool(out16) == bool(ops.BF16_GRADS):
        du = ops.linear_dgrad(dy, W, kscale=ks, aux_u=u)
    else:
        du = torch.empty(M, K, dtype=BF16 if out16 else F32, device=DEV)
        _lib.check(lib.leod_linear_dgrad_gelu16(ops._p(dy), ops._p(ks), ops._p(W), ops._p(u), ops._p(du), M, N, K, out16, ops._stream()), 'leod_linear_dgrad_gelu16')
    ref = p['ref']['dx'][0]
    assert du.dtype is (BF16 if out16 else F32)
    if out16:
        assert le.representable(ref, BF16), 'the reference does not fit bf16'
    if flags & MASKED:
        _same_masked(du, ref, p['aux_u'] > 0, 'du')
    else:
        _same(du, ref, 'du')


def run_row(ops, row):
    """precision mode, route assertion, the call, the comparison with the float64 reference"""
    from leod_amd import _lib
    entry, mode, M, N, K, a16, out16, flags, nsplit, pad, code = row
    ops.set_precision(mode)
    got = route_of(ops, row)
    assert got == code, f'route {got}, this row is here for {code}: re-derive its shape from the predicates'
    p = le.problem(entry, M, N, K, a16, out16, flags, nsplit)
    if flags & (COLSUM | ACCUMULATE) or entry == 7:
        assert le.reduction_bound(entry, M, N, K, flags, p['dy_max'], p['w_max']) < 2 ** 24
    lib = _lib.lib()
    k1 = nsplit if nsplit else K
    _poison(M, *{0: [(N, F32)] * (2 if flags & AUX else 1), 1: [(N, F32)] * (2 if flags & TOUT else 1), 2: [(N, F16)], 3: [(N, ops.act16_dtype())],
                 4: [(N, F32)], 5: [(N, F32)], 6: [(k1, BF16 if out16 else F32), (max(K - k1, 1), F32)], 7: [(K, F32)],
                 8: [(K, BF16 if out16 else F32)]}[entry])
    if entry in (0, 2, 3):
        _check_forward_ln(p, mode, flags, entry, *_forward_ln(ops, lib, p, mode, flags, pad, entry))
    elif entry in (1, 4, 5):
        _lsres(ops, p, mode, flags, entry)
    elif entry == 6:
        _dgrad(ops, lib, p, a16, out16, flags, nsplit, pad)
    elif entry == 7:
        _dgrad_lnbwd(ops, p, a16)
    else:
        _dgrad_gelu16(ops, lib, p, out16, flags)


@pytest.mark.parametrize('row', ROUTES, ids=_id)
def test_route_exact(ops, row):
    run_row(ops, row)


@pytest.mark.parametrize('row', STRIDED, ids=_id)
def test_route_exact_strided(ops, row):
    run_row(ops, row)


@pytest.mark.parametrize('row', EXTRAS, ids=_id)
def test_dgrad_extras_exact(ops, row):
    run_row(ops, row)


@pytest.mark.parametrize('row', REFUSALS, ids=_id)
def test_dgrad_refusals_touch_nothing(ops, row):
    """the error code of the routing query is what the call returns, and dx, dx2 and colsum keep their start values"""
    from leod_amd import _lib
    entry, mode, M, N, K, a16, out16, flags, nsplit, pad, code = row
    ops.set_precision(mode)
    assert route_of(ops, row) == code
    # operands of the widest legal subset of the flags: the refusal is decided before anything is read
    p = le.problem(6, M, N, K, a16, 0, flags & (KSCALE | AUX | DRES | ACCUMULATE | COLSUM | DX2), nsplit)
    p = dict(p, colsum0=le.start_vector(K, 2), dx0=le.start_values(M, K))
    b = dgrad_buffers(p, a16, out16, flags | ACCUMULATE, nsplit, 0)
    before = [t.clone() for t in (b['dx'][0], b['dx2'][0], b['colsum']) if t is not None]
    if not flags & COLSUM:
        b['colsum'] = None
    assert dgrad_raw(ops, _lib.lib(), b, M, N, K, a16, out16, flags, nsplit) == code
    torch.cuda.synchronize()
    for was, now in zip(before, (t for t in (b['dx'][0], b['dx2'][0], b['colsum']) if t is not None)):
        assert torch.equal(was, now), 'a refused call wrote to an output'


@pytest.mark.parametrize('entry,mode', [(e, m) for e in range(9) for m in ENTRY_MODES[e]])
def test_no_rows_is_ok_and_touches_nothing(ops, entry, mode):
    """M = 0: LEOD_OK from every entry in every mode that has it, the routing query says 0, no output is written"""
    from leod_amd import _lib
    ops.set_precision(mode)
    lib, s, P = _lib.lib(), ops._stream(), ops._p
    N, K = (144, 48) if entry == 7 else (192, 48) if entry in (0, 2, 3) else (48, 192)
    flags = {0: LN | STATS | AUX, 2: LN | STATS, 3: LN | STATS, 7: STATS, 8: AUX}.get(entry, 0)
    assert ops.linear_route(entry, 0, N, K, flags=flags) == 0
    rows32, rows16 = torch.full((4, 192), 3.0, device=DEV), torch.full((4, 192), 3.0, device=DEV, dtype=F16)
    vec, st = torch.ones(192, device=DEV), torch.ones(4, 2, device=DEV)
    out, out2, out16, acc1, acc2 = rows32.clone(), rows32.clone(), rows16.clone(), vec.clone(), vec.clone()
    rc = {0: lambda: lib.leod_ln_linear_fwd(P(rows32), K, P(vec), P(vec), le.EPS, P(rows32), P(vec), P(out), P(out2), P(st), 0, N, K, s),
          1: lambda: lib.leod_linear_lsres_fwd(P(rows32), P(rows32), P(vec), P(vec), P(rows32), P(out), P(out2), 0, N, K, s),
          2: lambda: lib.leod_ln_linear_gelu16_fwd(P(rows32), P(vec), P(vec), le.EPS, P(rows32), P(vec), P(out16), P(st), 0, N, K, s),
          3: lambda: lib.leod_ln_linear_bf16_fwd(P(rows32), P(vec), P(vec), le.EPS, P(rows32), P(vec), P(out16), P(st), 0, N, K, s),
          4: lambda: lib.leod_linear_lsres_bf16_fwd(P(rows16), P(rows32), P(vec), P(vec), P(rows32), P(out), 0, N, K, s),
          5: lambda: lib.leod_linear_lsres_gelu16_fwd(P(rows16), P(rows32), P(vec), P(vec), P(rows32), P(out), 0, N, K, s),
          6: lambda: lib.leod_linear_dgrad(P(rows32), N, P(vec), P(rows32), P(out), K, None, 0, 0, None, P(acc1), 0, None, 0, N, K, 0, 0, s),
          7: lambda: lib.leod_linear_dgrad_lnbwd(P(rows32), P(rows32), P(rows32), P(st), P(vec), None, P(out), P(acc1), P(acc2), 0, N, K, 0, s),
          8: lambda: lib.leod_linear_dgrad_gelu16(P(rows32), P(vec), P(rows32), P(rows16), P(out), 0, N, K, 0, s)}[entry]()
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(out, rows32) and torch.equal(out2, rows32) and torch.equal(out16, rows16) and torch.equal(acc1, vec) and torch.equal(acc2, vec)
    assert torch.equal(st, torch.ones(4, 2, device=DEV))


def test_row_count():
    assert 350 <= len(ALL_ROWS) <= 450, len(ALL_ROWS)
