"""Operands on which a Linear weight gradient (dW += dy^T X, dbias += colsum(dy)) has NO rounding error, in any precision mode and any
summation order -- so the tests of tests/test_wgrad_routes_gpu.py compare for equality instead of choosing a tolerance.  One dropped or
doubled row, a chunk summed twice, a padding column read as data: each changes an element by at least 0.5 and fails ``torch.equal``.

* rows / concat / 16-bit rows: dy in +-{1,2,3}, x in +-{1,2,3,4}.  At most 3 significant bits: bf16 / fp16 storage and any rounding of
  an operand to bf16 is the identity; every product is an integer of magnitude <= 12; every partial sum is an integer below 2^24, so
  fp32 accumulation (MFMA, partial tiles, the reduce launch, atomics) is exact in every order.
* LayerNorm from saved statistics (x_fmt 1): the kernels take (mean, rstd) from the caller and never recompute them, so the test
  chooses them: integer mean in [-2, 2], rstd in {0.5, 1, 2}, x - mean in +-{1,2,3}, ln_w in {1,2,-1,-2}, ln_b in {-1,0,1,2}.  xhat,
  xhat w and xhat w + b are multiples of 0.5 of magnitude <= 14 (5 significant bits): exact in bf16, in either evaluation order of the
  code (per element in the loader; (sum dy xhat) w + colsum(dy) b on the finished tile).
* GELU of the fp16 pre-activation (x_fmt 2): u in {8,10,12,14,16}.  common.hpp computes Phi(u) = 1 - 0.5 poly exp(-u^2 / 2), whose tail
  is below 1e-15 for u >= 8: Phi(u) == 1.0f and gelu(u) == u bit for bit.  No negative u (gelu(-8) is tiny but not zero).

tests/test_wgrad_exact_cpu.py checks these claims on the generated values themselves."""
import torch

XMODES = ('rows', 'ln', 'gelu16', 'concat', 'bf16rows', 'f16rows')
X_FMT = {'rows': 0, 'ln': 1, 'gelu16': 2, 'concat': 0, 'bf16rows': 3, 'f16rows': 4}
# largest row count the route tests may use per x mode, and the smallest step of dW there: (|dW0| + 2 M max|dy| max|X|) / step < 2^24
# (two accumulating calls on a non-zero start)
M_MAX = 66000
DY_MAX, X_MAX, STEP = 3.0, {'rows': 4.0, 'concat': 4.0, 'bf16rows': 4.0, 'f16rows': 4.0, 'ln': 14.0, 'gelu16': 16.0}, \
    {'rows': 1.0, 'concat': 1.0, 'bf16rows': 1.0, 'f16rows': 1.0, 'ln': 0.5, 'gelu16': 1.0}
W0_MAX = 5.0
PAD_VALUE = 64.0        # padding columns of the strided cases: exactly representable, and one of them read as data moves a sum by >= 64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pick(values, shape, g):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _signed(mags, shape, g):
    return _pick(mags, shape, g) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def make_dy(M, N, dy16, seed=0):
    dy = _signed([1., 2., 3.], (M, N), _gen(1000 + seed))
    return dy.to(torch.bfloat16) if dy16 else dy


def make_x(xmode, M, K, seed=0, K1=None):
    """-> dict: ``x`` (as stored: fp32 / fp16 / bf16), ``X`` (fp32 [M,K], the operand of the contraction), and per mode ``x2`` (concat),
    ``stats`` [M,2] + ``ln_w`` + ``ln_b`` + ``xhat`` (ln)."""
    g = _gen(2000 + seed)
    if xmode in ('rows', 'bf16rows', 'f16rows'):
        x = _signed([1., 2., 3., 4.], (M, K), g)
        st = {'rows': torch.float32, 'bf16rows': torch.bfloat16, 'f16rows': torch.float16}[xmode]
        return dict(x=x.to(st), X=x)
    if xmode == 'concat':
        K1 = K // 2 if K1 is None else K1
        x = _signed([1., 2., 3., 4.], (M, K), g)
        return dict(x=x[:, :K1].contiguous(), x2=x[:, K1:].contiguous(), X=x, K1=K1)
    if xmode == 'gelu16':
        u = _pick([8., 10., 12., 14., 16.], (M, K), g)
        return dict(x=u.to(torch.float16), X=u)
    assert xmode == 'ln', xmode
    mean = torch.randint(-2, 3, (M, 1), generator=g).float()
    rstd = _pick([0.5, 1., 2.], (M, 1), g)
    d = _signed([1., 2., 3.], (M, K), g)
    ln_w, ln_b = _pick([1., 2., -1., -2.], (K,), g), _pick([-1., 0., 1., 2.], (K,), g)
    # where xhat w == -b the operand would vanish; the mirrored deviation gives 2 b there (b != 0 in that case), still inside the value sets
    d = torch.where(d * rstd * ln_w + ln_b == 0, -d, d)
    xhat = d * rstd
    return dict(x=d + mean, stats=torch.cat([mean, rstd], 1).contiguous(), ln_w=ln_w, ln_b=ln_b, xhat=xhat, X=xhat * ln_w + ln_b)


def start_values(N, K):
    """dW and dbias never start from zero: two different non-zero integer patterns"""
    n, k = torch.arange(N).view(N, 1), torch.arange(K).view(1, K)
    return ((n * 7 + k * 3) % 11 - 5).float(), (torch.arange(N) % 7 - 3).float()


def reference(dy, X):
    """float64 BLAS: exact, every sum is far below 2^53"""
    d = dy.double()
    return (d.t() @ X.double()).float(), d.sum(0).float()


def padded(t, pad):
    """[M, C] -> ([M, C + pad] buffer whose extra columns hold PAD_VALUE, its row stride)"""
    if pad == 0:
        return t.contiguous(), t.shape[1]
    buf = torch.full((t.shape[0], t.shape[1] + pad), PAD_VALUE, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf, t.shape[1] + pad
