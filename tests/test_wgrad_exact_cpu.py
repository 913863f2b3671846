"""The operand recipes of tests/wgrad_exact.py do what their docstring says -- checked on the generated values, without a GPU.  This is
what makes ``torch.equal`` the right assertion in tests/test_wgrad_routes_gpu.py."""
import numpy as np
import pytest
import torch

import wgrad_exact as we

M, N, K = 4099, 20, 36


def _roundtrips(t):
    return torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t)


@pytest.mark.parametrize('xmode', we.XMODES)
def test_operands_are_exact_in_16_bits_and_never_zero(xmode):
    for dy16 in (False, True):
        dy = we.make_dy(M, N, dy16, seed=3).float()
        assert _roundtrips(dy) and bool((dy != 0).all()) and float(dy.abs().max()) <= we.DY_MAX
    o = we.make_x(xmode, M, K, seed=3, K1=12 if xmode == 'concat' else None)
    X = o['X']
    assert X.dtype is torch.float32 and X.shape == (M, K)
    assert _roundtrips(X) and bool((X != 0).all()), 'a zero operand would hide a dropped contribution'
    assert float(X.abs().max()) <= we.X_MAX[xmode]
    assert torch.equal(X / we.STEP[xmode], (X / we.STEP[xmode]).round())
    if xmode == 'concat':
        assert o['x'].shape[1] == 12 and torch.equal(torch.cat([o['x'], o['x2']], 1), X)
    elif xmode == 'ln':
        mean, rstd = o['stats'][:, :1], o['stats'][:, 1:]
        xhat = (o['x'] - mean) * rstd                      # fp32, the order of the kernels
        assert torch.equal(xhat, o['xhat']) and torch.equal(xhat * o['ln_w'] + o['ln_b'], X)
        for t in (o['x'], xhat, xhat * o['ln_w']):
            assert _roundtrips(t)
        assert bool((xhat != 0).all()) and float(xhat.abs().max()) <= 6
        assert set(rstd.flatten().tolist()) <= {0.5, 1.0, 2.0} and float(mean.abs().max()) <= 2
    else:
        assert torch.equal(o['x'].float(), X)
        assert o['x'].dtype is {'rows': torch.float32, 'gelu16': torch.float16, 'bf16rows': torch.bfloat16, 'f16rows': torch.float16}[xmode]
    # removing or doubling one (row, n, k) contribution moves dW[n, k] by |dy| |X| >= 1 * STEP
    assert float((dy.abs().min() * X.abs().min())) >= we.STEP[xmode]


@pytest.mark.parametrize('xmode', we.XMODES)
def test_every_partial_sum_is_an_fp32_integer(xmode):
    """two accumulating calls on the non-zero start, at the largest row count the route tests use, in units of the smallest step"""
    W0, b0 = we.start_values(N, K)
    assert float(W0.abs().max()) <= we.W0_MAX and bool((W0 != 0).any()) and bool((b0 != 0).any()) and not torch.equal(W0[0, :N], b0)
    worst = (we.W0_MAX + 2 * we.M_MAX * we.DY_MAX * we.X_MAX[xmode]) / we.STEP[xmode]
    assert worst < 2 ** 24, worst
    if xmode == 'ln':       # the tile-level order: (sum dy xhat) w + colsum(dy) b, every term on the 0.5 grid
        assert (2 * we.M_MAX * we.DY_MAX * 6.0 * 2.0 + 2 * we.M_MAX * we.DY_MAX * 2.0 + we.W0_MAX) / 0.5 < 2 ** 24


def test_gelu_of_the_chosen_preactivations_is_the_identity():
    """float32 transcription of normal_cdf / gelu_erf (csrc/common.hpp): Phi(u) = 1 - 0.5 poly(t) exp(-u^2 / 2), t = 1 / (1 + p u / sqrt 2)"""
    f = np.float32
    u = np.array([8, 10, 12, 14, 16], dtype=f)
    z = np.abs(u) * f(0.70710678118654752440)
    t = f(1) / (f(0.3275911) * z + f(1))
    poly = t * (f(0.254829592) + t * (f(-0.284496736) + t * (f(1.421413741) + t * (f(-1.453152027) + t * f(1.061405429)))))
    half_tail = f(0.5) * poly * np.exp(-z * z, dtype=f)
    assert half_tail.dtype == f and float(half_tail.max()) < 1e-15            # 2^-25 would already round away
    cdf = f(1) - half_tail
    assert np.array_equal(cdf, np.ones_like(u)) and np.array_equal(u * cdf, u)
    got = set(we.make_x('gelu16', 257, 24, seed=1)['X'].flatten().tolist())
    assert got <= set(u.tolist()) and min(got) >= 8


def test_reference_and_padding():
    dy, o = we.make_dy(300, 8, True, seed=5), we.make_x('rows', 300, 12, seed=5)
    rw, rb = we.reference(dy, o['X'])
    assert torch.equal(rw, (dy.float().long().t() @ o['X'].long()).float()) and torch.equal(rb, dy.float().long().sum(0).float())
    buf, ld = we.padded(o['x'], 8)
    assert ld == 20 and torch.equal(buf[:, :12], o['x']) and bool((buf[:, 12:] == we.PAD_VALUE).all())
    assert _roundtrips(torch.tensor([we.PAD_VALUE]))
