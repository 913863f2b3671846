"""Without a GPU: the claims of tests/rownorm_exact.py on the generated values of every problem tests/test_rownorm_exact_gpu.py uses -- the
value sets, xhat = +-1 with the caller's statistics, integer reductions below 2^24, the fp32-order evaluation of dx where C is a power of
two, the grid-stride passes and CJ instantiations the shapes reach."""
import pytest
import torch

import rownorm_exact as rx


def _halves(t, bits=3):
    return torch.equal(t * 2, (t * 2).round()) and float(t.abs().max()) <= 2 ** bits


@pytest.mark.parametrize('with_dres', [True, False], ids=['dres', 'nodres'])
@pytest.mark.parametrize('M,C', rx.LN_BWD_SHAPES)
def test_layernorm_bwd_problem(M, C, with_dres):
    p = rx.ln_bwd_problem(M, C, with_dres)
    assert set(p['dn'].unique().tolist()) <= {-3., -2., -1., 1., 2., 3.} and set(p['w'].abs().tolist()) <= {0.5, 1., 2.}
    assert (p['dres'] is not None) == with_dres and (not with_dres or (_halves(p['dres']) and bool((p['dres'] != 0).any())))
    st = p['stats']
    xh = (p['x'] - st[:, :1]) * st[:, 1:]
    assert set(xh.unique().tolist()) == {-1., 1.} and bool(((xh > 0).sum(1) == C // 2).all())
    assert torch.equal(st[:, 0], st[:, 0].round()) and set(st[:, 1].tolist()) <= {0.5, 1., 2.}
    assert p['reduction_bound'] < 2 ** 24
    for k in ('dw', 'db'):
        assert torch.equal(p['ref'][k], p['ref'][k].round()) and bool((p[k + '0'] != 0).any())
        assert float((p['true'][k] - p['ref'][k]).abs().max()) <= 1e-4 * p['reduction_bound']
    assert torch.equal(p['ref']['db'].long(), p['db0'].long() + p['dn'].long().sum(0))
    assert torch.equal(p['ref']['dw'].long(), p['dw0'].long() + (p['dn'] * xh).long().sum(0))
    pow2 = C & (C - 1) == 0
    assert p['dx_exact'] == pow2
    if pow2:
        dx = p['ref']['dx']
        assert torch.equal(dx * 2 ** 11, (dx * 2 ** 11).round()) and float(dx.abs().max()) < 2 ** 6
        assert torch.equal(dx.float().double(), dx)
    assert float((p['true']['dx'] - p['ref']['dx']).abs().max()) < 1e-3           # eps moves rstd by 1e-5 at most


def test_layernorm_bwd_dx_is_the_rational_formula():
    """C dx / rstd = C g - sum g - xhat sum(g xhat) in exact integer arithmetic (g in halves)"""
    p = rx.ln_bwd_problem(20, 512, True)
    C = 512
    xh = ((p['x'] - p['stats'][:, :1]) * p['stats'][:, 1:]).long()
    g2 = (p['dn'] * p['w'] * 2).long()
    lhs = ((p['ref']['dx'] - p['dres'].double()) / p['stats'][:, 1:].double() * 2 * C).round().long()
    assert torch.equal(lhs, C * g2 - g2.sum(1, keepdim=True) - xh * (g2 * xh).sum(1, keepdim=True))


@pytest.mark.parametrize('M,C', rx.LN_BWD_SHAPES)
def test_layerscale_bwd_problem(M, C):
    p = rx.ls_bwd_problem(M, C)
    for k in ('dz', 't'):
        assert set(p[k].unique().tolist()) <= {-3., -2., -1., 1., 2., 3.}
    assert set(p['gamma'].abs().tolist()) <= {0.5, 1., 2.} and p['reduction_bound'] < 2 ** 24
    assert torch.equal(p['ref']['dt'], p['dz'] * p['gamma'])
    assert torch.equal(p['ref']['dgamma'].long(), p['dgamma0'].long() + (p['dz'].long() * p['t'].long()).sum(0))
    assert bool((p['dgamma0'] != 0).any())


@pytest.mark.parametrize('M,C', rx.LN_FWD_SHAPES)
def test_layernorm_fwd_problem(M, C):
    p = rx.ln_fwd_problem(M, C)
    y = p['ref']['y']
    assert float((y - p['Xn'].double()).abs().max()) < 2e-4 and bool((p['Xn'] != 0).all()) and float(p['Xn'].abs().min()) >= 1
    assert torch.equal(p['ref']['stats'][:, 0], p['mean'].double().flatten())
    assert float((p['ref']['stats'][:, 1] - 1 / p['c'].double().flatten()).abs().max()) < 5e-5
    if M > 8:                                                   # neighbouring rows differ in their statistics and their sign pattern
        same = (p['x'][1:] == p['x'][:-1]).all(1)
        assert not bool(same.any())
        assert float((p['Xn'][1:] - p['Xn'][:-1]).abs().max(1).values.min()) >= 1


@pytest.mark.parametrize('N,K', rx.FINALIZE_SHAPES)
def test_finalize_problem(N, K):
    p = rx.finalize_problem(N, K)
    assert set(p['W'].abs().unique().tolist()) == {1., 2.} and set(p['G'].abs().unique().tolist()) == {1., 2.}
    assert set(p['gamma'].abs().tolist()) <= {0.5, 1., 2.} and K % 4 == 0
    for k in ('dW', 'db', 'dgamma', 'dgamma_nob'):
        assert _halves(p['ref'][k], 14)
    assert 4.0 * K + 9 + 3 < 2 ** 24                            # worst case of the dot product and the bias term
    assert torch.equal((p['ref']['dgamma'] - p['dgamma0'].double()).long(), (p['W'].long() * p['G'].long()).sum(1) + p['b'].long() * p['s'].long())
    assert bool((p['dW0'] != 0).any()) and bool((p['db0'] != 0).any()) and bool((p['dgamma0'] != 0).any())
    assert not torch.equal(p['ref']['dgamma'], p['ref']['dgamma_nob']) or N < 8


def test_shapes_reach_what_they_are_there_for():
    assert {rx.cj_of(C) for _, C in rx.LN_BWD_SHAPES} == {2, 3, 4, 6, 8} and rx.cj_of(320) == 6 and rx.cj_of(448) == 8 and rx.cj_of(512) == 8
    assert {rx.cj_of(C) for _, C in rx.LN_FWD_SHAPES} == {1, 2, 3, 6, 8}
    assert rx.passes(8192, 512) == (1, 1) and rx.passes(8211, 512) == (1, 2) and rx.passes(16391, 512) == (2, 3)
    assert rx.passes(32768, 2048) == (1, 1) and rx.passes(32851, 2048) == (1, 2) and rx.passes(3, 512) == (0, 1)
    assert 8211 % 4 == 3 and 16391 % 4 == 3 and 32851 % 4 == 3                   # the last row group is ragged
    # K below, equal to, above and not a multiple of one 256-element wave pass; N not a multiple of the 4 waves of a workgroup
    ks = {K for _, K in rx.FINALIZE_SHAPES}
    assert min(ks) < 256 and 260 in ks and any(K % 256 == 0 and K > 256 for K in ks) and any(K > 256 and K % 256 for K in ks)
    assert any(N % 4 for N, _ in rx.FINALIZE_SHAPES)
