"""Without a GPU: the claims of tests/mlp_exact.py, checked on the generated values of every problem tests/test_mlp_exact_gpu.py uses -- the
pre-activations, the 16-bit representability of every operand and stored row, the fp32 exactness of z, the reduction bounds and their caps,
the fp32-order evaluation of dy, the exits the ragged tile's owner takes through both fragment pipelines, ``gelu_parts2`` on the values that
occur, and that every mutation of the model moves an element that the GPU test compares for equality."""
import numpy as np
import pytest
import torch

import mlp_exact as me

BF16, F16 = torch.bfloat16, torch.float16
CASES = me.cases()
_ids = lambda c: '-'.join(str(v) for v in c)  # noqa: E731


def _both(t):
    return me.representable(t, BF16) and me.representable(t, F16)


def test_cases_cover_the_issue():
    assert len(CASES) == 18 and len(set(CASES)) == 18
    for K, H in me.WIDTHS:
        assert {c[2] for c in CASES if c[:2] == (K, H) and c[3:] == ('plain', None)} == set(me.ROW_COUNTS)
        assert (K, H, 32855, 'masked', None) in CASES
        assert {c[4] for c in CASES if c[:3] == (K, H, 16391)} == {None, 'b1', 'b2', 'gamma'}


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_problem_claims(case):
    K, H, M, kind, drop = case
    p = me.problem(K, H, M, kind)
    r = me.reference(p, drop)
    # operands: exact in both 16-bit formats, never zero where a zero would hide a dropped contribution
    for k in ('y', 'Xn', 'W1', 'W2', 'gamma', 'gamma_bwd', 'dz', 'ln_w', 'ln_b', 'b2'):
        assert p[k].dtype is torch.float32 and _both(p[k]), k
    assert _both(p['dz'] * p['gamma_bwd']) and _both(p['dz'] * p['gamma'])          # the operand the backward rounds: dz gamma
    for k in ('Xn', 'W1', 'W2', 'gamma', 'gamma_bwd'):
        assert bool((p[k] != 0).all()), k
    assert torch.equal(p['b1'], p['b1'].round()) and float(p['b1'].abs().max()) < 2 ** 20       # an fp32 integer, added in fp32
    frac = float((p['dz'] != 0).float().mean())
    assert 0.11 < frac < 0.14 and set(p['dz'].unique().tolist()) == {-2., -1., 0., 1., 2.}
    assert set(p['gamma'].tolist()) <= {0.5, 1., 2.} and set(p['gamma_bwd'].tolist()) == {1., 2.}
    assert bool((p['dgamma0'] != 0).any()) and bool((p['dbeta0'] != 0).any())
    # the caller's statistics: integer mean, rstd in {0.5, 1, 2}, xhat = +-1 exactly in fp32
    st = p['stats']
    assert torch.equal(st[:, 0], st[:, 0].round()) and set(st[:, 1].tolist()) == {0.5, 1., 2.}
    xh = (p['y'] - st[:, :1]) * st[:, 1:]
    assert torch.equal(xh, p['sign']) and set(xh.unique().tolist()) == {-1., 1.}
    assert torch.equal(xh * p['ln_w'] + p['ln_b'], p['Xn'])                        # the backward's recomputed LayerNorm operand, in fp32
    # pre-activations
    u = r['u'].float()
    assert torch.equal(u, u.round()) and r['u_min_abs'] >= 8 and r['u_max'] <= 256 and _both(u)
    if kind == 'plain':
        assert float(u.min()) >= 8 and not bool(r['neg'].any())
        if drop is None:
            assert float(u.min()) == 8
    else:
        assert float(u.abs().min()) >= 43           # exp2(-u^2 / 2 log2 e) underflows to 0 in fp32 from |u| = 15 on
        s_m = torch.sign(p['Xn'][:, p['kstar']:p['kstar'] + 1])
        assert set(p['Xn'][:, p['kstar']].abs().tolist()) == {2.} and torch.equal(torch.sign(u), s_m * p['sigma'])
        assert 0.45 < float(r['neg'].float().mean()) < 0.55
        # a free column's share of + rows depends on how many columns are forced: both signs in quantity is what matters
        assert 0.3 < float((s_m > 0).float().mean()) < 0.7 and 0.4 < float((p['sigma'] > 0).float().mean()) < 0.6
        assert float(p['W1'][:, p['kstar']].abs().min()) == 64 and float(p['W1'].abs().sum(1).max()) == 64 + K - 1
    # stored rows
    du = r['du'].float()
    assert torch.equal(du, du.round()) and float(du.abs().max()) <= 256
    assert bool((du[r['neg']] == 0).all()) and bool((du != 0).any())
    z = r['z']
    assert torch.equal(z * 4, (z * 4).round()) and float(z.abs().max()) < 2 ** 14 and r['dn_max'] < 2 ** 16
    # reductions over M
    for name in ('dgamma', 'dbeta'):
        ok, bound = r[name + '_exact'], r[name + '_bound']
        assert torch.equal(ok, bound < 2 ** 24)
        if kind == 'plain':
            assert bool(ok.all()), (name, float(bound.max()))            # every M: 1.12e7 at most (K = 64, M = 98451), 3.5e6 up to M = 32855
        else:
            miss = (~ok).nonzero().flatten().tolist()
            assert miss in ([], [p['kstar']]), (name, miss)
        assert torch.equal(r[name], r[name].round()) and float(r[name][ok].abs().max()) < 2 ** 24
    # dy: the kernel's fp32 operation order
    if K == 64:
        assert r['dy_emulation_equal'] and r['dy_exact'] == (kind == 'plain')
        assert torch.equal(r['dy64'] * 128, (r['dy64'] * 128).round())
        if kind == 'plain':
            assert float(r['dy64'].abs().max()) < 2 ** 13
    else:
        assert not r['dy_exact']
    assert torch.equal(r['dy'].double(), r['dy64']) or K == 48


def test_reference_is_the_integer_contraction():
    """the float64 model against exact integer arithmetic, masked problem (both signs of u)"""
    K, H, M = 48, 192, 32855
    p = me.problem(K, H, M, 'masked')
    r = me.reference(p)
    L = lambda t: t.double().round().long()  # noqa: E731
    u = L(p['Xn']) @ L(p['W1']).t() + L(p['b1'])
    assert torch.equal(L(r['u'].float()), u)
    t2 = (torch.where(u > 0, u, torch.zeros_like(u)) @ L(p['W2']).t() + L(p['b2'])) * L(p['gamma'] * 2)
    assert torch.equal(L(r['z'] * 2), L(p['y'] * 2) + t2)
    du = (L(p['dz'] * p['gamma_bwd']) @ L(p['W2'])) * (u > 0)
    assert torch.equal(L(r['du'].float()), du)
    dn = du @ L(p['W1'])
    assert torch.equal(L(r['dbeta']), L(p['dbeta0']) + dn.sum(0)) and torch.equal(L(r['dgamma']), L(p['dgamma0']) + (dn * L(p['sign'])).sum(0))
    tn, tmean, trstd = me.ln_true(p['y'], p['ln_w'], p['ln_b'])
    assert torch.equal(r['stats'], torch.cat([tmean, trstd], 1)) and float((tn - p['Xn'].double()).abs().max()) < 2e-4


def _walk(M, first, depth):
    """transcription of the control flow of a wave's fragment pipeline (depth 3: forward, 2: backward) -> (tiles computed, exit taken with
    the ragged tile behind it or None, lap of that exit, the tile whose fragment the ragged compute is given or None)"""
    tiles, nfull, stride = me.geometry(M)
    tile, done, lap = first, [], 0
    frag = [tile + k * stride for k in range(depth - 1)] + [None]          # f0, f1(, f2): the tile each holds
    while True:
        lap += 1
        frag[depth - 1] = tile + (depth - 1) * stride
        if tile >= nfull:
            ex = 1
            break
        done.append((tile, frag[0])); tile += stride
        frag[0] = tile + (depth - 1) * stride
        if tile >= nfull:
            frag[0], ex = frag[1], 2
            break
        done.append((tile, frag[1])); tile += stride
        if depth == 2:
            continue
        frag[1] = tile + 2 * stride
        if tile >= nfull:
            frag[0], ex = frag[2], 3
            break
        done.append((tile, frag[2])); tile += stride
    ragged = tile == nfull and M % 16 != 0
    assert all(t == f for t, f in done)
    return len(done), ex, lap, (frag[0] if ragged else None)


@pytest.mark.parametrize('M,full,fwd_exit,bwd_exit', [(16384, None, (2, 1), (2, 1)), (16391, 0, (1, 1), (1, 1)), (32855, 1, (2, 1), (2, 1)),
                                                       (70001, 2, (3, 1), (1, 2)), (98451, 3, (1, 2), (2, 2))])
def test_row_counts_reach_every_exit(M, full, fwd_exit, bwd_exit):
    """each row count puts the owner of the ragged tile on another exit of the two pipelines (exit, lap), and the fragment that exit
    restores is the ragged tile's"""
    tiles, nfull, stride = me.geometry(M)
    assert me.ragged_owner_full_tiles(M) == full
    owner = nfull % stride if full is not None else 0
    for depth, want in ((3, fwd_exit), (2, bwd_exit)):
        n, ex, lap, held = _walk(M, owner, depth)
        assert (ex, lap) == want and n == (full if full is not None else 1)
        assert held == (nfull if full is not None else None)
        computed = sum(_walk(M, first, depth)[0] + (_walk(M, first, depth)[3] is not None) for first in range(stride))
        assert computed == tiles                                                   # every tile exactly once over the whole grid
    assert max(_walk(M, first, 3)[0] for first in range(0, stride, 97)) >= (4 if M == 98451 else 1)


def test_gelu_parts2_on_the_values_that_occur():
    """float32 transcription of gelu_parts2 (csrc/k_mlp.hip), with a reciprocal a few ulp off: cdf == 1 from u = 8 on; cdf == 0 and the
    exponential == 0 for u <= -43 (the masked problems), so gelu(u) and gelu'(u) are +-0 there -- inside MASK_TOL in any case"""
    f = np.float32
    for scale in (f(1), f(1 + 3e-7), f(1 - 3e-7)):
        for x in (np.arange(8, 257, dtype=f), -np.arange(43, 257, dtype=f)):
            z = np.abs(x) * f(0.70710678118654752440)
            t = (f(1) / (z * f(0.3275911) + f(1))) * scale
            poly = t * (f(0.254829592) + t * (f(-0.284496736) + t * (f(1.421413741) + t * (f(-1.453152027) + t * f(1.061405429)))))
            e = np.exp2((z * z) * f(-1.4426950408889634)).astype(f)
            ht = (f(0.5) * poly) * e
            cdf = np.where(x >= 0, f(1) - ht, ht).astype(f)
            grad = (x * f(0.39894228040143267794)) * e + cdf
            if x[0] > 0:
                assert np.array_equal(cdf, np.ones_like(x)) and np.array_equal(x * cdf, x) and np.array_equal(grad, np.ones_like(x))
            else:
                assert not cdf.any() and not e.any() and not (x * cdf).any() and not grad.any()
    assert 1e-12 * 1e3 <= me.MASK_TOL


def _moved(p, r, m, outputs):
    """does the mutated model m differ from the reference r on an element the GPU test compares for equality by >= 0.5 (or on a masked
    element by more than 1e3 MASK_TOL)?"""
    hit = {}
    for name in outputs:
        ref = r[name].double() if name != 'dy' else r['dy64']
        d = (m[name] - ref).abs()
        if name in ('dgamma', 'dbeta'):
            d = d[r[name + '_exact']]
        hit[name] = float(d.max()) if d.numel() else 0.0
    if p['kind'] == 'masked':
        hit['du_masked'] = float((m['du'] - r['du'].double()).abs()[r['neg']].max())
    return hit


MUT_CASES = [(K, H, 32855, kind, mut) for K, H in me.WIDTHS for kind in ('plain', 'masked') for mut in me.MUTATIONS
             if kind == 'masked' or mut != 'gelu_grad_from_next_row']
MUT_CASES += [(48, 192, M, 'plain', mut) for M in (70001, 98451) for mut in ('ragged_from_previous_fragment', 'tile_twice_next_skipped')]


@pytest.mark.parametrize('case', MUT_CASES, ids=_ids)
def test_every_mutation_moves_an_element_compared_for_equality(case):
    K, H, M, kind, mut = case
    p = me.problem(K, H, M, kind)
    r = me.reference(p)
    m = me.mutate(p, mut)
    outputs = ['z', 'u', 'du', 'dgamma', 'dbeta'] + (['dy'] if r['dy_exact'] else [])
    hit = _moved(p, r, m, outputs)
    fwd, bwd = max(hit['z'], hit['u']), max(hit['du'], hit['dgamma'], hit['dbeta'])
    if mut == 'gelu_grad_from_next_row':
        assert hit['du_masked'] > 1e3 * me.MASK_TOL and hit['du_masked'] >= 0.5 and fwd == 0
    elif mut == 'no_gamma_in_backward':
        assert bwd >= 0.5 and fwd == 0
    elif mut == 'b1_natural_order':
        assert fwd >= 0.5 and hit['u'] >= 0.5        # plain: u stays positive, so the backward cannot see it
    else:
        assert fwd >= 0.5 and bwd >= 0.5, hit


def test_mutations_that_need_a_second_tile_say_so():
    p = me.problem(48, 192, 16391, 'plain')
    for mut in ('ragged_from_previous_fragment', 'tile_twice_next_skipped'):
        with pytest.raises(ValueError):
            me.mutate(p, mut)
    perm = [me.mlp_unit_of_row(R) for R in range(256)]
    assert sorted(perm) == list(range(256)) and perm != list(range(256)) and perm[:8] == [0, 1, 2, 3, 8, 9, 10, 11] and perm[16] == 4
