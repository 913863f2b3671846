"""Without a GPU: the claims of tests/bn_exact.py on the generated values of every problem tests/test_bn_exact_gpu.py uses -- the value
sets, the exact folds, the fp32-order evaluation wherever equality is claimed, the branches the shapes reach (from the launch model, no
threshold is written down here) -- and that the references can tell a wrong kernel from a right one: ``mirror_*`` are NumPy mirrors of the
index arithmetic of the three kernels of csrc/k_norm.hip; the right mirror equals the reference, each seeded defect differs from it."""
import numpy as np
import pytest
import torch

import bn_exact as bx

F = np.float32


# ---- NumPy mirrors of the kernels ------------------------------------------------------------------------------------------------------
def _fold(copies, defect):
    if defect == 'copy0':
        return copies[0].copy()
    acc = np.zeros_like(copies[0])
    for r in range(copies.shape[0]):                     # the kernel's order, in double
        acc = acc + copies[r]
    return acc


def _first_pass_only(out, M, N):
    """what a kernel without the grid-stride loop leaves unwritten"""
    flat = out.reshape(-1)
    flat[bx.flat_gx(M, N) * 256 * 4:] = np.nan
    return out


def _silu_grad32(u):
    with np.errstate(over='ignore'):
        s = F(1) / (F(1) + np.exp2(-u * F(1.4426950408889634)))
    return s * (F(1) + u * (F(1) - s))


def mirror_fwd(p, defect=None):
    N, M = p['N'], p['M']
    S = _fold(p['colstats'].numpy(), defect)
    count = float(M if defect == 'div_M' else p['count'])
    mean = S[0] / count
    var = np.maximum(S[1] / count - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + np.float64(F(bx.EPS)))).astype(F)
    mean32 = mean.astype(F)
    unb = (var * count / (count - 1.0) if count > 1.0 else var).astype(F)
    mom = F(p['momentum'])
    out = dict(mean=mean32, rstd=rstd, run_mean=(F(1) - mom) * p['rm0'].numpy() + mom * mean32, run_var=(F(1) - mom) * p['rv0'].numpy() + mom * unb)
    u = ((p['z'].numpy() - mean32) * rstd * p['w'].numpy() + p['b'].numpy()).astype(np.float64)
    with np.errstate(over='ignore'):
        y = u / (1.0 + np.exp(-u))
    out['y'] = _first_pass_only(y, M, N) if defect == 'one_pass' else y
    return out


def mirror_reduce(p, rep, rpt=None, dy_buf=None, c0=0, defect=None):
    """-> sums [rep, 2, N] float64.  dy_buf: the (wider) map dy is a slice of"""
    N, M = p['N'], p['M']
    dy_buf = p['dy'].numpy() if dy_buf is None else dy_buf
    lddy = N if defect == 'ignore_lddy' else dy_buf.shape[1]
    dy_flat = dy_buf.reshape(-1)[c0:]
    rs = bx.rstep(N)
    rpt = bx.reduce_rpt([M], N) if rpt is None else rpt
    gx = M // (rs * rpt) if defect == 'floor_gx' else bx.reduce_gx(M, N, rpt)
    z, mean, rstd, w, b = (p[k].numpy() for k in ('z', 'mean', 'rstd', 'w', 'b'))
    sums = np.zeros((rep, 2, N))
    cols = np.arange(N)
    for blk in range(gx):
        rows = blk * rs * rpt + np.arange(rs)[:, None] + np.arange(rpt)[None, :] * rs           # [row lane, e]
        ok = np.ones_like(rows, dtype=bool) if defect == 'tail_counted' else rows < M
        rc = np.minimum(rows, M - 1)
        xh = (z[rc] - mean) * rstd                                                               # [row lane, e, N]
        dv = dy_flat[rc[..., None] * lddy + cols]
        du = np.where(ok[..., None], dv * _silu_grad32(xh * w + b), F(0)).astype(F)
        s0, s1 = du.sum(1, dtype=F), (du * xh).sum(1, dtype=F)                                   # per thread, fp32
        sums[blk % rep, 0] += s0.astype(np.float64).sum(0)
        sums[blk % rep, 1] += s1.astype(np.float64).sum(0)
    return sums


def mirror_apply(p, sums, count, dy_buf=None, c0=0, defect=None):
    N, M = p['N'], p['M']
    dy_buf = p['dy'].numpy() if dy_buf is None else dy_buf
    lddy = N if defect == 'ignore_lddy' else dy_buf.shape[1]
    dy = dy_buf.reshape(-1)[c0:][np.arange(M)[:, None] * lddy + np.arange(N)]
    S = _fold(np.asarray(sums), defect)
    count = float(M if defect == 'div_M' else count)
    m0, m1 = (S[0] / count).astype(F), (S[1] / count).astype(F)
    z, mean, rstd, w, b = (p[k].numpy() for k in ('z', 'mean', 'rstd', 'w', 'b'))
    xh = (z - mean) * rstd
    du = dy * _silu_grad32(xh * w + b)
    dz = ((w * rstd) * (du - m0 - xh * m1)).astype(F)
    if defect == 'one_pass':
        dz = _first_pass_only(dz, M, N)
    return dict(dz=dz, dw=p['dw0'].numpy() + S[1].astype(F), db=p['db0'].numpy() + S[0].astype(F))


def _eq(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


# ---- the shapes reach their branches -------------------------------------------------------------------------------------------------------
def test_shapes_reach_what_they_are_there_for():
    rpt = {s: bx.reduce_rpt([s[1]], s[0]) for s in bx.SHAPES}
    second = {s: bx.flat_passes(s[1], s[0])[1] > 1 for s in bx.SHAPES}
    for N, M in ((256, 4099), (96, 10931), (1024, 1031)):
        # 8 rows per thread and a second grid-stride pass, both by the smallest margin that leaves a ragged tail
        assert rpt[(N, M)] == 8 and second[(N, M)]
        rs = bx.rstep(N)
        first8 = next(m for m in range(1, M + 1) if bx.reduce_rpt([m], N) == 8)
        first2 = next(m for m in range(1, M + 1) if bx.flat_passes(m, N)[1] > 1)
        assert first8 <= first2 <= M < first2 + rs * 8, (first8, first2)
        assert M % (rs * 8) != 0                                             # the last workgroup clamps rows
        assert bx.flat_passes(M, N)[0] == 1                                  # ... and only some threads take the second pass
    assert 4099 % (bx.rstep(256) * 8) == 3                                   # a tail of 3 rows
    assert (bx.rstep(96), bx.idle_lanes(96)) == (10, 16) and bx.rstep(1024) == 1 and bx.idle_lanes(1024) == 0
    assert (bx.rstep(48), bx.idle_lanes(48), rpt[(48, 77)]) == (21, 4, 4)
    assert (bx.rstep(20), bx.idle_lanes(20), rpt[(20, 103)]) == (51, 1, 4)
    assert (bx.rstep(4), bx.idle_lanes(4), rpt[(4, 300)]) == (256, 0, 4) and 4 // 4 == 1
    for M in (1, 3):
        assert M < bx.rstep(256) and rpt[(256, M)] == 4 and bx.reduce_gx(M, 256, 4) == 1
    reps = {r for _, _, r in bx.CASES}
    assert reps == {1, 2, 16, 32} and {(n, m) for n, m, _ in bx.CASES} == set(bx.SHAPES)
    # replica counts above and below the workgroup count of the reduce
    gxs = [(bx.reduce_gx(M, N, rpt[(N, M)]), r) for N, M, r in bx.CASES]
    assert any(r > gx for gx, r in gxs) and any(1 < r < gx for gx, r in gxs)
    # the groups
    N, Ms, _ = bx.HEAD_GROUP
    assert bx.reduce_rpt(Ms, N) == 4 and len({bx.reduce_gx(M, N, 4) for M in Ms}) == 3 and len({bx.flat_gx(M, N) for M in Ms}) == 3
    N, Ms, _ = bx.FORCED_GROUP
    assert bx.reduce_rpt(Ms, N) == 8 and bx.reduce_rpt([Ms[2]], N) == 4 and Ms[1] == 0 and bx.reduce_gx(0, N, 8) == 0 and bx.flat_gx(0, N) == 0
    assert bx.reduce_gx(Ms[2], N, 8) == 2 and Ms[2] % (bx.rstep(N) * 8) != 0
    for c in bx.RUN_COUNTS + tuple(bx.IMAGES * M for _, M in bx.SHAPES):
        host, images = bx.split_count(c)
        assert host * images == c
    assert set(bx.RUN_COUNTS) == {1, 64, 65} and bx.RUN_SHAPE[1] not in bx.RUN_COUNTS


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,M,rep', bx.CASES)
def test_fwd_problem(N, M, rep):
    p = bx.fwd_problem(N, M, rep)
    r, cs, count = p['ref'], p['colstats'], p['count']
    assert count == bx.IMAGES * M != M
    assert set(p['v'].tolist()) <= {0., 0.25, 1., 4.} and float(p['m'].abs().max()) <= 3 and bool((p['m'] != 0).any())
    # the fold is exact in every order, and lost in fp32 or without a copy
    want = torch.cat([count * p['m'].double(), count * (p['v'].double() + p['m'].double() ** 2)]).view(2, N).clone()
    want[1, p['neg']] -= count / 16.0
    for order in (range(rep), reversed(range(rep))):
        acc = torch.zeros(2, N, dtype=torch.float64)
        for k in order:
            acc = acc + cs[k]
            assert torch.equal(acc * 16, (acc * 16).round()) and float(acc.abs().max()) < 2.0 ** 48
        assert torch.equal(acc, want)
    if rep > 1:
        assert float(cs.abs().min()) >= bx.NOISE / 2                        # every copy is large
        assert not torch.equal(cs.float().sum(0).double(), want)
    # exact statistics: mean = m, var = v, the lowered channel clamps to the rstd of v = 0
    assert torch.equal(r['mean'], p['m']) and torch.equal(r['var'], p['v'].double())
    S = cs.sum(0)
    assert float((S[1] / count - (S[0] / count) ** 2)[p['neg']]) == -1.0 / 16
    zero = (p['v'] == 0).nonzero().flatten()
    assert len(zero) >= 1 and bool((r['rstd'][zero] == r['rstd'][p['neg']]).all()) and abs(float(r['rstd'][p['neg']]) - 1e-5 ** -0.5) < 0.01
    # z: neighbouring rows and channels differ by >= 0.5; a wrong row shows in y
    z = p['z']
    if M > 1:
        assert float((z[1:] - z[:-1]).abs().max(1).values.min()) >= 0.5
        assert N < 20 or float((r['y'][1:] - r['y'][:-1]).abs().max(1).values.min()) >= 0.01       # 100 x the bound of close_fp32
    assert float((z[:, 1:] - z[:, :-1]).abs().max(0).values.min()) >= 0.5 or M < 4
    # the mirror equals the reference; the seeded defects do not
    m = mirror_fwd(p)
    assert _eq(m['mean'], r['mean']) and _eq(m['rstd'], r['rstd'])
    bx.close_fp32(torch.from_numpy(m['y']), r['y'])
    if rep > 1:
        d = mirror_fwd(p, 'copy0')
        assert not _eq(d['mean'], r['mean']) and not _eq(d['rstd'], r['rstd'])
    d = mirror_fwd(p, 'div_M')
    assert not _eq(d['mean'], r['mean']) and not _eq(d['rstd'], r['rstd'])
    if bx.flat_passes(M, N)[1] > 1:
        assert not np.allclose(mirror_fwd(p, 'one_pass')['y'], r['y'].numpy(), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize('momentum', [0.5, 0.25, 0.1])
@pytest.mark.parametrize('count', bx.RUN_COUNTS)
def test_running_buffers_problem(count, momentum):
    N, M = bx.RUN_SHAPE
    p = bx.fwd_problem(N, M, 2, count, momentum)
    r = p['ref']
    for k in ('rm0', 'rv0'):
        assert torch.equal(p[k], p[k].round()) and bool((p[k] != 0).any()) and float(p['rv0'].min()) >= 0
    m = mirror_fwd(p)
    if momentum in (0.5, 0.25):
        # the float64 sum is exact, so its rounding to fp32 is the one rounding the kernel makes, with or without fma contraction
        for k in ('run_mean', 'run_var'):
            assert _eq(m[k], r[k].float())
        rm = r['run_mean']
        assert torch.equal(rm * 4, (rm * 4).round())
        f = np.float32
        unb = (r['var'] * count / (count - 1.0) if count > 1 else r['var']).float().numpy()
        fused = (np.float64(f(1) - f(momentum)) * p['rv0'].numpy().astype(np.float64) + np.float64(f(momentum)) * unb.astype(np.float64)).astype(f)
        assert _eq(fused, r['run_var'].float()) and _eq(m['run_var'], fused)
    else:
        bx.close_fp32(torch.from_numpy(m['run_var']), r['run_var'])
    var = r['var']
    unb = var * count / (count - 1.0) if count > 1 else var
    assert (count == 1) == torch.equal(unb, var) and (count == 65) == (torch.equal(unb.float().double(), unb) and count > 1)
    assert not _eq(mirror_fwd(p, 'div_M')['run_var'], r['run_var'].float())


# ---- reduce --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,M', bx.SHAPES)
def test_reduce_problem(N, M):
    p = bx.reduce_problem(N, M)
    kind = p['kind']
    for c0 in range(0, N, 4):
        assert set(kind[c0:c0 + 4].tolist()) == {0, 1, 2}
    xh = (p['z'] - p['mean']) * p['rstd']
    assert torch.equal(xh, p['k']) and set(p['k'].unique().tolist()) <= {-2., -1., 1., 2.} and set(p['dy'].unique().tolist()) <= {-3., -2., -1., 1., 2., 3.}
    u = xh * p['w'] + p['b']
    assert bool((u[:, kind == 0] == 0).all()) and float(u[:, kind == 1].min()) >= 60 and bool((u[:, kind == 2] == -128).all())
    assert _eq(_silu_grad32(u.numpy()), np.broadcast_to(p['grad'].numpy(), u.shape))             # 0.5, 1 and -0 exactly, in fp32
    s = p['ref']['sums']
    assert torch.equal(s * 2, (s * 2).round()) and float(s.abs().max()) * 2 < 2 ** 53 and p['thread_bound'] < 2 ** 24
    assert bool((s[:, kind == 2] == 0).all()) and bool((s[:, kind != 2] != 0).any())
    for rep in sorted({r for n, m, r in bx.CASES if (n, m) == (N, M)}):
        got = mirror_reduce(p, rep)
        assert _eq(got.sum(0), s)
        gx = bx.reduce_gx(M, N, bx.reduce_rpt([M], N))
        live = np.abs(got).sum((1, 2)) > 0
        assert live[:min(rep, gx)].all() and not live[min(rep, gx):].any()
        assert not _eq(got[0], s) or min(rep, gx) == 1                                           # folding copy 0 only
    rs = bx.rstep(N)
    per = rs * bx.reduce_rpt([M], N)
    assert M % per != 0
    assert not _eq(mirror_reduce(p, 1, defect='tail_counted').sum(0), s)
    assert not _eq(mirror_reduce(p, 1, defect='floor_gx').sum(0), s)
    assert _eq(mirror_reduce(p, 2, rpt=8).sum(0), s)                                            # 8 rows per thread forced by a group
    buf, c0 = bx.wide(p['dy'])
    assert c0 % 4 == 0 and buf.shape[1] % 4 == 0 and buf.shape[1] > N
    assert _eq(mirror_reduce(p, 1, dy_buf=buf.numpy(), c0=c0).sum(0), s)
    if M > 1:
        assert not _eq(mirror_reduce(p, 1, dy_buf=buf.numpy(), c0=c0, defect='ignore_lddy').sum(0), s)


# ---- apply and the chain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,M,rep', bx.CASES)
def test_apply_problem(N, M, rep):
    p = bx.apply_problem(N, M, rep)
    r, count = p['ref'], p['count']
    assert count == bx.IMAGES * M
    for k in ('a', 'bq'):
        assert torch.equal(p[k] * 8, (p[k] * 8).round()) and float(p[k].abs().max()) <= 2 and bool((p[k] != 0).any())
    assert torch.equal((p['z'] - p['mean']) * p['rstd'], p['k']) and float((p['k'] * p['w'] + p['b']).min()) >= 60
    assert torch.equal(r['dz'] * 32, (r['dz'] * 32).round()) and float(r['dz'].abs().max()) < 2 ** 6
    for k in ('dw', 'db'):
        assert torch.equal(r[k] * 8, (r[k] * 8).round()) and float(r[k].abs().max()) < 2 ** 18 and torch.equal(r[k].float().double(), r[k])
        assert bool((p[k + '0'] != 0).any())
    m = mirror_apply(p, p['sums'].numpy(), count)
    for k in ('dz', 'dw', 'db'):
        assert _eq(m[k], r[k]), k
    defects = ['div_M'] + (['copy0'] if rep > 1 else []) + (['one_pass'] if bx.flat_passes(M, N)[1] > 1 else [])
    for d in defects:
        m = mirror_apply(p, p['sums'].numpy(), count, defect=d)
        assert not _eq(m['dz'], r['dz']), d
        if d == 'copy0':
            assert not _eq(m['dw'], r['dw']) and not _eq(m['db'], r['db'])
    buf, c0 = bx.wide(p['dy'])
    assert _eq(mirror_apply(p, p['sums'].numpy(), count, dy_buf=buf.numpy(), c0=c0)['dz'], r['dz'])
    if M > 1:
        assert not _eq(mirror_apply(p, p['sums'].numpy(), count, dy_buf=buf.numpy(), c0=c0, defect='ignore_lddy')['dz'], r['dz'])


@pytest.mark.parametrize('N,M', bx.SHAPES)
def test_chain_problem(N, M):
    p = bx.reduce_problem(N, M)
    for count in bx.chain_counts(M):
        r = bx.chain_ref(p, float(count))
        got = bx.chain_fp32(p, float(count))
        if count & (count - 1) == 0:
            assert count != M and torch.equal(got.double(), r['dz'])
            m = mirror_apply(p, p['ref']['sums'].numpy()[None], count)
            assert _eq(m['dz'], r['dz'])
        else:
            bx.close_fp32(got, r['dz'])
        assert torch.equal(r['dw'].float().double(), r['dw']) and torch.equal(r['db'].float().double(), r['db'])
        d = mirror_apply(p, p['ref']['sums'].numpy()[None], count, defect='div_M')
        assert not np.allclose(d['dz'], r['dz'].numpy(), rtol=1e-3, atol=1e-3)
