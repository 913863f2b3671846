"""The training BatchNorm + SiLU kernels of csrc/k_norm.hip on the operands of tests/bn_exact.py: saved statistics, running buffers
(momentum 0.5 / 0.25), the fold of the reduce's copies, dz / dw / db of the apply and of the reduce -> apply chain with a power-of-two count
compared for EQUALITY with the float64 reference; y, momentum 0.1 and the chain with any other count within ``close_fp32``.  The argument is
the docstring of tests/bn_exact.py; tests/test_bn_exact_cpu.py checks it without a GPU.  The kernels ignore the precision mode.

* every forward and apply problem has count = 4 M and runs twice -- ``count`` = the product, and ``count`` = rows per image with
  ``count_dev`` = [images] on the device: bit-identical, and equal to the reference that divides by the product;
* every backward problem also runs with ``dy`` as a channel slice of a wider map whose other columns would wreck a sum;
* the six-member head group (wrappers) mixes members with and without ``count_dev``, strided and contiguous ``dy``, ``dw`` given and None;
  the three-member group (raw entries) has a large member that forces 8 rows per thread on the small one and an EMPTY middle member whose
  sentinel-filled outputs must stay as they are;
* the refused arguments return LEOD_ERR_ARG and write nothing.
``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_kernels_gpu as tk  # noqa: E402
from test_kernels_gpu import ops  # noqa: E402,F401  (fixture)
import bn_exact as bx  # noqa: E402
from mlp_exact import poison  # noqa: E402

F32, F64 = torch.float32, torch.float64
ERR_ARG = -1


def _dev(t):
    return None if t is None else t.to(tk.DEV)


def same(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.double()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: {len(bad)} of {ref.numel()} elements differ, first at {first}: got {got[first].item()}, exact {ref[first].item()}')


def _images(n):
    return torch.tensor([float(n)], dtype=F64, device=tk.DEV)


def _counts(count):
    """the two ways to state one count: (count, None) and (rows per image, [images] on the device)"""
    host, images = bx.split_count(count)
    return ((float(count), None), (float(host), _images(images)))


def _check_fwd(p, y, mean, rstd, rm, rv, what=''):
    r = p['ref']
    same(mean, r['mean'], what + 'save_mean')
    same(rstd, r['rstd'], what + 'save_rstd')
    assert float(rstd[p['neg']]) == float(r['rstd'][(p['v'] == 0).nonzero()[0, 0]]), 'negative variance must clamp to the rstd of variance 0'
    if rm is not None:
        if p['momentum'] in (0.5, 0.25):
            same(rm, r['run_mean'].float(), what + 'run_mean')
            same(rv, r['run_var'].float(), what + 'run_var')
        else:
            bx.close_fp32(rm, r['run_mean'], what=what + 'run_mean')
            bx.close_fp32(rv, r['run_var'], what=what + 'run_var')
    y = y.view(p['M'], p['N']).cpu()
    for name, cols in (('variance 0', p['v'] == 0), ('variance > 0', p['v'] != 0)):
        if bool(cols.any()):
            bx.close_fp32(y[:, cols], r['y'][:, cols], what=f'{what}y, channels of {name}')


def _run_fwd(ops, p, count, cd, with_running=True):
    rm, rv = (_dev(p['rm0'].clone()), _dev(p['rv0'].clone())) if with_running else (None, _dev(p['rv0'].clone()))
    poison(tk.DEV, ((p['M'], p['N']), F32))
    y, mean, rstd = ops.bn_silu_fwd(_dev(p['z']), _dev(p['colstats']), _dev(p['w']), _dev(p['b']), rm, rv, count, eps=bx.EPS,
                                    momentum=p['momentum'], count_dev=cd)
    return y, mean, rstd, rm, rv


@pytest.mark.parametrize('N,M,rep', bx.CASES)
def test_bn_fwd_exact(ops, N, M, rep):
    assert ops.get_precision() == 'f32'
    p = bx.fwd_problem(N, M, rep)
    outs = []
    for count, cd in _counts(p['count']):
        assert count != M or cd is not None
        o = _run_fwd(ops, p, count, cd)
        _check_fwd(p, *o, what='count_dev: ' if cd is not None else '')
        outs.append(o)
    for a, b, name in zip(outs[0], outs[1], ('y', 'save_mean', 'save_rstd', 'run_mean', 'run_var')):
        assert torch.equal(a, b), f'{name}: count = rows x images on the device must be bit-identical to the product on the host'


@pytest.mark.parametrize('momentum', [0.5, 0.25, 0.1])
@pytest.mark.parametrize('count', bx.RUN_COUNTS)
def test_bn_running_buffers(ops, count, momentum):
    N, M = bx.RUN_SHAPE
    p = bx.fwd_problem(N, M, 2, count, momentum)
    for c, cd in _counts(count):
        _check_fwd(p, *_run_fwd(ops, p, c, cd))
    y, mean, rstd, _, rv = _run_fwd(ops, p, float(count), None, with_running=False)
    _check_fwd(p, y, mean, rstd, None, None)
    same(rv, p['rv0'], 'run_var with run_mean = None')


def _strided(dy):
    buf, c0 = bx.wide(dy)
    buf = _dev(buf)
    return buf, buf[:, c0:c0 + dy.shape[1]]


def _check_sums(p, sums, rep, gx):
    got = sums.cpu().view(rep, 2, p['N'])
    fold = got.sum(0)
    for kind in (0, 1, 2):
        same(fold[:, p['kind'] == kind], p['ref']['sums'][:, p['kind'] == kind], f'sums of the channels of kind {kind}')
    live = got.abs().sum((1, 2)) > 0
    reach = min(rep, gx)
    assert bool(live[:reach].all()), f'copies that took no atomics: {(~live[:reach]).nonzero().flatten().tolist()} of {reach}'
    assert not bool(live[reach:].any()), 'a copy no workgroup maps to was written'


@pytest.mark.parametrize('N,M,rep', bx.CASES)
def test_bn_bwd_reduce_exact(ops, N, M, rep):
    p = bx.reduce_problem(N, M)
    z, mean, rstd, w, b = (_dev(p[k]) for k in ('z', 'mean', 'rstd', 'w', 'b'))
    gx = bx.reduce_gx(M, N, bx.reduce_rpt([M], N))
    sums = torch.zeros((rep, 2, N), dtype=F64, device=tk.DEV)
    ops.bn_silu_bwd_reduce(_dev(p['dy']), z, mean, rstd, w, b, out=sums)
    _check_sums(p, sums, rep, gx)
    keep, dy = _strided(p['dy'])
    assert M == 1 or not dy.is_contiguous()
    sums2 = torch.zeros((rep, 2, N), dtype=F64, device=tk.DEV)
    ops.bn_silu_bwd_reduce(dy, z, mean, rstd, w, b, out=sums2)
    _check_sums(p, sums2, rep, gx)


def _run_apply(ops, p, dy, count, cd, with_dw=True):
    dw, db = (_dev(p['dw0'].clone()), _dev(p['db0'].clone())) if with_dw else (None, None)
    poison(tk.DEV, ((p['M'], p['N']), F32))
    dz = ops.bn_silu_bwd_apply(dy, _dev(p['z']), _dev(p['mean']), _dev(p['rstd']), _dev(p['w']), _dev(p['b']), _dev(p['sums']), dw, db, count,
                               count_dev=cd)
    return dz, dw, db


def _check_apply(p, dz, dw, db, what=''):
    r = p['ref']
    same(dz.view(p['M'], p['N']), r['dz'], what + 'dz')
    if dw is not None:
        same(dw, r['dw'], what + 'dw')
        same(db, r['db'], what + 'db')


@pytest.mark.parametrize('N,M,rep', bx.CASES)
def test_bn_bwd_apply_exact(ops, N, M, rep):
    p = bx.apply_problem(N, M, rep)
    dy = _dev(p['dy'])
    outs = []
    for count, cd in _counts(p['count']):
        o = _run_apply(ops, p, dy, count, cd)
        _check_apply(p, *o, what='count_dev: ' if cd is not None else '')
        outs.append(o)
    for a, b, name in zip(outs[0], outs[1], ('dz', 'dw', 'db')):
        assert torch.equal(a, b), f'{name}: count = rows x images on the device must be bit-identical to the product on the host'
    keep, dys = _strided(p['dy'])
    _check_apply(p, *_run_apply(ops, p, dys, float(p['count']), None), what='strided dy: ')
    dz, dw, db = _run_apply(ops, p, dy, float(p['count']), None, with_dw=False)
    assert dw is None and db is None
    _check_apply(p, dz, None, None, what='dw = None: ')


@pytest.mark.parametrize('N,M', bx.SHAPES)
def test_bn_bwd_chain(ops, N, M):
    """reduce -> apply: the sums the reduce leaves (in the replica layout ``ops`` chooses) feed the apply"""
    p = bx.reduce_problem(N, M)
    dy, z, mean, rstd, w, b = (_dev(p[k]) for k in ('dy', 'z', 'mean', 'rstd', 'w', 'b'))
    for count in bx.chain_counts(M):
        sums = ops.bn_silu_bwd_reduce(dy, z, mean, rstd, w, b)
        dw, db = _dev(p['dw0'].clone()), _dev(p['db0'].clone())
        poison(tk.DEV, ((M, N), F32))
        dz = ops.bn_silu_bwd_apply(dy, z, mean, rstd, w, b, sums, dw, db, float(count))
        r = bx.chain_ref(p, float(count))
        if count & (count - 1) == 0:
            same(dz, r['dz'], f'dz, count {count}')
        else:
            bx.close_fp32(dz, r['dz'], what=f'dz, count {count} (the quotients are rounded)')
        same(dw, r['dw'], 'dw')
        same(db, r['db'], 'db')


def test_bn_head_group(ops):
    """the six same-depth layers of the head over three levels in ONE launch each: different grids per member"""
    N, Ms, reps = bx.HEAD_GROUP
    n = len(Ms)
    # forward: even members state their count as rows x images on the device
    ps = [bx.fwd_problem(N, M, rep, None, (0.5, 0.25)[i % 2], i) for i, (M, rep) in enumerate(zip(Ms, reps))]
    rms, rvs = [_dev(p['rm0'].clone()) for p in ps], [_dev(p['rv0'].clone()) for p in ps]
    counts, cds = [], []
    for i, p in enumerate(ps):
        c, cd = _counts(p['count'])[1 - i % 2]
        counts.append(c)
        cds.append(cd)
    assert any(c is None for c in cds) and any(c is not None for c in cds)
    res = ops.bn_silu_fwd_group([_dev(p['z']) for p in ps], [_dev(p['colstats']) for p in ps], [_dev(p['w']) for p in ps], [_dev(p['b']) for p in ps],
                                rms, rvs, counts, bx.EPS, [p['momentum'] for p in ps], count_devs=cds)
    for i, (p, (y, mean, rstd)) in enumerate(zip(ps, res)):
        _check_fwd(p, y, mean, rstd, rms[i], rvs[i], what=f'member {i}: ')
    # reduce: members 0 and 3 read dy in place from a wider map
    qs = [bx.reduce_problem(N, M, i) for i, M in enumerate(Ms)]
    keep = [_strided(q['dy']) if i % 3 == 0 else (None, _dev(q['dy'])) for i, q in enumerate(qs)]
    dys = [k[1] for k in keep]
    assert sum(not d.is_contiguous() for d in dys) == 2
    outs = [torch.zeros((rep, 2, N), dtype=F64, device=tk.DEV) for rep in reps]
    ops.bn_silu_bwd_reduce_group(dys, *[[_dev(q[k]) for q in qs] for k in ('z', 'mean', 'rstd', 'w', 'b')], outs)
    rpt = bx.reduce_rpt(Ms, N)
    for i, q in enumerate(qs):
        _check_sums(q, outs[i], reps[i], bx.reduce_gx(Ms[i], N, rpt))
    # apply: strided members 1 and 4, count_dev on the odd members, no dw / db for the last
    aps = [bx.apply_problem(N, M, rep, None, i) for i, (M, rep) in enumerate(zip(Ms, reps))]
    keep = [_strided(a['dy']) if i % 3 == 1 else (None, _dev(a['dy'])) for i, a in enumerate(aps)]
    dws = [_dev(a['dw0'].clone()) if i < n - 1 else None for i, a in enumerate(aps)]
    dbs = [_dev(a['db0'].clone()) if i < n - 1 else None for i, a in enumerate(aps)]
    counts, cds = zip(*[_counts(a['count'])[i % 2] for i, a in enumerate(aps)])
    dzs = ops.bn_silu_bwd_apply_group([k[1] for k in keep], *[[_dev(a[k]) for a in aps] for k in ('z', 'mean', 'rstd', 'w', 'b', 'sums')],
                                      dws, dbs, list(counts), count_devs=list(cds))
    for i, a in enumerate(aps):
        _check_apply(a, dzs[i], dws[i], dbs[i], what=f'member {i}: ')


def _sentinel(shape, dtype=F32):
    return torch.full(shape, bx.SENTINEL, dtype=dtype, device=tk.DEV)


def _untouched(ts, what):
    for name, t in ts.items():
        assert bool((t == bx.SENTINEL).all()), f'{what}: {name} was written'


def test_bn_forced_group_with_an_empty_member(ops):
    """raw group entries: member 0 forces 8 rows per thread on member 2 (which alone would take 4), member 1 has no rows"""
    N, Ms, reps = bx.FORCED_GROUP
    lib, A, I, st = ops._l(), ops._ptr_array, ops._int_array, ops._stream()
    live = (0, 2)
    # ---- forward
    ps = {k: bx.fwd_problem(N, Ms[k], reps[k], None, 0.25, k) for k in live}
    empty = dict(z=_sentinel((1, N)), colstats=_sentinel((reps[1], 2, N), F64), w=_sentinel((N,)), b=_sentinel((N,)))
    ins = {key: [_dev(ps[k][key]) if k in ps else empty[key] for k in range(3)] for key in ('z', 'colstats', 'w', 'b')}
    y = [torch.full((max(M, 1), N), float('nan'), device=tk.DEV) if k in ps else _sentinel((1, N)) for k, M in enumerate(Ms)]
    mean, rstd = [_sentinel((N,)) for _ in range(3)], [_sentinel((N,)) for _ in range(3)]
    rm = [_dev(ps[k]['rm0'].clone()) if k in ps else _sentinel((N,)) for k in range(3)]
    rv = [_dev(ps[k]['rv0'].clone()) if k in ps else _sentinel((N,)) for k in range(3)]
    cd = [None, None, _images(bx.IMAGES)]
    counts = [float(ps[0]['count']), 1.0, float(Ms[2])]
    rc = lib.leod_bn_silu_fwd_group(3, A(ins['z']), A(ins['colstats']), I(reps), A(ins['w']), A(ins['b']), A(y), A(mean), A(rstd), A(rm), A(rv), I(Ms), N,
                                    ops._f64_array(counts), A(cd), bx.EPS, ops._f32_array([0.25] * 3), st)
    assert rc == 0
    for k in live:
        _check_fwd(ps[k], y[k], mean[k], rstd[k], rm[k], rv[k], what=f'member {k}: ')
    _untouched(dict(y=y[1], save_mean=mean[1], save_rstd=rstd[1], run_mean=rm[1], run_var=rv[1]), 'empty member, forward')
    # ---- reduce: member 2 strided
    qs = {k: bx.reduce_problem(N, Ms[k], k) for k in live}
    wide2, dy2 = _strided(qs[2]['dy'])
    dy = [_dev(qs[0]['dy']), _sentinel((1, N)), dy2]
    lddy = [N, N, wide2.shape[1]]
    vec = {key: [_dev(qs[k][key]) if k in qs else _sentinel((1, N) if key == 'z' else (N,)) for k in range(3)] for key in ('z', 'mean', 'rstd', 'w', 'b')}
    sums = [torch.zeros((reps[k], 2, N), dtype=F64, device=tk.DEV) if k in qs else _sentinel((reps[k], 2, N), F64) for k in range(3)]
    rc = lib.leod_bn_silu_bwd_reduce_group(3, A(dy), A(vec['z']), A(vec['mean']), A(vec['rstd']), A(vec['w']), A(vec['b']), A(sums), I(reps), I(Ms), N,
                                           I(lddy), st)
    assert rc == 0
    rpt = bx.reduce_rpt(Ms, N)
    assert rpt == 8
    for k in live:
        _check_sums(qs[k], sums[k], reps[k], bx.reduce_gx(Ms[k], N, rpt))
    _untouched(dict(sums=sums[1]), 'empty member, reduce')
    # ---- apply: member 2 strided, member 0 with count_dev
    aps = {k: bx.apply_problem(N, Ms[k], reps[k], None, k) for k in live}
    wide2, dy2 = _strided(aps[2]['dy'])
    dy = [_dev(aps[0]['dy']), _sentinel((1, N)), dy2]
    vec = {key: [_dev(aps[k][key]) if k in aps else _sentinel((1, N) if key == 'z' else (N,)) for k in range(3)] for key in ('z', 'mean', 'rstd', 'w', 'b')}
    sums = [_dev(aps[k]['sums']) if k in aps else _sentinel((reps[k], 2, N), F64) for k in range(3)]
    dz = [torch.full((max(M, 1), N), float('nan'), device=tk.DEV) if k in aps else _sentinel((1, N)) for k, M in enumerate(Ms)]
    dw = [_dev(aps[k]['dw0'].clone()) if k in aps else _sentinel((N,)) for k in range(3)]
    db = [_dev(aps[k]['db0'].clone()) if k in aps else _sentinel((N,)) for k in range(3)]
    cd = [_images(bx.IMAGES), None, None]
    counts = [float(Ms[0]), 1.0, float(aps[2]['count'])]
    rc = lib.leod_bn_silu_bwd_apply_group(3, A(dy), A(vec['z']), A(vec['mean']), A(vec['rstd']), A(vec['w']), A(vec['b']), A(sums), I(reps), A(dz), A(dw),
                                          A(db), I(Ms), N, ops._f64_array(counts), A(cd), I(lddy), st)
    assert rc == 0
    for k in live:
        _check_apply(aps[k], dz[k], dw[k], db[k], what=f'member {k}: ')
    _untouched(dict(dz=dz[1], dw=dw[1], db=db[1], sums=sums[1]), 'empty member, apply')


def test_bn_refused_arguments_write_nothing(ops):
    """n = 0, n = 9, N % 4 != 0, N / 4 > 256 (backward), lddy < N, lddy % 4 != 0: LEOD_ERR_ARG before anything is launched.  Every buffer holds
    8 rows of the widest N passed (1028), so a call that were launched after all would stay inside them."""
    N, NBIG, M = 48, 1028, 8
    lib, P, A, I, st = ops._l(), ops._p, ops._ptr_array, ops._int_array, ops._stream()
    f = {k: _sentinel((M, NBIG)) for k in ('z', 'dy', 'w', 'b', 'mean', 'rstd', 'y', 'save_mean', 'save_rstd', 'run_mean', 'run_var', 'dz', 'dw', 'db')}
    cs, sums = _sentinel((2, NBIG), F64), _sentinel((2, NBIG), F64)
    outs = {k: f[k] for k in ('y', 'save_mean', 'save_rstd', 'run_mean', 'run_var', 'dz', 'dw', 'db')}
    outs.update(colstats=cs, sums=sums)

    def fwd_group(n):
        r = [1] * max(n, 1)
        return lib.leod_bn_silu_fwd_group(n, *[A([f[k]] * len(r)) for k in ('z',)], A([cs] * len(r)), I(r), *[A([f[k]] * len(r)) for k in
                                          ('w', 'b', 'y', 'save_mean', 'save_rstd', 'run_mean', 'run_var')], I([M] * len(r)), N,
                                          ops._f64_array([float(M)] * len(r)), None, bx.EPS, ops._f32_array([0.5] * len(r)), st)

    def reduce_group(n):
        r = [1] * max(n, 1)
        return lib.leod_bn_silu_bwd_reduce_group(n, *[A([f[k]] * len(r)) for k in ('dy', 'z', 'mean', 'rstd', 'w', 'b')], A([sums] * len(r)), I(r),
                                                 I([M] * len(r)), N, None, st)

    def apply_group(n):
        r = [1] * max(n, 1)
        return lib.leod_bn_silu_bwd_apply_group(n, *[A([f[k]] * len(r)) for k in ('dy', 'z', 'mean', 'rstd', 'w', 'b')], A([sums] * len(r)), I(r),
                                                *[A([f[k]] * len(r)) for k in ('dz', 'dw', 'db')], I([M] * len(r)), N,
                                                ops._f64_array([float(M)] * len(r)), None, None, st)

    def fwd(n_ch):
        return lib.leod_bn_silu_fwd(P(f['z']), P(cs), 1, P(f['w']), P(f['b']), P(f['y']), P(f['save_mean']), P(f['save_rstd']), P(f['run_mean']),
                                    P(f['run_var']), M, n_ch, float(M), None, bx.EPS, 0.5, st)

    def reduce(n_ch, lddy):
        return lib.leod_bn_silu_bwd_reduce(*[P(f[k]) for k in ('dy', 'z', 'mean', 'rstd', 'w', 'b')], P(sums), 1, M, n_ch, lddy, st)

    def apply(n_ch, lddy):
        return lib.leod_bn_silu_bwd_apply(*[P(f[k]) for k in ('dy', 'z', 'mean', 'rstd', 'w', 'b')], P(sums), 1, P(f['dz']), P(f['dw']), P(f['db']), M, n_ch,
                                          float(M), None, lddy, st)

    calls = {'fwd_group n = 0': lambda: fwd_group(0), 'fwd_group n = 9': lambda: fwd_group(9), 'fwd N = 6': lambda: fwd(6),
             'reduce_group n = 0': lambda: reduce_group(0), 'reduce_group n = 9': lambda: reduce_group(9),
             'apply_group n = 0': lambda: apply_group(0), 'apply_group n = 9': lambda: apply_group(9)}
    for name, fn in (('reduce', reduce), ('apply', apply)):
        calls.update({f'{name} N = 6': lambda fn=fn: fn(6, 0), f'{name} N / 4 > 256': lambda fn=fn: fn(NBIG, 0),
                      f'{name} lddy < N': lambda fn=fn: fn(N, N - 4), f'{name} lddy % 4 != 0': lambda fn=fn: fn(N, N + 2)})
    assert NBIG % 4 == 0 and NBIG // 4 > 256
    for what, call in calls.items():
        assert call() == ERR_ARG, what
    torch.cuda.synchronize()
    _untouched(outs, 'refused call')
    # the same calls with arguments in range are taken (the refusals above are not a side effect of the buffers)
    assert fwd_group(1) == 0 and reduce(N, 0) == 0 and apply(N, N + 4) == 0
    torch.cuda.synchronize()
