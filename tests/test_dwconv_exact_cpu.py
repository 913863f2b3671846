"""Without a GPU: the claims of tests/dwconv_exact.py on the generated values of every problem tests/test_dwconv_exact_gpu.py uses -- the
value sets, the bounds, references representable in fp32, ``dw_ref`` against ``F.conv2d(groups = C)`` and its autograd, the branches the
shapes reach (from the launch model) -- and that the references can tell a wrong kernel from a right one: ``mirror_*`` are NumPy mirrors of
the index arithmetic of the kernels of csrc/k_dwconv.hip in fp32; the right mirror equals the reference, each seeded defect differs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dwconv_exact as dx

F32 = np.float32


def _p(shape):
    return dx.problem(*shape)


def _ids(shape):
    return 'x'.join(str(v) for v in shape)


# ---- NumPy mirrors -------------------------------------------------------------------------------------------------------------------------
def _taps(n, no, ks, stride, pad, k):
    """output positions o < no whose tap k lies inside the map, and the input positions they read"""
    o = np.arange(no)
    i = o * stride - pad + k
    ok = (i >= 0) & (i < n)
    return o[ok], i[ok]


def mirror_fwd(p, bias=True, rep=1, defect=None):
    """-> y [B,Ho,Wo,C] fp32 (NaN where never written) and the statistics copies [rep,2,C] float64"""
    B, H, W, C, ks, s, pad, Ho, Wo = (p[k] for k in ('B', 'H', 'W', 'C', 'ks', 'stride', 'pad', 'Ho', 'Wo'))
    x, w = p['x'].numpy(), p['w'].numpy()
    y = np.zeros((B, Ho, Wo, C), dtype=F32) + (p['bias'].numpy() if bias else F32(0))
    for ky in range(ks):
        ho, hi = _taps(H, Ho, ks, s, pad, ky)
        for kx in range(ks):
            wo, wi = _taps(W, Wo, ks, s, pad, kx)
            y[:, ho[:, None], wo[None, :]] += w[:, 0, ky, kx] * x[:, hi[:, None], wi[None, :]]
    C4, items = C // 4, dx.fwd_items(p)
    grid = dx.flat_grid(items)
    done = min(items, grid * 256) if defect == 'one_pass' else items
    it = np.arange(done)
    yi = y.reshape(-1, 4)[:done]
    key = (it // 256) % grid * C4 + it % C4
    lds = np.zeros((2, grid * C4, 4), dtype=F32)                 # the workgroups' fp32 partials
    np.add.at(lds[0], key, yi)
    np.add.at(lds[1], key, yi * yi)
    lds = lds.reshape(2, grid, C)
    stats = np.zeros((rep, 2, C))
    for blk in range(grid):
        stats[blk & (rep - 1)] += lds[:, blk].astype(np.float64)
    y.reshape(-1, 4)[done:] = np.nan
    return y, stats


def mirror_dgrad(p, start=None, defect=None):
    B, H, W, C, ks, s, pad, Ho, Wo = (p[k] for k in ('B', 'H', 'W', 'C', 'ks', 'stride', 'pad', 'Ho', 'Wo'))
    dy, w = p['dy'].numpy(), p['w'].numpy()
    acc = np.zeros((B, H, W, C), dtype=F32) if start is None else start.astype(F32).copy()
    for ky in range(ks):
        hn = np.arange(H) + pad - ky
        hok = (hn >= 0) & (hn % s == 0) & (hn // s < Ho)
        for kx in range(ks):
            wn = np.arange(W) + pad - kx
            wok = (wn >= 0) & (wn % s == 0) & (wn // s < Wo)
            hi, wi = np.nonzero(hok)[0], np.nonzero(wok)[0]
            acc[:, hi[:, None], wi[None, :]] += w[:, 0, ky, kx] * dy[:, (hn[hi] // s)[:, None], (wn[wi] // s)[None, :]]
    if defect == 'one_pass':
        items = dx.dgrad_items(p)
        left = np.full((B, H, W, C), np.nan, dtype=F32) if start is None else start.astype(F32).copy()
        acc.reshape(-1, 4)[dx.flat_grid(items) * 256:] = left.reshape(-1, 4)[dx.flat_grid(items) * 256:]
    return acc


def mirror_wgrad(p, dw_buf, db_buf, defect=None):
    """one call of the wgrad on the guarded flat buffers (updated in place, fp32).  Lane c of tile z works on channel z * 256 + c whether
    or not the map has it when ``live`` is ignored: it then reads the flat arrays where that channel would lie"""
    B, H, W, C, ks, s, pad, Ho, Wo = (p[k] for k in ('B', 'H', 'W', 'C', 'ks', 'stride', 'pad', 'Ho', 'Wo'))
    gx, tiles, per, _ = dx.wgrad_grid(p)
    assert gx * per >= B * Ho * Wo
    Ct = tiles * 256 if defect == 'ignore_live' else C

    def lanes(t, rows):
        flat = np.concatenate([t.numpy().reshape(-1), np.zeros(Ct, dtype=F32)])
        return flat[np.arange(rows)[:, None] * C + np.arange(Ct)[None, :]]
    dy, x = lanes(p['dy'], B * Ho * Wo).reshape(B, Ho, Wo, Ct), lanes(p['x'], B * H * W).reshape(B, H, W, Ct)
    dw, db = dw_buf.reshape(-1, ks * ks), db_buf
    db[:Ct] += dy.sum((0, 1, 2), dtype=F32)
    for ky in range(ks):
        ho, hi = _taps(H, Ho, ks, s, pad, ky)
        for kx in range(ks):
            wo, wi = _taps(W, Wo, ks, s, pad, kx)
            dw[:Ct, ky * ks + kx] += (dy[:, ho[:, None], wo[None, :]] * x[:, hi[:, None], wi[None, :]]).sum((0, 1, 2), dtype=F32)


def _eq(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b.numpy() if torch.is_tensor(b) else b, dtype=np.float64))


# ---- the shapes reach their branches -------------------------------------------------------------------------------------------------------
def test_shapes_reach_what_they_are_there_for():
    ps = {s: _p(s) for s in dx.SHAPES}
    big = ps[dx.SHAPES[0]]
    # the second grid-stride pass of forward and dgrad, for some threads only; by the smallest number of columns
    assert dx.passes(dx.fwd_items(big)) == (1, 2) and dx.passes(dx.dgrad_items(big)) == (1, 2)
    B, H, W, C, ks, s, _ = dx.SHAPES[0]
    assert dx.passes(B * H * (W - 2) * C // 4)[1] == 1
    assert all(dx.passes(dx.fwd_items(p))[1] == 1 for sh, p in ps.items() if sh != dx.SHAPES[0])
    assert big['x'].numel() * 4 < 18e6
    # wgrad: pixel chunks longer than 64; a second channel tile with one live lane
    gx, tiles, per, live = dx.wgrad_grid(ps[dx.SHAPES[1]])
    assert gx == 256 and per > 64 and tiles == 1
    gx, tiles, per, live = dx.wgrad_grid(ps[dx.SHAPES[2]])
    assert tiles == 2 and live == 1
    assert all(dx.wgrad_grid(p)[1] == 1 or sh in (dx.SHAPES[0], dx.SHAPES[2]) for sh, p in ps.items())
    # stride 2 with (H + 2 pad - ks) % stride != 0: rows and columns of the PADDED map that no output reads, both parities of the dgrad's
    # stride selection; stride 3 with a remainder larger than the padding: rows and columns of the INPUT that no output reads
    # (of the two stride-2 shapes only the first leaves a remainder, in H, and it falls into the padding: hence the stride-3 shape)
    assert dx.SHAPES[3][5] == 2 and dx.SHAPES[4][5] == 2 and (ps[dx.SHAPES[3]]['H'] + 2 * ps[dx.SHAPES[3]]['pad'] - ps[dx.SHAPES[3]]['ks']) % 2 == 1
    rows, cols = dx.unread(ps[dx.SHAPES[7]])
    assert rows >= 1 and cols >= 1 and all(dx.unread(p) == (0, 0) for sh, p in ps.items() if sh != dx.SHAPES[7])
    assert {sh[4] for sh in dx.SHAPES} == {3, 5, 7}
    assert dx.SHAPES[5] == (3, 8, 12, 32, 3, 2, None)
    one = ps[dx.SHAPES[6]]
    assert (one['Ho'], one['Wo'], one['pad']) == (1, 1, 0)
    assert set(dx.STAT_REPS) == {1, 4, 32} and any(dx.flat_grid(dx.fwd_items(p)) < 32 for p in ps.values()) and dx.flat_grid(dx.fwd_items(big)) > 32


# ---- the operands --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', dx.SHAPES, ids=_ids)
def test_problem(shape):
    p = _p(shape)
    assert set(p['x'].unique().tolist()) <= set(range(-3, 4)) and set(p['w'].abs().unique().tolist()) <= {0.5, 1., 2.}
    assert set(p['dy'].unique().tolist()) <= {-2., -1., 1., 2.} and float(p['bias'].abs().max()) <= 3 and bool((p['bias'] != 0).any())
    b = dx.bounds(p)
    assert all(v < dx.LIMIT for v in b.values()), b
    r = p['ref']
    assert float(r['y'].abs().max()) <= (p['ks'] ** 2 * dx.X_MAX * dx.W_MAX + dx.BIAS_MAX)
    for k in ('y', 'dx', 'dw', 'dbias'):
        assert torch.equal(r[k] * 2, (r[k] * 2).round())
    assert torch.equal(r['stats'] * 4, (r['stats'] * 4).round()) and float(r['stats'].abs().max()) < 2.0 ** 53
    for k, start in (('dx0', 'dx'), ('dw0', 'dw'), ('db0', 'dbias')):
        assert bool((p[k] != 0).any()) and p[k].shape == r[start].shape
        acc = dx.accumulated(p, k, start, 2)
        assert torch.equal(acc.float().double(), acc)
    rows, cols = dx.unread(p)
    if rows:
        assert bool((r['dx'][:, p['H'] - rows:] == 0).all())
    if cols:
        assert bool((r['dx'][:, :, p['W'] - cols:] == 0).all())
    assert float(r['bn'].abs().max()) < 1e3 and float((r['bn'][..., 1:] - r['bn'][..., :-1]).abs().max()) > 0.5


@pytest.mark.parametrize('shape', dx.SHAPES[1:], ids=_ids)
def test_reference_is_the_grouped_convolution(shape):
    p = _p(shape)
    x = p['x'].permute(0, 3, 1, 2).double().requires_grad_(True)
    w, b = p['w'].double().requires_grad_(True), p['bias'].double().requires_grad_(True)
    y = F.conv2d(x, w, b, stride=p['stride'], padding=p['pad'], groups=p['C'])
    y.backward(p['dy'].permute(0, 3, 1, 2).double())
    r = p['ref']
    assert torch.equal(y.detach().permute(0, 2, 3, 1), r['y'].double()) and torch.equal(x.grad.permute(0, 2, 3, 1), r['dx'].double())
    assert torch.equal(w.grad, r['dw'].double()) and torch.equal(b.grad, r['dbias'].double())


# ---- the mirrors: right equals the reference, a seeded defect does not -------------------------------------------------------------------------
@pytest.mark.parametrize('shape', dx.SHAPES, ids=_ids)
def test_forward_and_dgrad_mirrors(shape):
    p = _p(shape)
    r = p['ref']
    for rep in dx.STAT_REPS:
        y, stats = mirror_fwd(p, True, rep)
        assert _eq(y, r['y']) and _eq(stats.sum(0), r['stats'])
        grid = dx.flat_grid(dx.fwd_items(p))
        assert not np.abs(stats[min(rep, grid):]).sum() and (rep == 1 or min(rep, grid) == 1 or not _eq(stats[0], r['stats']))
    assert _eq(mirror_fwd(p, False)[0], r['y_nobias'])
    assert _eq(mirror_dgrad(p), r['dx'])
    once = mirror_dgrad(p, p['dx0'].numpy())
    assert _eq(once, dx.accumulated(p, 'dx0', 'dx', 1)) and _eq(mirror_dgrad(p, once), dx.accumulated(p, 'dx0', 'dx', 2))
    if dx.passes(dx.fwd_items(p))[1] > 1:
        y, stats = mirror_fwd(p, True, 4, defect='one_pass')
        assert not _eq(y, r['y']) and not _eq(stats.sum(0), r['stats'])
        assert not _eq(mirror_dgrad(p, defect='one_pass'), r['dx'])
        assert not _eq(mirror_dgrad(p, p['dx0'].numpy(), defect='one_pass'), dx.accumulated(p, 'dx0', 'dx', 1))


@pytest.mark.parametrize('shape', dx.SHAPES[1:], ids=_ids)
def test_wgrad_mirror(shape):
    p = _p(shape)
    ks2 = p['ks'] ** 2

    def want(calls):
        dw, db = dx.guarded(p, 'dw0', ks2).numpy().astype(np.float64), dx.guarded(p, 'db0', 1).numpy().astype(np.float64)
        dw[:p['C'] * ks2] = dx.accumulated(p, 'dw0', 'dw', calls).reshape(-1).numpy()
        db[:p['C']] = dx.accumulated(p, 'db0', 'dbias', calls).numpy()
        return dw, db
    dw, db = dx.guarded(p, 'dw0', ks2).numpy(), dx.guarded(p, 'db0', 1).numpy()
    for calls in (1, 2):
        mirror_wgrad(p, dw, db)
        assert _eq(dw, want(calls)[0]) and _eq(db, want(calls)[1])
    _, tiles, _, live = dx.wgrad_grid(p)
    assert shape != dx.SHAPES[2] or (tiles == 2 and live < 64)
    if live < 64 and p['B'] * p['Ho'] * p['Wo'] > 1:         # the last tile has dead lanes: without the mask they write behind dw and dbias
        dw, db = dx.guarded(p, 'dw0', ks2).numpy(), dx.guarded(p, 'db0', 1).numpy()
        mirror_wgrad(p, dw, db, defect='ignore_live')
        want_dw, want_db = want(1)
        assert _eq(dw[:p['C'] * ks2], want_dw[:p['C'] * ks2]) and _eq(db[:p['C']], want_db[:p['C']])
        assert not _eq(dw[p['C'] * ks2:], want_dw[p['C'] * ks2:]) and not _eq(db[p['C']:], want_db[p['C']:])
