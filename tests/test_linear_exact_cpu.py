"""Without a GPU: (1) the operand recipes of tests/linear_exact.py do what their docstring says, checked on the generated values; (2) every row
of tests/test_linear_fwd_routes_gpu.py still routes to the kernel it is there for, in its mode, with its strides and flags; (3) that table
is complete: every positive (entry, mode, code) of the literal route table of tests/test_linear_routes_cpu.py has a row, every kernel family
meets every class of M and every option combination it is instantiated for."""
import numpy as np
import pytest
import torch

import linear_exact as le
import test_linear_fwd_routes_gpu as T
import test_linear_routes_cpu as R
from linear_exact import LN, STATS, KSCALE, AUX, TOUT, DX2, COLSUM, ACCUMULATE, DRES, MASKED

F, B, H = T.F, T.B, T.H
BF16, F16 = torch.bfloat16, torch.float16


def _roundtrips(t):
    return le.representable(t, BF16) and le.representable(t, F16)


def _bits(t):
    """significant bits of the largest magnitude: every value is an integer multiple of 0.5 here"""
    v = (t.abs() * 2).long()
    return int(max(int(x).bit_length() - (int(x) & -int(x)).bit_length() + 1 for x in v.unique().tolist() if x))


# ---- (1) the claims on the generated values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry,N,K,a16,out16,flags', [
    (0, 36, 48, 0, 0, 0), (0, 36, 48, 0, 0, AUX), (1, 20, 36, 0, 0, TOUT), (4, 20, 40, 0, 0, 0), (5, 20, 36, 0, 0, 0), (5, 20, 36, 0, 0, MASKED),
    (6, 36, 20, 0, 0, 0), (6, 36, 20, 1, 0, KSCALE), (6, 36, 20, 0, 0, KSCALE | AUX), (6, 36, 20, 0, 0, AUX | MASKED), (6, 36, 20, 0, 0, DRES),
    (6, 36, 20, 0, 1, 0), (8, 36, 20, 0, 1, AUX | KSCALE), (8, 36, 20, 0, 0, AUX | MASKED)])
def test_plain_operands_are_exact_in_16_bits_and_never_zero(entry, N, K, a16, out16, flags):
    M = 1031
    p = le.problem(entry, M, N, K, a16, out16, flags, 0)
    ops = [p[k] for k in ('x', 'a', 'A', 'dy', 'W', 'bias', 'gamma', 'res', 'kscale', 'aux_u', 'dres') if p.get(k) is not None]
    if flags & AUX and entry == 0:                     # the bias that lifts the pre-activations to >= 8: an fp32 integer, added in fp32
        assert torch.equal(p['bias'], p['bias'].round()) and float(p['bias'].abs().max()) < 2 ** 20
        ops = [t for t in ops if t is not p['bias']]
    for t in ops:
        assert t.dtype is torch.float32 and _roundtrips(t) and _bits(t) <= 4          # u = 10, 12, 14 apart: 3 bits
    for k in ('x', 'a', 'dy', 'W', 'gamma', 'kscale', 'aux_u'):
        if p.get(k) is not None:
            assert bool((p[k] != 0).all()) and _bits(p[k]) <= 3, f'{k}: a zero operand would hide a dropped contribution'
    if p.get('kscale') is not None:                    # the operand the 16-bit modes round: dy * kscale
        assert _roundtrips(p['dy'] * p['kscale'])
    for name, ref in p['ref'].items():                 # integers or half-integers far below 2^24, so that fp32 holds every partial sum
        for r in (ref if isinstance(ref, list) else [ref]):
            assert torch.equal(r * 2, (r * 2).round()) and float(r.abs().max()) * 2 < 2 ** 20, name
    if flags & AUX and entry == 0:
        assert float(p['ref']['out'].min()) >= 8 and torch.equal(p['ref']['out'], p['ref']['out'].round())
    if entry in (5, 6, 8) and (entry == 5 or flags & AUX):
        u = p['a'] if entry == 5 else p['aux_u']
        want = set(le.U_VALUES) | ({-v for v in le.U_VALUES} if flags & MASKED else set())
        assert set(u.flatten().tolist()) == want and le.representable(u, F16)


def test_reference_is_the_integer_contraction():
    p = le.problem(6, 300, 8, 12, 0, 0, KSCALE | ACCUMULATE | COLSUM, 0)
    g2 = (p['dy'] * p['kscale'] * 2).long() @ p['W'].long()                             # in halves: exact integer arithmetic
    assert p['calls'] == 2
    for n in (1, 2):
        assert torch.equal((p['ref']['dx'][n - 1] * 2).long(), (p['dx0'] * 2).long() + n * g2)
    c1 = (p['colsum0'] * 2).long() + ((p['dx0'] * 2).long() + g2).sum(0)
    assert torch.equal((p['ref_colsum'][0] * 2).long(), c1)
    assert torch.equal((p['ref_colsum'][1] * 2).long(), c1 + ((p['dx0'] * 2).long() + 2 * g2).sum(0))
    assert bool((p['dx0'] != 0).any()) and bool((p['colsum0'] != 0).any())
    q = le.problem(1, 300, 8, 12, 0, 0, TOUT, 0)
    t2 = (q['a'].long() @ q['W'].long().t() + q['bias'].long()) * 2
    assert torch.equal((q['ref']['tout'] * 2).long(), t2)
    assert torch.equal((q['ref']['out'] * 4).long(), q['res'].long() * 4 + (q['gamma'] * 2).long() * t2)
    buf, ld = le.padded(q['a'], 4)
    assert ld == 16 and torch.equal(buf[:, :12], q['a']) and bool((buf[:, 12:] == le.PAD_VALUE).all()) and _roundtrips(torch.tensor([le.PAD_VALUE]))


@pytest.mark.parametrize('K', [32, 48, 64, 80, 96, 320])
def test_layernorm_rows(K):
    """K / 2 of each sign, variance c^2, no zero operand -- and the kernels' own fp32 evaluation (two-pass mean / variance, rsqrt(var / K + eps))
    rounds to exactly that operand in bf16 and in fp16"""
    M = 2053
    x, ln_w, ln_b, mean, c, X = le.ln_rows(M, K, le._gen(K))
    assert set(ln_w.tolist()) <= {1., 2., -1., -2.} and set(ln_b.tolist()) <= {-1., 0., 1., 2.}
    s = (x - mean) / c
    assert set(s.flatten().tolist()) == {1., -1.} and bool(((s > 0).sum(1) == K // 2).all())
    assert torch.equal(X, s * ln_w + ln_b) and bool((X != 0).all()) and float(X.abs().max()) <= 4 and _roundtrips(X) and _roundtrips(x)
    assert len(set(c.flatten().tolist())) == 3 and len(set(mean.flatten().tolist())) == 5         # neighbouring rows differ in both statistics
    xd = x.double()
    assert torch.equal(xd.mean(1, keepdim=True), mean.double()) and torch.equal(((xd - mean.double()) ** 2).mean(1, keepdim=True), (c * c).double())
    f = np.float32
    xn = x.numpy()
    m32 = xn.sum(1, keepdims=True, dtype=f) * f(1.0 / K)
    d = xn - m32
    rstd = f(1) / np.sqrt((d * d).sum(1, keepdims=True, dtype=f) * f(1.0 / K) + f(le.EPS), dtype=f)
    for scale in (f(1), f(1 + 2e-6), f(1 - 2e-6)):     # a hardware rsqrt a few ulp off changes nothing
        op = torch.from_numpy((d * (rstd * scale) * ln_w.numpy() + ln_b.numpy()).astype(f))
        assert torch.equal(op.to(BF16).float(), X) and torch.equal(op.to(F16).float(), X)
    tn, tmean, trstd = le.ln_true(x, ln_w, ln_b)
    assert float((tn - X.double()).abs().max()) < 2e-4 and torch.equal(tmean, mean.double())
    assert float((trstd - 1 / c.double()).abs().max()) < 5e-5


def test_gelu_and_its_derivative_on_the_chosen_values():
    """float32 transcription of normal_cdf / gelu_erf / gelu_erf_grad (csrc/common.hpp)"""
    f = np.float32

    def cdf(u):
        z = np.abs(u) * f(0.70710678118654752440)
        t = f(1) / (f(0.3275911) * z + f(1))
        poly = t * (f(0.254829592) + t * (f(-0.284496736) + t * (f(1.421413741) + t * (f(-1.453152027) + t * f(1.061405429)))))
        e = np.exp(-z * z, dtype=f)
        half = f(0.5) * poly * e
        return np.where(u >= 0, f(1) - half, half).astype(f), e
    pos = np.concatenate([np.arange(8, 4200, dtype=f), np.array([8192, 20000, 70000], dtype=f)])   # every integer pre-activation from 8 on
    c, e = cdf(pos)
    assert np.array_equal(c, np.ones_like(pos)) and np.array_equal(pos * c, pos)                    # gelu(u) == u
    u = np.array(le.U_VALUES, dtype=f)
    c, e = cdf(u)
    assert np.array_equal(u * f(0.39894228040143267794) * e + c, np.ones_like(u))                   # gelu'(u) == 1
    c, e = cdf(-u)
    g, gp = -u * c, -u * f(0.39894228040143267794) * e + c
    assert float(np.abs(g).max()) < 1e-12 and float(np.abs(gp).max()) < 1e-12 and bool((g != 0).any()) and bool((gp != 0).any())
    assert 1e-12 * 1e3 <= le.MASK_TOL                  # times an exact result below 1e3 (3 * 2 * 2 * 48 .. 96 columns of the masked rows)
    # entry 5 feeds gelu(u) to the MFMA: as an fp16 operand gelu(u <= -8) is an exact zero, as a bf16 operand it is not -- the masked rows of
    # entry 5 are mode-16f rows (test_rows_are_well_formed)
    gt = torch.from_numpy(g.astype(f))
    assert bool((gt.to(F16) == 0).all()) and bool((gt.to(BF16) != 0).any())


def _rows16():
    rows = [r for r in T.ALL_ROWS if le.out16_kind(r[0], r[6]) is not None]
    top = {}
    for r in rows:
        if r[2] > top.get((r[0], r[10]), r)[2] or (r[0], r[10]) not in top:
            top[(r[0], r[10])] = r
    keep = {r[:1] + r[2:9] for r in rows if r[2] <= 20000} | {r[:1] + r[2:9] for r in top.values()}
    return sorted(keep)


@pytest.mark.parametrize('key', _rows16(), ids=lambda k: '-'.join(map(str, k)))
def test_16_bit_outputs_are_representable(key):
    """per (entry, code) the largest row and every row up to 20000: the reference fits bf16 (fp16 for the MLP hidden)"""
    entry, M, N, K, a16, out16, flags, nsplit = key
    p = le.problem(entry, M, N, K, a16, out16, flags, nsplit)
    ref = p['ref']['out'] if entry < 6 else p['ref']['dx'][0]
    assert le.representable(ref, F16 if entry == 2 else BF16)
    if entry == 3:
        assert le.representable(ref, F16)              # mode 16f stores these rows as fp16


def test_reduction_bounds():
    """every row that sums over M (colsum, an accumulating dx, dgamma / dbeta of entry 7) stays below 2^24 in the worst case"""
    n = 0
    for r in T.ALL_ROWS:
        entry, _, M, N, K, a16, out16, flags, nsplit = r[:9]
        if entry == 7 or (entry == 6 and flags & (COLSUM | ACCUMULATE)):
            assert le.reduction_bound(entry, M, N, K, flags) < 2 ** 24, r
            n += 1
    assert n >= 40
    # the generator uses the small value sets on exactly those rows
    p = le.problem(6, 64, 48, 20, 0, 0, COLSUM, 0)
    assert p['dy_max'] == 1.0 and p['w_max'] == 1.0 and float(p['dy'].abs().max()) == 1 and float(p['W'].abs().max()) == 1
    p = le.problem(7, 64, 144, 48, 0, 0, STATS | DRES, 0)
    assert p['dy_max'] == 1.0 and p['w_max'] == 1.0 and float(p['x'].sub(p['stats'][:, :1]).abs().max()) == 0.5
    assert float(((p['x'] - p['stats'][:, :1]) * p['stats'][:, 1:]).abs().max()) <= p['xhat_max']
    assert torch.equal(p['ref']['dn'], (p['dy'].long() @ p['W'].long()).float())


# ---- (2) the routes ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ops():
    import __graft_entry__ as g
    g.build()
    from leod_amd import ops
    prev = ops.get_precision()
    yield ops
    ops.set_precision(prev)


@pytest.mark.parametrize('mode', T.MODES)
def test_every_gpu_row_routes_where_it_says(ops, mode):
    ops.set_precision(mode)
    bad = [(r, got) for r in T.ALL_ROWS + T.REFUSALS if r[1] == mode for got in [T.route_of(ops, r)] if got != r[10]]
    assert not bad, f'{len(bad)} rows route elsewhere (row, got): {bad[:10]}'
    for e in range(9):                                 # no rows: nothing to do, whatever the entry has kernels for
        if mode in T.ENTRY_MODES[e]:
            assert ops.linear_route(e, 0, 144, 48, flags={0: 3, 2: 3, 3: 3, 7: 2, 8: 8}.get(e, 0)) == 0


def test_rows_are_well_formed():
    assert 350 <= len(T.ALL_ROWS) <= 450, len(T.ALL_ROWS)
    assert len(set(T.ALL_ROWS)) == len(T.ALL_ROWS)
    for r in T.ALL_ROWS + T.REFUSALS:
        entry, mode, M, N, K, a16, out16, flags, nsplit, pad, code = r
        assert mode in T.ENTRY_MODES[entry] and M > 0 and pad % 4 == 0 and (pad % 8 == 0 or not (a16 or out16)), r
        assert not pad or entry in (0, 6), r           # the entries with stride parameters
        assert bool(flags & DX2) == (nsplit > 0) and nsplit % 4 == 0 and nsplit < K, r
        assert not flags & MASKED or (entry == 5 and mode == H) or (entry in (6, 8) and flags & AUX), r
        assert not (flags & MASKED and flags & (COLSUM | ACCUMULATE | DRES)), r
    assert all(r[9] == 0 for r in T.ROUTES + T.EXTRAS) and all(r[9] > 0 for r in T.STRIDED) and all(r[10] < 0 for r in T.REFUSALS)


# ---- (3) completeness -------------------------------------------------------------------------------------------------------------------
def _a_fmt(r):
    return ('f16' if r[1] == H else 'bf16') if r[0] == 4 else 'f16pre' if r[0] == 5 else 'bf16' if r[5] else 'f32'


def test_every_triple_of_the_route_table_has_a_row():
    need = {(r[0], r[1], r[-1]) for r in R.ROWS if r[-1] > 0}
    have = {(r[0], r[1], r[10]) for r in T.ROUTES}
    assert len(need) == 297 and need <= have, sorted(need - have)
    assert {r[10] for r in T.ROUTES} == R.ALL_CODES


def test_every_class_of_M():
    by = {}
    for r in T.ROUTES:
        by.setdefault(r[10], set()).add(r[2])
    for c in (6011, 6014, 6021, 6024, 6031, 6034, 6041, 6044):
        assert {1, 15, 17, 63, 65, 300} <= by[c], c
    for r in T.ROUTES:                                 # KS = 4 needs a contraction of 128
        if r[10] // 1000 == 6:
            assert ((r[3] if r[0] >= 6 else r[4]) >= 128) == (r[10] % 10 == 4), r
    for c in (4348, 4364, 4448, 4464, 5148, 5164, 5248, 5264):
        m0 = 8129 if c < 5000 else 3265                # 96 / 128 columns: 2 workgroup columns, 80 / 160: 5; 64 rows each, 256 workgroups
        assert {m0, m0 + 1, m0 + 63} <= by[c] and 10007 in by[c] and min(by[c]) == m0, c
    for c in (3003, 3004):
        assert {4096, 4097, 4096 + 127, 4096 + 129, 32897} <= by[c], c
    sq = {(r[2], r[10]) for r in T.ROUTES if r[3] == r[4] == 192 and r[1] != F}
    assert {(60000, 3003), (60001, 4448)} <= sq
    # row-streaming: rows per pass of one launch (grid.x * waves * 16), written out from rowstream48_grid / rowstream_narrow_grid
    per_pass = {1309: 768 * 64, 1312: 512 * 64, 1412: 512 * 64, 1609: 256 * 64, 1408: 256 * 64, 1608: 168 * 64,
                2009: 512 * 64, 2012: 512 * 64, 2018: 256 * 128, 2024: 256 * 128}
    for c, P in per_pass.items():
        assert {16384, 16391} <= by[c], c
        for k in ((1,) if c == 2018 else (1, 2, 3)):    # some wave runs k and some k + 1 tiles; 2018 is entry 7 only, capped by its reductions
            assert any(k * P < m <= (k + 1) * P and m % P for m in by[c]), (c, k)
        assert {m % 16 for m in by[c]} >= {0, 7}, c
    assert max(r[2] for r in T.ALL_ROWS) < 150000 and max(max(r[3], r[4]) for r in T.ALL_ROWS if r[2] > 70000) <= 384


def test_every_option_combination_of_every_family():
    rows, missing = T.ALL_ROWS, []
    fam = lambda r: r[10] // 1000                      # noqa: E731

    def has(**want):
        def ok(r):
            d = dict(fam=fam(r), entry=r[0], mode=r[1], a=_a_fmt(r), out16=r[6], ln=bool(r[7] & LN), ks=bool(r[7] & KSCALE), aux=bool(r[7] & AUX),
                     tout=bool(r[7] & TOUT), masked=bool(r[7] & MASKED), a16=r[5], code=r[10])
            return all(d[k] == v for k, v in want.items())
        if not any(ok(r) for r in rows):
            missing.append(want)
        return True
    # launch_rowstream48: RS48_FWD / RS48_DG
    for mode in T.MODES:
        for ln in (False, True):
            for act in (False, True):
                assert has(fam=1, entry=0, mode=mode, ln=ln, aux=act), (mode, ln, act)
        for aux in (False, True):
            assert has(fam=1, entry=6, mode=mode, aux=aux), (mode, aux)
        assert has(fam=1, entry=6, mode=mode, ks=True)
        # launch_rowstream_narrow: NARROW
        assert has(fam=2, entry=1, mode=mode) and has(fam=2, entry=6, mode=mode) and has(fam=2, entry=7, mode=mode, a16=0)
    for mode in (B, H):
        assert has(fam=1, entry=2, mode=mode) and has(fam=1, entry=3, mode=mode) and has(fam=2, entry=5, mode=mode)
        for out16 in (0, 1):
            assert has(fam=1, entry=8, out16=out16), out16
        assert has(fam=2, entry=7, mode=mode, a16=1) and has(code=2018, mode=mode) and has(code=2024, entry=7, mode=mode)
    assert has(fam=1, entry=8, ks=True) and has(fam=1, entry=8, ks=False) and has(fam=1, entry=8, masked=True) and has(fam=2, entry=5, masked=True)
    # launch_gemm_lds: LEOD_WIDE
    for want in (dict(entry=0, ln=False), dict(entry=0, ln=True), dict(entry=2), dict(entry=3, ln=True), dict(entry=3, ln=False),
                 dict(entry=1), dict(entry=5), dict(entry=4, mode=H), dict(entry=6, a='f32', ks=False), dict(entry=6, a='f32', ks=True),
                 dict(entry=6, a='bf16'), dict(entry=8, ks=False), dict(entry=8, ks=True)):
        assert has(fam=3, **want), want
    # ... and LEOD_ALM: fp32 rows plain / LayerNorm / kscale, bf16 rows plain / kscale, fp16 pre-activation, fp16 rows
    for want in (dict(a='f32', ln=False, ks=False), dict(a='f32', ln=True), dict(a='f32', ks=True), dict(a='bf16', ks=False, entry=6),
                 dict(a='bf16', ks=True, entry=6), dict(a='bf16', entry=4), dict(a='f16pre'), dict(a='f16')):
        assert has(fam=4, **want), want
    # the epilogue options and A formats on every family that has them
    for f_ in (3, 4, 5, 6):
        assert has(fam=f_, entry=0, aux=True) and has(fam=f_, entry=0, aux=True, ln=True), f_       # GELU dual output
        assert has(fam=f_, entry=1, tout=True) and has(fam=f_, entry=1, tout=False), f_
        assert has(fam=f_, entry=6, aux=True) and has(fam=f_, entry=5, masked=True), f_             # GELU' and GELU on load
        assert has(fam=f_, entry=0, ln=True) and has(fam=f_, entry=0, ln=False), f_
        assert has(fam=f_, ks=True), f_
    for f_ in (3, 4, 5):
        assert has(fam=f_, entry=8, out16=0) and has(fam=f_, entry=8, out16=1) and has(fam=f_, entry=8, masked=True), f_
        assert has(fam=f_, entry=2) and has(fam=f_, entry=3), f_
        for a in ('f32', 'bf16', 'f16', 'f16pre'):
            assert has(fam=f_, a=a), (f_, a)
    assert not missing, f'no row for {missing}'
    # every extra of leod_linear_dgrad in f32 and a 16-bit mode, on both sides of the LDS threshold; dx_fmt = 1; strides
    for mode in (F, B):
        for f_ in (4, 6):
            for bit in (ACCUMULATE, DRES, DX2, COLSUM, AUX, AUX | KSCALE):
                assert any(r[0] == 6 and r[1] == mode and fam(r) == f_ and r[7] & (bit | MASKED) == bit for r in T.EXTRAS), (mode, f_, bit)
    assert any(r[6] == 1 and r[5] == 0 for r in T.EXTRAS) and any(r[6] == 1 and r[5] == 1 for r in T.EXTRAS)
    assert {fam(r) for r in T.STRIDED if r[0] == 0} >= {3, 4, 5, 6} and {fam(r) for r in T.STRIDED if r[0] == 6} >= {3, 4, 5, 6}
    assert any(r[8] for r in T.STRIDED) and any(r[5] for r in T.STRIDED) and any(r[6] for r in T.STRIDED)
    got = {(r[7] & le.ABI_FLAGS, r[6], r[10]) for r in T.REFUSALS}
    assert {(DRES | ACCUMULATE, 0, -1), (DRES | DX2, 0, -1), (ACCUMULATE, 1, -3), (0, 1, -3)} <= got
