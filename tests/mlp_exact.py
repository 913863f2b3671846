"""Operands on which the one-launch MLP of stage 1 (csrc/k_mlp.hip: ``mlp_fwd_fused_kernel``, ``mlp_bwd_dgrad_fused_kernel``) has NO rounding
error in either 16-bit mode and in any summation order, the float64 model of both kernels, and mutations of that model -- so that
tests/test_mlp_exact_gpu.py compares for equality and a hidden unit read from the wrong LDS row, a tile computed from the wrong fragment or a
row never written moves an element by at least 0.5.  Built on tests/linear_exact.py (``ln_rows``, the value sets, ``close_fp32``).

    forward    z = y + gamma (gelu(LN(y) W1^T + b1) W2^T + b2);  u16 = fp16(u), stats = (mean, rstd) of LN
    backward   du = ((dz gamma) W2) gelu'(u);  dn = du W1;  dy = dz + LN-backward(dn);  dgamma += sum_m dn xhat;  dbeta += sum_m dn

* LayerNorm operand: ``y`` are ``ln_rows``.  The forward kernel derives (mean, rstd) itself (sum * (1 / K), two-pass variance,
  rsqrt(var / K + eps)); the few ulp of that lie far below half a 16-bit ulp of a value of at most 3 bits, so after the rounding to
  bf16 / fp16 the MFMA operand IS the integer matrix Xn = +-ln_w + ln_b (tests/test_linear_exact_cpu.py::test_layernorm_rows evaluates the
  kernel's formula in fp32 for K = 48 and 64).  The statistics it writes are not exact: ``close_fp32`` against ``ln_true``.  The backward
  kernel takes the caller's statistics -- integer mean, rstd = 1 / c in {0.5, 1, 2} -- so (y - mean) rstd = +-1 = xhat exactly.  They are
  NOT the ones the forward kernel wrote: the two tests do not depend on each other.
* plain problem: W1, W2 in +-1, b1[j] = 8 - min_m (Xn W1^T)[m, j], so that every pre-activation is an integer >= 8, where
  ``gelu_parts2`` gives cdf = 1.0f exactly: gelu(u) == u, gelu'(u) == 1.0f.  u stays an integer <= 256: representable in bf16 (the hidden
  operand of mode bf16) and fp16 (the hidden operand of mode 16f, and u16).  b2 small integers, gamma in {0.5, 1, 2}: z is a multiple of
  0.25 below 2^14, exact in fp32.
* masked problem: the sign of u must depend on the row AND on the hidden unit, or a GELU' taken from a neighbouring row or unit is the
  right one.  A column k* of ``ln_rows`` with |ln_w| = 2, ln_b = 0 carries Xn[m, k*] = 2 s_m; W1[j, k*] = 64 sigma_j, the other entries of
  W1 +-1, and b1 centres what they contribute: u[m, j] = 128 s_m sigma_j + (|.| <= 85), half of the elements negative, |u| <= 256.  For
  u <= -8 gelu and gelu' are below 1e-12 in magnitude but in general not zero; the model takes them as 0.  Equality where a 16-bit
  rounding makes them 0 -- the fp16 hidden operand of the forward in mode 16f -- and ``MASK_TOL`` in mode bf16 (z behind the bf16 hidden
  operand, the masked elements of du), as linear_exact.py argues for its masked rows.  du in mode 16f is compared for equality too: the
  backward stores bf16 there as well, but with |u| >= 43 the exponential of ``gelu_parts2`` underflows and gelu' is +-0 in fp32 already
  (tests/test_mlp_exact_cpu.py::test_gelu_parts2_on_the_values_that_occur).
  ``b1 = None`` is a case of the masked problem: without a bias nothing lifts a plain pre-activation to >= 8, but 128 s_m sigma_j still
  keeps |u| >= 43.
* backward: dz in +-{1, 2} on about one element in eight and zero elsewhere, gamma in {1, 2}: dz gamma, du and dn are integers, du <= 256
  in magnitude (bf16 rows).
* reductions over M (dgamma, dbeta): an element is compared for equality if |start| + sum_m |dn[m, k]| (|xhat| = 1), i.e. the sum of the
  magnitudes of its terms in units of its smallest step, is below 2^24 -- then every partial sum of every order is an exact fp32 integer.
  ``reference`` computes that bound per element; the others are compared with ``close_fp32``.  Every element of every plain problem meets
  it; in a masked problem only the sign column k* (weights of 64) may miss it.  Both start from ``start_vector``.
* dy = dz + rstd (gw - mean(gw) - xhat mean(gw xhat)), gw = dn ln_w: the kernel multiplies the row sums by the fp32 constant 1 / K.  K = 48:
  not exact, ``close_fp32`` (as entry 7 of linear_exact.py).  K = 64: the row sums are integers below 2^24, 1 / 64 is a power of two and
  every intermediate value a multiple of 2^-7 below 2^13; ``dy_fp32`` evaluates the kernel's operation order in fp32 and ``reference``
  records in ``dy_exact`` whether it equals the float64 model -- it does for every plain K = 64 problem of the GPU test
  (tests/test_mlp_exact_cpu.py asserts it), which therefore compares dy for equality.  Masked problems: ``close_fp32``.

``mutate(problem, name)`` is the same model with one defect of the kind the kernels can have (``MUTATIONS``); tests/test_mlp_exact_cpu.py
checks every claim above on the generated values and that each mutation moves an element compared for equality by >= 0.5."""
import functools

import torch

from linear_exact import (MASK_TOL, _ints, _pick, _signed, _signs, close_fp32, ln_rows, ln_true, representable,  # noqa: F401  (re-exported)
                          start_vector)

WIDTHS = ((48, 192), (64, 256))
# M: full tiles the owner of the ragged tile runs first -> the exit its pipeline leaves by (forward: 3 fragments, backward: 2)
ROW_COUNTS = (16384, 16391, 32855, 70001, 98451)
BF16, F16 = torch.bfloat16, torch.float16
EXACT_LIMIT = float(2 ** 24)
MUTATIONS = ('w2_units_swapped', 'b1_natural_order', 'ragged_from_previous_fragment', 'tile_twice_next_skipped', 'gelu_grad_from_next_row',
             'no_gamma_in_backward')


def cases():
    """(K, H, M, kind, drop) of every problem of tests/test_mlp_exact_gpu.py; drop: the operand passed as None"""
    out = []
    for K, H in WIDTHS:
        out += [(K, H, M, 'plain', None) for M in ROW_COUNTS]
        out += [(K, H, 32855, 'masked', None), (K, H, 16391, 'masked', 'b1'), (K, H, 16391, 'plain', 'b2'), (K, H, 16391, 'plain', 'gamma')]
    return out


def poison(device, *specs):
    """Best effort against a row the kernel never writes: ``ops`` allocates outputs with ``torch.empty`` and the caching allocator may hand
    back the block that still holds the previous call's (correct) result.  Create and free a NaN-filled tensor of each output's (shape,
    dtype) on the current stream, so that the blocks the next call most likely receives hold NaN.  Nothing guarantees that reuse."""
    for shape, dtype in specs:
        t = torch.full(shape, float('nan'), dtype=dtype, device=device)
        del t


def mlp_unit_of_row(R):
    """csrc/k_mlp.hip: the hidden unit that LDS row R of the A-operand matrices and of the bias holds"""
    return 32 * (R >> 5) + 8 * ((R & 15) >> 2) + 4 * ((R >> 4) & 1) + (R & 3)


def geometry(M):
    """-> (tiles, full tiles, tile stride of a wave) of both launches: grid = min(ceil(ceil(M / 16) / 4), 512) workgroups of 4 waves"""
    tiles = (M + 15) // 16
    grid = min((tiles + 3) // 4, 512)
    return tiles, M // 16, 4 * grid


def ragged_owner_full_tiles(M):
    """full tiles the wave that owns the ragged tile computes before it, or None without a ragged tile"""
    tiles, nfull, stride = geometry(M)
    return None if tiles == nfull else nfull // stride


@functools.lru_cache(maxsize=None)
def problem(K, H, M, kind='plain'):
    """CPU operands of one problem as the values they hold (fp32), computed once, shared, never modified.  kind: 'plain' | 'masked'"""
    assert (K, H) in WIDTHS and kind in ('plain', 'masked')
    g = torch.Generator().manual_seed(K * 1000003 + M * 7 + (kind == 'masked'))
    y, ln_w, ln_b, mean, c, Xn = ln_rows(M, K, g)
    p = dict(K=K, H=H, M=M, kind=kind, y=y, ln_w=ln_w, ln_b=ln_b, mean=mean, c=c, Xn=Xn, sign=(y - mean) / c, kstar=None)
    if kind == 'masked':
        cand = ((ln_w.abs() == 2) & (ln_b == 0)).nonzero().flatten()
        assert len(cand), 'no column with |ln_w| = 2 and ln_b = 0: another seed'
        ks = int(cand[0])
        sigma = _signs((H,), g)
        W1 = _signs((H, K), g)
        W1[:, ks] = 64.0 * sigma
        rest = Xn.double() @ W1.double().t() - Xn[:, ks:ks + 1].double() * W1[:, ks].double()
        b1 = -torch.round((rest.max(0).values + rest.min(0).values) / 2).float()
        p.update(kstar=ks, sigma=sigma)
    else:
        W1 = _signs((H, K), g)
        b1 = (8.0 - (Xn.double() @ W1.double().t()).min(0).values).float()
    p.update(W1=W1, b1=b1, W2=_signs((K, H), g), b2=_ints(-3, 3, (K,), g), gamma=_pick([0.5, 1., 2.], (K,), g),
             gamma_bwd=_pick([1., 2.], (K,), g))
    keep = torch.rand((M, K), generator=g) < 0.125
    p['dz'] = _signed([1., 2.], (M, K), g) * keep
    p['stats'] = torch.cat([mean, 1.0 / c], 1).contiguous()        # the caller's: integer mean, rstd in {0.5, 1, 2}
    p['dgamma0'], p['dbeta0'] = start_vector(K, 1), start_vector(K, 4)
    return p


def dy_fp32(p, dn):
    """dy in the operation order of mlp_bwd_dgrad_fused_kernel, fp32 throughout (the row sums are exact integers in any order)"""
    K = p['K']
    f = torch.float32
    xh = ((p['y'] - p['stats'][:, :1]) * p['stats'][:, 1:]).to(f)
    gw = dn.to(f) * p['ln_w']
    inv = torch.tensor(1.0 / K, dtype=f)
    s1 = gw.sum(1, keepdim=True, dtype=torch.float64).to(f) * inv
    s2 = (gw * xh).sum(1, keepdim=True, dtype=torch.float64).to(f) * inv
    return ((gw - s1) - xh * s2) * p['stats'][:, 1:] + p['dz']


def _model(p, drop=None, mut=None):
    """float64 model of both kernels.  drop: the operand passed as None ('b1' | 'b2' | 'gamma'); mut: one of MUTATIONS"""
    K, H, M = p['K'], p['H'], p['M']
    tiles, nfull, stride = geometry(M)
    d = torch.float64
    W1, W2, Xn, y, dz = p['W1'].to(d), p['W2'].to(d), p['Xn'].to(d), p['y'].to(d), p['dz'].to(d)
    b1 = torch.zeros(H, dtype=d) if drop == 'b1' else p['b1'].to(d)
    b2 = torch.zeros(K, dtype=d) if drop == 'b2' else p['b2'].to(d)
    g_f = torch.ones(K, dtype=d) if drop == 'gamma' else p['gamma'].to(d)
    g_b = torch.ones(K, dtype=d) if drop == 'gamma' or mut == 'no_gamma_in_backward' else p['gamma_bwd'].to(d)
    W2r = W2                                                    # W2 as the contraction over the hidden units reads it
    if mut == 'w2_units_swapped':
        j1, j2 = 5, 2 * H // 3 + 1
        W2r = W2.clone()
        W2r[:, [j1, j2]] = W2[:, [j2, j1]]
    if mut == 'b1_natural_order':                               # LDS row e holds unit mlp_unit_of_row(e) and is given b1[e]
        rows = torch.arange(H)
        b1 = b1.clone().index_copy_(0, torch.tensor([mlp_unit_of_row(int(e)) for e in rows]), b1[rows])
    Xf, dzf, yf = Xn, dz, y                                     # the rows of the prefetched fragments
    skipped = None
    if mut == 'ragged_from_previous_fragment':
        if tiles == nfull or nfull < stride:
            raise ValueError('the owner of the ragged tile has no previous tile')
        rag = torch.arange(16 * nfull, M)
        Xf, dzf, yf = Xn.clone(), dz.clone(), y.clone()
        Xf[rag], dzf[rag], yf[rag] = Xn[rag - 16 * stride], dz[rag - 16 * stride], y[rag - 16 * stride]
    if mut == 'tile_twice_next_skipped':
        if nfull <= stride:
            raise ValueError('no wave runs two full tiles')
        skipped = torch.arange(16 * stride, 16 * stride + 16)   # wave 0 of workgroup 0: tile 0 twice, tile `stride` never
    u = Xf @ W1.t() + b1
    pos = (u > 0).to(d)
    t = (u * pos) @ W2r.t() + b2
    z = y + g_f * t
    _, tmean, trstd = ln_true(yf.float(), p['ln_w'], p['ln_b'])
    stats = torch.cat([tmean, trstd], 1)
    gp = pos
    if mut == 'gelu_grad_from_next_row':
        gp = torch.cat([pos[1:], pos[-1:]], 0)
    du = ((dzf * g_b) @ W2r) * gp
    dn = du @ W1
    xh = p['sign'].to(d)
    rstd = p['stats'][:, 1:].to(d)
    gw = dn * p['ln_w'].to(d)
    dy = dz + rstd * (gw - gw.mean(1, keepdim=True) - xh * (gw * xh).mean(1, keepdim=True))
    dnr = dn
    if skipped is not None:
        for out in (z, u, stats, dy, du):
            out[skipped] = 0.0
        dnr = dn.clone()
        dnr[skipped] = 0.0
        dnr[:16] *= 2.0
    dgamma = p['dgamma0'].to(d) + (dnr * xh).sum(0)
    dbeta = p['dbeta0'].to(d) + dnr.sum(0)
    bound = dnr.abs().sum(0)
    return dict(z=z, u=u, stats=stats, dy=dy, du=du, dn=dn, dgamma=dgamma, dbeta=dbeta, neg=u < 0,
                dgamma_bound=p['dgamma0'].abs().to(d) + bound, dbeta_bound=p['dbeta0'].abs().to(d) + bound)


_REFERENCES = {}


def reference(p, drop=None):
    """The float64 model of a problem (computed once per problem and ``drop``, shared, never modified) in the formats the test compares in: z, dy fp32 (the model is exact in fp32: asserted
    for z; dy see ``dy_exact``), u fp16 and du bf16 (asserted representable), stats / dgamma / dbeta float64; ``neg``: the elements of
    (u, du) whose pre-activation is negative; ``dgamma_exact`` / ``dbeta_exact``: the elements below the reduction bound."""
    K, kind = p['K'], p['kind']
    key = (K, p['H'], p['M'], kind, drop)
    if key in _REFERENCES:
        return _REFERENCES[key]
    r = _model(p, drop)
    assert representable(r['u'].float(), F16) and representable(r['du'].float(), BF16), 'u or du is not representable in 16 bits'
    assert torch.equal(r['z'].float().double(), r['z']), 'z is not exact in fp32'
    emu = dy_fp32(p, r['dn'])
    out = dict(z=r['z'].float(), u=r['u'].to(F16), stats=r['stats'], dy64=r['dy'], dy=r['dy'].float(), du=r['du'].to(BF16), neg=r['neg'],
               dgamma=r['dgamma'], dbeta=r['dbeta'], dgamma_exact=r['dgamma_bound'] < EXACT_LIMIT, dbeta_exact=r['dbeta_bound'] < EXACT_LIMIT,
               dgamma_bound=r['dgamma_bound'], dbeta_bound=r['dbeta_bound'], u_min_abs=float(r['u'].abs().min()), u_max=float(r['u'].abs().max()),
               dn_max=float(r['dn'].abs().max()), dy_exact=bool(K == 64 and kind == 'plain' and torch.equal(emu.double(), r['dy'])),
               dy_emulation_equal=torch.equal(emu.double(), r['dy']))
    _REFERENCES[key] = out
    return out


def mutate(p, name, drop=None):
    """the float64 model with one defect (``MUTATIONS``) -> z, u, stats, dy, du, dgamma, dbeta (float64); ValueError where the problem's
    geometry has no such case"""
    assert name in MUTATIONS
    return _model(p, drop, name)
