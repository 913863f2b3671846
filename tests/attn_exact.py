"""Operands on which the forward of the partition attention core (csrc/k_attn.hip, routed by csrc/attn_route.hpp) has NO rounding error, in
any precision mode, kernel family and summation order, its float64 reference, and a per-element bound for the backward that is derived from
that reference -- so that tests/test_attn_exact_gpu.py compares O for equality and dq / dk / dv against a bound without a free constant.

Softmax is not exact arithmetic; a tie pattern makes it exact.  The kernels scale the score in fp32 after the MFMA, form
``e = exp(s - mx)``, ``inv = 1 / sum`` and pack ``e * inv``.  If the best scores of every query tie at exactly 0 over 2^k keys and every
other score lies far below, then mx = 0, the tied e are exp(0) = 1, sum = 2^k, inv = 2^-k, P = 2^-k (a bf16 and an fp16 number) and O is a
dyadic average of the tied values.  A padded key that leaks into the softmax has score 0: it joins the tie and turns 2^-k into
1 / (2^k + 1) in every element of the row.

Construction, per (partition, head), every choice drawn afresh (``_head``); n = ph pw tokens:

* codes: a Hadamard matrix of order d (Sylvester for 32, Paley I with q = d - 1 for 12 / 20 / 24), normalised so that row 0 and column 0
  are all ones: rows 1 .. d-1 are orthogonal to each other and sum to zero.  NU = 4 of them, drawn at random, are noise rows h_u, the
  others group codes h_g.
* the n tokens fall into groups whose sizes are powers of two <= 16 (``group_sizes``: n // 16 groups of 16 and the binary digits of the
  rest, then the smallest group split twice so that small ties exist everywhere), scattered over the token positions by a random
  permutation: tile order carries no structure.
* key of token j of group g: k_j = A h_g - BETA 1 + ETA sum_u eps_ju h_u, eps in +-1 and distinct per token of a group (2^NU = 16
  patterns).  Query i targets a group t(i): q_i = A h_t(i) + GAMMA 1, BETA GAMMA = A^2.  By orthogonality q_i . k_j = A^2 d [t(i) = g] -
  BETA GAMMA d: exactly 0 on the target group and -A^2 d elsewhere, every partial sum a multiple of ETA far below 2^24.  A = 6, BETA = 2,
  GAMMA = 18, ETA = 1/2: q in {12, 24}, k in [2, 6] or [-10, -6] (multiples of 1/2, at most 5 significant bits).  The scaled gap A^2 sqrt(d)
  is 124.7 at d = 12: exp(-gap) < 2^-149 is ZERO in fp32, denormals flushed or not, so the other keys contribute exactly nothing to the
  sum, to O or to the backward.  (Merely below half an ulp is not enough: with A = 3 the probabilities of the other keys were 1e-19, and the
  bf16 MFMA of P V, which does not round its sum to nearest, returned 2 - 2^-23 for 2 - 1e-19 on an MI355X.)  ETA < (A - BETA) / NU keeps
  the sign of a key coordinate the same inside a group (see the backward bound below).  Every group is the target of at least two queries.
* values: v_j = vbar_g + sigma_j w_g e_c: vbar_g in +-{1, 2} except +-1.5 at ONE coordinate c = c_g, where w_g = +-0.5 and sigma_j = +-1
  is balanced over the group: every v_jc is in +-{1, 2}, never zero, and O = vbar_g is never zero either.  Groups of one token: sigma = +1.
* dO in +-{1, 2, 3}; at c_t(i) in +-{1, 2}, its sign alternating over the queries of a group; the other signs are chosen coordinate by
  coordinate so that |D_i| = |dO_i . mean(v)| <= 6.

Why the structure in v and dO.  dP_ij - D_i = sigma_j x_i with x_i = dO_i,c w in +-{0.5, 1}, so dS_ij = sigma_j x_i 2^-k scale: a power of
two times scale = d^-1/2.  (1) The kernels' D carries the error of exp (and of log in lse) that the model of ``simulate`` does not: a
relative delta of a few 1e-7 in P moves dq by delta D scale mean_j(k_j), which |D| <= 6 keeps below the fp32 floor.  (2) The bf16 rounding of
dS is then ONE number per head dimension (``ds_rounding``: 0.03 u at d = 24 and 32), and the bf16 rounding of a stored dq / dk meets a
reference that is at most half (dq: same-signed keys, balanced sigma) or strictly less than (dk: alternating x) the sum of magnitudes that
the bound adds to it: the clean model stays within half of every bound by construction, not by the luck of a seed.

Backward bound, per element, u = 2^-8 (unit roundoff of bf16's 8 significant bits), floor = ``linear_exact.close_fp32``'s
(2e-6 + 5e-6 max|ref| + 2e-5 |ref|, max over the tensor dq, dk or dv):
    mode f32, every family                       floor
    family 1 (register-direct), 16-bit modes     floor: attn_bwd_q_kernel / attn_bwd_kv_kernel load fp32 operands (ld_head4 / ld_head1) and
                                                 feed them, P and dS unrounded to v_mfma_f32_16x16x4f32 (mfma16) whatever the mode
    families 2 and 3, 16-bit modes               dq: floor + u sum_j |dS_ij| |k_jc|;  dk: floor + u sum_i |dS_ij| |q_ic|;  dv: floor (P packs
                                                 exactly); the operands themselves pack exactly
    a tensor written as bf16 (family 3)          + u |ref|

``simulate`` is a float64 model that rounds where the kernels pack (e and P to fp32, P to the tile format, dS and P to bf16 in the backward,
O and dqkv to their 16-bit storage) and takes the mutations of ``MUTATIONS``.  tests/test_attn_exact_cpu.py checks every claim above on the
generated values, and that each mutation is seen."""
import functools
import math

import numpy as np
import torch

from linear_exact import representable

A, BETA, GAMMA, ETA, NU = 6.0, 2.0, 18.0, 0.5, 4
MAX_GROUP, SPLITS = 16, 2
U = 2.0 ** -8
LIMIT = float(2 ** 24)
D_MAX = 6.0                              # |D_i|
RTOL, ATOL, ATOL_SCALE = 2e-5, 2e-6, 5e-6     # linear_exact.close_fp32
MUTATIONS = ('pad_key', 'drop_key', 'swap_v_rows', 'head_v', 'mask24')
F64 = torch.float64


# ---- codes ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hadamard(d):
    """Hadamard matrix of order d as a float64 numpy array, row 0 and column 0 all ones"""
    if d & (d - 1) == 0:
        H = np.ones((1, 1))
        while H.shape[0] < d:
            H = np.block([[H, H], [H, -H]])
    else:
        q = d - 1
        assert q % 4 == 3 and all(q % f for f in range(2, int(q ** 0.5) + 1)), f'no Paley I construction for order {d}'
        squares = {(x * x) % q for x in range(1, q)}
        chi = np.array([0] + [1 if x in squares else -1 for x in range(1, q)], dtype=np.float64)
        Q = chi[(np.arange(q)[None, :] - np.arange(q)[:, None]) % q]
        S = np.zeros((d, d))
        S[0, 1:], S[1:, 0], S[1:, 1:] = 1.0, -1.0, Q
        H = np.eye(d) + S
        H = H * H[0][None, :]                # column signs: row 0 becomes ones
        H = H * H[:, 0][:, None]             # row signs: column 0 becomes ones
    assert np.array_equal(H @ H.T, d * np.eye(d)) and (H[0] == 1).all() and (H[:, 0] == 1).all()
    return H


def group_sizes(n, gmax, splits=SPLITS):
    """n as a sum of powers of two <= MAX_GROUP, at most gmax terms: n // 16 sixteens and the binary digits of the rest, then the smallest
    group larger than one split in two, ``splits`` times (4 splits leave two groups of ONE token in a partition of 16)"""
    sizes = [MAX_GROUP] * (n // MAX_GROUP) + [1 << b for b in range(3, -1, -1) if (n % MAX_GROUP) >> b & 1]
    if len(sizes) > gmax:
        raise ValueError(f'{n} tokens need {len(sizes)} groups of at most {MAX_GROUP}; {gmax} codes')
    for _ in range(splits):
        big = [s for s in sizes if s > 1]
        if not big or len(sizes) >= gmax:
            break
        s = min(big)
        sizes.remove(s)
        sizes += [s // 2, s // 2]
    return sorted(sizes, reverse=True)


def _head(n, d, rng, splits):
    """one (partition, head): q, k, v, dO [n, d] as float64 numpy arrays, the group of every token, the target group of every query, the
    group sizes, and two tokens of different groups"""
    H = hadamard(d)
    rows = rng.permutation(np.arange(1, d))
    noise, codes = H[rows[:NU]], H[rows[NU:]]
    sizes = group_sizes(n, len(codes), splits)
    G = len(sizes)
    assert n >= 2 * G
    order = rng.permutation(n)                                   # token positions, group after group
    group, sigma, eps = np.empty(n, dtype=np.int64), np.ones(n), np.empty((n, NU))
    at = 0
    for g, s in enumerate(sizes):
        tok = order[at:at + s]
        at += s
        group[tok] = g
        if s > 1:
            sigma[tok] = rng.permutation(np.repeat([1.0, -1.0], s // 2))
        pat = rng.choice(1 << NU, size=s, replace=False)         # distinct per token of the group
        eps[tok] = ((pat[:, None] >> np.arange(NU)[None, :]) & 1) * 2.0 - 1.0
    k = A * codes[group] - BETA + ETA * (eps @ noise)
    target = np.concatenate([np.repeat(np.arange(G), 2), rng.integers(0, G, size=n - 2 * G)])
    target = target[rng.permutation(n)]
    q = A * codes[target] + GAMMA
    # values
    vbar = rng.choice([1.0, 2.0], size=(G, d)) * rng.choice([1.0, -1.0], size=(G, d))
    c_g, w_g = rng.integers(0, d, size=G), 0.5 * rng.choice([1.0, -1.0], size=G)
    vbar[np.arange(G), c_g] = 1.5 * rng.choice([1.0, -1.0], size=G)
    v = vbar[group].copy()
    v[np.arange(n), c_g[group]] += sigma * w_g[group]
    vmean = np.stack([v[group == g].mean(0) for g in range(G)])  # vbar, except for groups of one token
    # dO: magnitudes at random; x_i = dO_i,c w alternates in sign over the queries of a group; the other signs keep |D| small
    do = rng.choice([1.0, 2.0, 3.0], size=(n, d))
    ct = c_g[target]
    do[np.arange(n), ct] = rng.choice([1.0, 2.0], size=n)
    nth = np.zeros(n)
    for g in range(G):
        i = np.nonzero(target == g)[0]
        nth[i] = np.arange(len(i))
    do[np.arange(n), ct] *= np.where(nth % 2 == 0, 1.0, -1.0) * np.sign(w_g[target])
    run = do[np.arange(n), ct] * vmean[target, ct]
    for c in rng.permutation(d):
        i = np.nonzero(ct != c)[0]
        term = do[i, c] * vmean[target[i], c]                    # do is still positive here
        flip = np.where(run[i] == 0, rng.choice([1.0, -1.0], size=len(i)), -np.sign(run[i]) * np.sign(term))
        do[i, c] *= flip
        run[i] += do[i, c] * vmean[target[i], c]
        assert (np.abs(run) <= D_MAX).all()
    j1 = int(order[0])
    j2 = int(order[-1])
    assert group[j1] != group[j2]
    return q, k, v, do, group, target, np.array(sizes), (j1, j2)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def token_rows(B, nH, nW, ph, pw, window):
    """[partitions, n] row of the [B H W] map of token t of partition p (csrc/attn_common.hpp: token_row), partitions in (b, py, px) order"""
    H, W = nH * ph, nW * pw
    b, py, px = np.meshgrid(np.arange(B), np.arange(nH), np.arange(nW), indexing='ij')
    b, py, px = (a.reshape(-1, 1) for a in (b, py, px))
    t = np.arange(ph * pw)[None, :]
    ty, tx = t // pw, t % pw
    if window:
        return (b * H + py * ph + ty) * W + px * pw + tx
    return (b * H + py + ty * nH) * W + px + tx * nW


def to_image(x, rows, M):
    """[partitions, heads, n, e] -> [M, heads e]: head h owns the columns [h e, (h + 1) e)"""
    NP, heads, n, e = x.shape
    out = torch.zeros((M, heads * e), dtype=x.dtype)
    out[torch.as_tensor(rows).reshape(-1)] = x.permute(0, 2, 1, 3).reshape(NP * n, heads * e)
    return out


def from_image(y, rows, heads):
    """[M, heads e] (any leading shape) -> [partitions, heads, n, e]"""
    NP, n = rows.shape
    y = y.reshape(-1, y.shape[-1])
    return y[torch.as_tensor(rows).reshape(-1)].reshape(NP, n, heads, -1).permute(0, 2, 1, 3)


# ---- reference -----------------------------------------------------------------------------------------------------------------------------
def attention(q, k, v, do, scale):
    """float64, [.., n, d] each: the definitions themselves -> S (scaled), P, O, lse, dP, D, dS (scale included, as the kernels pack it), dq,
    dk, dv"""
    S = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(S, -1, keepdim=True)
    P = torch.exp(S - lse)
    O = P @ v
    dP = do @ v.transpose(-1, -2)
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D) * scale
    return dict(S=S, P=P, O=O, lse=lse.squeeze(-1), dP=dP, D=D.squeeze(-1), dS=dS, dq=dS @ k, dk=dS.transpose(-1, -2) @ q, dv=P.transpose(-1, -2) @ do)


@functools.lru_cache(maxsize=4)
def _core(part, d, heads, NP, seed, splits=SPLITS):
    n = part[0] * part[1]
    rng = np.random.default_rng([seed, part[0], part[1], d, heads, NP, splits])
    hs = [[_head(n, d, rng, splits) for _ in range(heads)] for _ in range(NP)]
    stack = lambda i, dt=F64: torch.as_tensor(np.stack([np.stack([h[i] for h in row]) for row in hs])).to(dt)          # noqa: E731
    q, k, v, do = (stack(i) for i in range(4))
    c = dict(q=q, k=k, v=v, do=do, group=stack(4, torch.int64), target=stack(5, torch.int64), sizes=[[h[6] for h in row] for row in hs],
             swap=stack(7, torch.int64), scale=float(d) ** -0.5, n=n, d=d, heads=heads, NP=NP, seed=seed, part=part, splits=splits)
    c['ref'] = attention(q, k, v, do, c['scale'])
    size_of = torch.stack([torch.stack([torch.as_tensor(h[6])[torch.as_tensor(h[4])] for h in row]) for row in hs])    # of every token's group
    c['tie'] = torch.stack([torch.stack([torch.as_tensor(h[6])[torch.as_tensor(h[5])] for h in row]) for row in hs])     # of every query's tie
    c['key_tie'] = size_of
    return c


@functools.lru_cache(maxsize=6)
def problem(part, d, heads=2, B=1, window=True, seed=0, grid=(2, 2), splits=SPLITS):
    """qkv [B, H, W, 3C] and dO [B, H, W, C] (fp32, CPU; H = grid[0] ph, W = grid[1] pw) with the float64 reference, in partition space
    ([partitions, heads, n, .]; ``rows`` maps it to the image) and as image tensors (``O``, ``lse``, ``dqkv``: fp32 casts).  Cached per shape,
    shared by the three precision modes, never modified; window and grid addressing share the partition-space values."""
    nH, nW = grid
    ph, pw = part
    c = _core(tuple(part), d, heads, B * nH * nW, seed, splits)
    rows = token_rows(B, nH, nW, ph, pw, window)
    M, H, W, C = B * nH * ph * nW * pw, nH * ph, nW * pw, heads * d
    assert np.array_equal(np.sort(rows.reshape(-1)), np.arange(M))
    r = c['ref']
    img = lambda x: to_image(x, rows, M)                                                                                 # noqa: E731
    p = dict(c, part=tuple(part), B=B, H=H, W=W, C=C, window=window, rows=rows,
             qkv=img(torch.cat([c['q'], c['k'], c['v']], -1)).float().view(B, H, W, 3 * C), dO=img(c['do']).float().view(B, H, W, C),
             O=img(r['O']).float().view(B, H, W, C), lse=img(r['lse'].unsqueeze(-1)).float().view(B, H, W, heads),
             dqkv=img(torch.cat([r['dq'], r['dk'], r['dv']], -1)).float().view(B, H, W, 3 * C))
    return p


# ---- the conditions that make the claim true -----------------------------------------------------------------------------------------------
def ds_rounding(d):
    """relative error, in units of u, of the bf16 rounding of a power of two times d^-1/2: every non-negligible dS of a problem"""
    s = torch.tensor([float(d) ** -0.5], dtype=F64)
    return float(((s.float().bfloat16().double() - s).abs() / s).item()) / U


def bounds(p):
    """{condition: (holds, the figure)} -- every one must hold, on every row: asserted by the CPU test and again by the GPU test"""
    return _bounds(p['part'], p['d'], p['heads'], p['NP'], p['seed'], p['splits'])


@functools.lru_cache(maxsize=None)
def _bounds(part, d, heads, NP, seed, splits):
    p = _core(part, d, heads, NP, seed, splits)
    q, k, v, do, r, n = p['q'], p['k'], p['v'], p['do'], p['ref'], p['n']
    both = lambda t: representable(t.float(), torch.bfloat16) and representable(t.float(), torch.float16) and torch.equal(t.float().double(), t)   # noqa: E731
    raw = q @ k.transpose(-1, -2)
    tied = p['group'].unsqueeze(2) == p['target'].unsqueeze(3)                            # [NP, heads, query, key]
    gap = float(A * A * d * p['scale'])
    Pt = torch.where(tied, r['P'], torch.zeros((), dtype=F64)).float()
    score_sum = float((q.abs() @ k.abs().transpose(-1, -2)).max())
    dp_sum = float((do.abs() @ v.abs().transpose(-1, -2)).max())
    x = (r['dS'] / p['scale']).abs()                                                       # 2^-k |dP - D|
    mant = torch.frexp(x)[0]
    pow2 = bool((((mant - 0.5).abs() < 1e-12) | ((mant - 1.0).abs() < 1e-12) | (x < 1e-40)).all()) and bool((x[~tied] < 1e-40).all())
    return {
        'operands are bf16 and fp16 numbers': (both(q) and both(k) and both(v) and both(do), None),
        'v and dO are never zero': (bool((v != 0).all() and (do != 0).all()), None),
        'partial sums of every score < 2^24, in units of ETA': (score_sum / ETA < LIMIT, score_sum / ETA),
        'partial sums of dP < 2^24, in units of 1/2': (2 * dp_sum < LIMIT, 2 * dp_sum),
        'tied scores are exactly 0': (bool((raw[tied] == 0).all()), None),
        'the other scores are exactly -A^2 d': (bool((raw[~tied] == -A * A * d).all()), None),
        'n exp(-gap) < 2^-26': (n * math.exp(-gap) < 2.0 ** -26, n * math.exp(-gap)),
        'exp(-gap) is zero in fp32: gap > 150 ln 2': (gap > 150 * math.log(2.0) and float(torch.exp(torch.tensor(-gap, dtype=F64)).float()) == 0.0, gap),
        'every query has a tie of 2^k keys': (bool((tied.sum(-1) == p['tie']).all()) and bool(((p['tie'] & (p['tie'] - 1)) == 0).all()), None),
        'P is a bf16 and fp16 number': (both(Pt.double()) and bool((Pt[tied] * p['tie'].unsqueeze(-1).expand_as(tied)[tied] == 1).all()), None),
        'O is a bf16 and fp16 number, never zero': (both(r['O'].float().double()) and bool((r['O'].float() != 0).all()), None),
        'dS is +- a power of two times scale on the tie, nothing elsewhere': (pow2, None),
        '|D| <= 6': (float(r['D'].abs().max()) <= D_MAX + 1e-9, float(r['D'].abs().max())),
        'dS rounds to bf16 within u / 4 (d = 24, 32: the head dimensions of the 16-bit contractions)': (d not in (24, 32) or ds_rounding(d) < 0.25, ds_rounding(d)),
    }


def family_of(code):
    return code // 10000


def tolerance(p, mode, family):
    """{'dq' | 'dk' | 'dv': per-element bound, [partitions, heads, n, d] float64} for a backward of this kernel family in this precision mode"""
    r = p['ref']
    tol = {t: ATOL + ATOL_SCALE * float(r[t].abs().max()) + RTOL * r[t].abs() for t in ('dq', 'dk', 'dv')}
    if mode != 'f32' and family in (2, 3):
        tol['dq'] = tol['dq'] + U * (r['dS'].abs() @ p['k'].abs())
        tol['dk'] = tol['dk'] + U * (r['dS'].abs().transpose(-1, -2) @ p['q'].abs())
        if family == 3:
            tol = {t: tol[t] + U * r[t].abs() for t in tol}
    return tol


# ---- a model of the kernels ------------------------------------------------------------------------------------------------------------------
def _rnd(t, dtype):
    return t if dtype is None else t.to(torch.float32).to(dtype).to(F64)


def simulate(p, fmt, family=3, mutation=None):
    """float64 arithmetic, rounded where the kernels round: e, P and dS are fp32 numbers; families 2 and 3 in a 16-bit mode (fmt 'bf16' |
    '16f') pack P to bf16 | fp16 for P V and P, dS to bf16 in the backward; family 3 stores O as bf16 | fp16 (``O16``) and dq, dk, dv as bf16.
    -> O, O16, lse, dq, dk, dv in partition space.  mutation: one of MUTATIONS --
      pad_key      one padded key (k = v = 0, score 0) is admitted to every softmax
      drop_key     the last real key of every partition is masked
      swap_v_rows  the row map of the V operand swaps two tokens of different groups (a swap applied to every operand and to the stores alike
                   would be invisible: attention is equivariant under a permutation of a partition's tokens)
      head_v       head 1 reads the v of head 0
      mask24       d = 24, 16-bit tiles: the q fragment keeps its lanes 24 .. 31, which hold the first 8 values of the token's k, against the
                   first 8 values of v behind the streamed k fragment"""
    assert fmt in ('f32', 'bf16', '16f') and family in (1, 2, 3) and mutation in (None,) + MUTATIONS
    tiles = fmt != 'f32' and family in (2, 3)
    fwd_t = {'bf16': torch.bfloat16, '16f': torch.float16}[fmt] if tiles else None
    bwd_t = torch.bfloat16 if tiles else None
    q, k, v, do, scale = p['q'], p['k'], p['v'].clone(), p['do'], p['scale']
    NP, heads, n, d = q.shape
    if mutation == 'head_v':
        assert heads > 1
        v[:, 1] = v[:, 0]
    if mutation == 'swap_v_rows':
        for pi in range(NP):
            for h in range(heads):
                j1, j2 = p['swap'][pi, h].tolist()
                v[pi, h, [j1, j2]] = v[pi, h, [j2, j1]]
    if mutation == 'pad_key':
        zero = torch.zeros((NP, heads, 1, d), dtype=F64)
        k, v = torch.cat([k, zero], 2), torch.cat([v, zero], 2)
    raw = q @ k.transpose(-1, -2)
    if mutation == 'mask24':
        assert d == 24
        raw = raw + p['k'][..., :8] @ v[..., :8].transpose(-1, -2)
    S = raw * scale
    if mutation == 'drop_key':
        S[..., n - 1] = -math.inf
    f32 = lambda t: t.to(torch.float32).to(F64)                                            # noqa: E731
    mx = S.max(-1, keepdim=True).values
    e = f32(torch.exp(S - mx))
    tot = f32(e.sum(-1, keepdim=True))
    P = f32(e / tot)
    lse = f32(mx + torch.log(tot))
    O = _rnd(P, fwd_t) @ v
    O16 = _rnd(O, {'bf16': torch.bfloat16, '16f': torch.float16}.get(fmt)) if family == 3 and fmt != 'f32' else None
    pr = f32(torch.exp(S - lse))
    dP = do @ v.transpose(-1, -2)
    D = (pr * dP).sum(-1, keepdim=True)
    dS = _rnd(f32(pr * (dP - D) * scale), bwd_t)
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q, _rnd(pr, bwd_t).transpose(-1, -2) @ do
    out_t = torch.bfloat16 if family == 3 and fmt != 'f32' else None
    return dict(O=O, O16=O16, lse=lse.squeeze(-1), dq=_rnd(dq, out_t), dk=_rnd(dk[..., :n, :], out_t), dv=_rnd(dv[..., :n, :], out_t))


def worst(got, ref, tol, p):
    """(largest |got - ref| / tol, a sentence that names the element): [partitions, heads, n, d] each"""
    ratio = (got.double() - ref).abs() / tol
    i = int(ratio.argmax())
    pi, h, t, c = np.unravel_index(i, ratio.shape)
    return float(ratio.reshape(-1)[i]), (f'partition {pi}, head {h}, token {t} (image row {int(p["rows"][pi, t])}), channel {c}: got {float(got[pi, h, t, c])!r}, '
                                         f'reference {float(ref[pi, h, t, c])!r}, bound {float(tol[pi, h, t, c]):.3e}; the query\'s tie has {int(p["tie"][pi, h, t])} '
                                         f'keys, the key\'s group {int(p["key_tie"][pi, h, t])}')
