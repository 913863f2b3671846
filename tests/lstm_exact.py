"""Operands on which the ConvLSTM sequence kernels (csrc/k_lstm.hip, routed by csrc/lstm_route.hpp) and the per-timestep cell kernels leave
NO rounding error in anything discrete, in any precision mode, and the float64 references -- so that tests/test_lstm_exact_gpu.py compares
gates, the whole c history, the gate gradients, dh0 and dc0 with ``torch.equal``, and h against a derived absolute bound.  An LSTM has
transcendentals; what the tie patterns were for the softmax of tests/attn_exact.py, SATURATED GATES are here.

Forward (``forward_problem`` / ``forward_model``).  common.hpp: sigmoidf_(x) = rcp(1 + exp2(-x log2 e)); k_lstm.hip: tanh_ is tanhf (mode f32)
or 2 sigmoidf_(2x) - 1 (16-bit modes, streamed kernels).  For x >= S = 128 the exponential underflows to 0 and rcp(1) = 1; for x <= -128
exp2(>= 184) = inf and rcp(inf) = 0; the tanh variants give exactly +-1.  Every pre-activation of every gate, row, channel and timestep has
magnitude >= 128, so f, i, o are exactly 0 or 1, g is exactly +-1, c_t = f c + i g is a small integer (exact), and h_t = o tanh(c_t) is the only
output with a function-evaluation error.  The gates re-quantise every step: neither that error, nor the bf16 / fp16 rounding of h in the A
tile, nor the summation order of the contraction can flip a gate, and nothing accumulates through time.  ONE float64 recurrence is the
reference of all three precision modes and all families.
  pre = W_x x + W_h h + b with three scales, so that h decides gates (which is what tests the recurrent weights):
  * |W_x| = 4096, one nonzero per gate row: the four gate rows of channel ch read x column ``xcol(C)[ch]`` (a permutation, never ch itself);
  * |W_h| = 512, three nonzeros per row at random columns with random signs;
  * |b| in {128, 256}, both signs; x in {0, +-1, +-2}; incoming state h0 in {0, +-0.75, +-1}, c0 in {0, +-1, +-2} (exact in bf16 and fp16).
  The generator runs the float64 recurrence and sets an x to 0 wherever all four gate rows it feeds keep the margin without it: where x is 0
  and the h part is not, h decides the gate (``decided`` == 1); where both are 0, the bias does (2); else x (0).
  THE MARGIN RULE.  |pre| >= 128 + the largest perturbation rounding can cause, per element:
      need = 128 + sum_j |W_h[row, j]| (2^-8 |h_j| + H_BOUND)
  2^-8 |h| bounds the rounding of h to bf16 (2^-9 relative) or fp16 with a factor 2 to spare, H_BOUND is the function error of h (below); the
  spare half (>= 2^-9 * 512 |h| per term) dwarfs the fp32 accumulation error of the contraction (<= 8 ulp of 2^14 = 2^-7).  At most
  1536 / 256 = 6.  Where every h_j a row reads is exactly 0 there is no perturbation, and |pre| = |b| = 128 is allowed.  An x that is not 0
  contributes >= 4096 against at most 1536 + 256 from the rest.
  For the hoisted and streamed routes the test passes gx = x W_x^T + b itself (``gx``: integers below 2^14, exact), which isolates the
  sequence kernel from the projection GEMM that the Linear suites cover.

THE h BOUND.  Reference: float64 o tanh(c), |c| <= 6 an integer, o in {0, 1}.  The fast formula is th = 2 rcp(1 + e) - 1, e = exp2(a),
a = fl(-2c log2e): the argument carries two roundings (the constant, the product), |da| <= |a| 2^-23, hence a relative error of e of at most
ln2 |a| 2^-23 + 2^-23 (v_exp_f32: 1 ulp) = (1 + 2|c|) 2^-23.  s = rcp(fl(1 + e)): relative error <= (1 + 2|c|) 2^-23 e / (1 + e) + 2^-24 (the
sum) + 2^-23 (v_rcp_f32: 1 ulp); th = fl(2s - 1) adds half an ulp of a value below 1, 2^-25:
      |dth| <= 2 s [(1 + 2|c|) 2^-23 e / (1 + e) + 3 * 2^-24] + 2^-25.
  Largest at c = 1 (s = 0.881, e / (1 + e) = 0.119): 7.05 * 2^-24; c = 0: 4.5 * 2^-24; c <= -1: s <= 0.12, below 2.5 * 2^-24.  H_BOUND is the
  maximum of this expression over |c| <= 6 (``tanh_error_bound``), 4.2e-7, absolute; tanhf (2 ulp) is held to the same.  The smallest effect
  a discrete error can have on h is tanh(6) - tanh(5) = 7.8e-5, 180 times the bound.

Backward (``backward_problem`` / ``backward_model``).  Saturated gates have zero derivative, so the forward operands are useless here.  The
backward entries are pure functions of (dh_seq, dc_last, gates, cbuf, W), and the test feeds them CONSTRUCTED saved tensors:
  f, i, o in {0, 1/2, 1} (f (1 - f) in {0, 1/4}), g in {0, +-1}, cbuf in {0, +-32} (tanh is exactly 0 or +-1), dh_seq and dc_last in
  {0, +-1, +-2}, W_h with two nonzeros per row from +-{1/2, 1} (not the forward's W: the entry takes W independently; the W_x half holds 3.0
  everywhere, which the backward must never read).  Every factor is 0 or a power of two and every value is dyadic.  The float64 model rounds
  the dgates tile to bf16 (round to nearest even) exactly where the 16-bit kernels do (a_elem / to_bf16 of k_lstm.hip); the values entering
  that rounding are exact in fp32, so the model's rounding is the device's bit for bit, and dgates, dh0, dc0 are compared for equality in every
  mode.  ``backward_exactness`` proves, for the committed operands, that every modelled intermediate is representable in fp32 and that
  every partial sum of dgates W_h in ANY order is: all terms of a timestep are multiples of one quantum q, and sum |terms| < 2^24 q (the span
  argument of linear_exact).
  The gates are themselves act(pre) of three-valued pre-activations S (w x + beta), w in +-{1, 2}, beta in {-1, 0, 1}, x in {0, +-1, +-2}:
  the G16 path keeps its fp16 gates in an opaque layout only a forward launch can write, so ``g16`` holds forward inputs (W_h = 0; gx on
  hoisted and streamed routes, a diagonal W_x -- shifted by 7 columns per gate, ``g16_xcol`` -- plus bias on fused ones) whose gates ARE the
  constructed tensor ("three-valued" is what matters: multiples of S, 0 among them).  sigmoid(0) = 1/2 and tanh(0) = 0 are observed by the
  probe test of the GPU module.  The cbuf handed to the backward is the constructed one, never the forward's.

``MUTATIONS``: defects applied inside the models; tests/test_lstm_exact_cpu.py shows that each changes a discrete output."""
import functools
import math

import torch

S = 128.0
WX_MAG, WH_MAG = 4096.0, 512.0
U16 = 2.0 ** -8
C_CAP = 6


def tanh_error_bound(c):
    """|error| of th = fl(2 rcp(fl(1 + exp2(fl(-2c log2e)))) - 1) with 1-ulp v_exp_f32 / v_rcp_f32: the derivation of the docstring"""
    e = math.exp(-2 * c)
    s = 1 / (1 + e)
    return 2 * s * ((1 + 2 * abs(c)) * 2.0 ** -23 * e / (1 + e) + 3 * 2.0 ** -24) + 2.0 ** -25


H_BOUND = max(tanh_error_bound(c) for c in range(-C_CAP, C_CAP + 1))
SENTINEL = -77.0                 # guard elements and the slots a call must leave alone (exact in fp32, bf16 and fp16)
GATE_NAMES = ('f', 'i', 'o', 'g')
DECIDED_BY = ('x', 'h', 'bias')

FWD_MUTATIONS = ('gate_order', 'x_next_row', 'stale_h', 'swap_chunks', 'neighbour_group', 'bias_ch16', 'row_leak')
BWD_MUTATIONS = ('slot0_read', 'wh_block_transposed')
MUTATIONS = FWD_MUTATIONS + BWD_MUTATIONS


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _pick(values, shape, g, probs=None):
    v = torch.tensor(values, dtype=torch.float64)
    if probs is None:
        return v[torch.randint(0, len(values), shape, generator=g)]
    n = 1
    for s in shape:
        n *= s
    idx = torch.multinomial(torch.tensor(probs, dtype=torch.float64), n, replacement=True, generator=g)
    return v[idx].view(shape)


def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g).double() * 2 - 1


def xcol(C):
    """the x column the four gate rows of channel ch read: a permutation of the channels without a fixed point (5 is coprime to every C)"""
    return (5 * torch.arange(C) + 3) % C


def _sparse_rows(rows, cols, k, mags, g):
    """[rows, cols] with k nonzeros per row at random distinct columns, magnitudes from ``mags``, random signs"""
    w = torch.zeros((rows, cols), dtype=torch.float64)
    at = torch.rand((rows, cols), generator=g).argsort(1)[:, :k]
    w.scatter_(1, at, _pick(mags, (rows, k), g) * _signs((rows, k), g))
    return w


# ------------------------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------------------------
def _need(h, Wh):
    """the margin rule, per (row, gate row): 128 + sum_j |W_h| (2^-8 |h_j| + H_BOUND) over the h_j that are not exactly 0"""
    return S + (h.abs() * U16 + (h != 0).double() * H_BOUND) @ Wh.abs().t()


def _cell(pre, c):
    """pre [M, 4, C] saturated -> gates [M, 4, C], c, h (float64; the step functions ARE sigmoid / tanh there: the CPU test shows it)"""
    gates = (pre > 0).double()
    gates[:, 3] = gates[:, 3] * 2 - 1
    cn = gates[:, 0] * c + gates[:, 1] * gates[:, 3]
    return gates, cn, gates[:, 2] * torch.tanh(cn)


@functools.lru_cache(maxsize=None)
def forward_problem(C, M, T, state, seed=0):
    """-> dict: x [T,M,C], W [4C,2C], b [4C], h0, c0 [M,C] (zeros without ``state``), gx [T,M,4C] (fp32, the operands), pre [T,M,4,C],
    decided [T,M,4,C] (0 x, 1 h, 2 bias), need [T,M,4,C] and ref = forward_model(p): gates [T,M,4,C], c and h [T+1,M,C] (float64)."""
    g = _gen(1, C, M, T, int(state), seed)
    col = xcol(C)
    Wx = torch.zeros((4 * C, C), dtype=torch.float64)
    Wx[torch.arange(4 * C), col.repeat(4)] = WX_MAG * _signs((4 * C,), g)
    Wh = _sparse_rows(4 * C, C, 3, [WH_MAG], g)
    b = _pick([128., 256.], (4 * C,), g) * _signs((4 * C,), g)
    if state:
        h0, c0 = _pick([0., .75, -.75, 1., -1.], (M, C), g), _pick([0., 1., -1., 2., -2.], (M, C), g)
    else:
        h0, c0 = torch.zeros((M, C), dtype=torch.float64), torch.zeros((M, C), dtype=torch.float64)
    xc = _pick([1., 2.], (T, M, C), g) * _signs((T, M, C), g)
    x = torch.zeros((T, M, C), dtype=torch.float64)
    h, c = h0, c0
    pres, needs, decided = [], [], []
    for t in range(T):
        hp = h @ Wh.t()
        need = _need(h, Wh)
        keeps = ((hp + b).abs() >= need).view(M, 4, C).all(1)                        # [M, channel]: all four gate rows hold without x
        x[t][:, col] = torch.where(keeps, torch.zeros(()).double(), xc[t][:, col])
        pre = (x[t] @ Wx.t() + hp + b).view(M, 4, C)
        xpart = (x[t] @ Wx.t()).view(M, 4, C)
        decided.append(torch.where(xpart != 0, 0, torch.where(hp.view(M, 4, C) != 0, 1, 2)))
        pres.append(pre); needs.append(need.view(M, 4, C))
        _, c, h = _cell(pre, c)
    p = {'C': C, 'M': M, 'T': T, 'state': bool(state), 'x': x.float(), 'W': torch.cat([Wx, Wh], 1).float(), 'b': b.float(),
         'h0': h0.float(), 'c0': c0.float(), 'gx': (torch.einsum('tmc,nc->tmn', x, Wx) + b).float(),
         'pre': torch.stack(pres), 'need': torch.stack(needs), 'decided': torch.stack(decided)}
    p['ref'] = forward_model(p)
    return p


def forward_model(p, mutation=None):
    """the float64 recurrence on the operands of ``p``, with one defect of FWD_MUTATIONS if asked"""
    C, M, T = p['C'], p['M'], p['T']
    assert mutation is None or mutation in FWD_MUTATIONS
    W, b, x = p['W'].double(), p['b'].double(), p['x'].double()
    Wx, Wh = W[:, :C], W[:, C:].clone()
    if mutation == 'swap_chunks':                      # two 16-column chunks of W_h exchanged
        Wh[:, 0:16], Wh[:, 16:32] = W[:, C + 16:C + 32], W[:, C:C + 16]
    if mutation == 'neighbour_group':                  # the first W_h fragment (16 k) of every channel group taken from its neighbour's rows
        rows = torch.arange(4 * C)
        Wh[:, 0:16] = W[rows ^ 16, C:C + 16]
    if mutation == 'bias_ch16':                        # the bias of channel ch + 16
        b = b.view(4, C).roll(-16, 1).reshape(-1)
    # row M is the phantom lane of the ragged tile with unclamped loads: it reads row 0 of the next slab
    x = torch.cat([x, x.roll(-1, 0)[:, :1]], 1)
    hs, cs, gs = [torch.cat([p['h0'].double(), p['h0'][:1].double()])], [torch.cat([p['c0'].double(), p['c0'][:1].double()])], []
    for t in range(T):
        xt, hin = x[t], hs[t]
        if mutation == 'x_next_row' and t + 1 < T:     # the prefetched x_{t+1} in place of x_t on the last row
            xt = xt.clone()
            xt[M - 1] = x[t + 1, M - 1]
        if mutation == 'stale_h' and t >= 1:           # the other LDS buffer: the h of timestep t - 2
            hin = hs[t - 1]
        pre = (xt @ Wx.t() + hin @ Wh.t() + b).view(M + 1, 4, C)
        if mutation == 'gate_order':                   # i and o exchanged
            pre = pre[:, [0, 2, 1, 3]]
        gates, cn, hn = _cell(pre, cs[t])
        gs.append(gates); cs.append(cn); hs.append(hn)
    gates, c, h = torch.stack(gs), torch.stack(cs), torch.stack(hs)
    if mutation == 'row_leak':                         # the phantom row stored over row M - 1
        gates[:, M - 1], c[1:, M - 1], h[1:, M - 1] = gates[:, M], c[1:, M], h[1:, M]
    return {'gates': gates[:, :M].contiguous(), 'c': c[:, :M].contiguous(), 'h': h[:, :M].contiguous()}


def discrete_differs(a, b):
    return not (torch.equal(a['gates'], b['gates']) and torch.equal(a['c'], b['c']))


def explain_forward(p, t, m, gate, ch):
    """what decided a gate element in the reference: tells a reader which operand went astray"""
    by = DECIDED_BY[int(p['decided'][t, m, gate, ch])]
    return (f'timestep {t}, row {m}, channel {ch}, gate {GATE_NAMES[gate]}: the reference has pre = {float(p["pre"][t, m, gate, ch])!r}, decided by '
            f'{by} (x column {int(xcol(p["C"])[ch])} holds {float(p["x"][t, m, xcol(p["C"])[ch]])!r}, bias {float(p["b"][gate * p["C"] + ch])!r})')


# ------------------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------------------
def act3(pre):
    """[..., 4, C] three-valued pre-activations -> gates: sigmoid -> {0, 1/2, 1}, tanh -> {-1, 0, 1}"""
    gates = (torch.sign(pre) + 1) / 2
    gates[..., 3, :] = torch.sign(pre[..., 3, :])
    return gates


def g16_xcol(C):
    """the x column gate g of channel ch reads in the G16 forward inputs: the diagonal, shifted by 7 g -- the four gates of a channel see four
    different x elements, so their values are independent of each other"""
    return (torch.arange(C).view(1, C) + 7 * torch.arange(4).view(4, 1)) % C


@functools.lru_cache(maxsize=None)
def backward_problem(C, M, T, seed=0):
    """-> dict: gates [T,M,4,C], cbuf [T+1,M,C], dh_seq [T,M,C], dc_last [M,C], W [4C,2C] (fp32, the operands of the backward entry) and
    g16: x [T,M,C], W [4C,2C], b [4C], gx [T,M,4C] -- forward inputs (W_h = 0) whose gates are ``gates``"""
    g = _gen(2, C, M, T, seed)
    x3 = _pick([0., 1., -1., 2., -2.], (T, M, C), g, [.5, .125, .125, .125, .125])
    w = _pick([1., 2.], (4, C), g) * _signs((4, C), g)
    beta = _pick([-1., 0., 1.], (4, C), g, [.15, .7, .15])
    col = g16_xcol(C)                                                                 # [4, C]
    pre = S * (w * x3[:, :, col] + beta)                                              # [T, M, 4, C]
    Wf = torch.zeros((4 * C, 2 * C), dtype=torch.float64)
    Wf[torch.arange(4 * C), col.reshape(-1)] = S * w.reshape(-1)
    W = torch.full((4 * C, 2 * C), 3.0, dtype=torch.float64)
    W[:, C:] = _sparse_rows(4 * C, C, 2, [.5, 1.], g)
    return {'C': C, 'M': M, 'T': T, 'seed': seed, 'gates': act3(pre).float(), 'cbuf': _pick([0., 32., -32.], (T + 1, M, C), g, [.4, .3, .3]).float(),
            'dh_seq': _pick([0., 1., -1., 2., -2.], (T, M, C), g).float(), 'dc_last': _pick([0., 1., -1., 2., -2.], (M, C), g).float(),
            'W': W.float(), 'g16': {'x': x3.float(), 'W': Wf.float(), 'b': (S * beta).reshape(-1).float(), 'gx': pre.reshape(T, M, 4 * C).float()}}


def round_bf16(v):
    """round to nearest even, as to_bf16 of k_lstm.hip does -- on values that are exact in fp32 (asserted)"""
    f = v.float()
    assert torch.equal(f.double(), v), 'a value entering the bf16 rounding is not exact in fp32'
    return f.to(torch.bfloat16).double()


def gate_backward(dhv, dcn, gates, cp, ct):
    """the lane-local gate backward of one timestep (rnn.py:58-68): -> dgates [M, 4, C], dc flowing to t - 1, dc"""
    f, i, o, g = gates[:, 0], gates[:, 1], gates[:, 2], gates[:, 3]
    th = torch.tanh(ct)
    assert bool(((th.abs() == 1) | (th == 0)).all())                                  # float64 tanh(+-32) == +-1
    dc = dhv * o * (1 - th * th) + dcn
    d = torch.stack([dc * cp * f * (1 - f), dc * g * i * (1 - i), dhv * th * o * (1 - o), dc * i * (1 - g * g)], 1)
    return d, dc * f, dc


@functools.lru_cache(maxsize=None)
def backward_model(key, mode16, mutation=None, dh_seq=True, dc_last=True, zero_state=False):
    """float64 model of lstm_seq_bwd_kernel / lstm_seq_bwd_stream_kernel on backward_problem(*key).  mode16: the dgates tile that feeds
    dh_{t-1} = dgates_t W_h is rounded to bf16 (both 16-bit modes; the backward operands are bf16 in either).
    -> dgates [T,M,4C] as the fp32 output holds them (unrounded), dgates16 (the bf16 rows of the G16 path), dh0, dc0 [M,C], and per timestep
    the intermediates (dhv, dc, dgates, tile, dhr) that backward_exactness looks at"""
    p = backward_problem(*key)
    C, M, T = p['C'], p['M'], p['T']
    assert mutation is None or mutation in BWD_MUTATIONS
    gates, cbuf, Wh = p['gates'].double(), p['cbuf'].double(), p['W'].double()[:, C:].clone()
    if mutation == 'wh_block_transposed':              # W_h transposed within its first 16 x 16 block
        Wh[0:16, 0:16] = Wh[0:16, 0:16].t().clone()
    dcn = p['dc_last'].double() if dc_last else torch.zeros((M, C), dtype=torch.float64)
    dhr = torch.zeros((M, C), dtype=torch.float64)
    out, out16, steps = [None] * T, [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        cp = cbuf[t]
        if zero_state and t == 0 and mutation != 'slot0_read':
            cp = torch.zeros_like(cp)
        dhv = (p['dh_seq'][t].double() if dh_seq else 0) + dhr
        d, dcn, dc = gate_backward(dhv, dcn, gates[t], cp, cbuf[t + 1])
        d = d.reshape(M, 4 * C)
        tile = round_bf16(d) if mode16 else d
        dhr = tile @ Wh
        out[t], out16[t], steps[t] = d, round_bf16(d), {'dhv': dhv, 'dc': dc, 'dcn': dcn, 'd': d, 'tile': tile, 'dhr': dhr, 'Wh': Wh}
    return {'dgates': torch.stack(out), 'dgates16': torch.stack(out16), 'dh0': dhr, 'dc0': dcn, 'steps': steps}


def lowbit(v):
    """the smallest set bit over the nonzero elements of a dyadic float64 tensor (as a float), inf if all are 0"""
    s = v * 2.0 ** 40
    assert torch.equal(s, s.round()) and float(s.abs().max()) < 2.0 ** 62, 'not dyadic at 2^-40'
    n = s.long()
    n = n[n != 0]
    return float((n & -n).min()) / 2.0 ** 40 if n.numel() else float('inf')


def backward_exactness(key, mode16, **kw):
    """-> {claim: (holds, figure)}: fp32-representability of every modelled intermediate and the span of the partial sums of dgates W_h"""
    r, out = backward_model(key, mode16, **kw), {}
    fits = lambda v: torch.equal(v.float().double(), v)  # noqa
    for t, s in enumerate(r['steps']):
        for n in ('dhv', 'dc', 'dcn', 'd', 'dhr'):
            out[f't{t} {n} fits fp32'] = (fits(s[n]), float(s[n].abs().max()))
        # every term tile[m, k] W_h[k, ch] is a multiple of q = lowbit(tile) * lowbit(W_h); any partial sum, in any order, is one below sum |terms|
        q = lowbit(s['tile']) * lowbit(s['Wh'])
        span = float((s['tile'].abs() @ s['Wh'].abs()).max()) / q if q != float('inf') else 0.0
        out[f't{t} partial sums of dgates W_h span < 2^24 quanta'] = (span < 2.0 ** 24, span)
        out[f't{t} widest value in significant bits <= 24'] = (widest_bits(s) <= 24, widest_bits(s))
    return out


def widest_bits(s):
    """the most significant bits any element of a timestep's dhv / dc / dgates / dhr needs"""
    worst = 0
    for n in ('dhv', 'dc', 'd', 'dhr'):
        v = s[n].reshape(-1)
        v = v[v != 0]
        if v.numel():
            n40 = (v * 2.0 ** 40).long().abs()
            low = n40 & -n40
            worst = max(worst, int(torch.log2((n40 // low).double()).floor().max()) + 1)
    return worst
