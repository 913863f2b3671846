"""Operands on which the depthwise convolution kernels of csrc/k_dwconv.hip (``dwconv_fwd_kernel<0|1|2>``, ``dwconv_dgrad_kernel``,
``dwconv_wgrad_kernel``) have no rounding error, the float64 reference of each, and a model of their launch arithmetic -- so that
tests/test_dwconv_exact_gpu.py compares for equality and one missing tap, an item of the second grid-stride pass never written, a channel of
the second wgrad tile or a pixel chunk counted twice moves an element by at least 0.5.  The kernels are fp32 in every precision mode.
Built on tests/linear_exact.py, in the style of tests/conv_exact.py.

* operands: NHWC maps x of integers in [-3, 3], weights [C, 1, ks, ks] in +-{0.5, 1, 2}, bias integers in [-3, 3], dy in +-{1, 2}.
  Every product is a multiple of 0.5 and exact; every accumulator adds such products.  ``bounds`` returns the worst partial sum of every
  accumulator in units of its smallest step, each to stay below 2^24 = LIMIT (asserted by the CPU test and again by the GPU test):
    fwd        the fma chain over the taps of one output element: ks^2 * 3 * 2 + 3, step 0.5
    stat_sum   the LDS fp32 partial of ONE workgroup and channel: the sum of |y| over the items the launch model gives that workgroup, step 0.5
    stat_sq    the same for y^2 (y^2 itself is a multiple of 0.25 below 2^24: one exact product), step 0.25
    dx_acc     start value (5) + two accumulating calls of ks^2 * 2 * 2, step 0.5
    dw         start value (5) + two calls of M_out * 2 * 3: the fp32 atomics of one (channel, tap), step 1
    dbias      start value (3) + two calls of M_out * 2, step 1
  Beyond the workgroup the statistics are double atomics: exact below 2^53 for any number of replicas.
* compared for EQUALITY with the float64 reference (``dw_ref``: the grouped convolution written out over its taps with shifted slices, and
  its two gradients; tests/test_dwconv_exact_cpu.py requires it to equal ``F.conv2d(groups = C)`` and its autograd): the forward with and
  without bias; the fold of the (sum, sumsq) copies for stat_rep in {1, 4, 32}; dgrad, and dgrad accumulating twice onto ``start_values``
  (rows and columns of the input that no output reads hold exact zeros, or stay as they were); dw and dbias accumulating twice onto
  non-zero starts.  No intrinsic is involved: these equalities rest on fp32 fma / add and double atomics alone.
* the eval-BatchNorm + SiLU epilogue (bn weight in +-{0.5, 1, 2}, bias and running mean integers, running variance in {0.25, 1, 4}) goes
  through rsqrtf, v_exp_f32 and v_rcp_f32: ``close_fp32`` against float64 silu((y - mean) w / sqrt(var + eps) + b).
* the wgrad writes through bare pointers: dw and dbias lie at the front of buffers that reach to the end of the last 256-channel tile
  (``guarded``); the rest holds start values too and must stay as it was -- that is where a dead lane of the last tile would write.
* refusals: C % 4 != 0, ks = 16, ks larger than the padded map (for stride 1 and for stride 2, where a truncating division used to
  report one output row), bn_w together with colstats, stat_rep = 3: LEOD_ERR_ARG; C = 20484 with colstats: LEOD_ERR_UNSUPPORTED; nothing
  written.

Launch model (``flat_grid``, ``passes``, ``wgrad_grid``): the arithmetic of the launchers at the end of csrc/k_dwconv.hip;
tests/test_dwconv_exact_cpu.py derives from it that every shape of ``SHAPES`` reaches the branch it is there for.

OBSERVED (MI355X, gfx950): every equality above holds at every shape; the epilogue stays within ``close_fp32``."""
import functools

import torch
import torch.nn.functional as F

from linear_exact import _ints, _pick, _signed, close_fp32, start_values, start_vector  # noqa: F401  (re-exported)

# (B, H, W, C, ks, stride, pad); pad None = (ks - 1) // 2, what the wrappers of ops pass
SHAPES = ((2, 64, 66, 512, 3, 1, None), (2, 96, 88, 8, 3, 1, None), (1, 6, 5, 260, 3, 1, None), (2, 10, 9, 16, 5, 2, None),
          (1, 9, 7, 48, 7, 2, None), (3, 8, 12, 32, 3, 2, None), (1, 3, 3, 4, 3, 1, 0), (2, 9, 12, 8, 3, 3, None))
STAT_REPS = (1, 4, 32)
LIMIT = float(2 ** 24)
BN_EPS = 1e-5
X_MAX, W_MAX, DY_MAX, BIAS_MAX, START_MAX, START_VEC_MAX = 3.0, 2.0, 2.0, 3.0, 5.0, 3.0
SENTINEL = -77.0
D = torch.float64


# ---- the launch arithmetic of csrc/k_dwconv.hip ----------------------------------------------------------------------------------------------
def out_hw(H, W, ks, stride, pad):
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def flat_grid(items):
    """workgroups of the forward / dgrad kernel: 256 items each, at most 4096"""
    return min(4096, max(1, (items + 255) // 256))


def passes(items):
    """(fewest, most) grid-stride passes of a thread"""
    threads = flat_grid(items) * 256
    return items // threads, (items + threads - 1) // threads


def fwd_items(p):
    return p['B'] * p['Ho'] * p['Wo'] * p['C'] // 4


def dgrad_items(p):
    return p['B'] * p['H'] * p['W'] * p['C'] // 4


def wgrad_grid(p):
    """(pixel chunks, channel tiles, pixels per chunk, live lanes of the last tile)"""
    M = p['B'] * p['Ho'] * p['Wo']
    gx = min(256, max(1, (M + 63) // 64))
    tiles = (p['C'] // 4 + 63) // 64
    return gx, tiles, (M + gx - 1) // gx, p['C'] // 4 - (tiles - 1) * 64


def unread(p):
    """(input rows, input columns) that no output position reads"""
    def count(n, no):
        read = {o * p['stride'] - p['pad'] + k for o in range(no) for k in range(p['ks'])}
        return sum(1 for i in range(n) if i not in read)
    return count(p['H'], p['Ho']), count(p['W'], p['Wo'])


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def dw_ref(x, w, bias, dy, stride, pad):
    """float64 depthwise convolution over its taps: x [B,H,W,C], w [C,1,ks,ks], dy [B,Ho,Wo,C] -> y (no bias added when None), dx, dw, dbias"""
    B, H, W, C = x.shape
    ks = w.shape[-1]
    Ho, Wo = out_hw(H, W, ks, stride, pad)
    xp = F.pad(x.double(), (0, 0, pad, pad, pad, pad))
    wd, dyd = w.double(), dy.double()
    y = torch.zeros(B, Ho, Wo, C, dtype=D) + (bias.double() if bias is not None else 0.0)
    dxp, dw = torch.zeros_like(xp), torch.zeros(C, 1, ks, ks, dtype=D)
    for ky in range(ks):
        for kx in range(ks):
            rows, cols = slice(ky, ky + (Ho - 1) * stride + 1, stride), slice(kx, kx + (Wo - 1) * stride + 1, stride)
            y += wd[:, 0, ky, kx] * xp[:, rows, cols]
            dxp[:, rows, cols] += wd[:, 0, ky, kx] * dyd
            dw[:, 0, ky, kx] = (dyd * xp[:, rows, cols]).sum((0, 1, 2))
    return y, dxp[:, pad:pad + H, pad:pad + W].contiguous(), dw, dyd.sum((0, 1, 2))


def _gen(*key):
    seed = 0
    for v in key:
        seed = seed * 1000003 + int(v) + 23
    return torch.Generator().manual_seed(seed % (2 ** 62))


def _fp32(t):
    assert torch.equal(t.float().double(), t), 'a reference is not representable in fp32'
    return t.float()


@functools.lru_cache(maxsize=None)
def problem(B, H, W, C, ks, stride, pad=None):
    """references are exact and kept as fp32 (asserted representable)"""
    pad = (ks - 1) // 2 if pad is None else pad
    g = _gen(B, H, W, C, ks, stride, pad)
    Ho, Wo = out_hw(H, W, ks, stride, pad)
    x, w = _ints(-3, 3, (B, H, W, C), g), _signed([0.5, 1., 2.], (C, 1, ks, ks), g)
    bias, dy = _ints(-3, 3, (C,), g), _signed([1., 2.], (B, Ho, Wo, C), g)
    p = dict(B=B, H=H, W=W, C=C, ks=ks, stride=stride, pad=pad, Ho=Ho, Wo=Wo, x=x, w=w, bias=bias, dy=dy)
    y, dx, dw, dbias = dw_ref(x, w, bias, dy, stride, pad)
    p['dx0'] = start_values(B * H * W, C, 1).view(B, H, W, C)
    p['dw0'], p['db0'] = start_values(C, ks * ks, 2).view(C, 1, ks, ks), start_vector(C, 4)
    p['ref'] = dict(y=_fp32(y), y_nobias=_fp32(y - bias.double()), dx=_fp32(dx), dw=_fp32(dw), dbias=_fp32(dbias),
                    stats=torch.stack([y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))]))
    p['bn'] = (_signed([0.5, 1., 2.], (C,), g), _ints(-3, 3, (C,), g), _ints(-3, 3, (C,), g), _pick([0.25, 1., 4.], (C,), g))
    bw, bb, rm, rv = (t.double() for t in p['bn'])
    u = (y - rm) * bw / torch.sqrt(rv + BN_EPS) + bb
    p['ref']['bn'] = u * torch.sigmoid(u)
    return p


def accumulated(p, start, delta, calls):
    """float64 start + calls * delta"""
    return p[start].double() + calls * p['ref'][delta].double()


def block_partials(p):
    """worst LDS statistics partial of one workgroup and channel: (sum |y|, sum y^2) over the items the forward grid gives it"""
    C4 = p['C'] // 4
    items = fwd_items(p)
    grid = flat_grid(items)
    it = torch.arange(items)
    key = (it // 256) % grid * C4 + it % C4
    y = p['ref']['y'].double().view(-1, 4)                                   # item it = pixel * C4 + channel group: the map's own order
    s = torch.zeros(grid * C4, 4, dtype=D).index_add_(0, key, y.abs())
    q = torch.zeros(grid * C4, 4, dtype=D).index_add_(0, key, y * y)
    return float(s.max()), float(q.max())


def bounds(p):
    """the worst partial sum of every accumulator, in units of its smallest step; each must be < LIMIT"""
    ks2, m_out = p['ks'] ** 2, p['B'] * p['Ho'] * p['Wo']
    s, q = block_partials(p)
    return dict(fwd=(ks2 * X_MAX * W_MAX + BIAS_MAX) / 0.5, stat_sum=s / 0.5, stat_sq=q / 0.25, y_sq=float(p['ref']['y'].abs().max()) ** 2 / 0.25,
                dx_acc=(START_MAX + 2 * ks2 * DY_MAX * W_MAX) / 0.5, dw=START_MAX + 2 * m_out * DY_MAX * X_MAX, dbias=START_VEC_MAX + 2 * m_out * DY_MAX)


def guarded(p, start, per_channel):
    """the start values of dw (per_channel = ks^2) or dbias (1) at the front of a buffer that reaches to the end of the last 256-channel
    tile of the wgrad, the rest filled with start values as well -> flat fp32 [tiles * 256 * per_channel]"""
    tiles = wgrad_grid(p)[1]
    buf = start_values(tiles * 256, per_channel, 9).reshape(-1).clone()
    buf[:p['C'] * per_channel] = p[start].reshape(-1)
    return buf
