"""Operands on which the training BatchNorm + SiLU kernels of csrc/k_norm.hip (``bn_silu_fwd_kernel``, ``bn_silu_bwd_reduce_kernel<4|8>``,
``bn_silu_bwd_apply_kernel`` and their ``_group`` entries) have no rounding error wherever their arithmetic allows it, the float64 reference
of each, and a model of their launch arithmetic -- so that tests/test_bn_exact_gpu.py compares for equality and a skipped replica, a
division by the local row count, a tail row counted twice or a column read from outside a strided ``dy`` moves a result by at least 0.5.
The kernels are fp32 (statistics in double) in every precision mode.  Built on tests/linear_exact.py.

The statistics, the saved (mean, rstd) and the sums are INPUTS of the kernel that consumes them: they are crafted directly, need not be
consistent with ``z``, and the reference is evaluated from the same crafted values.

* forward statistics (``fwd_problem``): per channel an integer mean m in [-3, 3] and a variance v in {0, 0.25, 1, 4};
  s = count m, ss = count (v + m^2), split over ``rep`` copies by ``split_copies``: the copies hold +-odd 2^40 that cancel, one of them
  carries the total.  Every partial sum in any order is a multiple of 2^-4 below 2^48: exact in double, lost in fp32, and a skipped copy
  is off by >= 2^40.  Channel N / 2 has v = 0 and ss lowered by count / 16: ss / count - mean^2 = -1/16, clamped to 0.
  save_mean, save_rstd: the reference evaluates in float64 in the kernel's order (s / count, ss / count - mean^2, clamp,
  1 / sqrt(var + (double)(float) eps)) and rounds to fp32.  s / count and ss / count are exact quotients, mean is an integer so mean^2 is
  exact with or without fma contraction, the double divide and sqrt are correctly rounded: EQUALITY.
* running buffers: integer starting values; momentum 0.5 and 0.25: (1 - momentum) is exact, both products are exact (a power of two, or
  0.75 times a small integer), so the result is ONE rounding of the exact sum with or without fma contraction: EQUALITY with the float64
  sum rounded to fp32.  momentum 0.1: ``close_fp32``.  count in {1, 64, 65}: the unbiased factor count / (count - 1), rounded (64),
  exact (65) and skipped (1).  ``run_mean = None``: run_var must stay as it was.
* forward output: z = m + d, d in +-{0.5, 1, 2} (neighbouring rows and channels differ by >= 0.5 somewhere); y is not exact (v_exp_f32,
  v_rcp_f32): ``close_fp32`` against float64 silu((z - mean) rstd w + b) evaluated with the kernel's fp32 mean and rstd, separately for
  the channels of variance 0 (rstd = 316, |y| up to 1300) and the others (|y| < 12), so that the floor of the bound follows each.
* count vs M: every forward and apply problem has count = 4 M (the statistics stand for 4 x the local rows); each is run with
  ``count`` = the product and again with ``count`` = rows per image and ``count_dev`` = [images] (a one-element float64 tensor): both
  bit-identical, both equal to the reference, which divides by the product.
* reduce (``reduce_problem``): mean integer, rstd in {0.5, 1, 2}, z = mean + k / rstd with k in +-{1, 2}: xhat = k exactly.
  dy in +-{1, 2, 3}.  Three kinds of channel, ``kind_of``: all three in every group of 4 channels:
    0  w = 0, b = 0:                u = 0,      silu' = 0.5   rests on v_exp_f32(-0) == 1 and v_rcp_f32(2) == 0.5
    1  w in +-{0.5, 1, 2}, b = 64:  u in 60..68, silu' = 1    rests on 1 + v_exp_f32(< -86) == 1 and v_rcp_f32(1) == 1
    2  w = 0, b = -128:             u = -128,   silu' = -0    rests on v_exp_f32(184.7) == inf and v_rcp_f32(inf) == 0
  A thread adds at most 8 terms of magnitude <= 6: integers and halves far below 2^24; the LDS fold and the atomics are double, sums
  below 2^53.  The fold of the copies: EQUALITY with float64, for each kind.  With rep > 1 every copy a workgroup can reach (r <
  min(rep, workgroups)) is non-zero and every other copy stays exactly zero.
  Observed on the MI355X: all three kinds hold -- see OBSERVED below.
* apply (``apply_problem``): s0 = count a, s1 = count b with a, b multiples of 1/8, |.| <= 2, split over the copies as above; every
  channel of kind 1, so du = dy.  s0 / count = a exactly, for any count; dz = (w rstd) (du - a - xhat b): multiples of 1/32 below 2^6:
  EQUALITY.  dw = dw0 + (float) s1, db = db0 + (float) s0 from ``start_vector``: multiples of 1/8 below 2^18: EQUALITY.  ``dw = None``.
* chain (``chain_ref``): the sums of the reduce feed the apply, on the reduce operands.  count a power of two: every quotient is exact,
  ``chain_fp32`` (the kernel's operation order in fp32) equals the float64 reference: EQUALITY.  Any other count: ``close_fp32``.
* strided dy (``wide``): dy is the channel slice [c0 : c0 + N] of a wider map whose other columns hold PAD_VALUE 2^20.
* refusals: n = 0, n = 9, N % 4 != 0, N / 4 > 256 in the backward, lddy < N, lddy % 4 != 0: LEOD_ERR_ARG, nothing written.

Launch model (``rstep``, ``reduce_rpt``, ``reduce_gx``, ``flat_gx``, ``flat_passes``, ``idle_lanes``): the arithmetic of the launchers at the
end of csrc/k_norm.hip.  tests/test_bn_exact_cpu.py derives from it that every shape of ``SHAPES`` reaches the branch it is there for.

OBSERVED (MI355X, gfx950): v_exp_f32(-0) == 1, v_rcp_f32(2) == 0.5, v_rcp_f32(1) == 1, v_exp_f32(184.7) == inf and
v_rcp_f32(inf) == 0 -- the reduce sums of all three channel kinds equal the float64 reference at every shape; no fallback to MASK_TOL
is in use.  The device's double divide and sqrt give the correctly rounded save_mean / save_rstd at every shape and replica count, and
the running buffers at momentum 0.5 / 0.25 equal the once-rounded exact sum.  y and the momentum-0.1 buffers stay within ``close_fp32``."""
import functools

import torch

from linear_exact import PAD_VALUE, _ints, _pick, _signed, close_fp32, start_vector  # noqa: F401  (re-exported)

# (N, M): what each reaches is asserted by tests/test_bn_exact_cpu.py from the launch model below
SHAPES = ((256, 4099), (96, 10931), (1024, 1031), (48, 77), (20, 103), (4, 300), (256, 1), (256, 3))
# every shape with two of the replica counts 1, 2, 16, 32; (48, 77), (20, 103), (4, 300), (256, 1), (256, 3) run fewer workgroups than copies
CASES = ((256, 4099, 1), (256, 4099, 16), (96, 10931, 2), (96, 10931, 32), (1024, 1031, 16), (1024, 1031, 1), (48, 77, 2), (48, 77, 32),
         (20, 103, 1), (20, 103, 16), (4, 300, 2), (4, 300, 32), (256, 1, 1), (256, 1, 2), (256, 3, 32), (256, 3, 16))
HEAD_GROUP = (96, (4 * 32 * 40, 4 * 16 * 20, 4 * 8 * 10) * 2, (16, 2, 1, 32, 1, 2))        # N, rows, replicas of the six members
FORCED_GROUP = (256, (4099, 0, 37), (16, 2, 2))                                            # the large member forces 8 rows per thread
RUN_COUNTS, RUN_SHAPE = (1, 64, 65), (48, 77)
EPS = 1e-5
IMAGES = 4                      # count = IMAGES * M
NOISE = float(2 ** 40)
WIDE_PAD = PAD_VALUE * 2 ** 20
HALVES = [0.5, 1., 2.]
SENTINEL = -77.0
D = torch.float64


# ---- the launch arithmetic of csrc/k_norm.hip ----------------------------------------------------------------------------------------------
def rstep(N):
    """row lanes of a reduce workgroup: 256 threads, N / 4 of them per row"""
    return 256 // (N // 4)


def idle_lanes(N):
    return 256 - rstep(N) * (N // 4)


def reduce_rpt(Ms, N):
    """rows per thread of ONE reduce launch over the members ``Ms``: 8 as soon as one member would run >= 128 workgroups with 8"""
    per = rstep(N) * 8
    return 8 if any((M + per - 1) // per >= 128 for M in Ms) else 4


def reduce_gx(M, N, rpt):
    return (M + rstep(N) * rpt - 1) // (rstep(N) * rpt) if M > 0 else 0


def flat_gx(M, N):
    """workgroups of the forward and the apply kernel: one thread per 4 elements, at most 1024"""
    return min(1024, max(1, (M * N // 4 + 255) // 256)) if M > 0 else 0


def flat_passes(M, N):
    """(fewest, most) grid-stride passes of a thread of the forward / apply kernel"""
    n4, threads = M * N // 4, flat_gx(M, N) * 256
    return (n4 // threads, (n4 + threads - 1) // threads) if threads else (0, 0)


def split_count(count):
    """count = rows per image (host) x images (device, ``count_dev``)"""
    for images in (IMAGES, 5, 1):
        if count % images == 0:
            return count // images, images


def chain_counts(M):
    """the counts of the reduce -> apply chain: a power of two that is not M, and IMAGES * M"""
    return 1 << (M.bit_length() + 1), IMAGES * M


# ---- operands --------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for v in key:
        seed = seed * 1000003 + int(v) + 17
    return torch.Generator().manual_seed(seed % (2 ** 62))


def kind_of(N):
    c = torch.arange(N)
    return (c + c // 4) % 3


def split_copies(total, rep, g):
    """float64 [K] -> [rep, K] whose fold is ``total``: copies 0 .. rep - 2 hold +-odd 2^40, the last one minus their sum, and copy
    k % rep carries the total of column k"""
    K = total.numel()
    out = torch.zeros(rep, K, dtype=D)
    if rep > 1:
        odd = (2 * torch.randint(0, 4, (rep - 1, K), generator=g) + 1).double() * (torch.randint(0, 2, (rep - 1, K), generator=g) * 2 - 1).double()
        out[:rep - 1] = odd * NOISE
        out[rep - 1] = -out[:rep - 1].sum(0)
    k = torch.arange(K)
    out[k % rep, k] += total.double()
    return out


def silu64(u):
    return u * torch.sigmoid(u)


def fwd_stats_ref(colstats, count, momentum=None, rm0=None, rv0=None):
    """float64 in the kernel's order -> save_mean, save_rstd (fp32) and, with a momentum, the running buffers (float64, to be rounded)"""
    S = colstats.sum(0)
    mean = S[0] / count
    var = torch.clamp(S[1] / count - mean * mean, min=0.0)
    eps = torch.tensor(EPS, dtype=torch.float32).double()
    r = dict(mean=mean.float(), rstd=(1.0 / torch.sqrt(var + eps)).float(), var=var)
    if momentum is not None:
        unb = (var * count / (count - 1.0) if count > 1 else var).float().double()
        mom = torch.tensor(momentum, dtype=torch.float32)
        keep = (torch.tensor(1.0, dtype=torch.float32) - mom).double()
        r['run_mean'] = keep * rm0.double() + mom.double() * r['mean'].double()
        r['run_var'] = keep * rv0.double() + mom.double() * unb
    return r


@functools.lru_cache(maxsize=None)
def fwd_problem(N, M, rep, count=None, momentum=0.5, salt=0):
    count = IMAGES * M if count is None else count
    g = _gen(1, N, M, rep, count, salt)
    m, v = _ints(-3, 3, (N,), g), _pick([0., 0.25, 1., 4.], (N,), g)
    neg = N // 2
    v[neg] = 0.0
    s, ss = count * m.double(), count * (v.double() + m.double() ** 2)
    ss[neg] -= count / 16.0
    colstats = split_copies(torch.cat([s, ss]), rep, g).view(rep, 2, N)
    w, b = _signed(HALVES, (N,), g), _ints(-3, 3, (N,), g)
    z = m + _signed(HALVES, (M, N), g)
    rm0, rv0 = start_vector(N, 1), start_vector(N, 4) + 3.0
    p = dict(N=N, M=M, rep=rep, count=count, momentum=momentum, m=m, v=v, neg=neg, colstats=colstats, w=w, b=b, z=z, rm0=rm0, rv0=rv0)
    r = fwd_stats_ref(colstats, float(count), momentum, rm0, rv0)
    r['y'] = silu64((z.double() - r['mean'].double()) * r['rstd'].double() * w.double() + b.double())
    p['ref'] = r
    return p


@functools.lru_cache(maxsize=None)
def reduce_problem(N, M, salt=0):
    g = _gen(2, N, M, salt)
    kind = kind_of(N)
    mean, rstd = _ints(-3, 3, (N,), g), _pick(HALVES, (N,), g)
    k = _signed([1., 2.], (M, N), g)
    z = mean + k / rstd
    dy = _signed([1., 2., 3.], (M, N), g)
    w = torch.where(kind == 1, _signed(HALVES, (N,), g), torch.zeros(N))
    b = torch.tensor([0., 64., -128.])[kind]
    grad = torch.tensor([0.5, 1., 0.])[kind]
    du = dy.double() * grad.double()
    p = dict(N=N, M=M, kind=kind, mean=mean, rstd=rstd, k=k, z=z, dy=dy, w=w, b=b, grad=grad, dw0=start_vector(N, 2), db0=start_vector(N, 5))
    p['ref'] = dict(sums=torch.stack([du.sum(0), (du * k.double()).sum(0)]))
    p['thread_bound'] = 8 * 3 * 2 * 2                    # 8 rows of |du xhat| <= 6, in halves
    return p


def chain_ref(p, count):
    """float64 apply on the reduce's own sums"""
    s0, s1 = p['ref']['sums'][0], p['ref']['sums'][1]
    du = p['dy'].double() * p['grad'].double()
    dz = (p['w'].double() * p['rstd'].double()) * (du - s0 / count - p['k'].double() * (s1 / count))
    return dict(dz=dz, dw=p['dw0'].double() + s1, db=p['db0'].double() + s0)


def chain_fp32(p, count):
    """dz of bn_silu_bwd_apply_kernel on the exact sums, in its operation order, fp32 behind the double quotients"""
    f = torch.float32
    s0, s1 = p['ref']['sums'][0], p['ref']['sums'][1]
    m0, m1 = (s0 / count).to(f), (s1 / count).to(f)
    xh = (p['z'] - p['mean']) * p['rstd']
    du = p['dy'] * p['grad']
    return (p['w'] * p['rstd']) * (du - m0 - xh * m1)


@functools.lru_cache(maxsize=None)
def apply_problem(N, M, rep, count=None, salt=0):
    count = IMAGES * M if count is None else count
    g = _gen(3, N, M, rep, count, salt)
    mean, rstd = _ints(-3, 3, (N,), g), _pick(HALVES, (N,), g)
    k = _signed([1., 2.], (M, N), g)
    z = mean + k / rstd
    dy = _signed([1., 2., 3.], (M, N), g)
    w, b = _signed(HALVES, (N,), g), torch.full((N,), 64.0)
    a, bq = _ints(-16, 16, (N,), g) / 8.0, _ints(-16, 16, (N,), g) / 8.0
    sums = split_copies(torch.cat([count * a.double(), count * bq.double()]), rep, g).view(rep, 2, N)
    p = dict(N=N, M=M, rep=rep, count=count, mean=mean, rstd=rstd, k=k, z=z, dy=dy, w=w, b=b, a=a, bq=bq, sums=sums,
             dw0=start_vector(N, 2), db0=start_vector(N, 5))
    dz = (w.double() * rstd.double()) * (dy.double() - a.double() - k.double() * bq.double())
    p['ref'] = dict(dz=dz, dw=p['dw0'].double() + count * bq.double(), db=p['db0'].double() + count * a.double())
    return p


def wide(dy, c0=8, tail=4):
    """[M, N] -> (the wider map whose columns [c0 : c0 + N] are ``dy`` and whose other columns hold WIDE_PAD, c0)"""
    M, N = dy.shape
    buf = torch.full((M, c0 + N + tail), WIDE_PAD, dtype=dy.dtype)
    buf[:, c0:c0 + N] = dy
    return buf, c0
