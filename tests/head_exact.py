"""Operands on which the head tail (csrc/k_head.hip: SimOTA assignment, IoU / BCE losses, batched NMS, pseudo-label filter, prediction convs)
has ONE right answer at every tie and on every threshold, and the references that state it -- so that tests/test_head_exact_gpu.py compares
masks, indices, counts, keep order and detection rows with ``torch.equal`` / ``np.array_equal``.  Continuous random inputs never produce two
equal costs, IoUs or scores and never put a value on a threshold; every rule that only matters there is invisible to them.

GEOMETRY.  ``SMALL``: a 128 x 160 frame, strides (8, 16, 32), levels 16 x 20, 8 x 10, 4 x 5, A = 420.  Every box coordinate is an integer
or a half-integer, so every corner, area, intersection and centre distance is exact in fp32 and in float64 alike.

DYADIC IoUs.  Against a 32 x 32 label, predictions with the same centre: 32 x 32 -> 1, 16 x 32 -> 1/2, 8 x 32 and 64 x 64 -> 1/4, 16 x 16 -> 1/4,
a far box -> 0.  A quotient of small integers with a power-of-two denominator is exact, so the fp32 IoU IS the float64 IoU (``check_assign``
asserts it for every gt x candidate pair of every case), top-10 sums are exact in any order and the dynamic k has one right answer.

SATURATED LOGITS (the saturated gates of lstm_exact).  common.hpp: sigmoidf_(x) = rcp(1 + exp2(-x log2 e)).  For x >= SAT = 128 the
exponential is below 2^-184, 1 + e rounds to 1 and rcp(1) = 1; for x <= -128 exp2(>= 184) = inf and rcp(inf) = 0.  torch's fp32 sigmoid
gives the same two values (exp(-128) = 2.6e-56 is below the smallest subnormal 1.4e-45).  At +-40, by contrast, sigmoid(-40) = 4.2e-18 is
NOT 0 and -log(sqrt(4.2e-18)) = 20, not 100 -- so "off" logits are -128, "on" logits +128.  Then p = sqrt(sig(cls) sig(obj)) is exactly
0 or 1 and the clamped BCE of the assignment cost (log terms clamped at -100) is
    p = 1, t = 1:  -(1 log 1 + 0 max(log 0, -100)) = 0          p = 0, t = 0:  -(0 (-100) + 1 log 1) = 0
    p = 1, t = 0:  -max(log(1 - 1), -100) = 100                 p = 0, t = 1:  -max(log 0, -100) = 100
on the device and in torch alike.  The cost is 3 (-log(iou + 1e-8)) plus a multiple of 100 (plus the 1e6 penalty), a function of
(IoU, logits, class, in-centre) alone: two candidates with the same four tie BIT FOR BIT, whatever the library's log does.  Cases that need
a graded class term use logits with |x| <= 4 (p within [1.8e-2, 0.982]); the band in between, where 1 - p is one ulp from 0 and one ulp
decides between 16.6 and 100, is never used (``check_assign`` asserts |x| <= 4 or |x| >= 128).

SEPARATION GUARD.  For every gt, two candidate costs that are not ties by construction (same IoU, same logits, same in-centre bit) differ in
float64 by at least MARGIN = 0.1 (with saturated logits every class term is exactly 0 or 100, so "same logits" widens to "same exact class
sum": ``tie_class``); the same holds for the costs of one candidate against different gts (what the multi-claim rule compares).
The fp32 evaluation error of an unpenalised cost (below 512: nc <= 3 terms of at most 100, and 3 x 18.5):
  * -log(iou + 1e-8): the sum rounds (2^-24 relative, i.e. 6e-8 absolute on the log), logf within 2 ulp of a value below 18.5 -> 2 x 2^-19,
    the product by 3 half an ulp of a value below 64 -> 2^-19; together below 6e-6;
  * a graded class term -log(p) or -log(1 - p), |x| <= 8: sigmoidf_ (v_exp_f32, v_rcp_f32: 1 ulp each, the argument product, the sum)
    4 x 2^-23 relative on each factor, the product and sqrtf another 2^-23: dp / p <= 5 x 2^-23 = 6e-7, which is also the absolute error of
    log p; for log(1 - p) the error of p is magnified: d log(1 - p) <= 6e-7 p / (1 - p), which is 1.8e-3 at x = 8 but below 3.3e-5 at
    |x| <= 4.  Graded cases therefore keep |x| <= GRADED_MAX = 4 (narrower than the |x| <= 8 that would still avoid the clamp): per term
    3.3e-5 + logf's 2 ulp of a value below 8 (1e-6), nc <= 3 terms and as many additions (half an ulp of 512 each, 1.5e-5): below 1.5e-4;
  * the final additions: two half-ulps of a value below 512, 3e-5.
  Total below 2e-4 = E_COST; MARGIN = 0.1 is 500 E_COST on graded cases and, on saturated cases (class terms exact: error below 4e-5),
  2500 times the error.  The smallest gap between two constructed levels is 3 log 2 = 2.08 (IoU 1, 1/2, 1/4), 20 times MARGIN.  ``check_assign`` asserts the guard
  and |x| <= 4 for graded logits.

THE 1e6 PENALTY.  A candidate outside the centre region of a gt costs about 1e6, where the fp32 ulp is 1/16: distinct float64 costs
collapse.  Every case keeps k_g within gt g's in-centre candidate count, so no penalised candidate is ever selected -- except the named case
``S8-penalised``, where the penalised candidates that compete for the remaining slots are exact duplicates (same key): they tie in fp32 and
in float64 alike and go by index.  ``check_assign`` asserts both.

``assign_reference``: float64 restatement of oracle.head.get_assignments + simota_matching (and of the n == 0 branches of get_losses) in
the kernel's output layout.  Its one change: both selections are stable, ties to the lowest candidate index (position in ascending anchor
order); torch.topk leaves that order unspecified, so the oracle cannot state the answer when a tie straddles k.  An anchor claimed by
several gts goes to the first minimal gt over ALL valid gts (torch.min(dim=0) of the oracle).

LOSS.  Reference: oracle.head.get_losses on the same tensors with autograd, the decode chain applied as test_simota_and_loss does;
tolerances of that test.  torch.max / torch.min give each side HALF the gradient at equality, so a predicted edge that coincides with a
label edge receives half the term; ``iou_loss_grad`` is the closed form with that share as a parameter (1/2: autograd; 0 and 1: mutants).

NMS.  Integer corners, dyadic scores.  ``nms_reference`` restates oracle/nms.py + oracle.postproc.postprocess (fp32 numpy, stable sort,
strict ``> thr``, coordinate trick up to ``vanilla_limit`` box elements and the per-class loop above) with the limit as a parameter and the
mutation hooks; tests/test_head_exact_cpu.py holds it to the oracle.  1/2 = 100 / 200 is exact, so a pair at IoU exactly nms_thre = 0.5
exists and is kept.  The ``4n > limit`` switch is fed at limits of the test's own and at torchvision's CPU limit (1000 and 1001 candidates
against 4000 box elements), where the oracle itself states both sides.  ``pseudo_reference`` restates oracle.postproc.pred2label the same way.

HEAD PREDICTION (``pred_problem``).  Features in {0, +-1, +-2}, weights in +-{1/2, 1, 2} with at most 4 nonzeros per row, biases in
{0, +-1/2, +-1}: every partial sum of every fmaf chain is a multiple of 1/2 below 2^6, exact in any order (the span argument of
linear_exact).  The raw outputs are therefore exact; xy = (raw + grid) stride is exact (a multiple of 4 below 2^15) and compared for
equality, as are the logits of out_train, the feature gradients and the six weight / bias gradients (d_raw in {0, +-1, +-2}, gscale a power
of two; a weight gradient sums at most B h w terms of magnitude <= 4 gscale: below 2^24 quanta for every shape used, exact in any atomic
order).  wh = expf(raw) stride and the probabilities sigmoidf_(raw) carry a function error: the box regression raws are clamped by
construction to |raw| <= 4 (``pred_problem`` asserts it) and
    expf: 2 ulp (HIP libm, documented 1) -> 2 x 2^-23 relative; the product by the stride is exact (power of two)
    sigmoidf_: argument product 2^-24 |x| log2e relative on the argument -> |x| 2^-24 relative on e; v_exp_f32 2^-23; the sum 2^-24;
               v_rcp_f32 2^-23: below (|x| + 5) 2^-24, |x| <= 17 -> 22 x 2^-24
  PRED_RTOL = 2^-19 (32 x 2^-24) covers both; the smallest change a discrete error (one weight or feature off by its quantum 1/2) can cause
  is a factor e^(1/2) on wh (65 %) or sigmoid(x + 1/2) - sigmoid(x) >= 5e-8 / sigmoid relative 39 % at the tail: five orders above the bound.

``MUTATIONS``: named defects applied inside the references; tests/test_head_exact_cpu.py shows that each changes a discrete output of a
committed case.  ``EQUIVALENT``: the IoU's ``tl < br`` written ``tl <= br`` is NOT observable -- where a corner pair is equal the
intersection's side is 0 and the area 0 either way -- and is recorded as such, with the test that proves it."""
import functools
import math

import numpy as np
import torch

from oracle import head as oh

F32 = np.float32
SAT = 128.0
ON, OFF = SAT, -SAT
GRADED_MAX = 4.0
E_COST = 2e-4
MARGIN = 0.1
assert MARGIN >= 100 * E_COST                 # at least two orders of magnitude over the evaluation error
IGNORE = 1024.0
STRIDES = (8, 16, 32)
FAR = (-1000.0, -1000.0, 1.0, 1.0)           # a prediction with IoU 0 against everything
SENTINEL = -77.0
PRED_RTOL = 2.0 ** -19

SIMOTA_MUTATIONS = ('center_ge', 'tie_highest', 'k_round', 'top9', 'no_max1', 'claimers_only', 'claim_last_gt', 'ignore_any_box')
NMS_MUTATIONS = ('nms_ge', 'conf_gt', 'tie_reversed', 'removed_suppresses', 'no_class_offset', 'limit_ge', 'argmax_last')
PSEUDO_MUTATIONS = ('thr_ge', 'w_gt5', 'maxw_float')
LOSS_MUTATIONS = ('edge_share_0', 'edge_share_1')
MUTATIONS = dict([(m, 'simota') for m in SIMOTA_MUTATIONS] + [(m, 'nms') for m in NMS_MUTATIONS] +
                 [(m, 'pseudo') for m in PSEUDO_MUTATIONS] + [(m, 'loss') for m in LOSS_MUTATIONS])
EQUIVALENT = ('iou_le',)


class Geom:
    def __init__(self, H, W):
        self.frame = (H, W)
        self.strides = STRIDES
        self.hws = [(H // s, W // s) for s in STRIDES]
        self.a0, a = [], 0
        for h, w in self.hws:
            self.a0.append(a)
            a += h * w
        self.A = a
        self.grids = tuple(t.double() for t in oh.make_grids(self.hws, STRIDES))

    def anchor(self, level, y, x):
        h, w = self.hws[level]
        assert 0 <= y < h and 0 <= x < w
        return self.a0[level] + y * w + x


SMALL = Geom(128, 160)
BIG = Geom(768, 768)                        # A = 12096: with Nmax >= 214 the candidate arrays of simota_kernel leave LDS
assert SMALL.A == 420 and BIG.A == 12096


# ------------------------------------------------------------------------------------------------------------------------------------------
# SimOTA reference
# ------------------------------------------------------------------------------------------------------------------------------------------
def in_centers(gt_xy, geom, ge=False):
    """oracle.head.is_in_centers in float64 (exact on half-integer operands); ``ge``: the mutant that lets the boundary in"""
    gx, gy, gs = geom.grids
    xc, yc, dist = ((gx + 0.5) * gs)[None], ((gy + 0.5) * gs)[None], (gs * 1.5)[None]
    cx, cy = gt_xy[:, 0:1].double(), gt_xy[:, 1:2].double()
    d = torch.stack([xc - (cx - dist), yc - (cy - dist), (cx + dist) - xc, (cy + dist) - yc], 2).min(dim=-1).values
    return d >= 0.0 if ge else d > 0.0


def _sig(x):
    if x >= SAT:
        return 1.0
    if x <= -SAT:
        return 0.0
    return 1.0 / (1.0 + math.exp(-x))


def _clog(p):
    return max(math.log(p), -100.0) if p > 0.0 else -100.0


@functools.lru_cache(maxsize=None)
def pair_cost(iou, obj, cls_logits, gcls, geom_in):
    """the SimOTA cost of one (gt, candidate) pair as a function of its key: scalar float64 code, so equal keys give equal bits"""
    so, c = _sig(obj), 0.0
    for ci, x in enumerate(cls_logits):
        p = math.sqrt(_sig(x) * so)
        t = 1.0 if ci == gcls else 0.0
        c += -(t * _clog(p) + (1.0 - t) * _clog(1.0 - p))
    return c + 3.0 * (-math.log(iou + 1e-8)) + (0.0 if geom_in else 1e6)


def tie_class(key):
    """what makes two costs tie by construction: the key itself, or -- all logits saturated, every class term exactly 0 or 100 -- the IoU,
    the in-centre bit and the exact class sum (the order of exact terms does not matter)"""
    iou, obj, cls_logits, gcls, geom_in = key
    if abs(obj) >= SAT and all(abs(x) >= SAT for x in cls_logits):
        return (iou, geom_in, pair_cost(1.0, obj, cls_logits, gcls, True))
    return key


def _image_problem(out_b, lab_b, geom, mut=None):
    """-> None (no valid gt) or the pairwise problem of one image: candidates, keys, IoUs, costs"""
    lab = lab_b.double()
    nz, valid = lab.sum(1) > 0, lab[:, 0] != IGNORE
    nw, n = int(nz.sum()), int((nz & valid).sum())
    assert bool(nz[:nw].all()), 'label rows are a prefix'
    if n == 0:
        return None
    rows, v = lab[:nw], valid[:nw]
    inc = in_centers(rows[:, 1:3], geom, ge=mut == 'center_ge')
    cand = torch.nonzero(inc[v].any(0)).flatten().tolist()
    gtb, gtc, gtrow = rows[v][:, 1:5], [int(c) for c in rows[v][:, 0]], torch.nonzero(v).flatten().tolist()
    P = dict(n=n, nw=nw, inc=inc, v=v, cand=cand, gtrow=gtrow, gtc=gtc, gtb=gtb)
    if not cand:
        return P
    o = out_b.double()[cand]
    ious = oh.bboxes_iou_cxcywh(gtb, o[:, :4])
    geo = inc[v][:, cand]
    keys = [[(float(ious[g, j]), float(o[j, 4]), tuple(o[j, 5:].tolist()), gtc[g], bool(geo[g, j])) for j in range(len(cand))]
            for g in range(n)]
    P.update(ious=ious, geo=geo, keys=keys, cost=[[pair_cost(*k) for k in row] for row in keys])
    return P


def _select(P, mut=None):
    """dynamic k and the k cheapest candidates of every gt, stable; -> (ks, selections, straddling-tie flags)"""
    npos, ks, sels, straddle = len(P['cand']), [], [], []
    for g in range(P['n']):
        top = sorted(P['ious'][g].tolist(), reverse=True)[:min(9 if mut == 'top9' else 10, npos)]
        s = math.fsum(top)
        k = int(math.floor(s + 0.5)) if mut == 'k_round' else int(s)
        if mut != 'no_max1':
            k = max(k, 1)
        c = P['cost'][g]
        order = sorted(range(npos), key=(lambda j: (c[j], -j)) if mut == 'tie_highest' else (lambda j: (c[j], j)))
        ks.append(k)
        sels.append(order[:min(k, npos)])
        straddle.append(0 < k < npos and c[order[k - 1]] == c[order[k]])
    return ks, sels, straddle


def assign_reference(outputs, labels, geom, mut=None):
    """outputs [B, A, 5 + nc] (decoded boxes + logits), labels [B, Nmax, 7] -> the tensors of ops.simota_assign (``status`` = totals[2])"""
    B, A = outputs.shape[0], geom.A
    r = dict(fg_mask=torch.zeros((B, A), dtype=torch.uint8), ignore_mask=torch.zeros((B, A), dtype=torch.uint8),
             matched_row=torch.full((B, A), -1, dtype=torch.int32), matched_valid_idx=torch.full((B, A), -1, dtype=torch.int32),
             pred_iou=torch.zeros((B, A), dtype=torch.float32), num_fg_img=torch.zeros((B,), dtype=torch.int32), totals=[0, 0], status=0)
    for b in range(B):
        P = _image_problem(outputs[b], labels[b], geom, mut)
        if P is None:
            lab = labels[b].double()
            if float(lab.sum()) != 0.0:           # only ignore boxes: the geometry of the first ``num_ignore`` rows
                nign = int((lab[:, 0] == IGNORE).sum())
                r['ignore_mask'][b] = in_centers(lab[:nign, 1:3], geom, ge=mut == 'center_ge').any(0).to(torch.uint8)
            continue
        inc, v = P['inc'], P['v']
        if not bool(v.all()):
            c_all, c_valid = inc.any(0), inc[v].any(0)
            r['ignore_mask'][b] = (c_all if mut == 'ignore_any_box' else c_all & ~c_valid).to(torch.uint8)
        r['totals'][1] += P['n']
        cand = P['cand']
        if not cand:                              # the reference raises here; the kernel reports status bit 1
            r['status'] |= 1
            continue
        _, sels, _ = _select(P, mut)
        claims = [[] for _ in cand]
        for g, sel in enumerate(sels):
            for j in sel:
                claims[j].append(g)
        nfg = 0
        for j, cl in enumerate(claims):
            if not cl:
                continue
            g = cl[0]
            if len(cl) > 1:
                pool = cl if mut == 'claimers_only' else range(P['n'])
                best = min(P['cost'][gg][j] for gg in pool)
                hits = [gg for gg in pool if P['cost'][gg][j] == best]
                g = hits[-1] if mut == 'claim_last_gt' else hits[0]
            a = cand[j]
            r['fg_mask'][b, a], r['matched_row'][b, a], r['matched_valid_idx'][b, a] = 1, P['gtrow'][g], g
            r['pred_iou'][b, a] = float(P['ious'][g, j])
            nfg += 1
        r['num_fg_img'][b] = nfg
        r['totals'][0] += nfg
    return r


def check_assign(case):
    """the generator's assertions (docstring): exact IoUs, logit bands, the separation guard, the penalty rule.  -> per-image info"""
    geom, info = case['geom'], []
    out, lab = case['outputs'], case['labels']
    assert out.dtype == torch.float32 and lab.dtype == torch.float32
    assert torch.equal(out[..., :4] * 2, (out[..., :4] * 2).round()) and torch.equal(lab[..., 1:5] * 2, (lab[..., 1:5] * 2).round())
    lg = out[..., 4:].abs()
    assert bool(((lg <= GRADED_MAX) | (lg >= SAT)).all()), 'logits: graded (|x| <= 4) or saturated (|x| >= 128), never in between'
    for b in range(out.shape[0]):
        P = _image_problem(out[b], lab[b], geom)
        if P is None or not P['cand']:
            info.append(None)
            continue
        cand = P['cand']
        i32 = oh.bboxes_iou_cxcywh(P['gtb'].float(), out[b][cand][:, :4])
        assert torch.equal(i32.double(), P['ious']), 'an IoU is not exact in fp32'
        ks, sels, straddle = _select(P)
        incount = [int(P['geo'][g].sum()) for g in range(P['n'])]
        for g in range(P['n']):
            by_key = {}
            for j in range(len(cand)):
                by_key.setdefault(tie_class(P['keys'][g][j]), P['cost'][g][j])
            free = sorted(c for k, c in by_key.items() if c < 1e5)
            assert all(b_ - a_ >= MARGIN for a_, b_ in zip(free, free[1:])), ('separation', case['name'], g, free)
            assert not free or free[-1] < 512.0
            if ks[g] > incount[g]:
                assert case.get('penalised') and g in case['penalised'], ('penalty rule', case['name'], g, ks[g], incount[g])
                pen = sorted((P['cost'][g][j], j) for j in range(len(cand)) if not P['geo'][g][j])
                m = ks[g] - incount[g]
                assert m < len(pen)
                near = {tie_class(P['keys'][g][j]) for c, j in pen if c <= pen[m][0] + 1.0}       # within 16 fp32 ulps of the last slot: duplicates
                assert len(near) == 1, ('penalised competitors are not duplicates', case['name'], g)
            else:
                assert not case.get('penalised') or g not in case['penalised']
        for j in range(len(cand)):                 # what the multi-claim rule compares
            col = {}
            for g in range(P['n']):
                col.setdefault(tie_class(P['keys'][g][j]), P['cost'][g][j])
            cs = sorted(c for k, c in col.items() if c < 1e5)
            assert all(b_ - a_ >= MARGIN for a_, b_ in zip(cs, cs[1:])), ('separation across gts', case['name'], j)
        info.append(dict(P=P, ks=ks, sels=sels, straddle=straddle, incount=incount))
    return info


# ------------------------------------------------------------------------------------------------------------------------------------------
# SimOTA / loss cases
# ------------------------------------------------------------------------------------------------------------------------------------------
class _Build:
    def __init__(self, name, geom=SMALL, B=1, nc=2, nmax=4):
        self.name, self.geom, self.nc = name, geom, nc
        self.out = torch.zeros((B, geom.A, 5 + nc), dtype=torch.float64)
        self.out[..., :4] = torch.tensor(FAR, dtype=torch.float64)
        self.out[..., 4:] = OFF
        self.lab = torch.zeros((B, nmax, 7), dtype=torch.float64)
        self.nrows = [0] * B
        self.extra = {}

    def gt(self, cls, cx, cy, w=32.0, h=32.0, b=0, conf=(1.0, 1.0)):
        r = self.nrows[b]
        self.lab[b, r] = torch.tensor([cls, cx, cy, w, h, conf[0], conf[1]], dtype=torch.float64)
        self.nrows[b] = r + 1
        return r

    def put(self, level, y, x, box, cls=0, b=0, obj=ON, logits=None):
        """prediction of one anchor: ``cls`` = the class whose logit is ON (None: all off), or explicit class ``logits``"""
        a = self.geom.anchor(level, y, x)
        self.out[b, a, :4] = torch.tensor(box, dtype=torch.float64)
        self.out[b, a, 4] = obj
        self.out[b, a, 5:] = OFF
        if logits is not None:
            self.out[b, a, 5:] = torch.tensor(logits, dtype=torch.float64)
        elif cls is not None:
            self.out[b, a, 5 + cls] = ON
        return a

    def done(self, nmax=None, **extra):
        lab = self.lab
        if nmax is not None and nmax > lab.shape[1]:            # zero padding rows: the per-gt arrays move to the workspace above 128
            lab = torch.cat([lab, torch.zeros((lab.shape[0], nmax - lab.shape[1], 7), dtype=torch.float64)], 1)
        d = dict(name=self.name, geom=self.geom, nc=self.nc, outputs=self.out.float(), labels=lab.float())
        d.update(self.extra)
        d.update(extra)
        return d


C0 = (68.0, 68.0)                              # a level-0 anchor centre: 27 in-centre candidates, 9 per level


def box(w, h, c=C0):
    return (c[0], c[1], float(w), float(h))


# in-centre anchors of a gt at C0, ascending: level 0 (y, x) in {7, 8, 9}^2, level 1 {3, 4, 5}^2, level 2 {1, 2, 3}^2
def _slots():
    s = [(0, y, x) for y in (7, 8, 9) for x in (7, 8, 9)] + [(1, y, x) for y in (3, 4, 5) for x in (3, 4, 5)] + \
        [(2, y, x) for y in (1, 2, 3) for x in (1, 2, 3)]
    return s


def _iou_list_case(name, boxes, geom=SMALL, nmax=None, nc=2, slots=None, classes=None):
    """one 32 x 32 gt of class 0 at C0; ``boxes[i]`` is the prediction of the i-th listed slot (same logits unless ``classes``)"""
    bd = _Build(name, geom, nc=nc)
    bd.gt(0, *C0)
    sl = slots or _slots()
    for i, wh in enumerate(boxes):
        bd.put(*sl[i], box(*wh), cls=0 if classes is None else classes[i])
    return bd.done(nmax)


P1, PH, PQ, PQ2 = (32, 32), (16, 32), (8, 32), (64, 64)          # IoU 1, 1/2, 1/4, 1/4 against the 32 x 32 label
SPREAD = [(0, 7, 7), (0, 9, 9), (1, 4, 4), (2, 2, 2), (0, 8, 8), (1, 3, 5), (2, 1, 3), (0, 7, 9), (1, 5, 3), (2, 3, 1), (0, 9, 7), (1, 4, 5)]


def s1_cases():
    out = []
    for name, c, want in (('S1-x-edge', (64.0, 68.0), (3, 2)), ('S1-xy-edge', (64.0, 64.0), (2, 2)),
                          ('S1-x-inside', (64.5, 68.0), (3, 3)), ('S1-xy-inside', (64.5, 64.5), (3, 3))):
        bd = _Build(name, nc=1)
        bd.gt(0, *c)
        # perfect predictions on the 4 x 4 level-0 anchors around the centre: whoever is a candidate is chosen (k = the number of them,
        # at most 10), so letting the boundary anchors in changes fg_mask
        for y in (6, 7, 8, 9):
            for x in (6, 7, 8, 9):
                bd.put(0, y, x, box(32, 32, c), cls=0)
        out.append(bd.done(level0_candidates=want))
    return out


def s2_cases(geom=SMALL, nmax=None, tag=''):
    mk = lambda n, b, **kw: _iou_list_case('S2-' + n + tag, b, geom, nmax, slots=SPREAD, **kw)  # noqa: E731
    return [mk('sum3', [P1, PH, PH, PH, PH]), mk('sum2.75', [P1, PH, PH, PH, PQ]), mk('sum0.75', [PH, PQ]), mk('sum0', []),
            mk('twelve-halves', [PH] * 12), mk('ten-halves', [PH] * 10), mk('rank10-tie', [P1, P1] + [PH] * 7 + [PQ, PQ2, PQ])]


def s3_cases(geom=SMALL, nmax=None, tag=''):
    # four candidates at IoU 1/2 on levels 0, 0, 1, 2 (identical decoded box and logits) and one at IoU 1 of the wrong class (cost 200):
    # top-10 sum 3, k = 3, the four-way tie straddles k and the level-2 anchor loses
    four = [(0, 7, 8), (0, 9, 8), (1, 4, 4), (2, 2, 2), (0, 8, 8)]
    return [_iou_list_case('S3-straddle-levels' + tag, [PH, PH, PH, PH, P1], geom, nmax, slots=four, classes=[0, 0, 0, 0, 1]),
            _iou_list_case('S3-inside' + tag, [P1, P1, P1], geom, nmax, slots=[(0, 7, 8), (1, 4, 4), (2, 2, 2)]),
            _iou_list_case('S3-inside-and-straddle' + tag, [P1, P1, PH, PH, PQ], geom, nmax, slots=SPREAD),
            _iou_list_case('S3-outside' + tag, [P1, P1, P1, PQ, PQ], geom, nmax, slots=SPREAD)]


def s4_cases(geom=SMALL, nmax=None, tag=''):
    out = []
    bd = _Build('S4-identical-rows' + tag, geom)
    bd.gt(0, *C0)
    bd.gt(0, *C0)
    for s, wh in zip(SPREAD, [P1, P1, PH, PH]):
        bd.put(*s, box(*wh))
    out.append(bd.done(nmax))
    for name, order in (('S4-unequal', (32, 64)), ('S4-unequal-swapped', (64, 32))):
        bd = _Build(name + tag, geom)
        for w in order:
            bd.gt(0, *C0, w, w)
        bd.put(0, 8, 8, box(32, 32))
        out.append(bd.done(nmax))
    # X is claimed by g0 and g1 (64 x 64, class 1: their cheapest candidate at 100 + 3 log 8), but g2 (32 x 32, class 0), which took Y,
    # holds the lowest cost on X (100 + 3 log 2): X goes to g2, which never claimed it
    bd = _Build('S4-third-gt' + tag, geom)
    bd.gt(1, *C0, 64, 64)
    bd.gt(1, *C0, 64, 64)
    bd.gt(0, *C0)
    x_ = bd.put(0, 8, 8, box(16, 32), logits=(ON, ON))
    y_ = bd.put(1, 4, 4, box(32, 32), cls=0)
    out.append(bd.done(nmax, third=(x_, y_)))
    return out


def s5_cases():
    out = []
    for nc in (1, 2, 3):
        bd = _Build(f'S5-nc{nc}', nc=nc)
        bd.gt(nc - 1, *C0)
        bd.put(0, 7, 7, box(16, 32), cls=None if nc == 1 else 0)       # wrong class (nc 1: class logit off) at the lower index
        bd.put(0, 9, 9, box(16, 32), cls=nc - 1)
        bd.put(1, 4, 4, box(16, 32), cls=None if nc == 1 else 0)
        out.append(bd.done())
    # graded class logits at equal IoU: the class term alone orders the candidates (sum 2: k = 2)
    bd = _Build('S5-graded', nc=2)
    bd.gt(1, *C0)
    for s, lg, ob in zip(SPREAD, [(-1.0, 2.0), (2.0, -1.0), (0.5, 3.0), (-4.0, 4.0)], (2.0, 2.0, 1.0, 0.5)):
        bd.put(*s, box(16, 32), obj=ob, logits=lg)
    out.append(bd.done())
    return out


def s6_cases():
    out = []
    # image 0: a valid box and an ignore box whose centre regions overlap; image 1: ignore boxes only; image 2: empty
    bd = _Build('S6-ignore', B=3)
    bd.gt(0, *C0)
    bd.gt(IGNORE, 100.0, 68.0)
    bd.put(0, 8, 8, box(32, 32))
    bd.put(1, 4, 5, box(16, 32))                    # inside both centre regions (level 1, centre x = 88): a candidate, not ignored
    bd.gt(IGNORE, 36.0, 36.0, b=1)
    bd.gt(IGNORE, 116.0, 100.0, b=1)
    out.append(bd.done())
    bd = _Build('S6-ignore-first-row', B=2)           # the ignore box in row 0: matched_row != matched_valid_idx
    bd.gt(IGNORE, 100.0, 68.0)
    bd.gt(1, *C0)
    bd.gt(0, *C0, 64, 64)
    bd.put(0, 8, 8, box(32, 32), cls=1)
    bd.put(1, 4, 4, box(64, 64), cls=0)
    bd.gt(0, 36.0, 36.0, b=1)
    bd.put(0, 4, 4, box(32, 32, (36.0, 36.0)), b=1)
    out.append(bd.done())
    bd = _Build('S6-empty-batch', B=2)
    out.append(bd.done(oracle=True))
    # a gt whose centre region holds no anchor: the reference raises, the kernel reports status bit 1 and counts the gt
    bd = _Build('S6-no-candidate', B=2)
    bd.gt(0, 1000.0, 1000.0)
    bd.gt(0, *C0, b=1)
    bd.put(0, 8, 8, box(32, 32), b=1)
    out.append(bd.done(oracle=False))
    return out


def s7_big_case():
    """the S3 straddling tie and the S4 third-gt problem in the corner of a 768 x 768 frame (A = 12096) with Nmax = 214: cap = 48 Nmax =
    10272 candidates exceed the 10240 of the LDS tier, and Nmax > 128 moves the per-gt arrays too"""
    bd = _Build('S7-big', BIG, B=2, nmax=214)
    bd.gt(0, *C0)
    for s, wh, c in zip([(0, 7, 8), (0, 9, 8), (1, 4, 4), (2, 2, 2), (0, 8, 8)], [PH, PH, PH, PH, P1], [0, 0, 0, 0, 1]):
        bd.put(*s, box(*wh), cls=c)
    bd.gt(1, *C0, 64, 64, b=1)
    bd.gt(1, *C0, 64, 64, b=1)
    bd.gt(0, *C0, b=1)
    bd.put(0, 8, 8, box(16, 32), logits=(ON, ON), b=1)
    bd.put(1, 4, 4, box(32, 32), cls=0, b=1)
    return bd.done()


def s8_case():
    """gt 0 sits on the frame corner: 3 in-centre candidates (one per level), all perfect.  Four anchors in gt 1's centre region carry
    the same half of gt 0's box (IoU 1/2, class 0), so gt 0's top-10 sum is 3 + 4 / 2 = 5 and k = 5 reaches two PENALISED candidates out
    of four exact duplicates: the two lowest indices win"""
    bd = _Build('S8-penalised', nc=2)
    c = (0.0, 0.0)
    bd.gt(0, *c)
    bd.gt(1, 116.0, 100.0)
    for l in range(3):
        bd.put(l, 0, 0, box(32, 32, c))
    dup = [bd.put(*s, box(16, 32, c), cls=0) for s in ((0, 12, 14), (0, 12, 15), (1, 6, 7), (2, 3, 3))]
    bd.put(0, 11, 13, box(32, 32, (116.0, 100.0)), cls=1)
    return bd.done(penalised=(0,), duplicates=dup)


SLOT_CENTRES = ((36.0, 36.0), (116.0, 36.0), (36.0, 100.0))       # level-0 anchor centres; the 32 x 32 labels there are pairwise disjoint


def loss_case(nc=2):
    """L1 - L4: nine sub-cases, three images x three disjoint 32 x 32 labels; the level-0 anchor at each label's centre carries the
    prediction and is the unique cheapest candidate (k = 1).  label confidences are powers of two (``label_w`` of L6)."""
    subs = [('L1-equal', lambda c: (c[0], c[1], 32.0, 32.0)),
            ('L2-left', lambda c: (c[0] - 4, c[1], 24.0, 24.0)), ('L2-right', lambda c: (c[0] + 4, c[1], 24.0, 24.0)),
            ('L2-top', lambda c: (c[0], c[1] - 4, 24.0, 24.0)), ('L2-bottom', lambda c: (c[0], c[1] + 4, 24.0, 24.0)),
            ('L3-disjoint', lambda c: FAR), ('L4-inside', lambda c: (c[0], c[1], 16.0, 16.0)),
            ('L4-outside', lambda c: (c[0], c[1], 64.0, 64.0)), ('L2-corner', lambda c: (c[0] - 4, c[1] - 4, 24.0, 24.0))]
    bd = _Build('L-batch', B=3, nc=nc)
    where = {}
    for i, (name, f) in enumerate(subs):
        b, c = i // 3, SLOT_CENTRES[i % 3]
        bd.gt(i % nc, *c, b=b, conf=(2.0 ** (i % 3 - 1), 2.0 ** -(i % 2)))
        a = bd.put(0, int(c[1] - 4) // 8, int(c[0] - 4) // 8, f(c), cls=i % nc, b=b)
        where[name] = (b, a)
    case = bd.done(where=where)
    # graded objectness logits on the anchors outside every centre region: the objectness column has substance, the assignment none of it
    out, lab = case['outputs'], case['labels']
    for b in range(out.shape[0]):
        free = ~in_centers(lab[b, :, 1:3], SMALL).any(0)
        idx = torch.nonzero(free).flatten()
        out[b, idx, 4] = ((idx % 5).float() - 2.0)
    return case


def iou_loss_grad(pred, tgt, share=0.5):
    """d(1 - iou^2) / d(cx, cy, w, h) of losses.py's IOUloss in float64, an edge that coincides with the label's taking ``share`` of the
    term (autograd of torch.max / torch.min: 1/2)"""
    px, py, pw, ph = [pred[:, i].double() for i in range(4)]
    tx, ty, tw, th = [tgt[:, i].double() for i in range(4)]
    p_l, p_r, p_t, p_b = px - pw / 2, px + pw / 2, py - ph / 2, py + ph / 2
    t_l, t_r, t_t, t_b = tx - tw / 2, tx + tw / 2, ty - th / 2, ty + th / 2
    tlx, tly, brx, bry = torch.max(p_l, t_l), torch.max(p_t, t_t), torch.min(p_r, t_r), torch.min(p_b, t_b)
    en = ((tlx < brx) & (tly < bry)).double()
    iw, ih = brx - tlx, bry - tly
    ai = iw * ih * en
    u = pw * ph + tw * th - ai + 1e-16
    iou = ai / u
    w = lambda a, b: torch.where(a == b, torch.full_like(a, share), (a > b).double())  # noqa: E731
    al, ar, at, ab = w(p_l, t_l), w(t_r, p_r), w(p_t, t_t), w(t_b, p_b)
    dI, dP = (u + ai) / (u * u), -ai / (u * u)
    dtlx, dbrx, dtly, dbry = -ih * en, ih * en, -iw * en, iw * en
    dpx, dpy = dtlx * al + dbrx * ar, dtly * at + dbry * ab
    dpw, dph = -0.5 * dtlx * al + 0.5 * dbrx * ar, -0.5 * dtly * at + 0.5 * dbry * ab
    k = -2.0 * iou
    return torch.stack([k * dI * dpx, k * dI * dpy, k * (dI * dpw + dP * ph), k * (dI * dph + dP * pw)], 1)


# ------------------------------------------------------------------------------------------------------------------------------------------
# NMS
# ------------------------------------------------------------------------------------------------------------------------------------------
def _nms(boxes, scores, thr, mut=None):
    """oracle.nms.nms with the mutation hooks"""
    n = boxes.shape[0]
    x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    areas = ((x2 - x1).astype(F32) * (y2 - y1).astype(F32)).astype(F32)
    order = np.argsort(-scores, kind='stable')
    if mut == 'tie_reversed':
        order = np.lexsort((-np.arange(n), -scores))
    thr = F32(thr)
    sup, keep = np.zeros(n, dtype=bool), []
    for pos in range(n):
        i = order[pos]
        if sup[i]:
            if mut != 'removed_suppresses':
                continue
        else:
            keep.append(i)
        rest = order[pos + 1:]
        if rest.size == 0:
            break
        w = np.maximum(F32(0), (np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest])).astype(F32))
        h = np.maximum(F32(0), (np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest])).astype(F32))
        inter = (w * h).astype(F32)
        with np.errstate(divide='ignore', invalid='ignore'):
            ovr = (inter / ((areas[i] + areas[rest]).astype(F32) - inter).astype(F32)).astype(F32)
        sup[rest[(ovr >= thr) if mut == 'nms_ge' else (ovr > thr)]] = True
    return np.asarray(keep, dtype=np.int64)


def nms_reference(pred, nc, conf_thre, nms_thre, class_agnostic=False, max_det=None, vanilla_limit=20000, mut=None):
    """one image.  pred [A, 5 + nc] (cx, cy, w, h, obj, cls..) or, nc == 0, [A, 7] (x1, y1, x2, y2, obj, cls_conf, cls_id) -> det [k, 7]"""
    p = np.asarray(pred, dtype=F32)
    if nc > 0:
        b = np.stack([p[:, 0] - p[:, 2] / F32(2), p[:, 1] - p[:, 3] / F32(2), p[:, 0] + p[:, 2] / F32(2), p[:, 1] + p[:, 3] / F32(2)], 1)
        cls = p[:, 5:5 + nc]
        cid = (nc - 1 - np.argmax(cls[:, ::-1], 1)) if mut == 'argmax_last' else np.argmax(cls, 1)
        cc = cls[np.arange(len(p)), cid]
    else:
        b, cc, cid = p[:, :4], p[:, 5], p[:, 6].astype(np.int64)
    score = (p[:, 4] * cc).astype(F32)
    m = score > F32(conf_thre) if mut == 'conf_gt' else score >= F32(conf_thre)
    det = np.concatenate([b, p[:, 4:5], cc[:, None], cid[:, None].astype(F32)], 1).astype(F32)[m]
    if not len(det):
        return det
    bx, sc, ids = det[:, :4], score[m], det[:, 6]
    if class_agnostic:
        keep = _nms(bx, sc, nms_thre, mut)
    elif (bx.size >= vanilla_limit) if mut == 'limit_ge' else (bx.size > vanilla_limit):
        mask = np.zeros(len(sc), dtype=bool)
        for c in np.unique(ids):
            cur = np.nonzero(ids == c)[0]
            mask[cur[_nms(bx[cur], sc[cur], nms_thre, mut)]] = True
        keep = np.nonzero(mask)[0]
        keep = keep[np.lexsort((-keep, -sc[keep]))] if mut == 'tie_reversed' else keep[np.argsort(-sc[keep], kind='stable')]
    else:
        off = np.zeros(len(sc), F32) if mut == 'no_class_offset' else (ids.astype(F32) * (bx.max() + F32(1)).astype(F32)).astype(F32)
        keep = _nms((bx + off[:, None]).astype(F32), sc, nms_thre, mut)
    det = det[keep]
    return det if max_det is None else det[:max_det]


def _xyxy_rows(boxes, obj, cls):
    """integer corner boxes -> rows (cx, cy, w, h, obj, cls..): the conversion back is exact"""
    b = np.asarray(boxes, dtype=np.float64)
    cls = np.asarray(cls, dtype=np.float64).reshape(len(b), -1)
    r = np.concatenate([(b[:, 0:1] + b[:, 2:3]) / 2, (b[:, 1:2] + b[:, 3:4]) / 2, b[:, 2:3] - b[:, 0:1], b[:, 3:4] - b[:, 1:2],
                        np.asarray(obj, dtype=np.float64).reshape(-1, 1), cls], 1)
    r32 = r.astype(F32)
    assert np.array_equal(r32.astype(np.float64), r)
    assert np.array_equal((r32[:, 0] - r32[:, 2] / F32(2)).astype(np.float64), b[:, 0]) and \
        np.array_equal((r32[:, 1] + r32[:, 3] / F32(2)).astype(np.float64), b[:, 3])
    return r32


def _grid_boxes(n, y0=0):
    """n pairwise disjoint 10 x 10 boxes, 40 per row"""
    i = np.arange(n)
    x, y = 20 * (i % 40), y0 + 20 * (i // 40)
    return np.stack([x, y, x + 10, y + 10], 1)


CHAIN = np.array([[0, 5000, 16, 5010], [5, 5000, 21, 5010], [10, 5000, 26, 5010]])      # A > B > C (IoU 11/21), A and C at 6/26: C survives
CHAIN_SCORES = (0.5, 0.4375, 0.375)


def _interleave_junk(rows, every=3):
    """a below-threshold row after every ``every`` rows: the ordered compaction has something to skip"""
    out = []
    junk = np.zeros(rows.shape[1], F32)
    junk[:4] = (5, 5, 2, 2)
    for i, r in enumerate(rows):
        out.append(r)
        if i % every == every - 1:
            out.append(junk)
    return np.stack(out)


def nms_case(name, rows, nc, conf=0.25, thr=0.45, **kw):
    d = dict(name=name, pred=np.ascontiguousarray(rows, dtype=F32), nc=nc, conf=conf, thr=thr, agnostic=False, limit=20000, max_det=None)
    d.update(kw)
    return d


def n1_cases():
    out = []
    for n in (1, 2, 63, 64, 65, 128, 129, 1025):
        cls = np.where((np.arange(n) % 2 == 0)[:, None], [[0.5, 0.25]], [[0.25, 0.5]])
        out.append(nms_case(f'N1-equal-{n}', _interleave_junk(_xyxy_rows(_grid_boxes(n), np.ones(n), cls)), 2))
    n = 200                                    # runs of equal scores: 0.5 x 7, 0.75 x 5, 0.5 x 7, ...
    sc = np.where((np.arange(n) // 6) % 2 == 0, 0.5, 0.75) * np.where(np.arange(n) % 11 == 0, 0.5, 1.0)
    out.append(nms_case('N1-runs', _interleave_junk(_xyxy_rows(_grid_boxes(n), np.ones(n), sc[:, None])), 1))
    return out


def n2_cases():
    pairs_half = [[0, 0, 20, 10], [0, 0, 10, 10], [100, 0, 110, 20], [100, 0, 110, 10]]                    # IoU 100 / 200
    pairs_916 = [[0, 100, 16, 116], [0, 100, 12, 112], [100, 100, 116, 116], [104, 104, 116, 116]]         # IoU 144 / 256
    zero = [[50, 50, 50, 50], [50, 50, 50, 50]]                                                            # 0 / 0: not greater
    boxes = np.array(pairs_half + pairs_916 + zero)
    sc = np.array([1, 0.5, 0.75, 0.5, 1, 0.5, 0.75, 0.5, 0.5, 0.5])
    rows = _xyxy_rows(boxes, np.ones(len(boxes)), sc[:, None])
    edge = _xyxy_rows(_grid_boxes(4, 300), [1, 1, 0.5, 0.5], np.array([0.25, 0.25 - 2.0 ** -12, 0.5, 0.5 - 2.0 ** -11])[:, None])
    return [nms_case('N2-half-kept', rows, 1, thr=0.5), nms_case('N2-production', rows, 1),
            nms_case('N2-conf-edge', edge, 1, conf=0.25)]


def _chain_rows(pos, nc=1):
    """``pos`` disjoint filler boxes with higher scores (equal: anchor order), then the chain: A sits at sorted position ``pos``"""
    boxes = np.concatenate([_grid_boxes(pos), CHAIN])
    sc = np.concatenate([np.full(pos, 0.75), CHAIN_SCORES])
    return _xyxy_rows(boxes, np.ones(len(boxes)), sc[:, None] if nc == 1 else np.stack([sc, sc / 2], 1))


def n3_cases():
    return [nms_case(f'N3-chain-at-{p}', _interleave_junk(_chain_rows(p), 7), 1, chain_at=p) for p in (61, 62, 63, 64, 125, 126, 127, 128)]


def n4_cases():
    same = _xyxy_rows([[0, 0, 20, 20], [0, 0, 20, 20]], [1, 1], [[0.5, 0.25], [0.25, 0.5]])
    tie = _xyxy_rows([[0, 0, 20, 20], [40, 0, 60, 20]], [1, 1], [[0.5, 0.5, 0.25], [0.25, 0.5, 0.5]])
    # the two regimes differ: class 1 carries the offset 2^23 in the coordinate trick, where 22.5 rounds to 22 and the IoU 100 / 225 = 0.444
    # becomes 100 / 220 = 0.4545 > 0.45; the per-class loop sees the true boxes
    big = 2 ** 23 - 1
    trick = _xyxy_rows([[big - 10, 0, big, 10], [0, 0, 10, 10], [0, 0, 10, 22.5]], [1, 1, 1], [[0.5, 0.25], [0.25, 0.5], [0.25, 0.375]])
    # the same switch at torchvision's CPU limit, where oracle.postproc itself can state both sides: 1000 candidates are 4000 box elements
    # (not above the limit: coordinate trick), 1001 are 4004 (per-class loop).  The fillers are class 0 (offset 0) and disjoint
    def at_limit(n):
        fill = _xyxy_rows(_grid_boxes(n - 3, 100), np.ones(n - 3), np.tile([[0.5, 0.25]], (n - 3, 1)))
        return np.concatenate([trick, fill])
    return [nms_case('N4-limit4000-at', at_limit(1000), 2, limit=4000), nms_case('N4-limit4000-above', at_limit(1001), 2, limit=4000),
            nms_case('N4-same-box-trick', same, 2, limit=8), nms_case('N4-same-box-loop', same, 2, limit=7),
            nms_case('N4-same-box-agnostic', same, 2, agnostic=True), nms_case('N4-equal-conf', tie, 3),
            nms_case('N4-rounding-trick', trick, 2, limit=12), nms_case('N4-rounding-loop', trick, 2, limit=11)]


def n5_case():
    return nms_case('N5-max-det', _interleave_junk(_chain_rows(62), 5), 1, max_det=10)


def n6_cases():
    out = []
    for A, ncand in ((5600, 4096), (5600, 4097), (5040, 5040)):
        rows = _chain_rows(ncand - 3)
        junk = np.zeros((A - ncand, rows.shape[1]), F32)
        junk[:, :4] = (5, 5, 2, 2)
        # the junk rows go in front and in the middle, the chain stays last in anchor and in sorted order
        k = (A - ncand) // 2
        out.append(nms_case(f'N6-A{A}-n{ncand}', np.concatenate([junk[:k], rows[:1000], junk[k:], rows[1000:]]), 1, ncand=ncand))
    return out


def n7_case():
    """TTA-merge rows (x1, y1, x2, y2, obj, cls_conf, cls_id), num_classes = 0; padding rows carry a score of -1"""
    boxes = np.concatenate([CHAIN, CHAIN, _grid_boxes(5, 300)]).astype(np.float64)
    n = len(boxes)
    rows = np.zeros((n + 4, 7))
    rows[:n, :4] = boxes
    rows[:n, 4] = 1
    rows[:n, 5] = list(CHAIN_SCORES) + list(CHAIN_SCORES) + [0.5] * 5
    rows[:n, 6] = [0, 0, 0, 1, 1, 1, 2, 0, 2, 1, 0]
    rows[n:, 4] = -1.0
    rows[n:, 5] = 1.0
    return nms_case('N7-tta-rows', rows.astype(F32), 0)


def nms_cases():
    return n1_cases() + n2_cases() + n3_cases() + n4_cases() + [n5_case()] + n6_cases() + [n7_case()]


# ------------------------------------------------------------------------------------------------------------------------------------------
# pseudo-label filter
# ------------------------------------------------------------------------------------------------------------------------------------------
def pseudo_reference(det, cnt, obj_thr, cls_thr, filter_boxes, frame_hw, mut=None):
    """oracle.postproc.pred2label on padded rows: det [B, max_det, 7], cnt [B] -> list of [m, 8] (t = 0, x, y, w, h, cls_id, cls_conf, obj)"""
    out = []
    fh, fw = frame_hw
    gt = (lambda a, t: a >= F32(t)) if mut == 'thr_ge' else (lambda a, t: a > F32(t))
    for b, n in enumerate(cnt):
        if n < 0:
            out.append(None)
            continue
        d = np.asarray(det[b][:n], dtype=F32)
        ob, cc, cid = d[:, 4], d[:, 5], d[:, 6]
        if isinstance(obj_thr, float):
            sel = gt(ob, obj_thr) & gt(cc, cls_thr)
        else:
            so, sc = np.zeros(n, bool), np.zeros(n, bool)
            for i, (to, tc) in enumerate(zip(obj_thr, cls_thr)):
                so |= (cid == i) & gt(ob, to)
                sc |= (cid == i) & gt(cc, tc)
            sel = so & sc
        x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
        if filter_boxes:
            x1, x2 = np.clip(x1, 0, F32(fw - 1)), np.clip(x2, 0, F32(fw - 1))
            y1, y2 = np.clip(y1, 0, F32(fh - 1)), np.clip(y2, 0, F32(fh - 1))
            w, h = x2 - x1, y2 - y1
            maxw = F32(0.9 * fw) if mut == 'maxw_float' else F32((9 * fw) // 10)
            sel &= (w > 0) & (h > 0) & ((w > 5) & (h > 5) if mut == 'w_gt5' else (w >= 5) & (h >= 5)) & (w <= maxw)
        z = np.zeros(n, F32)
        out.append(np.stack([z, x1, y1, x2 - x1, y2 - y1, cid, cc, ob], 1).astype(F32)[sel])
    return out


def pseudo_cases():
    S = 2.0 ** -10
    cases = []

    def rows(spec):             # (x1, y1, x2, y2, obj, cls_conf, cls_id)
        return np.asarray(spec, dtype=F32)

    def case(name, per_image, obj_thr, cls_thr, filt, frame, cnt=None):
        md = max(len(r) for r in per_image)
        det = np.full((len(per_image), md, 7), SENTINEL, F32)
        for b, r in enumerate(per_image):
            det[b, :len(r)] = r
        cases.append(dict(name=name, det=det, cnt=[len(r) for r in per_image] if cnt is None else cnt, obj_thr=obj_thr, cls_thr=cls_thr,
                          filter=filt, frame=frame))

    bx = [10, 10, 50, 50]
    case('P1-scalar', [rows([bx + [0.5, 0.75, 0], bx + [0.75, 0.5, 0], bx + [0.5 + S, 0.5 + S, 1], bx + [0.5 + S, 0.5, 1], bx + [1, 1, 0]])],
         0.5, 0.5, True, (240, 304))
    case('P1-per-class', [rows([bx + [0.5, 0.75, 0], bx + [0.5 + S, 0.5 + S, 0], bx + [0.25 + S, 0.25 + S, 1], bx + [0.25, 1, 1],
                                bx + [1, 1, 2], bx + [0.375, 0.375, 0], bx + [1, 1, 1]])], [0.5, 0.25], [0.5, 0.25], True, (240, 304))
    for name, frame, mw in (('P2-gen1', (240, 304), 273), ('P2-gen4ds2', (360, 640), 576)):
        fh, fw = frame
        case(name, [rows([[10, 10, 15, 20, 1, 1, 0], [10, 10, 14.5, 20, 1, 1, 0], [10, 10, 20, 15, 1, 1, 0], [10, 10, 20, 14.5, 1, 1, 0],
                          [-3, 10, 5, 20, 1, 1, 0], [-3, 10, 4.5, 20, 1, 1, 0],                      # clamped to width 5 / 4.5
                          [fw - 6, 10, fw + 9, 20, 1, 1, 0], [fw - 5.5, 10, fw + 9, 20, 1, 1, 0],     # right edge: fw - 1 - x1 = 5 / 4.5
                          [10, 10, 10 + mw, 20, 1, 1, 0], [10, 10, 11 + mw, 20, 1, 1, 0], [10, 10, 10.5 + mw, 20, 1, 1, 0],
                          [fw + 5, 10, fw + 50, 30, 1, 1, 0], [-50, -40, -5, -4, 1, 1, 0], [10, fh - 6, 30, fh + 10, 1, 1, 0],
                          [10, fh - 5.5, 30, fh + 10, 1, 1, 0]])], 0.5, 0.5, True, frame)
    case('P2-unfiltered', [rows([[10, 10, 14, 20, 1, 1, 0], [-50, -40, -5, -4, 1, 1, 0], [0, 0, 300, 20, 0.5, 1, 0]])], 0.5, 0.5, False,
         (240, 304))
    for n in (64, 65, 130):
        r = np.zeros((n, 7), F32)
        r[:, 0], r[:, 1], r[:, 2], r[:, 3] = np.arange(n), 10, np.arange(n) + 20, 40
        r[:, 4] = np.where(np.arange(n) % 2 == 0, 1.0, 0.5)
        r[:, 5] = 1
        # second image: keep two, drop one
        r2 = r.copy()
        r2[:, 4] = np.where(np.arange(n) % 3 != 2, 1.0, 0.5)
        case(f'P3-alternating-{n}', [r, r2[:n - 1]], 0.5, 0.5, True, (240, 304))
    case('P4-overflow-count', [rows([bx + [1, 1, 0]]), rows([bx + [1, 1, 0]])], 0.5, 0.5, True, (240, 304), cnt=[-1, 1])
    return cases


# ------------------------------------------------------------------------------------------------------------------------------------------
# head prediction convs
# ------------------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _sparse(rows, cols, k, mags, g, dtype=torch.float32):
    w = torch.zeros((rows, cols), dtype=dtype)
    m = torch.tensor(mags, dtype=dtype)
    for r in range(rows):
        c = torch.randperm(cols, generator=g)[:k]
        w[r, c] = m[torch.randint(0, len(mags), (k,), generator=g)] * (torch.randint(0, 2, (k,), generator=g).to(dtype) * 2 - 1)
    return w


@functools.lru_cache(maxsize=None)
def pred_problem(B, h, w, Hd, nc, stride, seed=0):
    """operands of one level (docstring) and the float64 reference: raw, decoded train / infer rows, and for ``d_raw`` in {0, +-1, +-2}
    the feature, weight and bias gradients"""
    g = _gen(B, h, w, Hd, nc, stride, seed)
    M = B * h * w
    feat = lambda: torch.randint(-2, 3, (M, Hd), generator=g).float()  # noqa: E731
    cf, rf = feat(), feat()
    mags = (0.5, 1.0, 2.0)
    cw, rw, ow = _sparse(nc, Hd, min(4, Hd), mags, g), _sparse(4, Hd, min(4, Hd), (0.5,), g), _sparse(1, Hd, min(4, Hd), mags, g)
    rw[:2] *= 2
    bias = lambda n: torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0])[torch.randint(0, 5, (n,), generator=g)]  # noqa: E731
    cb, rb, ob = bias(nc), bias(4), bias(1)
    rb[2:] = 0.0
    # |raw_wh| <= 4: four terms of at most 2 x 1/2
    raw = torch.cat([rf.double() @ rw.double().T + rb.double(), rf.double() @ ow.double().T + ob.double(),
                     cf.double() @ cw.double().T + cb.double()], 1)
    assert float(raw[:, 2:4].abs().max()) <= 4.0 and float(raw.abs().max()) <= 17.0
    assert torch.equal(raw * 2, (raw * 2).round())
    p = torch.arange(M) % (h * w)
    grid = torch.stack([(p % w).double(), (p // w).double()], 1)
    xy, wh = (raw[:, :2] + grid) * stride, torch.exp(raw[:, 2:4]) * stride
    train = torch.cat([xy, wh, raw[:, 4:]], 1).view(B, h * w, 5 + nc)
    infer = torch.cat([xy, wh, torch.sigmoid(raw[:, 4:])], 1).view(B, h * w, 5 + nc)
    d = torch.randint(-2, 3, (M, 5 + nc), generator=g).float()
    dd = d.double()
    grads = dict(dcf=dd[:, 5:] @ cw.double(), drf=dd[:, :4] @ rw.double() + dd[:, 4:5] @ ow.double(),
                 dcw=dd[:, 5:].T @ cf.double(), dcb=dd[:, 5:].sum(0), drw=dd[:, :4].T @ rf.double(), drb=dd[:, :4].sum(0),
                 dow=dd[:, 4:5].T @ rf.double(), dob=dd[:, 4:5].sum(0))
    span = max(float((dd.abs().T @ cf.double().abs()).max()) if nc else 0.0, float((dd.abs().T @ rf.double().abs()).max()))
    assert span * 16 < 2 ** 24, 'a weight gradient leaves the exact range (gscale <= 8, start value included)'
    return dict(cf=cf.view(B, h, w, Hd), rf=rf.view(B, h, w, Hd), cw=cw, cb=cb, rw=rw, rb=rb, ow=ow, ob=ob, raw=raw, train=train, infer=infer,
                d=d.view(B, h * w, 5 + nc), grads=grads)


# ------------------------------------------------------------------------------------------------------------------------------------------
# case lists, loss reference
# ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def assign_cases():
    """every SimOTA case, by name; S7: the S2 - S4 problems again with 130 label rows, and the big head"""
    cases = s1_cases() + s2_cases() + s3_cases() + s4_cases() + s5_cases() + s6_cases() + [s8_case(), loss_case()]
    cases += s2_cases(nmax=130, tag='@130') + s3_cases(nmax=130, tag='@130') + s4_cases(nmax=130, tag='@130') + [s7_big_case()]
    out = {c['name']: c for c in cases}
    assert len(out) == len(cases)
    return out


LOSS_KEYS = ('loss', 'iou_loss', 'conf_loss', 'cls_loss', 'l1_loss', 'num_fg')


def loss_reference(case, focal=False, weighted=False):
    """oracle.head.get_losses with autograd on the case's tensors -> (losses [6], d_raw reference with the decode chain applied, the
    oracle's result dict).  ``weighted``: bbox_loss_weighting = 'obj', i.e. label_w = labels[..., 5]"""
    geom = case['geom']
    gx, gy, gs = oh.make_grids(geom.hws, geom.strides)
    outr = case['outputs'].clone().requires_grad_(True)
    ref = oh.get_losses(gx, gy, gs, case['labels'].clone(), outr, num_classes=case['nc'], obj_focal_loss=focal, return_assign=True,
                        bbox_loss_weighting='obj' if weighted else '')
    want = torch.tensor([float(ref[k].detach() if torch.is_tensor(ref[k]) else ref[k]) for k in LOSS_KEYS])
    if ref['loss'].requires_grad:
        ref['loss'].backward()
    g = outr.grad.clone() if outr.grad is not None else torch.zeros_like(case['outputs'])
    g[..., 0:2] *= gs[None, :, None]
    g[..., 2:4] *= case['outputs'][..., 2:4]
    return want, g, ref


def pred_route(B, h, w, Hd, nc):
    """the launch condition of leod_head_pred_fwd (k_head.hip), restated: which forward kernel a shape reaches.  Mirrors, and has to
    follow, ``if (lds_on && Hd <= 128 && nc <= 16 && (long)B * h * w >= 4096)`` and ``if (Hd <= 96)`` in that function (the <96> / <128>
    instantiations of head_pred_fwd_lds_kernel; its grid is min(2048, ceil(B h w / 64)), which is what H4 overruns)"""
    if Hd <= 128 and nc <= 16 and B * h * w >= 4096:
        return 'lds96' if Hd <= 96 else 'lds128'
    return 'generic'


# (name, B, h, w, Hd, nc, stride, forward kernel, run the backward too)
PRED_CASES = [
    ('H1-hd96', 1, 67, 62, 96, 2, 8, 'lds96', False), ('H1-hd64', 1, 67, 62, 64, 2, 16, 'lds96', False),         # 4154 positions: 64 x 64 + 58
    ('H2-hd128', 1, 67, 62, 128, 3, 8, 'lds128', False), ('H2-hd100', 2, 67, 31, 100, 2, 32, 'lds128', False),
    ('H3-hd192', 1, 67, 62, 192, 2, 8, 'generic', False), ('H3-4095', 1, 63, 65, 96, 2, 8, 'generic', False),
    ('H3-nc17', 1, 67, 62, 96, 17, 8, 'generic', True),
    ('H4-grid-stride', 1, 66, 1987, 32, 1, 8, 'lds96', False),                                                  # 2048 x 64 + 70 positions
] + [(f'H5-nc{nc}', 3, 9, 11, 40, nc, 16, 'generic', True) for nc in (1, 3, 8, 9, 16)] + [
    ('H5-nc16-lds', 1, 64, 65, 32, 16, 8, 'lds96', False)]
H6_LEVELS = ((6, 8, 8, 5), (3, 4, 16, 5 + 48))                   # (h, w, stride, a0) of two levels sharing one output of A = 70 rows
H6_A = 70
