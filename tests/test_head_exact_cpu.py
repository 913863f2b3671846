"""Without a GPU: the operands and references of tests/head_exact.py do what its docstring says, on every case that
tests/test_head_exact_gpu.py runs --
(1) every generator assertion (exact IoUs, logit bands, the separation guard, the 1e6-penalty rule) and what each named case claims: the
    candidate counts at the centre boundary, the dynamic k, where the ties are and whether they straddle k;
(2) assign_reference equals oracle.head.get_assignments / get_losses on every case without a straddling tie, and on those with one the
    oracle's own choice has the same multiset of (gt, cost); zero-padding the labels to 130 rows changes nothing;
(3) nms_reference equals oracle.postproc.postprocess / tta_postprocess and oracle.nms on every case, pseudo_reference equals
    oracle.postproc.pred2label, iou_loss_grad with share 1/2 equals autograd of oracle.head.iou_loss_fn;
(4) every entry of MUTATIONS changes a discrete output of a committed case (the two gradient mutations: d_raw beyond the tolerance of the
    GPU test), and the one EQUIVALENT mutant changes none;
(5) the prediction-conv operands are exact and every row reaches the kernel it names; the case counts stay small."""
import numpy as np
import pytest
import torch

import head_exact as hx
from oracle import head as oh
from oracle import nms as onms
from oracle import postproc as op

CASES = hx.assign_cases()
INFO = {}


def info_of(name):
    if name not in INFO:
        INFO[name] = hx.check_assign(CASES[name])
    return INFO[name]


def ref_of(name, mut=None):
    c = CASES[name]
    return hx.assign_reference(c['outputs'], c['labels'], c['geom'], mut)


def discrete(r):
    return (r['fg_mask'].tolist(), r['ignore_mask'].tolist(), r['matched_valid_idx'].tolist(), r['matched_row'].tolist(),
            r['num_fg_img'].tolist(), r['totals'], r['status'])


# ---- (1) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_generator_assertions(name):
    info_of(name)


def _one(name, b=0):
    return info_of(name)[b]


def test_named_claims():
    # S1: level-0 candidates on the boundary and half a pixel inside it
    for c in hx.s1_cases():
        P = _one(c['name'])['P']
        l0 = [a for a in P['cand'] if a < hx.SMALL.a0[1]]
        ys, xs = {a // 20 for a in l0}, {a % 20 for a in l0}
        assert (len(ys), len(xs)) == c['level0_candidates'] and len(l0) == len(ys) * len(xs), c['name']
        assert int(ref_of(c['name'])['num_fg_img'][0]) == len(l0)
    # S2: the dynamic k
    want_k = {'S2-sum3': 3, 'S2-sum2.75': 2, 'S2-sum0.75': 1, 'S2-sum0': 1, 'S2-twelve-halves': 5, 'S2-ten-halves': 5, 'S2-rank10-tie': 5}
    for n, k in want_k.items():
        assert _one(n)['ks'] == [k] and _one(n + '@130')['ks'] == [k], n
    i = _one('S2-rank10-tie')
    top = sorted(i['P']['ious'][0].tolist(), reverse=True)
    assert top[9] == top[10] == top[11] == 0.25 and sum(top[:10]) == 5.75          # equal values across rank 10
    assert sum(1 for v in _one('S2-twelve-halves')['P']['ious'][0].tolist() if v > 0) == 12
    # S3: where the ties are
    i = _one('S3-straddle-levels')
    c = CASES['S3-straddle-levels']
    sel = [i['P']['cand'][j] for j in i['sels'][0]]
    g = hx.SMALL
    assert i['ks'] == [3] and i['straddle'] == [True]
    assert sel == [g.anchor(0, 7, 8), g.anchor(0, 9, 8), g.anchor(1, 4, 4)] and g.anchor(2, 2, 2) not in sel
    assert torch.equal(c['outputs'][0, g.anchor(0, 7, 8)], c['outputs'][0, g.anchor(1, 4, 4)])       # identical across two levels
    assert _one('S3-inside')['straddle'] == [False] and _one('S3-outside')['straddle'] == [False]
    for n in ('S3-inside', 'S3-outside'):
        cost = _one(n)['P']['cost'][0]
        assert len({cost[j] for j in _one(n)['sels'][0]}) == 1                    # a three-way tie wholly inside the top-k
    assert len({_one('S3-outside')['P']['cost'][0][j] for j in range(27)} - {_one('S3-outside')['P']['cost'][0][j] for j in _one('S3-outside')['sels'][0]}) >= 2
    # S4
    r = ref_of('S4-identical-rows')
    assert int(r['num_fg_img'][0]) == 3 and set(r['matched_valid_idx'][0][r['fg_mask'][0] > 0].tolist()) == {0}
    assert ref_of('S4-unequal')['matched_valid_idx'][0].max() == 0 and ref_of('S4-unequal-swapped')['matched_valid_idx'][0].max() == 1
    x_, y_ = CASES['S4-third-gt']['third']
    i, r = _one('S4-third-gt'), ref_of('S4-third-gt')
    jx = i['P']['cand'].index(x_)
    assert i['sels'][0] == [jx] and i['sels'][1] == [jx] and i['sels'][2] == [i['P']['cand'].index(y_)]
    assert r['matched_valid_idx'][0, x_] == 2 and r['matched_valid_idx'][0, y_] == 2 and int(r['num_fg_img'][0]) == 2
    # S5: the exact 100 decides
    for nc in (1, 2, 3):
        r = ref_of(f'S5-nc{nc}')
        assert r['fg_mask'][0].nonzero().flatten().tolist() == [hx.SMALL.anchor(0, 9, 9)]
        P = _one(f'S5-nc{nc}')['P']
        wrong, right = (P['cost'][0][P['cand'].index(hx.SMALL.anchor(0, y, y))] for y in (7, 9))
        assert wrong - right == (100.0 if nc == 1 else 200.0)
    # S6
    r, c = ref_of('S6-ignore'), CASES['S6-ignore']
    both, only = hx.SMALL.anchor(1, 4, 5), hx.SMALL.anchor(0, 8, 12)
    assert r['ignore_mask'][0, both] == 0 and both in _one('S6-ignore')['P']['cand'] and r['ignore_mask'][0, only] == 1
    assert int(r['ignore_mask'][1].sum()) > 0 and int(r['fg_mask'][1].sum()) == 0 and int(r['ignore_mask'][2].sum()) == 0
    r = ref_of('S6-ignore-first-row')
    fg = r['fg_mask'][0] > 0
    assert (r['matched_row'][0][fg] == r['matched_valid_idx'][0][fg] + 1).all()
    r = ref_of('S6-empty-batch')
    assert r['totals'] == [0, 0] and int(r['ignore_mask'].sum()) == 0
    r = ref_of('S6-no-candidate')
    assert r['status'] == 1 and r['totals'] == [1, 2] and r['num_fg_img'].tolist() == [0, 1]
    # S7: the tiers the shapes are here for.  Mirrors k_head.hip: ``#define MAXGT 128`` (per-gt arrays in LDS up to 128 label rows),
    # simota_cap() = min(A, 16 * nlv * Nmax) and, in leod_simota_assign, ``cand_in_lds = cap * 3 * sizeof(int) <= 120 * 1024``
    big = CASES['S7-big']
    nmax = big['labels'].shape[1]
    assert nmax > 128 and min(big['geom'].A, 48 * nmax) * 12 > 120 * 1024
    assert CASES['S3-inside@130']['labels'].shape[1] == 130 and min(420, 48 * 130) * 12 <= 120 * 1024
    # S8: two of four penalised duplicates, the lowest indices
    i, r, c = _one('S8-penalised'), ref_of('S8-penalised'), CASES['S8-penalised']
    assert i['ks'][0] == 5 and i['incount'][0] == 3 and i['straddle'][0]
    assert [bool(r['fg_mask'][0, a]) for a in c['duplicates']] == [True, True, False, False]
    # L: every sub-case's anchor is foreground, alone for its label
    r, c = ref_of('L-batch'), CASES['L-batch']
    assert r['num_fg_img'].tolist() == [3, 3, 3] and all(r['fg_mask'][b, a] == 1 for b, a in c['where'].values())
    assert not any(any(i['straddle']) for i in info_of('L-batch'))


# ---- (2) -----------------------------------------------------------------------------------------------------------------------------------
def _oracle(case):
    geom = case['geom']
    gx, gy, gs = oh.make_grids(geom.hws, geom.strides)
    return oh.get_losses(gx, gy, gs, case['labels'].clone(), case['outputs'].clone(), num_classes=case['nc'], return_assign=True)


@pytest.mark.parametrize('name', sorted(n for n in CASES if CASES[n].get('oracle', True)))
def test_reference_vs_oracle(name):
    case, info, r = CASES[name], info_of(name), ref_of(name)
    o = _oracle(case)
    assert torch.equal(r['ignore_mask'].bool(), o['_ignore_mask'])
    for b, a in enumerate(o['_assign']):
        fg_o = o['_fg_mask'][b]
        if a is None:
            assert int(r['num_fg_img'][b]) == 0 and int(r['fg_mask'][b].sum()) == 0
            continue
        assert int(r['num_fg_img'][b]) == a['num_fg']
        if not any(info[b]['straddle']):
            assert torch.equal(r['fg_mask'][b].bool(), fg_o)
            assert torch.equal(r['matched_valid_idx'][b][fg_o].long(), a['matched_gt_inds'])
            assert torch.equal(r['pred_iou'][b][fg_o], a['pred_ious'])
            continue
        # a tie straddles k: torch.topk picks other members of it, at the same costs
        cand = info[b]['P']['cand']
        col = {an: j for j, an in enumerate(cand)}
        mine = sorted((int(r['matched_valid_idx'][b, an]), float(a['cost'][int(r['matched_valid_idx'][b, an]), col[an]]))
                      for an in r['fg_mask'][b].nonzero().flatten().tolist())
        theirs = sorted((int(g), float(a['cost'][int(g), col[an]]))
                        for an, g in zip(fg_o.nonzero().flatten().tolist(), a['matched_gt_inds'].tolist()))
        assert mine == theirs, name
    assert r['totals'][1] == sum(int(a['cost'].shape[0]) for a in o['_assign'] if a is not None)


def test_padding_changes_nothing():
    for n in CASES:
        if n.endswith('@130'):
            assert discrete(ref_of(n)) == discrete(ref_of(n[:-4])) and torch.equal(ref_of(n)['pred_iou'], ref_of(n[:-4])['pred_iou'])


# ---- (3) -----------------------------------------------------------------------------------------------------------------------------------
NMS_CASES = hx.nms_cases()


@pytest.mark.parametrize('case', NMS_CASES, ids=lambda c: c['name'])
def test_nms_reference_vs_oracle(case):
    ref = hx.nms_reference(case['pred'], case['nc'], case['conf'], case['thr'], case['agnostic'], None, case['limit'])
    pred = torch.from_numpy(case['pred'])
    # corners integer (one half-integer in the rounding case), scores dyadic
    if case['nc'] > 0:
        sc = pred[:, 4].double() * pred[:, 5:].double().max(1).values
        assert torch.equal(sc * 4096, (sc * 4096).round())
    pad = torch.zeros((0, 7))
    if case['limit'] in (20000, 4000):
        sem = 'gpu' if case['limit'] == 20000 else 'cpu'
        if case['nc'] > 0:
            o = op.postprocess(pred[None].clone(), case['nc'], case['conf'], case['thr'], case['agnostic'], pad=pad, device_semantics=sem)[0]
        else:
            o = op.tta_postprocess([pred.clone()], case['conf'], case['thr'], case['agnostic'], pad=pad, device_semantics=sem)[0]
        assert np.array_equal(o.numpy(), ref), case['name']
    else:       # a limit of the test's own: the two regimes of oracle.nms, called directly
        m = (pred[:, 4] * pred[:, 5:].max(1).values) >= case['conf']
        p = case['pred'][m.numpy()]
        bx = np.stack([p[:, 0] - p[:, 2] / 2, p[:, 1] - p[:, 3] / 2, p[:, 0] + p[:, 2] / 2, p[:, 1] + p[:, 3] / 2], 1).astype(np.float32)
        cid = np.argmax(p[:, 5:], 1)
        sc = (p[:, 4] * p[:, 5:].max(1)).astype(np.float32)
        if bx.size > case['limit']:
            keep = np.zeros(len(sc), bool)
            for c in np.unique(cid):
                cur = np.nonzero(cid == c)[0]
                keep[cur[onms.nms(bx[cur], sc[cur], case['thr'])]] = True
            keep = np.nonzero(keep)[0]
            keep = keep[np.argsort(-sc[keep], kind='stable')]
        else:
            off = (cid.astype(np.float32) * (bx.max() + np.float32(1))).astype(np.float32)
            keep = onms.nms((bx + off[:, None]).astype(np.float32), sc, case['thr'])
        rows = np.concatenate([bx, p[:, 4:5], p[:, 5:].max(1)[:, None], cid[:, None].astype(np.float32)], 1).astype(np.float32)
        assert np.array_equal(ref, rows[keep]), case['name']


def test_nms_named_claims():
    by = {c['name']: c for c in NMS_CASES}
    run = lambda c, **kw: hx.nms_reference(c['pred'], c['nc'], c['conf'], c['thr'], c['agnostic'], c['max_det'], c['limit'], **kw)  # noqa: E731
    for n in (1, 2, 63, 64, 65, 128, 129, 1025):                        # equal scores: anchor order
        d = run(by[f'N1-equal-{n}'])
        assert len(d) == n and np.array_equal(d[:, :2], hx._grid_boxes(n)[:, :2].astype(np.float32))
    assert len(run(by['N2-half-kept'])) == 8 and len(run(by['N2-production'])) == 6       # IoU 1/2 kept at 0.5; 9/16 removed; 0/0 kept
    assert len(run(by['N2-conf-edge'])) == 2
    for c in hx.n3_cases():
        d, p = run(c), c['chain_at']
        assert len(d) == p + 2 and np.array_equal(d[p, :4], hx.CHAIN[0].astype(np.float32)) and np.array_equal(d[p + 1, :4], hx.CHAIN[2].astype(np.float32))
    assert len(run(by['N4-same-box-trick'])) == 2 and len(run(by['N4-same-box-loop'])) == 2 and len(run(by['N4-same-box-agnostic'])) == 1
    assert run(by['N4-equal-conf'])[:, 6].tolist() == [0.0, 1.0]
    assert len(run(by['N4-rounding-trick'])) == 2 and len(run(by['N4-rounding-loop'])) == 3
    assert len(run(by['N4-limit4000-at'])) == 999 and len(run(by['N4-limit4000-above'])) == 1001       # 4n > limit, not >=
    assert np.array_equal(by['N4-rounding-trick']['pred'], by['N4-rounding-loop']['pred'])
    assert len(run(by['N5-max-det'])) == 10 < len(run(dict(by['N5-max-det'], max_det=None)))
    for c in hx.n6_cases():
        A, n = c['pred'].shape[0], c['ncand']
        assert int(((c['pred'][:, 4] * c['pred'][:, 5]) >= c['conf']).sum()) == n and len(run(c)) == n - 1
        np2 = 1 << (A - 1).bit_length()
        # mirrors k_head.hip: nms_array_bytes(cap) = np2 * 8 + cap * 17 + 16 and, in leod_postprocess_nms,
        # ``cap = lds_bytes(A) <= 156 * 1024 ? A : 4096``: 5600 anchors get the 4096-candidate LDS tier plus the workspace
        assert (np2 * 8 + A * 17 + 16 > 156 * 1024) == (A == 5600)
    d = run(by['N7-tta-rows'])
    assert len(d) == 9 and (d[:, 4] == 1).all()


PSEUDO_CASES = hx.pseudo_cases()
DATASETS = {(240, 304): ('gen1', False), (360, 640): ('gen4', True)}


@pytest.mark.parametrize('case', PSEUDO_CASES, ids=lambda c: c['name'])
def test_pseudo_reference_vs_oracle(case):
    ref = hx.pseudo_reference(case['det'], case['cnt'], case['obj_thr'], case['cls_thr'], case['filter'], case['frame'])
    ds, ds2 = DATASETS[case['frame']]
    live = [b for b, n in enumerate(case['cnt']) if n >= 0]
    o = op.pred2label([torch.from_numpy(case['det'][b, :case['cnt'][b]]) for b in live], case['obj_thr'], case['cls_thr'], ds, ds2, case['filter'])
    for b, ob in zip(live, o):
        assert np.array_equal(ob.numpy(), ref[b]), case['name']
    assert [r is None for r in ref] == [n < 0 for n in case['cnt']]
    if case['name'].startswith('P3'):
        assert all(0 < len(r) < n for r, n in zip(ref, case['cnt']))


def _loss_boxes():
    case = CASES['L-batch']
    rows = sorted(case['where'].items())
    pred = torch.stack([case['outputs'][b, a, :4] for _, (b, a) in rows]).double()
    r = ref_of('L-batch')
    tgt = torch.stack([case['labels'][b, int(r['matched_row'][b, a]), 1:5] for _, (b, a) in rows]).double()
    return [n for n, _ in rows], pred, tgt


def test_iou_loss_grad_is_autograd_at_half():
    names, pred, tgt = _loss_boxes()
    p = pred.clone().requires_grad_(True)
    oh.iou_loss_fn(p, tgt).sum().backward()
    g = hx.iou_loss_grad(pred, tgt, 0.5)
    assert float((g - p.grad).abs().max()) < 1e-15
    tied = {n: int(((pred[i, :2] - pred[i, 2:] / 2 == tgt[i, :2] - tgt[i, 2:] / 2).sum() + (pred[i, :2] + pred[i, 2:] / 2 == tgt[i, :2] + tgt[i, 2:] / 2).sum()))
            for i, n in enumerate(names)}
    assert tied == {'L1-equal': 4, 'L2-left': 1, 'L2-right': 1, 'L2-top': 1, 'L2-bottom': 1, 'L2-corner': 2, 'L3-disjoint': 0, 'L4-inside': 0,
                    'L4-outside': 0}
    i = names.index('L3-disjoint')
    assert float(g[i].abs().max()) == 0.0 and float(oh.iou_loss_fn(pred[i:i + 1], tgt[i:i + 1])) == 1.0


# ---- (4) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mut', hx.SIMOTA_MUTATIONS)
def test_simota_mutation_is_seen(mut):
    seen = [n for n in CASES if discrete(ref_of(n, mut)) != discrete(ref_of(n))]
    assert seen, f'{mut}: no committed case notices'
    print(mut, seen)


def test_iou_le_is_equivalent():
    """``tl <= br`` in the IoU: where it differs from ``tl < br`` a side of the intersection is 0, so the area is 0 either way"""
    for n, c in CASES.items():
        for b in range(c['outputs'].shape[0]):
            lab = c['labels'][b].double()
            gt = lab[lab.sum(1) > 0][:, 1:5]
            if not len(gt):
                continue
            pr = c['outputs'][b, :, :4].double()
            tl = torch.max(gt[:, None, :2] - gt[:, None, 2:] / 2, pr[:, :2] - pr[:, 2:] / 2)
            br = torch.min(gt[:, None, :2] + gt[:, None, 2:] / 2, pr[:, :2] + pr[:, 2:] / 2)
            lt, le = (tl < br).double().prod(2), (tl <= br).double().prod(2)
            assert torch.equal(torch.prod(br - tl, 2) * lt, torch.prod(br - tl, 2) * le), n
    assert any(True for _ in hx.EQUIVALENT)


@pytest.mark.parametrize('mut', hx.NMS_MUTATIONS)
def test_nms_mutation_is_seen(mut):
    seen = []
    for c in NMS_CASES:
        a = hx.nms_reference(c['pred'], c['nc'], c['conf'], c['thr'], c['agnostic'], c['max_det'], c['limit'])
        b = hx.nms_reference(c['pred'], c['nc'], c['conf'], c['thr'], c['agnostic'], c['max_det'], c['limit'], mut=mut)
        if not np.array_equal(a, b):
            seen.append(c['name'])
    assert seen, f'{mut}: no committed case notices'
    print(mut, seen)


@pytest.mark.parametrize('mut', hx.PSEUDO_MUTATIONS)
def test_pseudo_mutation_is_seen(mut):
    seen = []
    for c in PSEUDO_CASES:
        a = hx.pseudo_reference(c['det'], c['cnt'], c['obj_thr'], c['cls_thr'], c['filter'], c['frame'])
        b = hx.pseudo_reference(c['det'], c['cnt'], c['obj_thr'], c['cls_thr'], c['filter'], c['frame'], mut=mut)
        if any((x is None) != (y is None) or (x is not None and not np.array_equal(x, y)) for x, y in zip(a, b)):
            seen.append(c['name'])
    assert seen, f'{mut}: no committed case notices'


@pytest.mark.parametrize('mut,share', [('edge_share_0', 0.0), ('edge_share_1', 1.0)])
@pytest.mark.parametrize('weighted', [False, True])
def test_loss_mutation_is_beyond_the_tolerance(mut, share, weighted):
    """d_raw with the edge-tie share 0 (a tied edge gets nothing) or 1 against autograd: outside rtol 1e-4, atol 1e-7 + 5e-6 max |ref| of
    test_kernels_gpu.close on every sub-case that has a tied edge, inside it (equal) on every other"""
    assert hx.MUTATIONS[mut] == 'loss'
    case = CASES['L-batch']
    names, pred, tgt = _loss_boxes()
    want, gref, o = hx.loss_reference(case, weighted=weighted)
    scale = float(gref.abs().max())
    num_fg = 9.0
    gs = oh.make_grids(case['geom'].hws, case['geom'].strides)[2]
    delta = hx.iou_loss_grad(pred, tgt, share) - hx.iou_loss_grad(pred, tgt, 0.5)          # d(1 - iou^2) per box, before the weights
    for i, n in enumerate(names):
        b, a = case['where'][n]
        w = 1.0
        if weighted:
            lw = torch.stack([case['labels'][bb, int(ref_of('L-batch')['matched_row'][bb, aa]), 5] for bb, aa in case['where'].values()]).double()
            w = float(case['labels'][b, int(ref_of('L-batch')['matched_row'][b, a]), 5]) / float(lw.mean())
        chain = torch.tensor([float(gs[a]), float(gs[a]), float(pred[i, 2]), float(pred[i, 3])], dtype=torch.float64)
        d = delta[i] * 5.0 / num_fg * w * chain
        tol = 1e-7 + 5e-6 * scale + 1e-4 * gref[b, a, :4].abs().double()
        tied = n.startswith(('L1', 'L2'))
        assert bool((d.abs() > tol).any()) == tied, (n, d.tolist(), tol.tolist())
        if tied:
            assert float(d.abs().max()) > 100 * float(tol.max()), n


# ---- (5) -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', hx.PRED_CASES, ids=lambda r: r[0])
def test_pred_operands(row):
    name, B, h, w, Hd, nc, stride, route, bwd = row
    assert hx.pred_route(B, h, w, Hd, nc) == route and Hd % 4 == 0
    p = hx.pred_problem(B, h, w, Hd, nc, stride)
    assert hx.pred_problem(B, h, w, Hd, nc, stride) is p
    # every |term| sum of a row stays far below 2^24 quanta of 1/2: exact in any order
    for f, ws in ((p['rf'], (p['rw'], p['ow'])), (p['cf'], (p['cw'],))):
        for wt in ws:
            assert float((f.view(-1, Hd).abs().double() @ wt.abs().double().T).max()) + 1 < 2 ** 6
            assert int((wt != 0).sum(1).max()) <= 4
    assert torch.equal(p['train'][..., :2], p['train'][..., :2].float().double())          # xy exact in fp32
    assert float(p['train'][..., 2:4].min()) >= stride * np.exp(-4.0) * 0.999
    for v in p['grads'].values():
        assert torch.equal(v * 2, (v * 2).round()) and float(v.abs().max()) * 16 < 2 ** 24
    if name.startswith('H1') or name.startswith('H2'):
        assert B * h * w == 4154 and (B * h * w) % 64 == 58
    if name == 'H4-grid-stride':
        assert B * h * w == 2048 * 64 + 70
    if name == 'H3-4095':
        assert B * h * w == 4095


def test_pred_rows_cover_the_routes():
    routes = {(r[7], r[4]) for r in hx.PRED_CASES}
    assert {('lds96', 96), ('lds96', 64), ('lds128', 128), ('lds128', 100), ('generic', 192), ('generic', 96)} <= routes
    assert {r[5] for r in hx.PRED_CASES if r[8]} >= {1, 3, 8, 9, 16, 17}
    assert hx.PRED_RTOL == 2.0 ** -19
    a = sorted((a0, a0 + h * w) for h, w, s, a0 in hx.H6_LEVELS)
    assert a[0][0] > 0 and a[0][1] == a[1][0] and a[1][1] < hx.H6_A


def test_case_counts():
    n = len(CASES) + len(NMS_CASES) + len(PSEUDO_CASES) + len(hx.PRED_CASES) + 1 + 4 + 2
    assert n < 200, n
    assert set(hx.MUTATIONS.values()) == {'simota', 'nms', 'pseudo', 'loss'} and len(hx.MUTATIONS) == 20
