"""The head tail (csrc/k_head.hip) on the operands of tests/head_exact.py, where every tie and every threshold has one right answer:
``torch.equal`` / ``np.array_equal`` on the assignment masks, indices and counts, the NMS keep order and detection rows and the pseudo-label
rows; the tolerances of test_kernels_gpu.test_simota_and_loss on the losses and d_raw; equality on everything exact of the prediction
convs and the bound head_exact.PRED_RTOL on their exp / sigmoid columns.

Groups (head_exact's docstring and case builders say what each case holds):
  SimOTA  S1 centre boundary, S2 dynamic k, S3 cost ties (inside, outside, straddling k, across FPN levels), S4 anchors claimed by several
          boxes, S5 class term, S6 ignore boxes / empty images / a box without candidates, S7 the workspace tiers (130 label rows; the
          768 x 768 head with 214), S8 selection among penalised duplicates -- against head_exact.assign_reference
  loss    L1 - L8 on the nine sub-cases of head_exact.loss_case (prediction equal to its label, one edge tied, a corner tied, disjoint,
          inside, outside), plain / focal / weighted / without gradient, and the empty batch -- against oracle.head.get_losses + autograd
  NMS     N1 score ties, N2 thresholds, N3 chains across the 64-box chunk boundary, N4 classes and the two regimes, N5 max_det,
          N6 the LDS / workspace tiers, N7 TTA rows -- against head_exact.nms_reference (= the oracle, tests/test_head_exact_cpu.py)
  filter  P1 - P4 -- against head_exact.pseudo_reference (= oracle.postproc.pred2label)
  pred    H1 - H6: both LDS instantiations, the generic kernel, the grid-stride loop, the class-channel groups of the backward, two levels
          into one output.  The route of every row is head_exact.pred_route, the launch condition restated.
Outputs are pre-filled with a sentinel wherever the entry point takes the buffer: what a call must leave alone stays bit-identical.
``pytest -m gpu``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_exact as hx  # noqa: E402
import test_kernels_gpu as tk  # noqa: E402

DEV = 'cuda'


@pytest.fixture
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as _ops
    prev = _ops.get_precision()
    _ops.set_precision('f32')
    yield _ops
    _ops.set_precision(prev)


def same(got, ref, what):
    got = got.cpu()
    ref = ref.to(got.dtype)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: {len(bad)} of {ref.numel()} elements differ, first at {first}: got {got[first].item()}, exact {ref[first].item()}')


# ---- SimOTA --------------------------------------------------------------------------------------------------------------------------------
def run_assign(ops, case):
    geom = case['geom']
    od, td = case['outputs'].to(DEV), case['labels'].to(DEV)
    return od, td, ops.simota_assign(od, td, geom.hws, geom.strides)


def check_assign(asg, ref, name):
    for k in ('fg_mask', 'ignore_mask', 'matched_valid_idx', 'matched_row', 'num_fg_img', 'pred_iou'):
        same(asg[k], ref[k], f'{name}: {k}')
    totals = asg['totals'].cpu().tolist()
    assert totals[:2] == ref['totals'], (name, totals)
    assert totals[2] == ref['status'], (name, 'status bits', totals[2])


@pytest.mark.parametrize('name', sorted(hx.assign_cases()))
def test_simota_exact(ops, name):
    case = hx.assign_cases()[name]
    _, _, asg = run_assign(ops, case)
    check_assign(asg, hx.assign_reference(case['outputs'], case['labels'], case['geom']), name)


# ---- losses --------------------------------------------------------------------------------------------------------------------------------
LOSS_MODES = ('plain', 'focal', 'weighted', 'weighted-focal')


def _report(name, d_raw, gref, case):
    err = (d_raw.cpu() - gref).abs()
    print(f'{name}: max |d_raw - autograd| box columns {float(err[..., :4].max()):.3e}, obj {float(err[..., 4].max()):.3e}, '
          f'cls {float(err[..., 5:].max()):.3e}; max |autograd| {float(gref.abs().max()):.3e}')
    for sub, (b, a) in sorted(case.get('where', {}).items()):
        print(f'  {sub}: d_raw[0:4] {d_raw[b, a, :4].cpu().tolist()} autograd {gref[b, a, :4].tolist()}')


@pytest.mark.parametrize('mode', LOSS_MODES)
def test_loss_edge_ties(ops, mode):
    """L1 - L6: a predicted edge on a label edge takes HALF the gradient term, as autograd of torch.max / torch.min gives it"""
    case = hx.assign_cases()['L-batch']
    focal, weighted = 'focal' in mode, 'weighted' in mode
    od, td, asg = run_assign(ops, case)
    check_assign(asg, hx.assign_reference(case['outputs'], case['labels'], case['geom']), 'L-batch')
    want, gref, _ = hx.loss_reference(case, focal, weighted)
    geom = case['geom']
    lw = td[..., 5].contiguous() if weighted else None
    losses, d_raw = ops.yolox_loss(od, td, asg, geom.hws, geom.strides, focal=focal, label_w=lw)
    print(mode, 'losses', losses.cpu().tolist(), 'oracle', want.tolist())
    _report(mode, d_raw, gref, case)
    tk.close(losses, want, rtol=2e-5, atol=1e-6)
    tk.close(d_raw, gref, rtol=1e-4, atol=1e-7)
    # L8: the same losses without the gradient
    losses2, none = ops.yolox_loss(od, td, asg, geom.hws, geom.strides, want_grad=False, focal=focal, label_w=lw)
    assert none is None
    tk.close(losses2, want, rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize('focal', [False, True])
def test_loss_empty_batch(ops, focal):
    """L7: no label in the whole batch -- totals 0, finite losses, the objectness gradient of the oracle"""
    case = hx.assign_cases()['S6-empty-batch']
    od, td, asg = run_assign(ops, case)
    od = od.clone()
    od[..., 4] = ((torch.arange(od.shape[1], device=DEV) % 5).float() - 2.0)[None]       # graded objectness: the loss has substance
    case = dict(case, outputs=od.cpu())
    assert asg['totals'].cpu().tolist() == [0, 0, 0]
    want, gref, _ = hx.loss_reference(case, focal)
    geom = case['geom']
    losses, d_raw = ops.yolox_loss(od, td, asg, geom.hws, geom.strides, focal=focal)
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(d_raw).all())
    tk.close(losses, want, rtol=2e-5, atol=1e-6)
    tk.close(d_raw, gref, rtol=1e-4, atol=1e-7)


# ---- NMS -----------------------------------------------------------------------------------------------------------------------------------
def run_nms(case, B=2):
    from leod_amd._lib import lib
    pred = torch.from_numpy(case['pred'])[None].repeat(B, 1, 1).contiguous()
    A, nc = pred.shape[1], case['nc']
    max_det = A if case['max_det'] is None else case['max_det']
    p = pred.to(DEV)
    det = torch.full((B * max_det * 7 + 64,), hx.SENTINEL, device=DEV)                   # 64 guard floats behind the rows
    cnt = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    nws = int(lib().leod_postprocess_nms_workspace_bytes(B, A))
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=DEV)
    rc = lib().leod_postprocess_nms(p.data_ptr(), det.data_ptr(), cnt.data_ptr(), ws.data_ptr() if nws else None, B, A, nc,
                                    float(case['conf']), float(case['thr']), 1 if case['agnostic'] else 0, max_det, int(case['limit']),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    det = det.cpu()
    assert bool((det[B * max_det * 7:] == hx.SENTINEL).all()), 'written behind the detection rows'
    return det[:B * max_det * 7].view(B, max_det, 7).numpy(), cnt.cpu().tolist(), p.cpu()


@pytest.mark.parametrize('case', hx.nms_cases(), ids=lambda c: c['name'])
def test_nms_exact(ops, case):
    ref = hx.nms_reference(case['pred'], case['nc'], case['conf'], case['thr'], case['agnostic'], case['max_det'], case['limit'])
    det, cnt, p = run_nms(case)
    assert cnt == [len(ref)] * len(cnt), (case['name'], cnt, len(ref))
    for b in range(len(cnt)):
        assert np.array_equal(det[b, :len(ref)], ref), f"{case['name']}: image {b}"
        assert bool((det[b, len(ref):] == hx.SENTINEL).all()), f"{case['name']}: rows past the count were written"
    if case['nc'] > 0:                      # boxes converted in place, exactly
        q = torch.from_numpy(case['pred'])
        assert torch.equal(p[0, :, 0], q[:, 0] - q[:, 2] / 2) and torch.equal(p[1, :, 3], q[:, 1] + q[:, 3] / 2)


# ---- pseudo-label filter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', hx.pseudo_cases(), ids=lambda c: c['name'])
def test_pseudo_filter_exact(ops, case):
    ref = hx.pseudo_reference(case['det'], case['cnt'], case['obj_thr'], case['cls_thr'], case['filter'], case['frame'])
    det = torch.from_numpy(case['det']).to(DEV)
    cnt = torch.tensor(case['cnt'], dtype=torch.int32, device=DEV)
    lab, lcnt = ops.pseudo_filter(det, cnt, case['obj_thr'], case['cls_thr'], case['filter'], case['frame'])
    lab, lcnt = lab.cpu().numpy(), lcnt.cpu().tolist()
    assert lcnt == [-1 if r is None else len(r) for r in ref], (case['name'], lcnt)
    for b, r in enumerate(ref):
        if r is not None:
            assert np.array_equal(lab[b, :len(r)], r), f"{case['name']}: image {b}"


# ---- prediction convs ----------------------------------------------------------------------------------------------------------------------
def _rel_close(got, ref, what):
    got, ref = got.cpu().double(), ref.double()
    err = (got - ref).abs()
    bad = err > hx.PRED_RTOL * ref.abs()
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} elements beyond {hx.PRED_RTOL:.2e} relative, worst {float((err / ref.abs()).max()):.3e}'


def run_pred_level(ops, p, stride, a0, out_train, out_infer):
    D = lambda t: t.to(DEV)  # noqa: E731
    ops.head_pred_fwd(D(p['cf']), D(p['rf']), D(p['cw']), D(p['cb']), D(p['rw']), D(p['rb']), D(p['ow']), D(p['ob']), out_train, out_infer,
                      stride, a0)


def check_pred_fwd(p, ot, oi, a0, name):
    hw = p['train'].shape[1]
    for out, ref, tag in ((ot, p['train'], 'train'), (oi, p['infer'], 'infer')):
        lvl = out[:, a0:a0 + hw]
        same(lvl[..., :2], ref[..., :2], f'{name}: {tag} xy')
        _rel_close(lvl[..., 2:4], ref[..., 2:4], f'{name}: {tag} wh')
        if tag == 'train':
            same(lvl[..., 4:], ref[..., 4:], f'{name}: logits')
        else:
            _rel_close(lvl[..., 4:], ref[..., 4:], f'{name}: probabilities')


def run_pred_bwd(ops, p, a0, A, grads, gscale):
    D = lambda t: t.to(DEV)  # noqa: E731
    B, hw, nch = p['d'].shape
    d_raw = torch.full((B, A, nch), float('nan'))
    d_raw[:, a0:a0 + hw] = p['d']
    return ops.head_pred_bwd(D(d_raw), D(p['cf']), D(p['rf']), D(p['cw']), D(p['rw']), D(p['ow']), *grads, a0, gscale=gscale)


GRAD_NAMES = ('dcw', 'dcb', 'drw', 'drb', 'dow', 'dob')


def _grad_start(p, fill=3.0):
    return [torch.full(tuple(p[n].shape), fill, device=DEV) for n in ('cw', 'cb', 'rw', 'rb', 'ow', 'ob')]


@pytest.mark.parametrize('row', hx.PRED_CASES, ids=lambda r: r[0])
def test_head_pred_exact(ops, row):
    name, B, h, w, Hd, nc, stride, route, bwd = row
    assert hx.pred_route(B, h, w, Hd, nc) == route, 'the shape no longer reaches the kernel this row is here for'
    p = hx.pred_problem(B, h, w, Hd, nc, stride)
    a0, A = 3, h * w + 8                      # rows outside [a0, a0 + h w) belong to nobody
    ot = torch.full((B, A, 5 + nc), hx.SENTINEL, device=DEV)
    oi = torch.full((B, A, 5 + nc), hx.SENTINEL, device=DEV)
    run_pred_level(ops, p, stride, a0, ot, oi)
    check_pred_fwd(p, ot, oi, a0, name)
    for out in (ot, oi):
        assert bool((out[:, :a0] == hx.SENTINEL).all()) and bool((out[:, a0 + h * w:] == hx.SENTINEL).all()), f'{name}: rows outside the level'
    # one output only
    ot2 = torch.full((B, A, 5 + nc), hx.SENTINEL, device=DEV)
    run_pred_level(ops, p, stride, a0, ot2, None)
    same(ot2, ot.cpu(), f'{name}: out_train alone')
    if not bwd:
        return
    for gs in (0.5, 2.0):
        grads = _grad_start(p)
        gscale = torch.tensor([gs], device=DEV)
        dcf, drf = run_pred_bwd(ops, p, a0, A, grads, gscale)
        same(dcf.view(-1, Hd), p['grads']['dcf'] * gs, f'{name}: d_cls_feat')
        same(drf.view(-1, Hd), p['grads']['drf'] * gs, f'{name}: d_reg_feat')
        for g, n in zip(grads, GRAD_NAMES):
            same(g, 3.0 + gs * p['grads'][n].view(g.shape), f'{name}: {n} gscale {gs}')
    # without a gscale pointer: factor 1
    grads = _grad_start(p, 0.0)
    run_pred_bwd(ops, p, a0, A, grads, None)
    for g, n in zip(grads, GRAD_NAMES):
        same(g, p['grads'][n].view(g.shape), f'{name}: {n}')


def test_head_pred_two_levels(ops):
    """H6: two levels written into one output at different a0; the weight gradients accumulate over both calls"""
    B, Hd, nc = 2, 36, 3
    ot = torch.full((B, hx.H6_A, 5 + nc), hx.SENTINEL, device=DEV)
    oi = torch.full((B, hx.H6_A, 5 + nc), hx.SENTINEL, device=DEV)
    probs = [hx.pred_problem(B, h, w, Hd, nc, s, seed=i) for i, (h, w, s, a0) in enumerate(hx.H6_LEVELS)]
    # each level has its own problem (features, weights, d_raw); only the output rows and the six gradient buffers are shared
    for p, (h, w, s, a0) in zip(probs, hx.H6_LEVELS):
        run_pred_level(ops, p, s, a0, ot, oi)
    covered = torch.zeros(hx.H6_A, dtype=torch.bool)
    for p, (h, w, s, a0) in zip(probs, hx.H6_LEVELS):
        check_pred_fwd(p, ot, oi, a0, f'H6 level stride {s}')
        covered[a0:a0 + h * w] = True
    assert bool((ot.cpu()[:, ~covered] == hx.SENTINEL).all()) and bool((oi.cpu()[:, ~covered] == hx.SENTINEL).all())
    grads = _grad_start(probs[0])
    want = [torch.full(tuple(g.shape), 3.0, dtype=torch.float64) for g in grads]
    gscale = torch.tensor([2.0], device=DEV)
    for p, (h, w, s, a0) in zip(probs, hx.H6_LEVELS):
        dcf, drf = run_pred_bwd(ops, p, a0, hx.H6_A, grads, gscale)
        same(dcf.view(-1, Hd), p['grads']['dcf'] * 2.0, 'H6: d_cls_feat')
        same(drf.view(-1, Hd), p['grads']['drf'] * 2.0, 'H6: d_reg_feat')
        for wnt, n in zip(want, GRAD_NAMES):
            wnt += 2.0 * p['grads'][n].view(wnt.shape)
    for g, wnt, n in zip(grads, want, GRAD_NAMES):
        same(g, wnt, f'H6: {n} over both levels')
