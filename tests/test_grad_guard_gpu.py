"""The non-finite guard of the optimiser step and the per-parameter gradient statistics on the GPU: ``leod_grad_stats`` against a float64
numpy reference (exact: the inputs are chosen so that every sum is representable), ``leod_adamw_clip_step_guarded`` against
``torch.optim.AdamW`` stepping only on the finite steps, and both through ``FlatAdamW(skip_nonfinite=True)``, ``grad_flow`` and ``fit``.
A NaN in a gradient buffer is data: nothing here faults.  ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.synth import synth_state_dict, synth_events  # noqa: E402
from test_module_gpu import micro_module, micro_labels, loader_batch, HW  # noqa: E402

DEV = 'cuda'
POISON = 777.0


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return True


def seg_lengths(C):
    return [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3, 70001]


def layout(lengths, seed):
    """Segments at 4-float alignment, values k/256 with integer k in [-1024, 1024], the padding between them filled with a finite poison:
    |g| and g^2 are multiples of 2^-16 below 2^5 and every sum stays below 2^22 -- at most 38 significant bits, exact in double in any order."""
    offs, n = [], 0
    for k in lengths:
        offs.append(n)
        n += (k + 3) // 4 * 4
    rng = np.random.default_rng(seed)
    buf = np.full(n, POISON, dtype=np.float32)
    for o, k in zip(offs, lengths):
        buf[o:o + k] = rng.integers(-1024, 1025, size=k).astype(np.float32) / 256
    return offs, buf


def reference(buf, offs, lengths):
    stats, cnt = np.zeros((len(offs), 3)), np.zeros(len(offs), dtype=np.int32)
    for s, (o, k) in enumerate(zip(offs, lengths)):
        x = buf[o:o + k].astype(np.float64)
        fin = np.isfinite(x)
        a = np.abs(x[fin])
        stats[s] = (a.sum(), (a * a).sum(), a.max() if a.size else 0.0)
        cnt[s] = int((~fin).sum())
    return stats, cnt


def run_stats(ops, buf, offs, lengths):
    plan = ops.GradStatsPlan(offs, lengths, DEV)
    plan.total.fill_(-5)                                       # the call must write it, not add to it
    stats, cnt, total = ops.grad_stats(torch.from_numpy(buf).to(DEV), plan)
    return stats.cpu().numpy(), cnt.cpu().numpy(), int(total.cpu()[0])


def test_exact_sums(ops):
    lengths = seg_lengths(ops.GRAD_STATS_CHUNK)
    offs, buf = layout(lengths, 11)
    ref, _ = reference(buf, offs, lengths)
    stats, cnt, total = run_stats(ops, buf, offs, lengths)
    assert np.array_equal(stats, ref), np.abs(stats - ref).max(axis=0)   # equality: the poison in the padding was not read into a segment
    assert not cnt.any() and total == 0
    again, cnt2, _ = run_stats(ops, buf, offs, lengths)
    assert again.tobytes() == stats.tobytes() and cnt2.tobytes() == cnt.tobytes()


def test_nonfinite_placement(ops):
    C = ops.GRAD_STATS_CHUNK
    lengths = seg_lengths(C)
    offs, buf = layout(lengths, 12)
    seg = {k: s for s, k in enumerate(lengths)}
    nan, inf = np.float32('nan'), np.float32('inf')
    plant = [(seg[257], 0, nan), (seg[257], 256, -inf),                    # first and last element of a segment
             (seg[2 * C + 3], C - 1, inf), (seg[2 * C + 3], C, nan),         # either side of a chunk boundary
             (seg[2 * C + 3], 2 * C, -inf), (seg[2 * C + 3], 2 * C + 2, nan),  # ... of the second one, and the last of the masked tail
             (seg[70001], 70000, inf), (seg[C], C - 1, nan),
             (seg[1], 0, nan)]                                              # the length-1 segment
    for s, i, v in plant:
        buf[offs[s] + i] = v
    assert buf[offs[seg[1]] + 1] == POISON
    buf[offs[seg[1]] + 1] = nan                                             # a padding slot: belongs to no segment
    ref, ref_cnt = reference(buf, offs, lengths)
    assert ref_cnt.sum() == len(plant)
    stats, cnt, total = run_stats(ops, buf, offs, lengths)
    assert np.array_equal(cnt, ref_cnt) and total == len(plant)
    assert np.array_equal(stats, ref)                                       # the finite rest of every segment, still exact
    assert stats[seg[1]].tolist() == [0.0, 0.0, 0.0]


def test_many_small_segments(ops):
    rng = np.random.default_rng(13)
    lengths = [int(k) for k in rng.integers(4, 13, size=3000)]
    offs, buf = layout(lengths, 14)
    ref, _ = reference(buf, offs, lengths)
    stats, cnt, total = run_stats(ops, buf, offs, lengths)
    assert np.array_equal(stats, ref) and not cnt.any() and total == 0


def test_refusals(ops):
    from leod_amd._lib import LeodHipError
    g = torch.zeros(16, device=DEV)
    plan = ops.GradStatsPlan([], [], DEV)
    plan.total.fill_(9)
    _, _, total = ops.grad_stats(g, plan)                      # no segments: accepted, total 0
    assert int(total.cpu()[0]) == 0
    with pytest.raises(LeodHipError):
        ops.grad_stats(g, ops.GradStatsPlan([2], [4], DEV))    # a segment that does not start on 16 bytes
    with pytest.raises(LeodHipError):
        ops.grad_stats(g, ops.GradStatsPlan([0, 12], [4, 8], DEV))   # ... that ends behind the buffer
    with pytest.raises(LeodHipError):
        ops.grad_stats(g, ops.GradStatsPlan([0, 0], [4, 4], DEV))    # ... that overlaps its predecessor
    with pytest.raises(LeodHipError):
        ops.grad_stats(g[1:], ops.GradStatsPlan([0], [4], DEV))      # a buffer that is not 16-byte aligned


# ---- the guarded step ---------------------------------------------------------------------------------------------------------
def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def bits(t):
    return t.detach().view(torch.int32)


def test_guarded_step_vs_torch_adamw(ops):
    """The inputs of test_kernels_gpu.py::test_adamw_clip, five steps, a NaN gradient element at step 2 and an inf at step 4: torch steps on
    1, 3, 5 only.  The parameters after step 3 match only if the bias corrections use the APPLIED count (2), not the call count (3)."""
    n = 10007
    p0, g0 = rnd((n,), 1), rnd((n,), 2, 2.0)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=2e-4, weight_decay=0.01)
    pd, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    state, scratch = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(8, device=DEV)
    plan = ops.GradStatsPlan([0], [n], DEV)
    for step in range(1, 6):
        gi = g0 * (1 + 0.1 * step)
        if step == 2:
            gi[1234] = float('nan')
        if step == 4:
            gi[n - 1] = float('inf')
        gd = gi.to(DEV)
        before = [t.clone() for t in (pd, m, v, gd)]
        _, _, total = ops.grad_stats(gd, plan)
        ops.adamw_clip_step_guarded(pd, gd, m, v, 2e-4, total, state, scratch, weight_decay=0.01, clip_value=1.0)
        if step in (2, 4):
            for t, b in zip((pd, m, v, gd), before):
                assert torch.equal(bits(t), bits(b))           # bit patterns: the gradient holds a NaN
        else:
            p.grad = gi.clone()
            torch.nn.utils.clip_grad_value_([p], 1.0)
            opt.step()
            np.testing.assert_allclose(pd.cpu().numpy(), p.detach().numpy(), rtol=1e-6, atol=1e-7, err_msg=f'step {step}')
    assert state.cpu().tolist() == [3, 2]


def test_guard_on_all_finite_equals_plain_entry(ops):
    n = 10007
    p0, g0 = rnd((n,), 1), rnd((n,), 2, 2.0)
    pa, ma, va = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pb, mb, vb = pa.clone(), ma.clone(), va.clone()
    state, scratch = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(8, device=DEV)
    plan = ops.GradStatsPlan([0], [n], DEV)
    for step in range(1, 4):
        ga = (g0 * (1 + 0.1 * step)).to(DEV)
        gb = ga.clone()
        ops.adamw_clip_step(pa, ga, ma, va, 2e-4, step, weight_decay=0.01, clip_value=1.0, grad_scale=0.5)
        _, _, total = ops.grad_stats(gb, plan)
        ops.adamw_clip_step_guarded(pb, gb, mb, vb, 2e-4, total, state, scratch, weight_decay=0.01, clip_value=1.0, grad_scale=0.5)
        # not bitwise: the bias corrections come from the device's pow.  The moments and the written-back gradient do not depend on them.
        np.testing.assert_allclose(pb.cpu().numpy(), pa.cpu().numpy(), rtol=1e-6, atol=1e-7, err_msg=f'step {step}')
        assert torch.equal(mb, ma) and torch.equal(vb, va) and torch.equal(gb, ga)
    assert state.cpu().tolist() == [3, 0]


# ---- optimiser and drivers (the micro module of test_module_gpu.py) ---------------------------------------------------------------
def micro_batch(seed, B=2):
    L = 4
    ev = synth_events(L, B, 20, HW[0], HW[1], seed=seed, as_uint8=True)
    flat = micro_labels(2 * B, seed + 1, [1e6] * B + [2e6] * B)
    labels_tb = [[None] * B, flat[:B], [None] * B, flat[B:]]
    return loader_batch(ev, labels_tb, torch.ones(B, dtype=torch.bool))


def backward_only(mod, opt, batch):
    opt.zero_grad()
    out = mod.training_step(batch, 0, log=False)
    mod.backward(out['loss'])


def test_skip_through_flat_adamw(gpu, manifest):
    from leod_amd.optim import FlatAdamW, fit_step
    mod, _, _ = micro_module(manifest, 5, 'fit')
    mod.train()
    mod.plan_mode = False
    opt = FlatAdamW(mod.mdl, lr=2e-4, weight_decay=0.01, clip_value=1.0, skip_nonfinite=True)
    mod._flat = opt.flat
    fit_step(mod, opt, None, micro_batch(41))
    assert (opt.applied_steps, opt.skipped_steps) == (1, 0)
    after1 = [t.clone() for t in (opt.flat.data, opt.flat.exp_avg, opt.flat.exp_avg_sq)]
    backward_only(mod, opt, micro_batch(43))
    k = next(i for i, p in enumerate(opt.flat.params) if p.numel() >= 8)
    opt.flat.grad[opt.flat.offsets[k] + 5] = float('nan')
    opt.step()
    for t, b in zip((opt.flat.data, opt.flat.exp_avg, opt.flat.exp_avg_sq), after1):
        assert torch.equal(t, b)
    assert (opt.applied_steps, opt.skipped_steps) == (1, 1)
    fit_step(mod, opt, None, micro_batch(45))
    assert all(bool(torch.isfinite(p).all()) for p in mod.mdl.parameters())
    assert not torch.equal(opt.flat.data, after1[0])
    assert (opt.applied_steps, opt.skipped_steps) == (2, 1)
    sd = opt.state_dict()
    assert sd['state']['step'] == 2 and sd['state']['skipped'] == 1
    mod2, _, _ = micro_module(manifest, 5, 'fit')
    opt2 = FlatAdamW(mod2.mdl, skip_nonfinite=True)
    opt2.load_state_dict(sd)
    assert (opt2.applied_steps, opt2.skipped_steps) == (2, 1)
    assert opt2.flat.guard_state().cpu().tolist() == [2, 1]
    assert torch.equal(opt2.flat.exp_avg, opt.flat.exp_avg)
    plain = FlatAdamW(micro_module(manifest, 5, 'fit')[0].mdl)             # the same checkpoint with the guard off: 'step' is the applied count
    plain.load_state_dict(sd)
    assert plain.flat.step_count == 2 and plain.state_dict()['state']['step'] == 2


def test_grad_flow(gpu, manifest):
    from leod_amd.optim import FlatAdamW, fit_step
    mod, _, _ = micro_module(manifest, 5, 'fit')
    mod.train()
    mod.plan_mode = False
    opt = FlatAdamW(mod.mdl, lr=2e-4, clip_value=1.0)
    mod._flat = opt.flat
    fit_step(mod, opt, None, micro_batch(41))
    flow = opt.grad_flow()
    named = [(n, p) for n, p in mod.mdl.named_parameters() if p.requires_grad]
    assert list(flow) == [n for n, _ in named] and len(named) > 50
    ref = [float(p.grad.double().abs().mean()) for _, p in named]
    np.testing.assert_allclose(list(flow.values()), ref, rtol=1e-12, atol=0)
    assert max(ref) > 0
    triples = opt.flat.named_grad_stats(mod.mdl)
    assert [n for n, _, _ in triples] == [n for n, _ in named] and all(int(c) == 0 for _, _, c in triples)
    assert float(triples[0][1][2]) == float(named[0][1].grad.abs().max())


def _guard_world2_worker(rank, port, manifest, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE='2', LOCAL_RANK='0')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=2)
    mod, _, cfg = micro_module(manifest, 9, 'fit')
    cfg.training.skip_nonfinite_steps = True
    mod.train()
    mod.plan_mode = False
    oc = mod.configure_optimizers()                # world size 2 -> gradient exchange + SyncBatchNorm; the guard from the config key
    opt = oc['optimizer']
    assert opt.world_size == 2 and opt.skip_nonfinite
    before = opt.flat.data.clone()
    T, B = 4, 4
    ev = synth_events(T, B, 20, HW[0], HW[1], seed=70, as_uint8=True)
    labs_all = micro_labels(T * B, 71, [1e6] * (T * B))
    mine = [2 * rank, 2 * rank + 1]
    labels_tb = [[labs_all[t * B + b] if t in (1, 3) else None for b in mine] for t in range(T)]
    opt.zero_grad()
    out = mod.training_step(loader_batch(ev[:, mine], labels_tb, torch.ones(2, dtype=torch.bool)), 0, log=False)
    mod.backward(out['loss'])
    # Only this rank's gradient is bad: the exchange carries it to both.  The buckets of the later stages were all-reduced during the
    # backward pass; the first stage's bucket (the front of the flat buffer) is released by ``step``, so that is where a plant made
    # here still is a LOCAL gradient.
    torch.cuda.synchronize()
    assert opt.dp.buckets is not None and opt.dp.buckets.ranges[0][0] == 0 and 0 not in opt.dp.buckets.done
    if rank == 1:
        opt.flat.grad[1] = float('nan')
    opt.step()
    q.put((rank, opt.skipped_steps, opt.applied_steps, bool(torch.equal(opt.flat.data, before)), opt.flat.data.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_ranks_take_the_same_decision(gpu, manifest):
    import os
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 35000 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_guard_world2_worker, args=(r, port, manifest, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in res:
        assert r[1] == 1 and r[2] == 0 and r[3], r[:4]
    np.testing.assert_array_equal(res[0][4], res[1][4])


def test_fit_grad_flow_and_skipped_steps(gpu, manifest, tmp_path):
    from oracle.synth import synth_dataset_tree
    from leod_amd.config import full_config, dynamically_modify_train_config
    from leod_amd.modules.utils.fetch import fetch_model_module, fetch_data_module
    from leod_amd.train import fit
    tree = synth_dataset_tree(str(tmp_path / 'src'), 'gen1', False, frame_hw=HW)
    over = dict(model=dict(backbone=dict(embed_dim=16, stage=dict(attention=dict(dim_head=8)))),
                training=dict(skip_nonfinite_steps=True),
                dataset=dict(path=tree, sequence_length=4, data_augmentation=dict(
                    random=dict(prob_hflip=0, zoom=dict(prob=0)), stream=dict(start_from_zero=True, prob_hflip=0, zoom=dict(prob=0)))))
    cfg = dynamically_modify_train_config(full_config('gen1', 'small', overrides=over))
    cfg.dataset.ev_repr_hw = HW
    cfg.model.backbone.in_res_hw = (64, 96)
    cfg.model.backbone.stage.attention.partition_size = (2, 3)
    cfg.model.postprocess.confidence_threshold = 0.001
    cfg.training.max_steps = 4
    cfg.training.lr_scheduler.total_steps = 4
    mod = fetch_model_module(cfg)
    mod.mdl.load_state_dict(synth_state_dict(manifest['micro'], 8))
    mod.to(DEV)
    cfg.batch_size.train = cfg.batch_size.eval = 2
    cfg.hardware.num_workers.train, cfg.hardware.num_workers.eval = 2, 1
    dm = fetch_data_module(cfg, prefetch=2)
    hist = fit(cfg, mod, dm, max_steps=4, log_every_n_steps=2, val_check_interval=0, limit_val_batches=1, grad_flow_every=2)
    assert hist['global_step'] == 4
    assert [s for s, _ in hist['grad_flow']] == [2, 4]
    names = [n for n, p in mod.mdl.named_parameters() if p.requires_grad]
    for _, flow in hist['grad_flow']:
        assert list(flow) == names and all(np.isfinite(v) for v in flow.values()) and max(flow.values()) > 0
    assert hist['skipped_steps'] == 0
