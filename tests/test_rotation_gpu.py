"""Rotation augmentation on the device: ``leod_augment_rot_u8`` (flip -> rotate -> zoom in one gather pass) against the
torch-only restatement of torchvision's ``rotate`` (tests/rotation_ref.py), against the reference's composition recorded in
tests/golden/g26_rotation.npz, and through ``Module.training_step``.  ``pytest -m gpu``.

The kernel evaluates the source index in fp32 in its own operation order; the restatement goes through ``bmm`` and
``grid_sample``'s un-normalisation.  Where a source coordinate lies within 1e-3 of a half-integer the two may legitimately pick
neighbouring pixels (``near_tie_mask``, computed in float64): those pixels are excluded, and the tests bound how many there are
(1.5 % of a frame; the sizes and angles used here have at most 1.04 %, at 12 x 16 and 33 degrees)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import augment as oa  # noqa: E402
from oracle.synth import synth_augment_sample, synth_labels, synth_state_dict, AUGMENT_CASES  # noqa: E402
from rotation_ref import rotate as ref_rotate, near_tie_mask  # noqa: E402

DEV = 'cuda'
ANGLES = [7.3, -12.9, 33.0, -20.0, 15.0, 90.0, 0.0]
TIE_CAP = 0.015


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return True


def _aug():
    from leod_amd.data.utils import augmentor
    return augmentor


def rot_state(angle, **kw):
    A = _aug()
    return A.AugmentationState(rotation=A.RotationState(True, angle), **kw)


def random_frames(T, B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 255, (T, B, C, H, W), generator=g).to(torch.uint8)        # 1..254: a zero in the output is a dead pixel


@pytest.mark.parametrize('H,W', [(12, 16), (48, 64), (60, 76)])
def test_rotation_only_vs_restatement(gpu, H, W):
    """Per-sample angles in one launch, each sample against the restatement: equal outside the near-tie band, which stays under
    the cap; 0 degrees reproduces the input and 90 degrees the restatement exactly (no near ties), with dead corners."""
    A = _aug()
    T, B, C = 2, 4, 4
    for n, angles in enumerate((ANGLES[:4], ANGLES[3:])):
        ev = random_frames(T, B, C, H, W, seed=100 * H + n)
        out = A.augment_events(ev.to(DEV), [rot_state(a) for a in angles]).cpu()
        for b, angle in enumerate(angles):
            want = ref_rotate(ev[:, b], angle)
            tie = near_tie_mask(H, W, angle)
            print(f'{H}x{W} angle {angle}: near-tie pixels {tie.mean():.4%}, dead pixels {(want == 0).float().mean():.4%}')
            assert tie.mean() <= TIE_CAP, (angle, tie.mean())
            keep = torch.from_numpy(~tie)
            assert torch.equal(out[:, b][..., keep], want[..., keep]), f'angle {angle}'
            if angle == 0.0:
                assert not tie.any() and torch.equal(out[:, b], ev[:, b])
            else:
                corners = out[:, b][..., [0, 0, -1, -1], [0, -1, 0, -1]]
                assert int(corners.max()) == 0, f'angle {angle}: the corners of a rotated frame are dead'
            if angle == 90.0:
                assert not tie.any() and torch.equal(out[:, b], want)
                assert 0.21 <= float((out[:, b] == 0).float().mean()) <= 0.25


def recorded_state(s):
    A = _aug()
    return A.AugmentationState(apply_h_flip=bool(s[0]), rotation=A.RotationState(bool(s[9]), float(s[10])),
                               zoom_in=A.ZoomInState(bool(s[1]), int(s[2]), int(s[3]), float(s[4])),
                               zoom_out=A.ZoomOutState(bool(s[5]), int(s[6]), int(s[7]), float(s[8])))


def tie_mask_after_zoom(H, W, st):
    """The near-tie pixels of the rotated frame, carried to the output through the state's zoom (the flip precedes the rotation
    and does not move them)."""
    tie = near_tie_mask(H, W, st.rotation.angle_deg).astype(np.uint8)
    if st.zoom_in.active and st.zoom_in.zoom_in_factor != 1:
        tie = oa.zoom_in(tie, (st.zoom_in.x0, st.zoom_in.y0), st.zoom_in.zoom_in_factor)
    elif st.zoom_out.active and st.zoom_out.zoom_out_factor != 1:
        tie = oa.zoom_out(tie, (st.zoom_out.x0, st.zoom_out.y0), st.zoom_out.zoom_out_factor)
    return tie.astype(bool)


def test_composition_vs_reference_golden(gpu, golden_dir):
    """flip -> rotate -> zoom-in | zoom-out as the reference composes them (g26 (b): its ``__call__`` with ``rotate.prob = 1``,
    the pixel rule of the rotation being the restatement), batched [T, B] with a different recorded state per sample."""
    A = _aug()
    g = np.load(os.path.join(golden_dir, 'g26_rotation.npz'))
    modes = set()
    for hw in ((60, 76), (48, 64)):
        cases = [c for c in AUGMENT_CASES if (c[1], c[2]) == hw]
        evs, states = [], []
        for seed, H, W in cases:
            ev, _ = synth_augment_sample(seed, H, W)
            evs.append(torch.stack(ev))
            states.append(recorded_state(g[f'b_s{seed}_state']))
        batch = torch.stack(evs, 1).contiguous().to(DEV)                   # [T, B, 20, H, W]
        out = A.augment_events(batch, states).cpu().numpy()
        for b, (seed, H, W) in enumerate(cases):
            st = states[b]
            modes.add((st.apply_h_flip, st.zoom_in.active, st.zoom_out.active))
            tie = tie_mask_after_zoom(H, W, st)
            print(f'seed {seed}: angle {st.rotation.angle_deg:.3f}, near-tie pixels after the zoom {tie.mean():.4%}')
            assert near_tie_mask(H, W, st.rotation.angle_deg).mean() <= TIE_CAP
            np.testing.assert_array_equal(out[:, b][..., ~tie], g[f'b_s{seed}_ev'][..., ~tie], err_msg=f'seed {seed}')
    assert len(modes) >= 3, modes                                          # the recorded states do mix flip / no flip, zoom-in / no zoom


def test_rotation_then_zoom_out_vs_restatement(gpu):
    """The recorded states of g26 draw no zoom-out (weight 2 of 10): flip -> rotate -> zoom-out composed from the restatement and
    the oracle's zoom-out (nearest-exact resize + paste on zeros), and the same for a zoom-in, at a frame size off the golden's."""
    A = _aug()
    T, C, H, W = 2, 3, 36, 52
    states = [rot_state(12.0, apply_h_flip=True, zoom_out=A.ZoomOutState(True, 4, 3, 1.15)),
              rot_state(-17.0, zoom_out=A.ZoomOutState(True, 0, 0, 1.2)),
              rot_state(5.0, zoom_in=A.ZoomInState(True, 9, 6, 1.4))]
    ev = random_frames(T, len(states), C, H, W, seed=21)
    out = A.augment_events(ev.to(DEV), states).cpu().numpy()
    for b, st in enumerate(states):
        x = torch.flip(ev[:, b], dims=[-1]) if st.apply_h_flip else ev[:, b]
        x = ref_rotate(x, st.rotation.angle_deg).numpy()
        if st.zoom_out.active:
            want = oa.zoom_out(x, (st.zoom_out.x0, st.zoom_out.y0), st.zoom_out.zoom_out_factor)
        else:
            want = oa.zoom_in(x, (st.zoom_in.x0, st.zoom_in.y0), st.zoom_in.zoom_in_factor)
        tie = tie_mask_after_zoom(H, W, st)
        assert near_tie_mask(H, W, st.rotation.angle_deg).mean() <= TIE_CAP
        np.testing.assert_array_equal(out[:, b][..., ~tie], want[..., ~tie], err_msg=f'sample {b}')
        if st.zoom_out.active:
            assert (want[..., ~tie] == 0).mean() > 0.2                     # the canvas around the pasted window, and the corners in it


def test_rotation_with_time_flip_and_hflip(gpu):
    """tflip rides in the same pass for rotated samples too: out[t, b, c] = aug(in[T-1-t, b, C-1-c]), exactly."""
    A = _aug()
    T, B, H, W = 5, 3, 48, 64
    ev = random_frames(T, B, 20, H, W, seed=5).to(DEV)
    spatial = [rot_state(11.0), rot_state(-7.5, apply_h_flip=True),
               rot_state(16.0, apply_h_flip=True, zoom_in=A.ZoomInState(True, 5, 3, 1.25))]
    flipped = [rot_state(11.0, apply_t_flip=True), spatial[1],
               rot_state(16.0, apply_h_flip=True, apply_t_flip=True, zoom_in=A.ZoomInState(True, 5, 3, 1.25))]
    out, plain = A.augment_events(ev, flipped), A.augment_events(ev, spatial)
    for b in (0, 2):
        assert torch.equal(out[:, b], torch.flip(plain[:, b], dims=[0, 1]))
    assert torch.equal(out[:, 1], plain[:, 1])
    # hflip acts BEFORE the rotation: hflip + rotation of the input == the same rotation alone of the flipped input
    only_rot = A.augment_events(torch.flip(ev, dims=[-1]).contiguous(), [rot_state(11.0), rot_state(-7.5), rot_state(16.0)])
    assert torch.equal(plain[:, 1], only_rot[:, 1])


class CountingLib:
    """Stands in for ``lib()`` of the augmentor module: forwards every symbol, counts which ones were fetched."""

    def __init__(self, dll):
        self._dll, self.calls = dll, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._dll, name)


def test_mixed_batch_and_inactive_batches_keep_the_plain_kernel(gpu, monkeypatch):
    """One rotated sample next to zoom-in, zoom-out and hflip samples: the unrotated columns are bit-identical to what
    ``leod_augment_u8`` gives them; a batch without an active non-zero rotation never reaches the new entry point."""
    A = _aug()
    from leod_amd._lib import lib
    T, B, C, H, W = 3, 4, 6, 48, 64
    ev = random_frames(T, B, C, H, W, seed=9).to(DEV)
    others = [A.AugmentationState(zoom_in=A.ZoomInState(True, 7, 5, 1.3)),
              A.AugmentationState(apply_h_flip=True, zoom_out=A.ZoomOutState(True, 4, 3, 1.15)),
              A.AugmentationState(apply_h_flip=True)]
    counter = CountingLib(lib())
    monkeypatch.setattr(A, 'lib', lambda: counter)
    plain = A.augment_events(ev, [A.AugmentationState()] + others)
    assert counter.calls == ['leod_augment_u8']
    mixed = A.augment_events(ev, [rot_state(-9.0)] + others)
    assert counter.calls == ['leod_augment_u8', 'leod_augment_rot_u8']
    assert torch.equal(mixed[:, 1:], plain[:, 1:])
    want = ref_rotate(ev[:, 0].cpu(), -9.0)
    keep = torch.from_numpy(~near_tie_mask(H, W, -9.0))
    assert torch.equal(mixed[:, 0].cpu()[..., keep], want[..., keep])
    # inactive rotation (whatever its angle field says) and an active one of 0 degrees: the plain entry point
    del counter.calls[:]
    idle = [A.AugmentationState(rotation=A.RotationState(False, 12.0)), A.AugmentationState(rotation=A.RotationState(True, 0.0))] + others[:2]
    assert torch.equal(A.augment_events(ev, idle)[:, :2], ev[:, :2])
    assert counter.calls == ['leod_augment_u8']


def test_rot_entry_point_refuses_bad_arguments(gpu):
    """Plain argument checks of the C entry point; nothing is launched."""
    from leod_amd._lib import lib
    T, B, C, H, W = 1, 2, 2, 8, 16
    src = torch.zeros((T, B, C, H, W), dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    params = torch.tensor([[0, 0, 0, 0, H, W, 0]] * B, dtype=torch.int32, device=DEV)
    rot = torch.tensor([[1.0, 0.0]] * B, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    f = lib().leod_augment_rot_u8
    ERR_ARG = -1
    assert f(src.data_ptr(), dst.data_ptr(), params.data_ptr(), None, T, B, C, H, W, stream) == ERR_ARG
    assert f(src.data_ptr(), dst.data_ptr(), params.data_ptr(), rot.data_ptr(), T, B, C, H, 18, stream) == ERR_ARG
    assert f(src.data_ptr(), src.data_ptr(), params.data_ptr(), rot.data_ptr(), T, B, C, H, W, stream) == ERR_ARG
    assert f(src.data_ptr(), dst.data_ptr(), params.data_ptr(), rot.data_ptr(), 40000, B, C, H, W, stream) == -3     # > 65535 planes
    assert f(src.data_ptr(), dst.data_ptr(), params.data_ptr(), rot.data_ptr(), T, B, C, H, W, stream) == 0
    torch.cuda.synchronize()
    assert int(dst.max()) == 0


def test_training_step_warps_a_batch_whose_only_augmentation_is_a_rotation(gpu, manifest, monkeypatch):
    """``Module.get_data_from_batch``: a batch whose states carry nothing but a rotation must still go through the frame warp (the
    loaders rotated its labels already) -- the frames the backbone receives are ``augment_events`` of the input."""
    A = _aug()
    from leod_amd.config import full_config, dynamically_modify_train_config
    from leod_amd.data.genx_utils.labels import ObjectLabels, SparselyBatchedObjectLabels
    from leod_amd.data.utils.types import DataType
    from leod_amd.modules.detection import Module
    from leod_amd.modules.utils.detection import WORKER_ID_KEY, DATA_KEY
    HW = (64, 96)                                                          # the micro config's own resolution: W % 4 == 0
    over = dict(model=dict(backbone=dict(embed_dim=16, stage=dict(attention=dict(dim_head=8)))), dataset=dict(sequence_length=4))
    cfg = dynamically_modify_train_config(full_config('gen1', 'small', overrides=over))
    cfg.model.backbone.in_res_hw = HW
    cfg.model.backbone.stage.attention.partition_size = (2, 3)
    mod = Module(cfg)
    mod.mdl.load_state_dict(synth_state_dict(manifest['micro'], 5))
    mod.to(DEV)
    mod.setup('fit')
    mod.train()
    L, B = 4, 2
    ev = random_frames(L, B, 20, HW[0], HW[1], seed=77)
    ev = torch.where(torch.rand(ev.shape, generator=torch.Generator().manual_seed(78)) < 0.15, ev % 12 + 1, torch.zeros_like(ev))
    states = [rot_state(10.0), rot_state(-6.0)]
    flat = synth_labels(4, HW, 2, seed=42, max_boxes=3)
    for l in flat:                                                         # boxes around the centre: they survive the rotation
        l[:, 3], l[:, 4] = l[:, 3].clamp(min=12, max=30), l[:, 4].clamp(min=12, max=24)
        l[:, 1], l[:, 2] = l[:, 1].clamp(20, 40), l[:, 2].clamp(12, 24)
    grid = [[None, None], [flat[0], flat[1]], [None, None], [flat[2], flat[3]]]
    seq = []
    for t in range(L):
        row = [None if grid[t][b] is None else ObjectLabels(grid[t][b].clone(), HW) for b in range(B)]
        for b in range(B):
            A.augment_labels([row[b]], states[b])
        assert all(l is None or len(l) > 0 for l in row)
        seq.append(SparselyBatchedObjectLabels(row))
    data = {DataType.EV_REPR: [ev[t].to(DEV) for t in range(L)], DataType.OBJLABELS_SEQ: seq, DataType.AUGM_STATE: states,
            DataType.IS_FIRST_SAMPLE: torch.ones(B, dtype=torch.bool, device=DEV), DataType.IS_PADDED_MASK: [[False] * B for _ in range(L)]}
    seen = []
    inner = mod.mdl.backbone.forward_sequence

    def spy(x_seq, *a, **k):
        seen.append(x_seq.detach().clone())
        return inner(x_seq, *a, **k)
    monkeypatch.setattr(mod.mdl.backbone, 'forward_sequence', spy)
    out = mod.training_step({DATA_KEY: data, WORKER_ID_KEY: 0}, 0, log=False)
    assert len(seen) == 1
    want = A.augment_events(ev.to(DEV).contiguous(), states)
    assert torch.equal(seen[0], want) and not torch.equal(want, ev.to(DEV))
    assert math.isfinite(float(out['loss'].detach()))
