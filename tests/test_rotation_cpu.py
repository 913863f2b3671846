"""Host side of the rotation augmentation against the reference (tests/golden/g26_rotation.npz, recorded by
tests/golden/make_golden_rotation.py): ``ObjectLabels.rotate_``, the augmentor's random draws and label transforms with
``rotate.prob = 1``, and the {cos, sin} hand-over to the gather kernel.  No GPU."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from oracle.synth import synth_augment_sample, AUGMENT_CASES, AUGMENT_CFG

LABEL_CASES = [(0, 60, 76), (1, 60, 76), (2, 60, 76), (3, 60, 76), (100, 48, 64)]


@pytest.fixture(scope='module')
def g26(golden_dir):
    return np.load(os.path.join(golden_dir, 'g26_rotation.npz'))


def rotation_cfg():
    from leod_amd.config.dictconfig import DictConfig
    cfg = copy.deepcopy(AUGMENT_CFG)
    cfg['rotate'] = dict(prob=1, min_angle_deg=2, max_angle_deg=20)
    return DictConfig(cfg)


def test_object_labels_rotate_matches_reference(g26):
    """Same fp32 arithmetic on both sides (fp32 matrix, integer centre (W // 2, H // 2), hull, clamp): 1e-4 px covers only the
    summation order inside ``einsum``; which rows survive ``remove_flat_labels_``, and their order, must be exact."""
    from leod_amd.data.genx_utils.labels import ObjectLabels
    angles = [float(a) for a in g26['label_angles']]
    assert angles == [4.0, -4.0, 15.0, -33.0, 90.0]
    n = 0
    for seed, H, W in LABEL_CASES:
        _, labels = synth_augment_sample(seed, H, W)
        for t, l in enumerate(labels):
            if l is None:
                continue
            for a, angle in enumerate(angles):
                obj = ObjectLabels(l.clone(), (H, W))
                obj.rotate_(angle)
                want = g26[f'a_s{seed}_t{t}_a{a}']
                assert tuple(obj.object_labels.shape) == want.shape, (seed, t, angle)
                np.testing.assert_allclose(obj.object_labels.numpy(), want, rtol=0, atol=1e-4, err_msg=f'{seed} {t} {angle}')
                assert obj.input_size_hw == (H, W)
                n += 1
    assert n == 11 * 5


def test_object_labels_rotate_drops_boxes_that_leave_the_frame(g26):
    from leod_amd.data.genx_utils.labels import ObjectLabels, SparselyBatchedObjectLabels
    hw = tuple(int(v) for v in g26['corner_hw'])
    lens = []
    for a, angle in enumerate(float(v) for v in g26['corner_angles']):
        obj = ObjectLabels(torch.from_numpy(g26['corner_rows'].copy()), hw)
        obj.rotate_(angle)
        want = g26[f'a_corner_a{a}']
        assert tuple(obj.object_labels.shape) == want.shape, angle
        np.testing.assert_allclose(obj.object_labels.numpy(), want, rtol=0, atol=1e-4, err_msg=str(angle))
        lens.append(len(obj))
    assert min(lens) == 1 and max(lens) == 2                   # the fixture does contain both outcomes
    # the batched wrapper keeps a frame that lost every box as an EMPTY label (labels.py:685-688), unlike the zooms
    only_corner = ObjectLabels(torch.from_numpy(g26['corner_rows'][:1].copy()), hw)
    batch = SparselyBatchedObjectLabels([only_corner, None])
    batch.rotate_(angle_deg=33.0)
    assert batch[0] is only_corner and len(batch[0]) == 0 and batch[1] is None
    empty = ObjectLabels(torch.zeros((0, 8)), hw)
    empty.rotate_(12.0)
    assert len(empty) == 0


def test_augmentor_with_rotation_draws_the_reference_state_and_labels(g26):
    """With the reference's seeds the mirror draws the same state -- ``angle_deg`` exact -- and, flip -> rotate -> zoom-in window
    sampled from the ROTATED labels -> zoom, the same labels, including which frames are left empty or become None."""
    from leod_amd.data.genx_utils.labels import ObjectLabels, SparselyBatchedObjectLabels
    from leod_amd.data.utils.augmentor import RandomSpatialAugmentorGenX
    from leod_amd.data.utils.types import DataType
    cfg = rotation_cfg()
    for seed, H, W in AUGMENT_CASES:
        _, labels = synth_augment_sample(seed, H, W)
        aug = RandomSpatialAugmentorGenX((H, W), True, cfg)
        objs = SparselyBatchedObjectLabels([None if l is None else ObjectLabels(l.clone(), (H, W)) for l in labels])
        torch.manual_seed(900 + seed)
        res = aug({DataType.OBJLABELS_SEQ: objs})
        st = res[DataType.AUGM_STATE]
        got = np.array([float(st.apply_h_flip), float(st.zoom_in.active), st.zoom_in.x0, st.zoom_in.y0, st.zoom_in.zoom_in_factor,
                        float(st.zoom_out.active), st.zoom_out.x0, st.zoom_out.y0, st.zoom_out.zoom_out_factor,
                        float(st.rotation.active), st.rotation.angle_deg])
        np.testing.assert_array_equal(got, g26[f'b_s{seed}_state'], err_msg=str(seed))
        assert st.rotation.active and 2 <= abs(st.rotation.angle_deg) <= 20
        for t, l in enumerate(res[DataType.OBJLABELS_SEQ]):
            if l is None:
                assert f'b_s{seed}_lab{t}' not in g26.files, (seed, t)
                continue
            want = g26[f'b_s{seed}_lab{t}']
            assert tuple(l.object_labels.shape) == want.shape, (seed, t)
            np.testing.assert_allclose(l.object_labels.numpy(), want, rtol=0, atol=1e-4, err_msg=f'{seed} {t}')
            assert tuple(float(v) for v in l.input_size_hw) == tuple(g26[f'b_s{seed}_hw{t}'])


def test_augment_labels_applies_the_recorded_rotation(g26):
    """``augment_labels`` (labels of one sample from a given state) follows the same order as ``augment_sample_labels``."""
    from leod_amd.data.genx_utils.labels import ObjectLabels
    from leod_amd.data.utils.augmentor import (AugmentationState, RotationState, ZoomInState, ZoomOutState, augment_labels)
    for seed, H, W in AUGMENT_CASES:
        s = g26[f'b_s{seed}_state']
        st = AugmentationState(apply_h_flip=bool(s[0]), rotation=RotationState(bool(s[9]), float(s[10])),
                               zoom_in=ZoomInState(bool(s[1]), int(s[2]), int(s[3]), float(s[4])),
                               zoom_out=ZoomOutState(bool(s[5]), int(s[6]), int(s[7]), float(s[8])))
        _, labels = synth_augment_sample(seed, H, W)
        objs = augment_labels([None if l is None else ObjectLabels(l.clone(), (H, W)) for l in labels], st)
        for t, l in enumerate(objs):
            key = f'b_s{seed}_lab{t}'
            if l is None or (len(l) == 0 and key not in g26.files):   # the reference's batched zoom-in turns emptied frames into None
                assert key not in g26.files
                continue
            np.testing.assert_allclose(l.object_labels.numpy(), g26[key], rtol=0, atol=1e-4, err_msg=f'{seed} {t}')


def test_state_to_rot_and_params():
    from leod_amd.data.utils.augmentor import AugmentationState, RotationState, state_to_params, state_to_rot
    assert state_to_rot(AugmentationState()) == [1.0, 0.0]
    assert state_to_rot(AugmentationState(rotation=RotationState(False, 12.0))) == [1.0, 0.0]       # inactive: the angle is ignored
    assert state_to_rot(AugmentationState(rotation=RotationState(True, 0.0))) == [1.0, 0.0]
    c, s = state_to_rot(AugmentationState(rotation=RotationState(True, 30.0)))
    assert c == math.cos(math.radians(30.0)) and s == math.sin(math.radians(30.0)) and s > 0        # counter-clockwise positive
    c, s = state_to_rot(AugmentationState(rotation=RotationState(True, -90.0)))
    assert s == -1.0 and abs(c) < 1e-15
    st = AugmentationState(apply_h_flip=True, rotation=RotationState(True, 7.0))
    assert state_to_params(st, (60, 76)) == [1, 0, 0, 0, 60, 76, 0]                                 # no longer refuses a rotation


def test_restatement_agrees_with_the_kernels_index_rule():
    """tests/rotation_ref.py (torchvision's affine_grid + grid_sample chain) against an fp32 emulation of the index rule that
    ``leod_augment_rot_u8`` documents (include/leod_hip.h), at the sizes and angles of the GPU test: they may differ only inside
    the near-tie band, and 0 / 90 degrees have no near ties at all."""
    from rotation_ref import rotate, near_tie_mask
    f = np.float32
    for H, W in ((12, 16), (48, 64), (60, 76)):
        img = torch.arange(1, H * W + 1, dtype=torch.float32).reshape(1, H, W)
        for angle in (7.3, -12.9, 33.0, -20.0, 15.0, 90.0, 0.0):
            a = math.radians(angle)
            c, s = f(math.cos(a)), f(math.sin(a))
            cx, cy = f(0.5) * f(W) - f(0.5), f(0.5) * f(H) - f(0.5)
            y, x = np.meshgrid(np.arange(H, dtype=f), np.arange(W, dtype=f), indexing='ij')
            dx, dy = x - cx, y - cy
            sx = np.rint((c * dx - s * dy) + cx).astype(np.int64)
            sy = np.rint((s * dx + c * dy) + cy).astype(np.int64)
            live = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
            want = np.where(live, (np.clip(sy, 0, H - 1) * W + np.clip(sx, 0, W - 1) + 1).astype(f), f(0))
            got = rotate(img, angle)[0].numpy()
            tie = near_tie_mask(H, W, angle)
            assert tie.mean() <= 0.015, (H, W, angle, tie.mean())
            if angle in (0.0, 90.0):
                assert not tie.any()
            np.testing.assert_array_equal(got[~tie], want[~tie], err_msg=f'{H}x{W} {angle}')
        assert torch.equal(rotate(img, 0.0), img)
