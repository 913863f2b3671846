#!/usr/bin/env python
"""Record tests/golden/g26_rotation.npz by importing and running the REFERENCE (/root/reference) on CPU, like make_golden.py
(same ``ref_stubs`` path; runs only in the build container, never on the GPU box).

(a) Labels: ``ObjectLabels.rotate_`` of the reference (data/genx_utils/labels.py:327-370) on the label rows of
    ``oracle.synth.synth_augment_sample`` and on one hand-made frame whose corner box a 33 degree rotation pushes out of the frame
    (``remove_flat_labels_`` fires).  The labels need no torchvision: pure reference output.
(b) Whole augmentor: ``RandomSpatialAugmentorGenX.__call__`` of the reference (data/utils/augmentor.py:455-476) with the g14
    configuration changed to ``rotate.prob = 1, max_angle_deg = 20`` and g14's seeding: drawn state (now with ``rotation.active`` and
    ``angle_deg``), augmented uint8 frames, transformed labels.  torchvision is absent here (its stand-in raises on purpose), so the
    name ``rotate`` in the namespace of the reference's augmentor module is replaced, for this run only, by ``tests/rotation_ref.py``.
    What (b) pins is therefore the reference's COMPOSITION ORDER (flip -> rotate -> zoom), its random draws and its label arithmetic;
    the pixel rule inside the rotation is the restatement of torchvision's code path, not torchvision itself.

Usage:  python tests/golden/make_golden_rotation.py        # rewrites tests/golden/g26_rotation.npz
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, 'ref_stubs'))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.get_device_name = lambda *a, **k: 'none'  # called at import time by the reference's coco_eval
torch.set_num_threads(8)

from omegaconf import DictConfig  # noqa: E402  (stand-in)
from oracle.synth import synth_augment_sample, AUGMENT_CASES, AUGMENT_CFG  # noqa: E402
import rotation_ref  # noqa: E402

# ---- reference imports ---------------------------------------------------------------------------
from data.genx_utils.labels import ObjectLabels, SparselyBatchedObjectLabels  # noqa: E402
from data.utils import augmentor as ref_augmentor  # noqa: E402
from data.utils.types import DataType  # noqa: E402

LABEL_CASES = [(0, 60, 76), (1, 60, 76), (2, 60, 76), (3, 60, 76), (100, 48, 64)]
LABEL_ANGLES = [4.0, -4.0, 15.0, -33.0, 90.0]
# a frame with a box in the top-left corner (leaves the frame at +-33 degrees) and one around the centre (stays)
CORNER_HW = (60, 76)
CORNER_ROWS = np.array([[1000., 0., 0., 6., 5., 0., 1., 1.], [1000., 30., 22., 14., 12., 1., 1., 1.]], dtype=np.float32)
CORNER_ANGLES = LABEL_ANGLES + [33.0]


def rotation_cfg():
    cfg = copy.deepcopy(AUGMENT_CFG)
    cfg['rotate'] = dict(prob=1, min_angle_deg=2, max_angle_deg=20)
    return cfg


def main():
    out = {'label_angles': np.array(LABEL_ANGLES), 'corner_angles': np.array(CORNER_ANGLES), 'corner_rows': CORNER_ROWS,
           'corner_hw': np.array(CORNER_HW, dtype=np.int64)}
    # (a) labels
    for seed, H, W in LABEL_CASES:
        _, labels = synth_augment_sample(seed, H, W)
        for t, l in enumerate(labels):
            if l is None:
                continue
            for a, angle in enumerate(LABEL_ANGLES):
                obj = ObjectLabels(l.clone(), (H, W))
                obj.rotate_(angle)
                out[f'a_s{seed}_t{t}_a{a}'] = obj.object_labels.numpy().astype(np.float32)
    dropped = 0
    for a, angle in enumerate(CORNER_ANGLES):
        obj = ObjectLabels(torch.from_numpy(CORNER_ROWS.copy()), CORNER_HW)
        obj.rotate_(angle)
        out[f'a_corner_a{a}'] = obj.object_labels.numpy().astype(np.float32)
        dropped += len(obj) < len(CORNER_ROWS)
    assert dropped >= 2, 'the corner box was meant to leave the frame at +-33 degrees'
    # (b) the whole augmentor
    ref_augmentor.rotate = rotation_ref.rotate
    cfg = DictConfig(rotation_cfg())
    for seed, H, W in AUGMENT_CASES:
        ev, labels = synth_augment_sample(seed, H, W)
        aug = ref_augmentor.RandomSpatialAugmentorGenX(dataset_hw=(H, W), automatic_randomization=True, augm_config=cfg)
        objs = [None if l is None else ObjectLabels(l.clone(), (H, W)) for l in labels]
        torch.manual_seed(900 + seed)
        res = aug({DataType.EV_REPR: [e.clone() for e in ev], DataType.OBJLABELS_SEQ: SparselyBatchedObjectLabels(objs)})
        st = res[DataType.AUGM_STATE]
        assert st.rotation.active
        out[f'b_s{seed}_state'] = np.array([float(st.apply_h_flip), float(st.zoom_in.active), st.zoom_in.x0, st.zoom_in.y0,
                                            st.zoom_in.zoom_in_factor, float(st.zoom_out.active), st.zoom_out.x0, st.zoom_out.y0,
                                            st.zoom_out.zoom_out_factor, float(st.rotation.active), st.rotation.angle_deg],
                                           dtype=np.float64)
        out[f'b_s{seed}_ev'] = torch.stack(res[DataType.EV_REPR]).numpy()
        for t, l in enumerate(res[DataType.OBJLABELS_SEQ]):
            if l is not None:                                   # a frame emptied by the rotation alone stays, with 0 rows
                out[f'b_s{seed}_lab{t}'] = l.object_labels.numpy().astype(np.float32).reshape(-1, 8)
                out[f'b_s{seed}_hw{t}'] = np.array(l.input_size_hw, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, 'g26_rotation.npz'), **out)
    print('wrote g26_rotation.npz', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
