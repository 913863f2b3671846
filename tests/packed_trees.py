"""Shared by tests/test_packed_cpu.py and tests/test_packed_gpu.py: frame contents for the codec cases and a pair of dataset trees that
hold the same recordings, once as raw ``.npy`` twins and once as packed ``.evp`` stores."""
import os
import shutil

import numpy as np

from oracle.synth import synth_dataset_tree

SHAPES = [(3, 2, 5, 7), (2, 20, 6, 8), (2, 20, 24, 19)]          # E = 70: one full + one partial block; 960; 9120: two groups + 14.25 blocks
CONTENTS = ['zero', 'full', 'first', 'last', 'd0.001', 'd0.03', 'd0.5']
FRAME_HW = (12, 16)
STEM = 'event_representations'


def make_frames(shape, content, seed=0):
    rng = np.random.default_rng(seed)
    x = np.zeros(shape, dtype=np.uint8)
    flat = x.reshape(shape[0], -1)
    if content == 'full':
        x[:] = 255
    elif content == 'first':
        flat[:, 0] = 7
    elif content == 'last':
        flat[:, -1] = 9
    elif content.startswith('d'):
        x[:] = ((rng.random(shape) < float(content[1:])) * rng.integers(1, 256, shape)).astype(np.uint8)
    return x


def frame_files(tree, ext):
    out = []
    for root, _, files in sorted(os.walk(tree)):
        out += [os.path.join(root, f) for f in sorted(files) if f.startswith(STEM) and f.endswith(ext)]
    return out


def make_tree_pair(root):
    """-> (raw tree, packed tree): gen1 trees of the loader recordings with [20, 12, 16] frames thinned to ~10 % non-zeros (the
    frame / channel / recording tags in the first row stay); the packed tree holds only .evp frame files written by the numpy codec."""
    from leod_amd.data.utils.packed import PackedWriter
    raw = synth_dataset_tree(os.path.join(root, 'raw'), 'gen1', False, frame_hw=FRAME_HW)
    rng = np.random.default_rng(5)
    for fn in frame_files(raw, '.npy'):
        frames = np.load(fn)
        keep = rng.random(frames.shape) < 0.1
        keep[:, :, 0, :3] = True
        np.save(fn, frames * keep)
    packed = os.path.join(root, 'packed', 'gen1')
    shutil.copytree(raw, packed)
    for fn in frame_files(packed, '.npy'):
        frames = np.load(fn)
        w = PackedWriter(os.path.splitext(fn)[0] + '.evp', *frames.shape[1:])
        w.append_frames(frames[:len(frames) // 2])
        w.append_frames(frames[len(frames) // 2:])
        w.close()
        os.remove(fn)
        os.remove(os.path.splitext(fn)[0] + '.h5')
    return raw, packed


def dataset_cfg(tree, **over):
    from leod_amd.config import full_config
    return full_config('gen1', 'small', overrides=dict(dataset=dict(path=tree, sequence_length=5, **over))).dataset


LOADER_CASES = ['fit-stream', 'fit-random', 'fit-mixed', 'fit-mixed-tflip', 'test']


def loader_batches(tree, case, packed_decode, limit=6):
    """The first ``limit`` batches of one loader over ``tree`` (L = 5, B = 3), seeded; 'test' streams every recording from frame 0 with
    padded tails and exhausted slots."""
    import torch
    from leod_amd.data.utils import misc
    from leod_amd.modules.data.genx import DataModule
    misc.FRAME_STORES.clear()
    torch.manual_seed(7)
    np.random.seed(7)
    import random
    random.seed(7)
    over = {}
    if case.startswith('fit'):
        mode = case.split('-')[1]
        over['train'] = dict(sampling=mode)
        if case.endswith('tflip'):
            over['data_augmentation'] = dict(random=dict(prob_tflip=1.0), stream=dict(prob_tflip=1.0))
    else:
        over['data_augmentation'] = dict(stream=dict(start_from_zero=True))
    dm = DataModule(dataset_cfg(tree, **over), num_workers_train=2, num_workers_eval=1, batch_size_train=3, batch_size_eval=3,
                    prefetch=0, io_threads=1, pin_memory=False, packed_decode=packed_decode)
    dm.setup('fit' if case.startswith('fit') else 'test')
    loader = dm.train_dataloader() if case.startswith('fit') else dm.test_dataloader()
    out = []
    for k, batch in enumerate(loader):
        out.append(batch)
        if len(out) >= limit and case != 'test':
            break
    return out


def flatten(o, out, prefix='', device=None):
    """Batch structure -> [(path, value)]: tensors as numpy, labels by their fields, recording paths by their last component; a
    ``PackedBatch`` is expanded through ``packed.batch_to_device`` (``device`` None: on the host) so that it compares with dense frames."""
    import torch
    from leod_amd.data.genx_utils.labels import ObjectLabels, SparselyBatchedObjectLabels
    from leod_amd.data.utils.packed import PackedBatch, batch_to_device
    if isinstance(o, PackedBatch):
        o = batch_to_device(o, 'cpu' if device is None else device)
    if torch.is_tensor(o):
        out.append((prefix, o.detach().cpu().clone().numpy()))
    elif isinstance(o, ObjectLabels):
        out.append((prefix + '/ol', o.object_labels.clone().numpy()))
        out.append((prefix + '/hw', np.asarray(o.input_size_hw)))
    elif isinstance(o, SparselyBatchedObjectLabels):
        for i, l in enumerate(o.sparse_object_labels_batch):
            flatten(l, out, f'{prefix}/sb{i}', device)
    elif isinstance(o, dict):
        for k, v in o.items():
            flatten(v, out, f'{prefix}/{k}', device)
    elif isinstance(o, (list, tuple)):
        for i, v in enumerate(o):
            flatten(v, out, f'{prefix}/{i}', device)
    elif isinstance(o, str):
        out.append((prefix, os.path.basename(o)))
    elif o is None or isinstance(o, (int, float, bool)):
        out.append((prefix, o))
    else:                                                       # augmentation states: compare by repr of their fields
        out.append((prefix, repr(getattr(o, '__dict__', o))))
    return out


def assert_same_batches(got, want, device=None):
    assert len(got) == len(want) and len(want) > 0
    n_frames = 0
    for g, w in zip(got, want):
        fg, fw = flatten(g, [], device=device), flatten(w, [], device=device)
        assert [k for k, _ in fg] == [k for k, _ in fw]
        for (k, a), (_, b) in zip(fg, fw):
            if isinstance(a, np.ndarray):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
                n_frames += 'EV_REPR' in k
            else:
                assert a == b, (k, a, b)
    assert n_frames > 0
