"""The packed event-frame store on the device: ``ops.pack_frames`` / ``ops.unpack_frames`` (csrc/k_pack.hip) byte for byte against the
numpy codec, the slot table, the loaders' packed batches through ``packed.batch_to_device`` against the raw tree's batches, and
ingestion with ``write='packed'``.  Every comparison is exact; only well-formed blobs go to the device."""
import os

import numpy as np
import pytest
import torch

from packed_trees import CONTENTS, LOADER_CASES, SHAPES, assert_same_batches, loader_batches, make_frames, make_tree_pair

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def tree_pair(tmp_path_factory):
    return make_tree_pair(str(tmp_path_factory.mktemp('packed')))


def _aligned(blob: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(blob if blob.size else np.zeros(16, np.uint8)).to(DEV)


CASES = [(s, c) for s in SHAPES for c in CONTENTS] + [((2, 20, 240, 304), 'd0.03')]


@pytest.mark.parametrize('shape,content', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_pack_is_the_numpy_codec_and_unpack_inverts_it(ops, shape, content):
    from leod_amd.data.utils import packed
    x = make_frames(shape, content)
    ref_blob, ref_off = packed.encode_frames(x)
    blob, off = ops.pack_frames(torch.from_numpy(x).to(DEV))
    assert blob.is_cuda and blob.dtype is torch.uint8 and not off.is_cuda and off.dtype is torch.int64
    assert np.array_equal(off.numpy(), ref_off)
    assert np.array_equal(blob.cpu().numpy(), ref_blob)
    slot_off = off[:-1].to(DEV)
    out = ops.unpack_frames(blob, slot_off, None, *shape[1:])
    assert out.shape == shape and out.dtype is torch.uint8
    assert np.array_equal(out.cpu().numpy(), x)
    flipped = ops.unpack_frames(blob, slot_off, torch.ones(shape[0], dtype=torch.int32, device=DEV), *shape[1:])
    assert np.array_equal(flipped.cpu().numpy(), x[:, ::-1])


@pytest.mark.parametrize('shape', [(4, 20, 24, 19), (4, 20, 12, 16), (4, 3, 5, 7)], ids=str)        # H*W = 456 and 35: no multiple of 64 or 16; 192: of both
def test_unpack_slot_table(ops, shape):
    """An [L, B] table of permuted, repeated, zero (-1) and channel-flipped slots into a buffer pre-filled with 0xFF: every byte of it
    is compared with the numpy composition, so the zeros are written too."""
    from leod_amd.data.utils import packed
    L, B = 5, 3
    x = make_frames(shape, 'd0.03', seed=8)
    x[3] = make_frames(shape, 'd0.5', seed=9)[3]
    blob, off = packed.encode_frames(x)
    frame = np.array([[2, -1, 0], [3, 3, 1], [-1, -1, -1], [0, 2, 3], [1, 0, -1]])                  # [L, B]
    flip = np.array([[1, 0, 0], [0, 1, 1], [1, 0, 0], [0, 1, 0], [1, 1, 1]], dtype=np.int32)
    slot_off = np.where(frame >= 0, off[np.maximum(frame, 0)], -1).astype(np.int64)
    want = np.zeros((L, B) + shape[1:], dtype=np.uint8)
    for t in range(L):
        for b in range(B):
            if frame[t, b] >= 0:
                want[t, b] = x[frame[t, b]][::-1] if flip[t, b] else x[frame[t, b]]
    out = torch.full((L, B) + shape[1:], 0xFF, dtype=torch.uint8, device=DEV)
    got = ops.unpack_frames(_aligned(blob), torch.from_numpy(slot_off.reshape(-1)).to(DEV), torch.from_numpy(flip.reshape(-1)).to(DEV),
                            *shape[1:], out=out)
    assert got is out
    assert np.array_equal(out.cpu().numpy(), want)


def test_ops_refuse_host_tensors_and_other_dtypes(ops):
    from leod_amd._lib import LeodHipError
    x = torch.zeros((2, 2, 5, 7), dtype=torch.uint8)
    with pytest.raises(LeodHipError):
        ops.pack_frames(x)
    with pytest.raises(LeodHipError):
        ops.pack_frames(x.to(DEV).float())
    blob, off = ops.pack_frames(x.to(DEV))
    slots = off[:-1].to(DEV)
    with pytest.raises(LeodHipError):
        ops.unpack_frames(blob.cpu(), slots, None, 2, 5, 7)
    with pytest.raises(LeodHipError):
        ops.unpack_frames(blob, slots.cpu(), None, 2, 5, 7)
    with pytest.raises(LeodHipError):
        ops.unpack_frames(blob.to(torch.int8), slots, None, 2, 5, 7)
    with pytest.raises(LeodHipError):
        ops.unpack_frames(blob, slots.to(torch.int32), None, 2, 5, 7)
    with pytest.raises(LeodHipError):
        ops.unpack_frames(blob, slots, torch.zeros(2, dtype=torch.int64, device=DEV), 2, 5, 7)
    with pytest.raises(LeodHipError):
        ops.unpack_frames(blob, slots, None, 2, 5, 7, out=torch.empty((3, 2, 5, 7), dtype=torch.uint8, device=DEV))
    with pytest.raises(LeodHipError):
        ops.unpack_frames(blob, slots, None, 2, 5, 7, out=torch.empty((2, 2, 5, 7), dtype=torch.uint8))


@pytest.mark.parametrize('case', LOADER_CASES)
def test_packed_batches_through_batch_to_device_equal_the_raw_trees(ops, tree_pair, case):
    """Stream / random / mixed loaders (L = 5, B = 3; time flip with probability 1 in one case; padded tails and exhausted slots in
    'test') over the packed tree with packed_decode='device', moved by ``packed.batch_to_device``, against the raw tree's batches
    moved as dense tensors: frames per timestep, labels, flags and padding masks."""
    from leod_amd.data.utils.packed import PackedBatch
    from leod_amd.data.utils.types import DataType
    from leod_amd.modules.utils.detection import DATA_KEY
    raw, packed_tree = tree_pair
    got = loader_batches(packed_tree, case, 'device')
    want = loader_batches(raw, case, 'device')
    halves = lambda batches: [h[DATA_KEY][DataType.EV_REPR] for b in batches for h in (b.values() if DATA_KEY not in b else [b])]
    assert all(isinstance(e, PackedBatch) for e in halves(got)) and not any(isinstance(e, PackedBatch) for e in halves(want))
    for e, w in zip(halves(got), halves(want)):                      # per timestep, on the device
        from leod_amd.data.utils.packed import batch_to_device
        moved = batch_to_device(e, DEV)
        assert len(moved) == len(w) == 5
        for t in range(5):
            assert moved[t].is_cuda and torch.equal(moved[t], w[t].to(DEV)), t
    assert_same_batches(got, want, device=DEV)


def test_module_transfer_expands_packed_batches(ops, tree_pair):
    """``Module.transfer_batch_to_device`` is where a training loop meets a packed batch: the same L device tensors as for the raw tree."""
    from leod_amd.data.utils.types import DataType
    from leod_amd.modules.detection import Module
    from leod_amd.modules.utils.detection import DATA_KEY
    raw, packed_tree = tree_pair
    got = loader_batches(packed_tree, 'fit-stream', 'device', limit=2)
    want = loader_batches(raw, 'fit-stream', 'device', limit=2)
    mod = Module.__new__(Module)                                  # the method reads one class attribute and no instance state
    for g, w in zip(got, want):
        ev = Module.transfer_batch_to_device(mod, g, torch.device(DEV), 0)[DATA_KEY][DataType.EV_REPR]
        ref = Module.transfer_batch_to_device(mod, w, torch.device(DEV), 0)[DATA_KEY][DataType.EV_REPR]
        assert isinstance(ev, list) and len(ev) == len(ref) == 5
        assert all(a.is_cuda and a.shape == b.shape and torch.equal(a, b) for a, b in zip(ev, ref))


@pytest.mark.parametrize('dataset', ['gen1', 'gen4'])
def test_ingest_writes_a_packed_store_equal_to_the_raw_twin(ops, tmp_path, dataset):
    from test_ingest_gpu import BOX_TIMES, D, _write_recording
    from leod_amd.data import ingest
    from leod_amd.data.genx_utils.sequence_rnd import SequenceForRandomAccess
    from leod_amd.data.utils import misc, packed
    from leod_amd.data.utils.types import DatasetType, DataType
    src = str(tmp_path / 'raw')
    if dataset == 'gen1':
        _write_recording(src, 'rec', 1, (240, 304), 6000, 1.0, BOX_TIMES, 2)
        L, dtype = 3, DatasetType.GEN1
    else:
        _write_recording(src, 'rec', 9, (720, 1280), 8000, 0.15, [D, 2 * D, 2 * D, 2 * D, 2 * D, 3 * D], 5)
        L, dtype = 2, DatasetType.GEN4
    dirs = {w: str(tmp_path / w / dataset / 'train' / 'rec') for w in ('npy', 'packed')}
    reps = {w: ingest.ingest_recording(os.path.join(src, 'rec_td.dat'), os.path.join(src, 'rec_bbox.npy'), dirs[w], dataset, write=w)
            for w in ('npy', 'packed')}
    assert {k: v for k, v in reps['npy'].items() if k != 'recording'} == {k: v for k, v in reps['packed'].items() if k != 'recording'}
    ev_dir = misc.get_ev_dir(dirs['packed'])
    assert sorted(f for f in os.listdir(ev_dir) if f.startswith('event_representations')) == \
        ['event_representations' + ('_ds2_nearest' if dataset == 'gen4' else '') + '.evp']
    dense = np.load(misc.get_ev_raw_fn(dirs['npy'], dataset))
    st = misc.open_ev_repr(dirs['packed'], dataset)
    assert isinstance(st, packed.PackedFrames) and st.shape == dense.shape
    assert np.array_equal(st.read(0, len(st)), dense)             # validates every frame on the way
    blob, off = st.read_packed(0, len(st))
    st.close()
    ref_blob, ref_off = packed.encode_frames(dense)
    assert np.array_equal(off, ref_off) and np.array_equal(blob, ref_blob)
    for fn in ('objframe_idx_2_repr_idx.npy',):
        assert np.array_equal(np.load(os.path.join(ev_dir, fn)), np.load(os.path.join(misc.get_ev_dir(dirs['npy']), fn)))
    misc.FRAME_STORES.clear()
    seqs = {w: SequenceForRandomAccess(dirs[w], misc.EV_REPR_NAME, L, dtype, downsample_by_factor_2=dataset == 'gen4',
                                       only_load_end_labels=False) for w in dirs}
    assert len(seqs['packed']) == len(seqs['npy']) > 0
    for i in range(len(seqs['npy'])):
        a, b = seqs['npy'][i], seqs['packed'][i]
        assert a[DataType.EV_IDX] == b[DataType.EV_IDX]
        assert all(torch.equal(p, q) for p, q in zip(a[DataType.EV_REPR], b[DataType.EV_REPR]))


def test_ingest_command_line_writes_packed_trees_the_loaders_read(ops, tmp_path):
    """``python -m leod_amd.data.ingest SRC DST --dataset gen1 --write packed`` (its ``main``, in this process), then the evaluation
    loader over the packed tree with the device decoder against the same loader over the ``--write npy`` tree."""
    from test_ingest_gpu import BOX_TIMES, _write_recording
    from leod_amd.data import ingest
    from leod_amd.data.utils import misc
    from leod_amd.data.utils.packed import PackedBatch
    from leod_amd.data.utils.types import DataType
    from leod_amd.modules.data.genx import DataModule
    from leod_amd.modules.utils.detection import DATA_KEY
    from packed_trees import dataset_cfg, frame_files
    src = str(tmp_path / 'raw')
    for name, seed in (('recA', 3), ('recB', 4)):
        _write_recording(os.path.join(src, 'test'), name, seed, (240, 304), 3000, 1.0, BOX_TIMES, 2)
    batches = {}
    for write in ('npy', 'packed'):
        dst = str(tmp_path / write / 'gen1')
        assert ingest.main([src, dst, '--dataset', 'gen1', '--write', write]) == 0
        assert len(frame_files(dst, '.evp' if write == 'packed' else '.npy')) == 2 and frame_files(dst, '.tmp') == []
        misc.FRAME_STORES.clear()
        dm = DataModule(dataset_cfg(dst), num_workers_train=1, num_workers_eval=1, batch_size_train=2, batch_size_eval=2, prefetch=0,
                        io_threads=1, packed_decode='device')
        dm.setup('test')
        batches[write] = list(dm.test_dataloader())
    assert all(isinstance(b[DATA_KEY][DataType.EV_REPR], PackedBatch) for b in batches['packed'])
    assert_same_batches(batches['packed'], batches['npy'], device=DEV)


def test_converter_encodes_on_the_device(ops, tree_pair, tmp_path):
    import shutil
    from leod_amd.data import pack
    from leod_amd.data.utils import misc
    from packed_trees import frame_files
    tree = str(tmp_path / 'gen1')
    shutil.copytree(os.path.join(tree_pair[0], 'val'), os.path.join(tree, 'val'))
    before = {fn: np.load(fn) for fn in frame_files(tree, '.npy')}
    reports = pack.pack_tree(tree, remove_raw=True)
    assert len(reports) == 5 and all(r['encoder'] == 'device' for r in reports) and frame_files(tree, '.npy') == []
    misc.FRAME_STORES.clear()
    for fn, x in before.items():
        assert np.array_equal(misc.read_ev_repr(os.path.dirname(os.path.dirname(os.path.dirname(fn)))), x)
        # the device encoder wrote what the numpy encoder writes
        ref = str(tmp_path / 'ref.evp')
        w = pack.PackedWriter(ref, *x.shape[1:])
        for a in range(0, len(x), pack.FRAMES_PER_CHUNK):
            w.append_frames(x[a:a + pack.FRAMES_PER_CHUNK])
        w.close()
        assert open(ref, 'rb').read() == open(os.path.splitext(fn)[0] + '.evp', 'rb').read()
