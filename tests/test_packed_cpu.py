"""The packed event-frame store (leod_amd/data/utils/packed.py) on the host: the numpy codec that states the format, validation, the
file store and its writer, the frame-file preference of the tree helpers, the sequences and loaders over a packed tree against the raw
twin of the same frames, the tree converter and the committed fixture that pins format version 1."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from packed_trees import (CONTENTS, LOADER_CASES, SHAPES, assert_same_batches, flatten, frame_files, loader_batches, make_frames,
                          make_tree_pair)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
EV_NAME = 'stacked_histogram_dt=50_nbins=10'


@pytest.fixture(scope='module')
def tree_pair(tmp_path_factory):
    return make_tree_pair(str(tmp_path_factory.mktemp('packed')))


# ---- codec ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('content', CONTENTS)
def test_decode_of_encode_is_the_frame(shape, content):
    from leod_amd.data.utils import packed
    x = make_frames(shape, content)
    blob, off = packed.encode_frames(x)
    C, H, W = shape[1:]
    E, G = C * H * W, -(-C * H * W // 4096)
    assert off[0] == 0 and off[-1] == blob.size and blob.dtype == np.uint8 and off.dtype == np.int64
    for k in range(shape[0]):
        b = blob[off[k]:off[k + 1]]
        assert b.size % 16 == 0
        packed.validate_frame(b, C, H, W)
        packed.validate_frame_host(b, C, H, W)
        assert np.array_equal(packed.decode_frame(b, C, H, W), x[k])
        host = np.full((C, H, W), 0xFF, dtype=np.uint8)          # the host library's decoder: every byte written, zeros included
        assert np.array_equal(packed.decode_frame_host(b, C, H, W, out=host), x[k])
        assert np.array_equal(packed.decode_frame_host(b, C, H, W, flip_channels=True, out=host), x[k][::-1])
        assert np.array_equal(packed.decode_frame(b, C, H, W, flip_channels=True), x[k][::-1])
        out = np.full((C, H, W), 0xFF, dtype=np.uint8)
        assert packed.decode_frame(b, C, H, W, out=out) is out and np.array_equal(out, x[k])
        if content == 'zero':
            assert b.size == 16 + 16 * G == packed.zero_frame_bytes(E)
        if content == 'full':
            assert b.size == -(-(16 + 16 * G + 8 * -(-E // 64) + E) // 16) * 16 == packed.worst_frame_bytes(E)
    # one byte string per frame: the same frames encode to the same bytes, whatever array they come from
    again, off2 = packed.encode_frames(np.asfortranarray(x))
    assert np.array_equal(again, blob) and np.array_equal(off2, off)


def _u32(b, pos):
    return b[pos:pos + 4].view('<u4')


def test_validate_frame_refuses_what_a_decoder_could_trip_over():
    from leod_amd.data.utils import packed
    C, H, W = 20, 24, 19                                         # E = 9120, G = 3, 143 blocks, the last one of 32 elements
    G = 3
    x = make_frames((1, C, H, W), 'd0.03', seed=3)[0]
    x.reshape(-1)[[0, 4100, 9119]] = 5                            # every group and the partial block are populated
    x.reshape(-1)[1:4] = 0
    good, _ = packed.encode_frames(x[None])
    if (8 * int(good[:4].view('<u4')[0]) + int(good[4:8].view('<u4')[0])) % 16 == 0:
        x.reshape(-1)[1] = 1                                      # one more value in a block that has one: the blob gets padding bytes
        good, _ = packed.encode_frames(x[None])
    packed.validate_frame(good, C, H, W)
    n_masks, n_values = (int(v) for v in good[:8].view('<u4'))
    assert (16 + 16 * G + 8 * n_masks + n_values) % 16 != 0, 'the case needs padding bytes'

    def bad(mutate, match):
        b = good.copy()
        b = mutate(b)
        with pytest.raises(ValueError, match=match):
            packed.validate_frame(b, C, H, W)
        with pytest.raises(ValueError):                          # the host library's validator refuses the same blobs
            packed.validate_frame_host(b, C, H, W)

    bad(lambda b: b[:-16], 'bytes')                              # truncated
    bad(lambda b: b[:32], 'bytes')                               # not even the group entries
    bad(lambda b: np.concatenate([b, np.zeros(16, np.uint8)]), 'bytes')

    def bump(pos, by=1):
        def f(b):
            _u32(b, pos)[0] += by
            return b
        return f
    bad(bump(0), 'bytes|n_masks')                                # n_masks
    bad(bump(4), 'bytes|n_values')                               # n_values
    bad(bump(4, 16), 'bytes|n_values')                           # a whole padding unit off: sizes cannot tell, the popcounts do
    bad(bump(16 + 16 + 8), 'mask_base')                          # group 1
    bad(bump(16 + 32 + 12), 'value_base')                        # group 2

    def mask_bit_beyond(b):
        m0 = 16 + 16 * G
        b[m0 + 8 * (n_masks - 1):m0 + 8 * n_masks].view('<u8')[0] |= np.uint64(1) << np.uint64(9120 % 64)
        return b
    bad(mask_bit_beyond, 'beyond')

    def block_beyond(b):
        b[16 + 32:16 + 40].view('<u8')[0] |= np.uint64(1) << np.uint64(143 - 128)   # block 143 does not exist
        return b
    bad(block_beyond, 'n_masks|beyond')

    def padding(b):
        b[-1] = 1
        return b
    bad(padding, 'padding')

    def header_padding(b):
        b[12] = 1
        return b
    bad(header_padding, 'padding')


def test_validate_frame_grown_n_values_with_matching_size():
    """n_values raised by 16 together with 16 more bytes: the size fits, the mask popcounts do not."""
    from leod_amd.data.utils import packed
    x = make_frames((1, 2, 5, 7), 'd0.5', seed=1)[0]
    good, _ = packed.encode_frames(x[None])
    b = np.concatenate([good, np.ones(16, np.uint8)])
    _u32(b, 4)[0] += 16
    with pytest.raises(ValueError):
        packed.validate_frame(b, 2, 5, 7)
    with pytest.raises(ValueError):
        packed.validate_frame_host(b, 2, 5, 7)


# ---- store ---------------------------------------------------------------------------------------------------------------------------
def test_writer_and_store(tmp_path):
    from leod_amd.data.utils import misc, packed
    x = make_frames((9, 20, 6, 8), 'd0.03', seed=2)
    fn = str(tmp_path / 'event_representations.evp')
    w = packed.PackedWriter(fn, 20, 6, 8)
    w.append(*packed.encode_frames(x[:4]))
    assert os.path.exists(fn + '.tmp') and not os.path.exists(fn)
    w.append_frames(x[4:])
    with pytest.raises(ValueError):
        w.append(np.zeros(8, np.uint8), np.array([0, 8]))
    w.close()
    assert os.path.exists(fn) and not os.path.exists(fn + '.tmp')
    assert misc.read_frame_header(fn) == (9, (20, 6, 8))
    raw = open(fn, 'rb').read()
    assert raw[:8] == b'LEODEVP1' and np.frombuffer(raw[8:28], '<u4').tolist() == [1, 9, 20, 6, 8]
    data_pos, table_pos = np.frombuffer(raw[32:48], '<u8').tolist()
    table = np.frombuffer(raw[table_pos:table_pos + 80], '<u8')
    assert data_pos == 64 and table[0] == 0 and data_pos + table[-1] == table_pos and len(raw) == table_pos + 80
    st = packed.PackedFrames(fn)
    assert st.shape == (9, 20, 6, 8) and len(st) == 9
    assert np.array_equal(st.read(0, 9), x) and np.array_equal(st.read(3, 5), x[3:5])
    out = np.full((4, 20, 6, 8), 0xFF, np.uint8)                 # contiguous
    assert st.read(2, 6, out=out) is out and np.array_equal(out, x[2:6])
    batch = np.full((4, 3, 20, 6, 8), 0xFF, np.uint8)            # per-frame contiguous: a slot of a batch buffer
    st.read(5, 9, out=batch[:, 1])
    assert np.array_equal(batch[:, 1], x[5:9]) and (batch[:, 0] == 0xFF).all() and (batch[:, 2] == 0xFF).all()
    blob, off = st.read_packed(2, 5)
    ref_blob, ref_off = packed.encode_frames(x[2:5])
    assert np.array_equal(blob, ref_blob) and np.array_equal(off, ref_off)
    st.close()
    # a store whose frame does not validate refuses to hand it out
    broken = bytearray(raw)
    broken[64 + 4] ^= 1                                          # n_values of frame 0
    fn2 = str(tmp_path / 'broken.evp')
    open(fn2, 'wb').write(bytes(broken))
    st = packed.PackedFrames(fn2)
    with pytest.raises(ValueError, match='frame 0'):
        st.read(0, 2)
    assert np.array_equal(st.read(1, 3), x[1:3])
    st.close()
    with pytest.raises(ValueError):
        packed.read_header(__file__)                             # no .evp file at all


def test_frame_store_lru_serves_packed_stores(tmp_path):
    from leod_amd.data.utils import misc, packed
    cache = misc.FrameStoreCache(capacity=2)
    fns = []
    for k in range(3):
        fn = str(tmp_path / f'r{k}.evp')
        w = packed.PackedWriter(fn, 2, 5, 7)
        w.append_frames(make_frames((3, 2, 5, 7), 'd0.5', seed=k))
        w.close()
        fns.append(fn)
    a = cache.get(fns[0])
    assert isinstance(a, packed.PackedFrames) and cache.get(fns[0]) is a
    cache.get(fns[1]); cache.get(fns[2])
    assert len(cache) == 2 and cache.get(fns[0]) is not a
    assert np.array_equal(a.read(0, 3), make_frames((3, 2, 5, 7), 'd0.5', seed=0))       # an evicted store still serves its holder


def test_open_ev_repr_prefers_npy_then_evp_then_h5(tmp_path):
    from h5_writer import write_h5
    from leod_amd.data.utils import misc, packed
    x = make_frames((4, 20, 6, 8), 'd0.03', seed=4)

    def tree(name, kinds):
        seq = str(tmp_path / name / 'gen1' / 'train' / 'rec')
        ev = os.path.join(seq, 'event_representations_v2', EV_NAME)
        os.makedirs(ev)
        stem = os.path.join(ev, 'event_representations')
        if 'npy' in kinds:
            np.save(stem + '.npy', x)
        if 'evp' in kinds:
            w = packed.PackedWriter(stem + '.evp', 20, 6, 8)
            w.append_frames(x)
            w.close()
        if 'h5' in kinds:
            write_h5(stem + '.h5', x)
        return seq
    for kinds, want in ((('npy', 'evp'), misc.RawFrames), (('evp', 'h5'), packed.PackedFrames), (('evp',), packed.PackedFrames),
                        (('npy', 'evp', 'h5'), misc.RawFrames)):
        seq = tree('_'.join(kinds), kinds)
        st = misc.open_ev_repr(seq, 'gen1')
        assert type(st) is want, kinds
        assert np.array_equal(st.read(0, 4), x)
        st.close()
        assert [os.path.splitext(f)[1][1:] for f in misc.ev_repr_files(seq, 'gen1')] == [k for k in ('npy', 'evp', 'h5') if k in kinds]
        assert np.array_equal(misc.read_ev_repr(seq), x)
    with pytest.raises(FileNotFoundError):
        misc.open_ev_repr(tree('none', ()), 'gen1')


# ---- sequences and loaders ------------------------------------------------------------------------------------------------------------
def test_sequences_over_a_packed_tree_yield_the_raw_trees_samples(tree_pair):
    from leod_amd.data.genx_utils.sequence_rnd import SequenceForRandomAccess
    from leod_amd.data.genx_utils.sequence_streaming import SequenceForIter
    from leod_amd.data.utils import misc
    from leod_amd.data.utils.types import DatasetType
    raw, packed_tree = tree_pair
    misc.FRAME_STORES.clear()
    n = 0
    for rec in ('rec_a', 'rec_c', 'rec_e'):
        for flip in (False, True):
            pair = []
            for tree in (raw, packed_tree):
                kw = dict(path=os.path.join(tree, 'train', rec), ev_representation_name=EV_NAME, sequence_length=5,
                          dataset_type=DatasetType.GEN1, downsample_by_factor_2=False)
                it = SequenceForIter(**kw, start_from_zero=True)
                rnd = SequenceForRandomAccess(**kw, only_load_end_labels=False)
                assert str(it.ev_repr_file).endswith('.npy' if tree == raw else '.evp')
                np.random.seed(1)
                pair.append([it.sample(i, time_flip=flip) for i in range(len(it))] +
                            [rnd.sample(i, time_flip=flip) for i in range(len(rnd))])
            fa, fb = flatten(pair[0], []), flatten(pair[1], [])
            assert [k for k, _ in fa] == [k for k, _ in fb]
            for (k, a), (_, b) in zip(fa, fb):
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, k
            n += len(fa)
    assert n > 0


@pytest.mark.parametrize('case', LOADER_CASES)
def test_loaders_with_host_decode_equal_the_raw_tree(tree_pair, case):
    """StreamLoader / RandomLoader / MixedLoader over the packed tree, decoding on the reader threads: the raw tree's batches."""
    raw, packed_tree = tree_pair
    want = loader_batches(raw, case, 'host')
    assert_same_batches(loader_batches(packed_tree, case, 'host'), want)
    if case == 'test':                                           # the cases the slot table has to express are in here
        from leod_amd.data.utils.types import DataType
        from leod_amd.modules.utils.detection import DATA_KEY
        assert any('' in b[DATA_KEY][DataType.PATH] for b in want), 'an exhausted slot'
        assert any(bool(m.any()) and not bool(m.all()) for b in want for m in b[DATA_KEY][DataType.IS_PADDED_MASK]), 'a padded tail'


@pytest.mark.parametrize('case', LOADER_CASES)
def test_loaders_with_packed_batches_decode_to_the_raw_tree_on_the_host(tree_pair, case):
    """packed_decode='device' without a device: the batches carry blobs + slot table, ``batch_to_device(.., 'cpu')`` expands them."""
    from leod_amd.data.utils.packed import PackedBatch
    from leod_amd.data.utils.types import DataType
    from leod_amd.modules.utils.detection import DATA_KEY
    raw, packed_tree = tree_pair
    got = loader_batches(packed_tree, case, 'device')
    halves = [h for b in got for h in (b.values() if DATA_KEY not in b else [b])]
    assert all(isinstance(h[DATA_KEY][DataType.EV_REPR], PackedBatch) for h in halves)
    assert all(int(o) % 16 == 0 for h in halves for o in h[DATA_KEY][DataType.EV_REPR].slot_off if o >= 0)
    assert_same_batches(got, loader_batches(raw, case, 'host'))
    # a tree without packed stores is assembled densely whatever the setting
    dense = loader_batches(raw, case, 'device', limit=1)
    assert not any(isinstance(h[DATA_KEY][DataType.EV_REPR], PackedBatch)
                   for b in dense for h in (b.values() if DATA_KEY not in b else [b]))


def test_unknown_packed_decode_is_refused(tree_pair):
    from leod_amd.modules.data.genx import DataModule
    from packed_trees import dataset_cfg
    with pytest.raises(ValueError, match='packed_decode'):
        DataModule(dataset_cfg(tree_pair[0]), 1, 1, 2, 2, packed_decode='gpu')


# ---- converter ------------------------------------------------------------------------------------------------------------------------
def test_pack_converter_on_a_raw_tree(tree_pair, tmp_path, monkeypatch):
    from leod_amd.data import pack
    from leod_amd.data.utils import misc
    tree = str(tmp_path / 'gen1')
    shutil.copytree(os.path.join(tree_pair[0], 'val'), os.path.join(tree, 'val'))
    before = {fn: np.load(fn) for fn in frame_files(tree, '.npy')}
    assert len(before) == 5
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, '-m', 'leod_amd.data.pack', tree, '--device', 'cpu'], cwd=ROOT, env=env, capture_output=True,
                         text=True)
    assert res.returncode == 0, res.stderr
    assert len(frame_files(tree, '.evp')) == 5 and len(frame_files(tree, '.npy')) == 5          # nothing removed without the flag
    for fn, x in before.items():
        st = misc.open_frame_file(os.path.splitext(fn)[0] + '.evp')
        assert np.array_equal(st.read(0, len(st)), x)
        st.close()
    # --remove-raw: a conversion that does not decode to its source removes nothing ...
    real = pack.PackedFrames.read
    monkeypatch.setattr(pack.PackedFrames, 'read', lambda self, a, b, out=None: real(self, a, b, out) ^ np.uint8(a == 0))
    with pytest.raises(IOError, match='do not decode'):
        pack.pack_tree(tree, device='cpu', remove_raw=True)
    assert len(frame_files(tree, '.npy')) == 5
    monkeypatch.undo()
    # ... and one that does removes the .npy and the .h5 of the stem, after which the tree reads the same through the .evp
    reports = pack.pack_tree(tree, device='cpu', remove_raw=True)
    assert len(reports) == 5 and all(r['encoder'] == 'numpy' and len(r['removed']) == 2 for r in reports)
    assert frame_files(tree, '.npy') == [] and frame_files(tree, '.h5') == []
    misc.FRAME_STORES.clear()
    for fn, x in before.items():
        seq = os.path.dirname(os.path.dirname(os.path.dirname(fn)))
        assert np.array_equal(misc.read_ev_repr(seq), x)


# ---- the committed fixture: format version 1 ------------------------------------------------------------------------------------------
def test_golden_fixture_pins_format_version_1(golden_dir):
    from leod_amd.data.utils import packed
    fn = os.path.join(golden_dir, 'p01_frames.evp')
    x = np.load(os.path.join(golden_dir, 'p01_frames.npy'))
    assert os.path.getsize(fn) < 100_000 and x.shape == (6, 20, 24, 19) and x.dtype == np.uint8
    st = packed.PackedFrames(fn)
    assert st.shape == x.shape and np.array_equal(st.read(0, len(st)), x)
    blob, off = st.read_packed(0, len(st))
    st.close()
    ref_blob, ref_off = packed.encode_frames(x)
    assert np.array_equal(off, ref_off) and np.array_equal(blob, ref_blob)
    raw = open(fn, 'rb').read()
    table = np.concatenate([[0], np.cumsum(np.diff(ref_off))]).astype('<u8').tobytes()
    header = b'LEODEVP1' + np.array([1, 6, 20, 24, 19, 0], '<u4').tobytes() + np.array([64, 64 + blob.size], '<u8').tobytes() + bytes(16)
    assert raw == header + blob.tobytes() + table


def test_ingest_still_refuses_other_frame_files(tmp_path):
    from leod_amd.data import ingest
    for write in ('h5', 'evp', ''):
        with pytest.raises(ValueError, match='npy'):
            ingest.ingest_recording('a_td.dat', 'a_bbox.npy', str(tmp_path), 'gen1', write=write)
