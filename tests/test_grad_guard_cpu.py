"""Host side of the non-finite guard and the per-parameter gradient statistics (leod_grad_stats, leod_adamw_clip_step_guarded): the
C-ABI declarations, the refusal of CPU tensors, the host builder of the segment and chunk tables against a brute-force map, and
the default of ``FlatAdamW``'s new argument.  No GPU."""
import inspect

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as g
    g.build()
    from leod_amd import _lib
    return _lib


def seg_lengths(C):
    return [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3, 70001]


def aligned_offsets(lengths, align=4):
    offs, n = [], 0
    for k in lengths:
        offs.append(n)
        n += (k + align - 1) // align * align
    return offs, n


def test_header_declares_the_entries(built):
    protos = built.parse_header()
    for name in ('leod_grad_stats', 'leod_grad_stats_query', 'leod_adamw_clip_step_guarded'):
        assert name in protos
    names = [a.__name__ if hasattr(a, '__name__') else str(a) for a in protos['leod_adamw_clip_step_guarded'][1]]
    assert names[:4] == ['Ptr_float'] * 4 and names[-4:-1] == ['Ptr_int', 'Ptr_int', 'Ptr_float']
    # the plain entry's arguments without `step` and `hp_dev`, plus total, state and scratch
    assert len(protos['leod_adamw_clip_step_guarded'][1]) == len(protos['leod_adamw_clip_step'][1]) - 2 + 3
    stats = [a.__name__ if hasattr(a, '__name__') else str(a) for a in protos['leod_grad_stats'][1]]
    assert stats[0] == 'Ptr_float' and stats[-4:-1] == ['Ptr_double', 'Ptr_int', 'Ptr_int']


def test_chunk_query(built):
    from leod_amd import ops
    C = ops.GRAD_STATS_CHUNK
    assert C >= 1024 and C % 1024 == 0                        # whole 256-lane x 16-byte rounds
    assert ops._grad_stats_query(0) == (C, 0)
    assert ops._grad_stats_query(7)[1] == 7 * ops._grad_stats_query(1)[1] > 0
    with pytest.raises(built.LeodHipError):
        ops._grad_stats_query(-1)


def test_ops_refuse_cpu_tensors(built):
    from leod_amd import ops
    plan = ops.GradStatsPlan([0, 4], [3, 4], 'cpu')
    with pytest.raises(built.LeodHipError):
        ops.grad_stats(torch.zeros(8), plan)
    z = torch.zeros(8)
    with pytest.raises(built.LeodHipError):
        ops.adamw_clip_step_guarded(z, z.clone(), z.clone(), z.clone(), 1e-3, torch.zeros(1, dtype=torch.int32),
                                    torch.zeros(2, dtype=torch.int32), torch.zeros(8))


def test_tables_against_a_brute_force_map(built):
    from leod_amd import ops
    C = ops.GRAD_STATS_CHUNK
    lengths = seg_lengths(C)
    offs, n = aligned_offsets(lengths)
    seg, chunk = ops.grad_stats_tables(offs, lengths)
    assert seg.dtype == torch.int64 and chunk.dtype == torch.int32
    seg, chunk = seg.numpy(), chunk.numpy()
    owner = np.full(n, -1, dtype=np.int64)                    # brute force: the segment every float of the buffer belongs to (-1: padding)
    for s, (o, k) in enumerate(zip(offs, lengths)):
        assert (owner[o:o + k] == -1).all()
        owner[o:o + k] = s
    assert seg.shape == (len(lengths), 3) and (seg[:, 0] == offs).all() and (seg[:, 1] == lengths).all()
    assert chunk.shape == (sum(-(-k // C) for k in lengths), 2)
    covered = np.zeros(n, dtype=np.int64)
    for c, (s, k) in enumerate(chunk):
        o, ln, first = seg[s]
        assert first <= c < first + -(-ln // C) and k == c - first            # consecutive chunks of a segment, in order
        lo, hi = o + k * C, min(o + ln, o + (k + 1) * C)
        assert lo < hi and lo % 4 == 0
        assert (owner[lo:hi] == s).all(), f'chunk {c} straddles segments'
        covered[lo:hi] += 1
    assert (covered[owner >= 0] == 1).all() and (covered[owner < 0] == 0).all()   # every element once, the padding never


def test_skip_nonfinite_defaults_to_off():
    from leod_amd.optim import FlatAdamW
    from leod_amd.train import fit
    assert inspect.signature(FlatAdamW.__init__).parameters['skip_nonfinite'].default is False
    assert inspect.signature(fit).parameters['grad_flow_every'].default is None
    from leod_amd.config import full_config
    assert 'skip_nonfinite_steps' not in full_config('gen1', 'small').training     # opt-in key: the shipped defaults do not carry it
    lin = torch.nn.Linear(3, 2)
    opt = FlatAdamW(lin)
    assert opt.skip_nonfinite is False and opt.skipped_steps == 0 and opt.applied_steps == 0
    assert set(opt.state_dict()['state']) == {'step', 'exp_avg', 'exp_avg_sq'}
