"""The host-side planning of a conv + BatchNorm + SiLU group (leod_amd/functions.py): the rounds of its input gradients, the carving of
its statistics block and the replica rule (leod_amd/ops.py).  Nothing here touches a device."""
import itertools

import pytest
import torch

from leod_amd import functions as Fn
from leod_amd import ops


def key(name, shape=(2, 5, 7, 48), stride=1):
    """what the planner sees of a member's input: (data_ptr, shape, stride); equal keys = the same map"""
    return (hash(name), shape, stride)


def check_rounds(keys, need_dx):
    """The properties every plan must have; -> (plan, rounds)"""
    plan, rounds = Fn._dgrad_rounds(keys, need_dx)
    assert len(plan) == len(keys)
    placed = list(itertools.chain.from_iterable(rounds))
    assert sorted(placed) == [i for i, need in enumerate(need_dx) if need], 'every member that wants dx exactly once, the others never'
    assert all(r for r in rounds), 'no empty round'
    for i, need in enumerate(need_dx):
        assert (plan[i] is not None) == need
    for rnd, idx in enumerate(rounds):
        assert idx == sorted(idx), 'member order inside a round'
        assert all(plan[i][1] == rnd for i in idx)
        outs = [plan[i][0] for i in idx]
        assert len(set(outs)) == len(outs), f'round {rnd} holds two problems with one output'
    # one buffer per distinct map among the members that want dx, and only for those
    wanted = {k for k, need in zip(keys, need_dx) if need}
    bufs = {}
    for k, p in zip(keys, plan):
        if p is not None:
            assert bufs.setdefault(k, p[0]) == p[0], 'the readers of one map share one buffer'
    assert len(set(bufs.values())) == len(bufs) == len(wanted), 'different maps, different buffers'
    # the first reader of a map writes (round 0: accumulate=False), the j-th adds in round j: the writer comes before every adder
    for k in wanted:
        readers = [i for i, (kk, need) in enumerate(zip(keys, need_dx)) if kk == k and need]
        assert [plan[i][1] for i in readers] == list(range(len(readers)))
    return plan, rounds


@pytest.mark.parametrize('sharers', [1, 2, 3, 5])
def test_rounds_k_sharers_of_one_map(sharers):
    """k readers of one map among unshared members and members that want no input gradient: k rounds"""
    keys = [key('a'), key('shared'), key('b'), key('nodx')] + [key('shared')] * (sharers - 1) + [key('c'), key('shared')]
    need = [True, True, True, False] + [True] * (sharers - 1) + [True, False]          # the last reader of the map wants no dx: not a sharer
    plan, rounds = check_rounds(keys, need)
    assert len(rounds) == sharers
    assert rounds[0] == [0, 1, 2] + [4 + sharers - 1]
    assert rounds[1:] == [[4 + j] for j in range(sharers - 1)]
    assert plan[3] is None and plan[-1] is None


def test_rounds_same_address_other_geometry_is_another_map():
    """a map is (address, shape, stride): a stride-2 reader of the same tensor, or a view of another shape at its address, shares nothing"""
    keys = [key('x'), key('x', stride=2), key('x', shape=(1, 10, 7, 48)), key('x')]
    plan, rounds = check_rounds(keys, [True] * 4)
    assert rounds == [[0, 1, 2], [3]]
    assert plan[3][0] == plan[0][0]


def test_rounds_nobody_wants_dx():
    assert Fn._dgrad_rounds([key('a'), key('a')], [False, False]) == ([None, None], [])


def test_rounds_head_pattern():
    """cls_k and reg_k of three head levels read x_k (members in the order of YOLOXHead: the cls convs of the levels, then the reg convs):
    exactly two rounds of three, in member order -- writers cls_0..2, then adders reg_0..2 into the same three buffers"""
    levels = [key(f'x{k}', shape=(3, 8 >> k, 12 >> k, 96)) for k in range(3)]
    plan, rounds = check_rounds(levels + levels, [True] * 6)
    assert rounds == [[0, 1, 2], [3, 4, 5]]
    assert plan == [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]


def test_rounds_csp_pattern():
    """conv1 / conv2 of a CSP layer read the same map: writer, then adder"""
    plan, rounds = check_rounds([key('x'), key('x')], [True, True])
    assert plan == [(0, 0), (0, 1)] and rounds == [[0], [1]]


# ---- the statistics block -------------------------------------------------------------------------------------------------------
MAPS = [(3, 32 * 40), (3, 16 * 20), (1, 5 * 7), (8, 120 * 152)]           # (images, pixels per image)
CHANNELS = [96, 96, 48, 128]


@pytest.mark.parametrize('replicas', [ops.stat_replicas, ops.bn_bwd_replicas])
@pytest.mark.parametrize('sync', [False, True])
def test_stat_block_slices(replicas, sync):
    block, views = Fn._stat_block(MAPS, CHANNELS, replicas, torch.device('cpu'), sync=sync)
    assert block.dtype is torch.float64 and block.dim() == 1 and not block.any()
    off = 0
    for (images, pixels), N, v in zip(MAPS, CHANNELS, views):
        R = replicas((32 if sync else images) * pixels)
        assert tuple(v.shape) == (R, 2, N) and v.is_contiguous()
        assert v.data_ptr() == block.data_ptr() + 8 * off, 'slices back to back, in member order: disjoint'
        off += v.numel()
    assert off == block.numel(), 'the slices cover the block'
    for k, v in enumerate(views):                                            # and they are views of it, not copies
        v.fill_(k + 1)
    assert torch.equal(block, torch.cat([torch.full((v.numel(),), k + 1.0, dtype=torch.float64) for k, v in enumerate(views)]))


@pytest.mark.parametrize('replicas', [ops.stat_replicas, ops.bn_bwd_replicas])
def test_stat_block_sync_layout_ignores_batch(replicas):
    """SyncBatchNorm: the block is all-reduced, so its layout must be the same whatever number of images this rank holds"""
    ref = [tuple(v.shape) for v in Fn._stat_block(MAPS, CHANNELS, replicas, torch.device('cpu'), sync=True)[1]]
    for images in (1, 2, 7, 32, 100):
        maps = [(images, pixels) for _, pixels in MAPS]
        block, views = Fn._stat_block(maps, CHANNELS, replicas, torch.device('cpu'), sync=True)
        assert [tuple(v.shape) for v in views] == ref
    # without it the layout follows the rows (the last map: 1 image -> 8 images crosses several thresholds)
    one = Fn._stat_block([(1, 120 * 152)], [128], replicas, torch.device('cpu'), sync=False)[1][0]
    many = Fn._stat_block([(8, 120 * 152)], [128], replicas, torch.device('cpu'), sync=False)[1][0]
    assert one.shape[0] < many.shape[0]


# ---- the replica rule ---------------------------------------------------------------------------------------------------------------
def old_stat_replicas(rows):
    r = 1
    while r < 32 and r * 1280 < rows:
        r *= 2
    return r


def old_bn_bwd_replicas(rows):
    r = 1
    while r < 16 and r * 2560 < rows:
        r *= 2
    return r


@pytest.mark.parametrize('rows', [1, 1279, 1280, 1281, 2560, 2561, 40960, 10 ** 7])
def test_replica_rule_equals_the_two_old_functions(rows):
    assert ops.STAT_REPLICAS == 32
    assert ops.stat_replicas(rows) == old_stat_replicas(rows)
    assert ops.bn_bwd_replicas(rows) == old_bn_bwd_replicas(rows)
