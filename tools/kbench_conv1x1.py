#!/usr/bin/env python
"""The 1x1 / stride-1 convolutions of the PAFPN and the head stems at the flagship step's shapes (32 labelled frames): the single-call route
(leod_conv_nhwc_fwd / _dgrad) against the grouped short-problem kernel (leod_conv1x1_group_fwd / _dgrad), both directions, then the grouped
forms (conv1 | conv2 of a CSP layer on one map, the three head stems) against the sum of their single calls.  Every figure is device time per
call: `reps` calls captured in one graph and replayed (tools/kbench_gemm.py, KBENCH_GRAPH), over a rotation of four operand sets.
usage: python tools/kbench_conv1x1.py [reps=40]   (GPU box; LEOD_PRECISION=16f | bf16)"""
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
from leod_amd import ops  # noqa: E402

DEV = 'cuda'
# (rows, Cin, N): the ten distinct 1x1 shapes of the step
SHAPES = [(2560, 384, 192), (2560, 192, 192), (2560, 384, 384), (2560, 384, 96),
          (10240, 384, 96), (10240, 96, 96), (10240, 192, 192), (10240, 192, 96),
          (40960, 192, 48), (40960, 48, 48), (40960, 96, 96)]
PAIRS = [(2560, 384, 192), (10240, 384, 96), (10240, 192, 96), (40960, 192, 48)]
STEMS = [(40960, 96, 96), (10240, 192, 96), (2560, 384, 96)]
ROT = 4


def timeit(fn, reps):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for r in range(reps):
            fn(r % ROT)
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (3 * reps)


class Member:
    def __init__(self, M, cin, n, x=None):
        rows = (M // 80, 8, 10)
        self.shape = (M, cin, n)
        self.x = x if x is not None else [torch.randn(*rows, cin, device=DEV) for _ in range(ROT)]
        self.dy = [torch.randn(*rows, n, device=DEV) for _ in range(ROT)]
        self.w = torch.randn(n, cin, 1, 1, device=DEV) * .1
        self.stats = torch.zeros(ops.stat_replicas(M), 2, n, dtype=torch.float64, device=DEV)
        self.dx = torch.empty(*rows, cin, device=DEV)


def fwd_single(ms):
    return lambda r: [ops.conv_nhwc_fwd(m.x[r], m.w, None, colstats=m.stats) for m in ms]


def fwd_group(ms):
    return lambda r: ops.conv1x1_group_fwd([m.x[r] for m in ms], [m.w for m in ms], [m.stats for m in ms])


def dgrad_single(ms, acc):
    return lambda r: [ops.conv_nhwc_dgrad(m.dy[r], m.w, m.x[0].shape, out=m.dx, accumulate=acc) for m in ms]


def dgrad_group(ms, acc):
    return lambda r: ops.conv1x1_group_dgrad([m.dy[r] for m in ms], [m.w for m in ms], [m.dx for m in ms], [acc] * len(ms))


def line(name, ms, reps):
    gf = ops.conv1x1_group_route(0, [m.shape for m in ms])
    gd = ops.conv1x1_group_route(1, [(m.shape[0], m.shape[2], m.shape[1]) for m in ms])
    out = []
    for single, group, code in ((fwd_single(ms), fwd_group(ms), gf), (dgrad_single(ms, False), dgrad_group(ms, False), gd)):
        out += [timeit(single, reps), timeit(group, reps) if code > 0 else float('nan')]      # nan: the route refuses the group
    fr = [ops.conv_route(0, m.shape[0] // 80, 8, 10, m.shape[1], m.shape[2], 1, 1, 0, ops.CF_COLSTATS) for m in ms]
    dr = [ops.conv_route(1, m.shape[0] // 80, 8, 10, m.shape[1], m.shape[2], 1, 1, 0, 0) for m in ms]
    mb = sum(4 * (M * (c + n) + c * n) for M, c, n in (m.shape for m in ms)) / 1e6
    print(f'{name:<34} {mb:6.1f} | {out[0]:7.1f} {out[1]:7.1f} | {out[2]:7.1f} {out[3]:7.1f} | '
          f'{"+".join(map(str, fr))} -> {gf}; {"+".join(map(str, dr))} -> {gd}')


def main():
    ops.set_precision(os.environ.get('LEOD_PRECISION', '16f'))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    print(f'precision mode {ops.get_precision()}; us per call, graph replay of {reps} calls x 3')
    print(f'{"rows x Cin -> N":<34} {"MB":>6} | {"fwd 1":>7} {"fwd grp":>7} | {"dgrad 1":>7} {"dg grp":>7} | routes (single -> group; forward; dgrad)')
    for M, c, n in SHAPES:
        line(f'{M} x {c} -> {n}', [Member(M, c, n)], reps)
    for M, c, n in PAIRS:
        a = Member(M, c, n)
        line(f'pair on one map {M} x {c} -> {n}', [a, Member(M, c, n, a.x)], reps)
    line('three stems 96|192|384 -> 96', [Member(*s) for s in STEMS], reps)
    m = Member(2560, 384, 192)
    print(f'dgrad with accumulate, 2560 x 384 -> 192: single {timeit(dgrad_single([m], True), reps):.1f}  group {timeit(dgrad_group([m], True), reps):.1f}')


if __name__ == '__main__':
    main()
