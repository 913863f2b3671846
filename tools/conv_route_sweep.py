"""Runs every launching row of the dense-convolution route table (tests/test_conv_routes_cpu.py) once through the ops wrapper that reaches its
entry point and prints one JSON line per row: the row, the route ``ops.conv_route`` reports (null on a library without the query), the
SHA-256 of every output written without atomics and the float64 sum of every atomically accumulated one.  Two builds that route every row
to the same kernel print the same hashes; under ``rocprofv3 --kernel-trace`` the kernel names tell which kernel that was.

    python tools/conv_route_sweep.py [--no-hash] > sweep.jsonl

It runs unchanged on a build without the query: copy this file and tests/test_conv_routes_cpu.py (the table; it needs nothing of the build
at import) into that tree.

Rows the wrappers cannot express are left out: a padding other than (ks - 1) // 2, a forward / dgrad of ks > 1 with no pack offered or of a strided
1x1 with one, and a 3x3 weight gradient with no workspace (the wrappers offer pack and workspace wherever the library reads them)."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from leod_amd import ops                                                                    # noqa: E402
from test_conv_routes_cpu import ROWS, BIAS, COLSTATS, BN, PACK, WS, DBIAS, ACCUMULATE, U8, ALIGN4   # noqa: E402

DEV = torch.device('cuda', 0)


def expressible(e, ks, stride, pad, flags):
    if e < 3 and pad != (ks - 1) // 2:
        return False
    if e in (0, 1):                                 # a pack is offered to ks > 1, never to ks == 1 (1x1 / stride 1 has no route that reads one)
        return (ks > 1) == bool(flags & PACK) or (ks == 1 and stride == 1)
    return e != 2 or bool(flags & WS) or not (ks == 3 and pad == 1)


def run(e, B, H, W, Cin, N, ks, stride, pad, flags, padded, gen):
    """-> ({name: tensor written without atomics}, {name: tensor accumulated with atomics})"""
    def r(*shape, scale=1.0):
        return torch.randn(*shape, device=DEV, generator=gen) * scale
    if e >= 3:
        Hp, Wp = padded if padded is not None else (H, W)
        x = torch.randint(0, 10, (B, Cin, H, W), device=DEV, generator=gen).to(torch.uint8) if flags & U8 else r(B, Cin, H, W)
        if not flags & ALIGN4:                                                              # the same values at an address that is no multiple of 4
            buf = torch.empty(x.numel() * x.element_size() + 16, dtype=torch.uint8, device=DEV)
            off = (-buf.data_ptr()) % 16 + 1
            x = buf[off:off + x.numel() * x.element_size()].view(x.dtype).view(x.shape).copy_(x)
        if e == 3:
            return dict(y=ops.stem_conv_fwd(x, r(N, Cin, ks, ks, scale=0.05), (Hp, Wp), stride, pad)), {}
        dw = torch.zeros(N, Cin, ks, ks, device=DEV)
        ops.stem_conv_wgrad(r(B, (Hp + 2 * pad - ks) // stride + 1, (Wp + 2 * pad - ks) // stride + 1, N), x, dw, (Hp, Wp), stride, pad)
        return {}, dict(dw=dw)
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    w = r(N, Cin, ks, ks, scale=(Cin * ks * ks) ** -0.5)
    if e == 0:
        cs = torch.zeros(ops.stat_replicas(B * Ho * Wo), 2, N, dtype=torch.float64, device=DEV) if flags & COLSTATS else None
        bn = (r(N) + 1.0, r(N), r(N), r(N).abs() + 0.5) if flags & BN else None
        return dict(y=ops.conv_nhwc_fwd(r(B, H, W, Cin), w, r(N) if flags & BIAS else None, stride=stride, colstats=cs, bn=bn)), dict(colstats=cs)
    if e == 1:
        out = r(B, H, W, Cin) if flags & ACCUMULATE else None
        return dict(dx=ops.conv_nhwc_dgrad(r(B, Ho, Wo, N), w, (B, H, W, Cin), stride=stride, out=out, accumulate=bool(flags & ACCUMULATE))), {}
    dw, db = torch.zeros_like(w), (torch.zeros(N, device=DEV) if flags & DBIAS else None)
    ops.conv_nhwc_wgrad(r(B, Ho, Wo, N), r(B, H, W, Cin), dw, db, stride=stride)
    return {}, dict(dw=dw, dbias=db)           # (the direct 3x3 kernel reduces without atomics: its sums are then equal to the last bit)


def main():
    hashing = '--no-hash' not in sys.argv
    for i, (e, mode, B, H, W, Cin, N, ks, stride, pad, flags, padded, want) in enumerate(ROWS):
        if want <= 0 or not expressible(e, ks, stride, pad, flags):
            continue
        ops.set_precision(mode)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(i)
        plain, atomic = run(e, B, H, W, Cin, N, ks, stride, pad, flags, padded, gen)
        torch.cuda.synchronize()
        rec = dict(row=[e, mode, B, H, W, Cin, N, ks, stride, pad, flags, padded], expect=want,
                   route=ops.conv_route(e, B, H, W, Cin, N, ks, stride, pad, flags, padded) if hasattr(ops, 'conv_route') else None)
        if hashing:
            rec['sha256'] = {k: hashlib.sha256(v.contiguous().view(torch.uint8).cpu().numpy()).hexdigest() for k, v in plain.items() if v is not None}
            rec['sums'] = {k: float(v.double().sum()) for k, v in atomic.items() if v is not None}
        print(json.dumps(rec), flush=True)
        del plain, atomic


if __name__ == '__main__':
    main()
