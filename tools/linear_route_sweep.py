"""Runs every launching row of the Linear route table (tests/test_linear_routes_cpu.py) once through the ops wrapper that reaches its entry
point and prints one JSON line per row: the row, the route ``ops.linear_route`` reports (null on a library without the query), the SHA-256
of every output written without atomics and the float64 sum of every atomically accumulated one.  Two builds that route every row to the
same kernel print the same hashes; under ``rocprofv3 --kernel-trace`` the kernel names tell which kernel that was.

    python tools/linear_route_sweep.py [--no-hash] > sweep.jsonl

Rows the wrappers cannot express are left out: padded strides, LayerNorm without a statistics buffer, and an fp16-hidden dgrad whose
output format is not the build's (ops.BF16_GRADS)."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from leod_amd import ops                                                                    # noqa: E402
from test_linear_routes_cpu import ROWS, LN, STATS, KSCALE, AUX, TOUT, DX2, COLSUM, ACCUMULATE, DRES   # noqa: E402

DEV = torch.device('cuda', 0)


def expressible(e, a16, out16, flags, lda, ldo):
    if lda is not None or ldo is not None or (e == 0 and bool(flags & LN) != bool(flags & STATS)):
        return False
    return e != 8 or bool(out16) == bool(ops.BF16_GRADS)


def run(e, M, N, K, a16, out16, flags, nsplit, gen):
    """-> ({name: tensor written without atomics}, {name: tensor accumulated with atomics})"""
    def r(*shape, dtype=torch.float32, scale=1.0):
        return (torch.randn(*shape, device=DEV, generator=gen) * scale).to(dtype)
    W, rows16 = r(N, K, scale=K ** -0.5), ops.act16_dtype()
    opt = lambda bit, *shape: r(*shape) if flags & bit else None                            # noqa: E731
    if e in (0, 2, 3):
        ln_w, ln_b = (r(K) + 1.0, r(K)) if flags & LN else (None, None)
        out, act, stats = ops.ln_linear_fwd(r(M, K), ln_w, ln_b, W, r(N), want_act=e == 2 or bool(flags & AUX), want_stats=e == 2, out_bf16=e == 3)
        return dict(out=out, act=act, stats=stats), {}
    if e in (1, 4, 5):
        a = r(M, K, dtype={1: torch.float32, 4: rows16, 5: torch.float16}[e])
        out, t = ops.linear_lsres_fwd(a, W, r(N), r(N), r(M, N), want_t=bool(flags & TOUT), a_gelu=False if e == 4 else None)
        return dict(out=out, t=t), {}
    dy = r(M, N, dtype=torch.bfloat16 if a16 else torch.float32)
    if e == 7:
        dw, db = torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)
        stats = torch.stack((r(M), r(M).abs() + 0.5), 1).contiguous()
        return dict(dx=ops.linear_dgrad_ln_bwd(dy, W, r(M, K), stats, r(K) + 1.0, opt(DRES, M, K), dw, db)), dict(dgamma=dw, dbeta=db)
    if e == 8:
        return dict(du=ops.linear_dgrad(dy, W, kscale=opt(KSCALE, N), aux_u=r(M, K, dtype=torch.float16))), {}
    colsum = torch.zeros(K, device=DEV) if flags & COLSUM else None
    dx = ops.linear_dgrad(dy, W, kscale=opt(KSCALE, N), aux_u=opt(AUX, M, K), colsum=colsum, out=opt(ACCUMULATE, M, K), accumulate=bool(flags & ACCUMULATE),
                          split=nsplit, dres=opt(DRES, M, K), out_bf16=bool(out16))
    dx, dx2 = dx if nsplit else (dx, None)
    return dict(dx=dx, dx2=dx2), dict(colsum=colsum)


def main():
    hashing = '--no-hash' not in sys.argv
    for i, (e, mode, M, N, K, a16, out16, flags, nsplit, lda, ldo, want) in enumerate(ROWS):
        if want <= 0 or not expressible(e, a16, out16, flags, lda, ldo):
            continue
        ops.set_precision(mode)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(i)
        plain, atomic = run(e, M, N, K, a16, out16, flags, nsplit, gen)
        torch.cuda.synchronize()
        rec = dict(row=[e, mode, M, N, K, a16, out16, flags, nsplit], expect=want,
                   route=ops.linear_route(e, M, N, K, a16=a16, out16=out16, flags=flags, nsplit=nsplit) if hasattr(ops, 'linear_route') else None)
        if hashing:
            rec['sha256'] = {k: hashlib.sha256(v.contiguous().view(torch.uint8).cpu().numpy()).hexdigest() for k, v in plain.items() if v is not None}
            rec['sums'] = {k: float(v.double().sum()) for k, v in atomic.items() if v is not None}
        print(json.dumps(rec), flush=True)
        del plain, atomic


if __name__ == '__main__':
    main()
