"""Runs every launching row of the attention and ConvLSTM-sequence route tables (tests/test_attn_lstm_routes_cpu.py) once through the ops
wrappers that reach the entry points and prints one JSON line per call: the arguments, the routes ``ops.partition_attn_route`` /
``ops.convlstm_seq_route`` report (null on a library without the queries) and the SHA-256 of every tensor the call wrote.  Neither family
uses float atomics, so two builds that launch the same kernels with the same geometry print the same hashes, every one of them.

    python tools/attn_lstm_route_sweep.py [f32|bf16|16f ...] > sweep.jsonl

It runs unchanged on a build without the queries: copy this file and tests/test_attn_lstm_routes_cpu.py (the tables; they need nothing
of the build at import) into that tree.

Rows the wrappers cannot express are left out: they hand the backward a bf16 dqkv exactly when qkv is 16-bit, so the flag sets that run are
forward 0 / 1 / 1|2 and backward 0 / 1|4 / 1|2|4.  Rows that differ only in flags the route does not look at (the dqkv flag of a forward,
the projection flag of a backward) run once."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from leod_amd import ops                                                                    # noqa: E402
import test_attn_lstm_routes_cpu as T                                                        # noqa: E402

DEV = torch.device('cuda', 0)


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy()).hexdigest()


def route(name, *args):
    return getattr(ops, name)(*args) if hasattr(ops, name) else None


def attn(mode, seed):
    rows = [r for r in list(T.attn_rows()) + list(T.ATTN_EXTRA) if r[0] == mode and r[-1] > 0]
    launching = {(r[1],) + r[2:9] for r in rows}
    for geom in sorted({r[2:8] for r in rows}):
        B, H, W, C, heads, part = geom
        for t16 in (False, True):
            for o16 in ((False, True) if t16 else (False,)):
                ff, fb = (1 if t16 else 0) | (2 if o16 else 0), (1 | 4 if t16 else 0) | (2 if o16 else 0)
                if (T.FWD,) + geom + (ff,) not in launching or (T.BWD,) + geom + (fb,) not in launching:
                    continue
                for window in (True, False):
                    gen = torch.Generator(device=DEV)
                    gen.manual_seed(seed)
                    qkv = torch.randn(B, H, W, 3 * C, device=DEV, generator=gen)
                    dout = torch.randn(B, H, W, C, device=DEV, generator=gen)
                    if t16:
                        qkv = qkv.to(ops.act16_dtype())
                    if o16:
                        dout = dout.to(torch.bfloat16)
                    out, lse = ops.partition_attn_fwd(qkv, heads, part, window, want_lse=True, out_bf16=o16)
                    dqkv = ops.partition_attn_bwd(qkv, dout, lse, heads, part, window)
                    torch.cuda.synchronize()
                    yield dict(op='attn', mode=mode, geom=[B, H, W, C, heads, list(part)], window=window, flags=[ff, fb],
                               route=[route('partition_attn_route', e, B, H, W, C, heads, part, f) for e, f in ((0, ff), (1, fb))],
                               sha256=dict(out=sha(out), lse=sha(lse), dqkv=sha(dqkv)))


def lstm(mode, seed, steps=3, M=35):
    rows = [r for r in T.lstm_rows() if r[0] == mode and r[-1] > 0]
    for C in sorted({r[2] for r in rows}):
        seq_mode = ops.convlstm_seq_mode(C)
        for g16 in ((False, True) if ops.convlstm_gates16_ok(C) else (False,)):
            for state in (True, False):
                gen = torch.Generator(device=DEV)
                gen.manual_seed(seed)
                r = lambda *shape, scale=1.0: torch.randn(*shape, device=DEV, generator=gen) * scale      # noqa: E731
                W, b = r(4 * C, 2 * C, scale=0.15 if C <= 192 else 0.06), r(4 * C, scale=0.1)
                xin = r(steps, M, C) if seq_mode == 1 else r(steps, M, 4 * C)
                hbuf, cbuf = torch.zeros(steps + 1, M, C, device=DEV), torch.zeros(steps + 1, M, C, device=DEV)
                if state:
                    hbuf[0], cbuf[0] = r(M, C, scale=0.5), r(M, C, scale=0.5)
                gates = ops.convlstm_gates16_buffer(steps, M, C, DEV).zero_() if g16 else torch.zeros(steps, M, 4, C, device=DEV)
                wpack = ops.convlstm_seq_pack(W, C) if seq_mode == 3 else None
                ops.convlstm_seq_fwd(xin, seq_mode >= 2, hbuf, cbuf, W, b, gates, zero_state=not state, wpack=wpack)
                dgates = torch.zeros(steps, M, 4 * C, dtype=torch.bfloat16 if g16 else torch.float32, device=DEV)
                dh0, dc0 = torch.zeros(M, C, device=DEV), torch.zeros(M, C, device=DEV)
                ok = ops.convlstm_seq_bwd(r(steps, M, C), r(M, C), gates, cbuf, W, dgates, dh0, dc0, zero_state=not state, wpack=wpack)
                torch.cuda.synchronize()
                fl = (1 if seq_mode >= 2 else 0) | (2 if g16 else 0) | (4 if wpack is not None else 0)
                yield dict(op='lstm', mode=mode, C=C, gates16=g16, state=state, bwd_ran=bool(ok),
                           route=[route('convlstm_seq_route', 0, C, fl), route('convlstm_seq_route', 1, C, fl & ~1)],
                           sha256=dict(h=sha(hbuf), c=sha(cbuf), gates=sha(gates), dgates=sha(dgates), dh0=sha(dh0), dc0=sha(dc0)))


def main():
    for mode in [a for a in sys.argv[1:] if a in T.MODES] or T.MODES:
        ops.set_precision(mode)
        for i, rec in enumerate(attn(mode, 1)):
            print(json.dumps(rec), flush=True)
        for rec in lstm(mode, 2):
            print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
