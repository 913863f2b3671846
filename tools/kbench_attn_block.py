#!/usr/bin/env python
"""The one-launch attention sub-block (csrc/k_attn_block.hip) against the three launches it replaces (ln_linear_fwd -> partition_attn_fwd ->
linear_lsres_fwd) at the stage-1 and stage-2 shapes of the RVT-S step: window and grid partitions, tensors saved (training) and not saved
(inference).  The two variants alternate in one process; us per call are medians over the repetitions.  Also prints the largest
fused-versus-composed difference of qkv, O (ulps of the 16-bit format) and y (ulps of fp32).
usage: kbench_attn_block.py [16f|bf16] [repetitions]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
from leod_amd import ops
mode = sys.argv[1] if len(sys.argv) > 1 else '16f'
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
ops.set_precision(mode)
dev = 'cuda'
PART = (8, 10)
g = torch.Generator(device=dev).manual_seed(0)
r = lambda *s, sc=1.0: sc * torch.randn(*s, generator=g, device=dev)


def composed(x, lw, lb, Wq, bq, Wp, bp, ga, heads, window, saved):
    geom = (*x.shape, heads, PART)
    q16 = ops.partition_attn_16bit_ok(*geom)
    qkv, _, st = ops.ln_linear_fwd(x, lw, lb, Wq, bq, want_stats=saved or q16, out_bf16=q16)
    o, lse = ops.partition_attn_fwd(qkv, heads, PART, window, want_lse=saved, out_bf16=q16 and ops.attn_block_o16_ok(*geom))
    y, _ = ops.linear_lsres_fwd(o, Wp, bp, ga, x, want_t=False, a_gelu=False)
    return y, qkv, st, o, lse


def fused(x, lw, lb, Wq, bq, Wp, bp, ga, heads, window, saved):
    return ops.attn_block_fwd(x, lw, lb, Wq, bq, Wp, bp, ga, heads, PART, window, want_saved=saved)


def time_us(fn, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def ulps(a, b):
    """largest difference in units of the last place of the tensors' own format (sign-magnitude bit patterns -> a monotonic integer scale)
    over the elements of ordinary size, |b| >= max|b| / 64: next to zero a difference of one ulp of the tensor's scale spans thousands of
    the element's own ulps and says nothing"""
    it = torch.int16 if a.element_size() == 2 else torch.int32
    ia, ib = a.contiguous().view(it).long(), b.contiguous().view(it).long()
    top = (1 << (8 * a.element_size() - 1)) - 1
    ia, ib = torch.where(ia < 0, -(ia & top), ia), torch.where(ib < 0, -(ib & top), ib)
    big = b.float().abs() >= b.float().abs().max() / 64
    return int((ia - ib).abs()[big].max())


med = lambda v: sorted(v)[len(v) // 2]
print(f'precision mode {mode}, {reps} alternating repetitions of 10 calls; us per call (median)')
for stage, (B, H, W, C, heads) in ((1, (168, 64, 80, 48, 2)), (2, (168, 32, 40, 96, 4))):
    assert ops.attn_block_fwd_route(B, H, W, C, heads, PART) > 0, 'the shape must take the fused route'
    x = r(B, H, W, C)
    args = (x, 1 + 0.1 * r(C), 0.1 * r(C), r(3 * C, C, sc=0.2), r(3 * C, sc=0.1), r(C, C, sc=0.2), r(C, sc=0.1), 0.5 + 0.1 * r(C))
    M = B * H * W
    for window in (True, False):
        for saved in (True, False):
            f = lambda: fused(*args, heads, window, saved)
            c = lambda: composed(*args, heads, window, saved)
            for _ in range(3):
                f(); c()
            torch.cuda.synchronize()
            tf, tc = [], []
            for _ in range(reps):
                tf.append(time_us(f)); tc.append(time_us(c))
            nbytes = 8 * M * C + (M * (8 * C + 8 + 4 * heads) if saved else 0)       # x in, y out (+ 16-bit qkv, O, stats, lse)
            a, b = med(tf), med(tc)
            print(f'stage {stage} (M {M}, C {C}) {"window" if window else "grid  "} {"saved    " if saved else "not saved"}: fused {a:7.1f} us '
                  f'({nbytes / a / 1e3:5.0f} GB/s)  three launches {b:7.1f} us  ratio {a / b:.3f}', flush=True)
        yf, qf, sf, of, lf = fused(*args, heads, window, True)
        yc, qc, sc_, oc, lc = composed(*args, heads, window, True)
        print(f'  fused vs three launches, {"window" if window else "grid"}: qkv {ulps(qf, qc)} ulp, O {ulps(of, oc)} ulp (16-bit), y {ulps(yf, yc)} ulp (fp32), '
              f'max |dy| {float((yf - yc).abs().max()):.3e}, max |dstats| {float((sf - sc_).abs().max()):.3e}, max |dlse| {float((lf - lc).abs().max()):.3e}', flush=True)
