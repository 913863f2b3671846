"""The one-launch MLP of stage 1 (csrc/k_mlp.hip, ``ops.mlp_fwd_fused`` / ``ops.mlp_bwd_dgrad_fused``) on the operands of tests/mlp_exact.py,
compared for EQUALITY with the float64 model in both 16-bit modes and both widths.  The argument for exactness is the docstring of
tests/mlp_exact.py; tests/test_mlp_exact_cpu.py checks it on the values without a GPU.

* row counts: 16384 (no ragged tile), 16391, 32855, 70001, 98451 -- the owner of the ragged tile has run 0, 1, 2, 3 full tiles and leaves
  the forward pipeline by its first, second (f0 = f1), third (f0 = f2) exit and by the first exit of the second lap; the backward pipeline
  by its first, second, first and second exit, the last two on the second lap (test_mlp_exact_cpu.py::test_row_counts_reach_every_exit);
* forward: z and u16 equal to the model, stats within ``close_fp32`` of the float64 LayerNorm; ``want_saved`` True and False give the same
  z bits.  Masked problem: z within ``MASK_TOL`` in mode bf16 (the bf16 hidden operand does not round gelu(u <= -8) to zero by itself),
  equal in mode 16f;
* backward, on the caller's exact statistics (not the forward kernel's): du equal (masked elements within ``MASK_TOL`` in mode bf16),
  dgamma / dbeta equal on every element below the reduction bound of 2^24 and within ``close_fp32`` elsewhere (only the sign column of a
  masked problem), dy equal at K = 64 in plain problems and within ``close_fp32`` otherwise (1 / 48 is not a power of two; the sign column
  of a masked problem is not covered by the CPU evaluation's magnitude bound); ``want_du`` True and False give the same dy bits;
* ``b1 = None`` (masked problem), ``b2 = None``, ``gamma = None`` at M = 16391.

Output buffers: ``ops`` allocates them with ``torch.empty`` and the caching allocator can hand back the block that still holds an earlier
call's correct result, so a row the kernel never writes could pass.  Before every call a NaN-filled tensor of each output's size and type
is created and freed on the same stream (``mlp_exact.poison``).  That is best effort: nothing guarantees the allocator reuses that block.
``pytest -m gpu``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_kernels_gpu as tk  # noqa: E402
from test_bf16_gpu import bf16_ops  # noqa: E402,F401  (fixture: runs a test in modes 'bf16' and '16f')
import mlp_exact as me  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
CASES = me.cases()
_ids = lambda c: '-'.join(str(v) for v in c)  # noqa: E731


def _dev(t):
    return None if t is None else t.to(tk.DEV)


def _equal(got, want, what, M):
    """equality, and where it fails: which element -- row, column, the row's tile and the first tile of the wave that owns it"""
    got = got.detach().cpu()
    if torch.equal(got, want):
        return
    bad = (got.float() != want.float()).nonzero()           # a NaN (a row never written) differs from everything
    _, _, stride = me.geometry(M)
    row, col = (int(v) for v in bad[0]) if bad.shape[1] == 2 else (None, int(bad[0][0]))
    where = f'column {col}' if row is None else f'row {row} (tile {row // 16}, wave starting at tile {(row // 16) % stride}), column {col}'
    idx = tuple(bad[0].tolist())
    raise AssertionError(f'{what}: {len(bad)} of {got.numel()} elements differ, first at {where}: got {float(got[idx])}, want {float(want[idx])}; '
                         f'rows affected {sorted(set(bad[:, 0].tolist()))[:8] if row is not None else "-"}')


def _within(got, want, tol, what):
    err = float((got.detach().cpu().double() - want.double()).abs().max())
    assert err <= tol, f'{what}: off by {err}, allowed {tol}'          # a NaN fails the comparison


def _operands(p, drop, backward):
    names = ('dz', 'y', 'stats', 'ln_w', 'ln_b', 'W1', 'b1', 'W2', 'gamma_bwd') if backward else ('y', 'ln_w', 'ln_b', 'W1', 'b1', 'W2', 'b2', 'gamma')
    return [None if drop is not None and n.startswith(drop) else _dev(p[n]) for n in names]


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_mlp_fwd_fused_exact(bf16_ops, case):
    ops = bf16_ops
    K, H, M, kind, drop = case
    p = me.problem(K, H, M, kind)
    r = me.reference(p, drop)
    args = _operands(p, drop, False)
    outs = (((M, K), F32), ((M, H), F16), ((M, 2), F32))
    me.poison(tk.DEV, *outs)
    out = ops.mlp_fwd_fused(*args, want_saved=True)
    assert out is not None, 'the fused kernel covers (48, 192) and (64, 256) from M = 16384 on in the 16-bit modes'
    z, u16, st = out
    assert u16.dtype is F16 and tuple(u16.shape) == (M, H) and tuple(st.shape) == (M, 2) and tuple(z.shape) == (M, K)
    _equal(u16, r['u'], 'fp16 pre-activation', M)
    if kind == 'masked' and ops.get_precision() == 'bf16':
        _within(z, r['z'], me.MASK_TOL, 'z (masked problem, bf16 hidden operand)')
    else:
        _equal(z, r['z'], 'z', M)
    me.close_fp32(st, r['stats'], what='LayerNorm statistics written by the forward')
    zc = z.cpu()
    del z, u16, st
    me.poison(tk.DEV, outs[0])
    z2, u2, st2 = ops.mlp_fwd_fused(*args, want_saved=False)
    assert u2 is None and st2 is None
    _equal(z2, zc, 'z without the saved tensors against z with them', M)


@pytest.mark.parametrize('case', [c for c in CASES if c[4] != 'b2'], ids=_ids)
def test_mlp_bwd_dgrad_fused_exact(bf16_ops, case):
    ops = bf16_ops
    K, H, M, kind, drop = case
    p = me.problem(K, H, M, kind)
    r = me.reference(p, drop)
    args = _operands(p, drop, True)
    dg, db = _dev(p['dgamma0'].clone()), _dev(p['dbeta0'].clone())
    outs = (((M, K), F32), ((M, H), BF16))
    me.poison(tk.DEV, *outs)
    out = ops.mlp_bwd_dgrad_fused(*args, dg, db, want_du=True)
    assert out is not None
    dy, du = out
    assert du.dtype is BF16 and tuple(du.shape) == (M, H) and tuple(dy.shape) == (M, K)
    if kind == 'masked' and ops.get_precision() == 'bf16':
        duc, neg = du.cpu(), r['neg']
        _equal(torch.where(neg, torch.zeros((), dtype=BF16), duc), r['du'], 'du where the pre-activation is positive', M)
        _within(duc.float()[neg], r['du'].float()[neg], me.MASK_TOL, 'du where the pre-activation is negative')
    else:
        _equal(du, r['du'], 'du', M)
    for name, got in (('dgamma', dg), ('dbeta', db)):
        ok = r[name + '_exact']
        _equal(got.cpu().double()[ok], r[name][ok], f'{name} (elements below the reduction bound)', M)
        if not bool(ok.all()):
            me.close_fp32(got.cpu()[~ok], r[name][~ok], what=f'{name} (sign column of the masked problem)')
    if r['dy_exact']:
        _equal(dy, r['dy'], 'dy', M)
    else:
        me.close_fp32(dy, r['dy64'], what='dy')
    dyc = dy.cpu()
    del dy, du
    dg2, db2 = _dev(p['dgamma0'].clone()), _dev(p['dbeta0'].clone())
    me.poison(tk.DEV, outs[0])
    dy2, du2 = ops.mlp_bwd_dgrad_fused(*args, dg2, db2, want_du=False)
    assert du2 is None
    _equal(dy2, dyc, 'dy without du against dy with it', M)
    for name, got in (('dgamma', dg2), ('dbeta', db2)):
        ok = r[name + '_exact']
        _equal(got.cpu().double()[ok], r[name][ok], f'{name} without du', M)
