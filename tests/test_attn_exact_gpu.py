"""Every route of the partition attention core (csrc/attn_route.hpp: attn_route / launch_attn in csrc/k_attn.hip) on the tie-pattern operands
of tests/attn_exact.py, in the three precision modes, window and grid addressing: the forward is EXACT (``torch.equal`` against the float64
CPU reference, fp32 O and 16-bit O rows alike), lse is compared at the fp32 bound, and dq, dk, dv against the per-element bounds that
attn_exact derives from the reference (``tolerance``: no free constant).

Rows: the per-route lists of the tolerance tests (test_kernels_gpu.ATTN_ROUTE_CASES_F32 in mode f32, test_bf16_gpu.ATTN_ROUTE_CASES_16 in
modes bf16 and 16f: one image of 2 x 2 partitions, two heads, a full and a padded partition per tile count, d = 12 / 20 / 24 / 32), plus
geometry rows (``GEOM_SHAPES_*`` x ``VARIANTS``) at the smallest partition of each family: two images (the image offset), one head and three heads (the odd head
offset), and one partition per image (H = ph, W = pw).  A row is ((ph, pw), d, 16-bit tensors, (forward code, backward code), heads, B,
partitions per image).  Every test first asserts that the router still sends the row there; tests/test_attn_exact_cpu.py asserts the same
without a GPU, and that every (entry, code) pair that launches in the tables of tests/test_attn_lstm_routes_cpu.py has a row here.

Per row and addressing: (1) fp32 O equal, lse close; (2) 16-bit rows: O written as 16-bit rows equal, lse bit-identical; (3) backward within
the bounds, run twice with identical bits (the pass has no atomics), and 16-bit rows: bit-identical from bf16 dO (the same values, hence the
same packed operands).  ``test_exp_of_zero_is_one`` observes exp(0) == 1 and 1 / 1 == 1 on the device through ties of ONE key in a full
partition, where O == v: if a forward comparison fails while it passes, the tie arithmetic holds and the defect is in the kernel's indexing
or masking.
``pytest -m gpu``; ``-s`` shows the largest backward error of every case as a fraction of its bound.

What the equality buys, measured once on an MI355X with ONE padded key admitted to the softmax of attn_fwd_lds16_kernel (``key < P + 1``):
all 52 cases of the 16-bit-tile family on a padded partition failed here, every O element of them wrong; under the 3e-2 bound of
test_attn_every_route_16bit the same build passed the six rows of mode bf16 with 121, 156 and 225 tokens."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_exact as ae  # noqa: E402
import linear_exact as le  # noqa: E402
import test_bf16_gpu as tb  # noqa: E402
import test_kernels_gpu as tk  # noqa: E402

DEV = 'cuda'
MODES = ('f32', 'bf16', '16f')
QKV16, O16, DQKV16 = 1, 2, 4

# (heads, B, partitions per image): what each geometry row is there for
VARIANTS = ((2, 2, (2, 2)), (1, 1, (2, 2)), (3, 1, (2, 2)), (2, 1, (1, 1)), (3, 2, (1, 2)))
GEOM_SHAPES_F32 = [((3, 5), 12, False, (10116, 10116)), ((5, 7), 20, False, (10332, 10332)), ((3, 5), 24, False, (20124, 20124)),
                   ((4, 8), 32, False, (20232, 20232))]
GEOM_SHAPES_16 = GEOM_SHAPES_F32 + [((3, 5), 24, True, (30124, 30124)), ((5, 6), 32, True, (30232, 30232))]


def _rows(base, shapes):
    return [tuple(r) + (2, 1, (2, 2)) for r in base] + [s + v for s in shapes for v in VARIANTS]


ROWS = {'f32': _rows(tk.ATTN_ROUTE_CASES_F32, GEOM_SHAPES_F32), '16': _rows(tb.ATTN_ROUTE_CASES_16, GEOM_SHAPES_16)}


def klass(mode):
    return 'f32' if mode == 'f32' else '16'


def cases():
    """(mode, index in the row list, row), the modes of one shape side by side: the cached reference of a shape is computed once"""
    out = [(m, i, r) for m in MODES for i, r in enumerate(ROWS[klass(m)])]
    return sorted(out, key=lambda c: (c[2][0], c[2][1], c[2][4:], MODES.index(c[0]), c[1]))


def routes_of(ops, row, flags):
    (ph, pw), d, _, _, heads, B, (nH, nW) = row
    return tuple(ops.partition_attn_route(e, B, nH * ph, nW * pw, heads * d, heads, (ph, pw), flags[e]) for e in (0, 1))


def flag_sets(t16):
    """(forward flags, backward flags) of the calls a row makes"""
    return ((QKV16, QKV16 | DQKV16), (QKV16 | O16, QKV16 | O16 | DQKV16)) if t16 else ((0, 0),)


def _id(case):
    mode, i, (part, d, t16, want, heads, B, grid) = case
    return f'{mode}-{want[0]}-{want[1]}@{part[0]}x{part[1]}-h{heads}-b{B}-{grid[0]}x{grid[1]}#{i}'


@pytest.fixture
def ops_in():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from leod_amd import ops
    prev = ops.get_precision()

    def enter(mode):
        ops.set_precision(mode)
        return ops
    yield enter
    ops.set_precision(prev)


def bounded(p):
    b = ae.bounds(p)
    assert all(ok for ok, _ in b.values()), {k: v for k, v in b.items() if not v[0]}


def same(got, ref, p, what):
    """got [B, H, W, heads e] on the device equals ref (the same shape, fp32), element for element"""
    got, ref = got.float().cpu(), ref.float()
    if torch.equal(got, ref):
        return
    g, r = ae.from_image(got, p['rows'], p['heads']), ae.from_image(ref, p['rows'], p['heads'])
    bad = (g != r).nonzero()
    pi, h, t, c = bad[0].tolist()
    raise AssertionError(f'{what}: {len(bad)} of {r.numel()} elements differ, first at partition {pi}, head {h}, token {t} (image row {int(p["rows"][pi, t])}), '
                         f'channel {c}: got {g[pi, h, t, c].item()!r}, exact {r[pi, h, t, c].item()!r}; the query\'s tie has '
                         f'{int(p["tie"][pi, h, t])} keys.  (If test_exp_of_zero_is_one passes in this mode, the tie arithmetic holds on the device.)')


def backward_within_bounds(dqkv, p, mode, fam, what):
    g = ae.from_image(dqkv.float().cpu(), p['rows'], p['heads']).double()
    d, tol, worst = p['d'], ae.tolerance(p, mode, fam), {}
    for n, t in enumerate(('dq', 'dk', 'dv')):
        worst[t] = ae.worst(g[..., n * d:(n + 1) * d], p['ref'][t], tol[t], p)
    print(f'ATTN_EXACT {mode} family {fam} {what}: ' + ' '.join(f'{t} {worst[t][0]:.4f}' for t in worst))
    for t, (ratio, where) in worst.items():
        assert ratio <= 1.0, f'{what}, {t}: {ratio:.3f} of its bound at {where}'


@pytest.mark.parametrize('case', cases(), ids=_id)
def test_attn_exact(ops_in, case):
    mode, idx, row = case
    ops = ops_in(mode)
    part, d, t16, want, heads, B, grid = row
    for fl in flag_sets(t16):
        assert routes_of(ops, row, fl) == tuple(want), 'the shape no longer reaches the routes this row is here for'
    fam, a16 = ae.family_of(want[0]), ops.act16_dtype()
    assert ae.family_of(want[1]) == fam
    for window in (True, False):
        p = ae.problem(tuple(part), d, heads, B, window, 0, tuple(grid))
        bounded(p)
        tag = f'{"window" if window else "grid"}, routes {want}'
        q = (p['qkv'].to(a16) if t16 else p['qkv']).to(DEV)
        O, lse = ops.partition_attn_fwd(q, heads, part, window, want_lse=True)
        assert O.dtype is torch.float32
        same(O, p['O'], p, f'forward, {tag}')
        le.close_fp32(lse, p['lse'], what=f'lse against log(2^k), {tag}')
        if t16:
            o16, lse2 = ops.partition_attn_fwd(q, heads, part, window, want_lse=True, out_bf16=True)
            assert o16.dtype is a16
            same(o16, p['O'], p, f'forward with 16-bit O rows, {tag}')
            assert torch.equal(lse2, lse), f'lse differs between the fp32-O and the 16-bit-O forward, {tag}'
        dO = p['dO'].to(DEV)
        g1 = ops.partition_attn_bwd(q, dO, lse, heads, part, window)
        g2 = ops.partition_attn_bwd(q, dO, lse, heads, part, window)
        assert g1.dtype is (torch.bfloat16 if t16 else torch.float32)
        assert torch.equal(g1, g2), f'two runs of the backward differ, {tag}'
        backward_within_bounds(g1, p, mode, fam, f'backward, {tag}')
        if t16:
            do16 = p['dO'].to(torch.bfloat16)
            assert torch.equal(do16.float(), p['dO'])
            g3 = ops.partition_attn_bwd(q, do16.to(DEV), lse, heads, part, window)
            assert torch.equal(g3, g1), f'backward from bf16 dO differs from the one from fp32 dO, {tag}'


# a FULL partition of 16 tokens (no padded key exists, so no masking defect can reach this test), split until it holds two groups of one key.
# (d, 16-bit tensors): family 1, family 2, family 3
ONE_KEY_PART, ONE_KEY_SPLITS = (4, 4), 4
ONE_KEY_ROWS = {'f32': ((12, False), (24, False)), '16': ((12, False), (24, False), (24, True))}


@pytest.mark.parametrize('mode', MODES)
def test_exp_of_zero_is_one(ops_in, mode):
    """a tie of ONE key: e = exp(0), sum = e, P = e / sum and O = P v -- O == v and lse == 0 bit for bit say that the device takes exp(0) and
    1 / 1 as exactly 1, the two assumptions under the equality of every other forward comparison"""
    ops = ops_in(mode)
    part, heads = ONE_KEY_PART, 2
    for d, t16 in ONE_KEY_ROWS[klass(mode)]:
        fl = flag_sets(t16)[0]
        assert ae.family_of(ops.partition_attn_route(0, 1, 2 * part[0], 2 * part[1], heads * d, heads, part, fl[0])) == (3 if t16 else 1 if d == 12 else 2)
        p = ae.problem(part, d, heads, 1, True, 0, (2, 2), ONE_KEY_SPLITS)
        bounded(p)
        one = p['tie'] == 1                                                    # [partitions, heads, query]
        assert int(one.sum()) >= 2 * p['NP'] * heads
        key = (p['group'].unsqueeze(2) == p['target'].unsqueeze(3)).double().argmax(-1)
        v_of_key = torch.gather(p['v'], 2, key.unsqueeze(-1).expand(-1, -1, -1, d))
        q = (p['qkv'].to(ops.act16_dtype()) if t16 else p['qkv']).to(DEV)
        O, lse = ops.partition_attn_fwd(q, heads, part, True, want_lse=True)
        Op = ae.from_image(O.cpu(), p['rows'], heads)
        Lp = ae.from_image(lse.cpu(), p['rows'], 1).squeeze(1).permute(0, 2, 1)  # [partitions, heads, n]
        assert torch.equal(Op[one], v_of_key[one].float()), f'mode {mode}, d = {d}, 16-bit rows {t16}: O != v on a tie of one key: exp(0) or 1 / 1 is not 1'
        assert bool((Lp[one] == 0).all()), f'mode {mode}, d = {d}, 16-bit rows {t16}: lse != 0 on a tie of one key'
