"""K12 (fused add + LayerNorm, patch-merging LayerNorm, position tokens, csrc/layernorm.hip) against float64 on the paths
production takes.

The reference is torch on the CPU with autograd — F.layer_norm (F.unfold in front of it for patch merging) — on the inputs as
their dtype holds them, in float64 (the reference) and in float32 (its error sets the bar, f64_bars.f32_bar; no bar may exceed
1e-5); upstream gradients are created in the dtype the kernel receives.  f32-stored tensors take the bar, 16-bit stored ones may
add one rounding of the type; bit-equal claims (the f32 sum, the 16-bit copy of a gradient, the branch copy of y) use
torch.equal.  Compared: y, s, d a, d b, d gamma, d beta, the branch Linear's bias gradient.  Every comparison prints ``err … bar …``.

Routes, asserted by the C-ABI calls a ``lib.hook`` sees: few rows take the one-kernel "direct" backward
(mbv_add_layernorm_bwd_direct = 1, at most 64 blocks); more rows leave per-block partial rows that k_ln_param_reduce adds up at
once (plain parameters; arena parameters with ``wgrad_group`` off) or that join the grouped column-sum launch at the end of the
backward pass (arena parameters, default switches: mbv_colsum_accum_group with one entry per parameter — three with a branch
bias).  Arena gradients are pre-filled and the backward runs twice.  Measured: DESIGN.md §2."""
import functools

import pytest
import torch

from tests import norm_ref as R
from tests.f64_bars import LO, NAME
from tests.norm_ref import F32, F64

pytestmark = pytest.mark.gpu
MOD = 'k12-paths'
FORMS = ('plain', 'arena', 'arena-now')         # stored gradients | accumulated, deferred column sums | accumulated, reduced at once

# every ITERS class of iters_for, one float4 per row, a partly filled last 64-lane step, a forward block with 1 or 3 of its 4
# rows; 512 rows = 64 blocks: the last count on the direct route
FEW_ROWS = [(1, 4), (3, 8), (5, 252), (37, 256), (5, 260), (3, 512), (37, 516), (5, 1024), (3, 1028), (37, 2048), (512, 192)]
MANY_ROWS = [
    (513, 192),        # 65 blocks: a second reducer chunk holding one row
    (1032, 48),        # three reducer chunks
    (8200, 192),       # block cap 1024; waves take a second row, ragged
    (4100, 768),       # ITERS 4, per-row LDS adds, cap 512
    (2056, 1536),      # ITERS 8, cap 256
]
STORAGE_SHAPES = [(37, 256), (513, 192), (600, 768)]
BRANCH_SHAPES = [(400, 256), (1032, 192), (600, 768)]          # direct | partial rows | per-row LDS adds
FANOUT_SHAPES = [(37, 256), (513, 192)]
MERGE_SHAPES = [(2, 8, 12, 48), (1, 10, 6, 96), (1, 6, 4, 192), (1, 4, 6, 320), (1, 4, 4, 768), (2, 48, 44, 48)]


def _sid(shape):
    return 'x'.join(map(str, shape))


@functools.lru_cache(maxsize=4)
def _case(shape, a_dt=F32, b_dt=F32, gy_dts=(F32,), gs_dt=F32):
    """Inputs and the float64 / float32 references; upstream gradients of y in ``gy_dts`` (none, one or two), of s in ``gs_dt``."""
    k = R.ln_inputs(1200 + sum(shape), shape, a_dt, b_dt)
    k.gys = tuple(g.to(dt) for g, dt in zip((k.g1, k.g2), gy_dts))
    k.gs = None if gs_dt is None else k.g3.to(gs_dt)
    return k, R.ln_reference(k.a, k.b, k.w, k.bias, k.gys, k.gs)


class _Params(torch.nn.Module):
    def __init__(self, k, branch):
        super().__init__()
        self.weight, self.bias = torch.nn.Parameter(k.w.clone()), torch.nn.Parameter(k.bias.clone())
        self.branch = torch.nn.Parameter(torch.zeros(k.c)) if branch else None


def _params(k, device, form, branch=False):
    """The affine parameters (and the branch Linear's bias) as the form wants them, and what their gradients were pre-filled with."""
    from mask_bev_amd.arena import ParameterArena
    m = _Params(k, branch).to(device)
    g = torch.Generator().manual_seed(12)
    pre = {n: torch.randn(k.c, generator=g) for n in ('dw', 'dbias', 'dbranch')}
    arena = []
    if form != 'plain':
        arena = list(m.parameters())
    elif branch:
        arena = [m.branch]                                         # a branch bias gradient is always an arena accumulation
    if arena:
        holder = torch.nn.Module()
        holder.p = torch.nn.ParameterList(arena)
        ParameterArena([('ln', holder)], shadow_dtype=None)
    with torch.no_grad():
        for n, p in (('dw', m.weight), ('dbias', m.bias), ('dbranch', m.branch)):
            if p is not None and getattr(p, '_mbv_arena', False):
                p.grad.copy_(pre[n])
            else:
                pre[n] = torch.zeros(k.c)
    return m, pre


def _twice(pre, ref, name):
    """What two accumulating backward passes leave: float64, and the float32 reference's way there."""
    return (pre[name] + ref[F32][name]) + ref[F32][name], pre[name].double() + 2 * ref[F64][name]


def _run(device, capsys, tag, k, ref, form, bad, out_dt=F32, branch=False):
    """Two forward + backward passes through ops.add_layernorm(return_sum=True) in ``form``; compares every tensor and returns
    the C-ABI calls seen."""
    from mask_bev_amd import _lib, ops, switches
    lib = _lib.load()
    m, pre = _params(k, device, form, branch)
    calls = []
    lib.hook = lambda name, fn, args: (calls.append((name, args)), fn(*args))[1]
    try:
        with switches.override(wgrad_group=(form != 'arena-now')):
            for _ in range(2):
                a = k.a.clone().to(device).requires_grad_()
                b = None if k.b is None else k.b.clone().to(device).requires_grad_()
                y, s = ops.add_layernorm(a, b, m.weight, m.bias, R.EPS, out_dt, return_sum=True,
                                         branch_bias=m.branch if branch else None)
                outs = ([y] if k.gys else []) + ([s] if k.gs is not None else [])
                gos = [g.to(device) for g in k.gys[:1]] + ([k.gs.to(device)] if k.gs is not None else [])
                torch.autograd.backward(outs, gos)
            ops.flush_deferred_grads()
    finally:
        lib.hook = None
    assert y.dtype == out_dt and s.dtype == F32
    if b is not None:
        assert torch.equal(s, a.detach().float() + b.detach().float())          # the f32 sum of the two inputs, bit for bit
    for name, got in (('y', y.detach()), ('s', s.detach()), ('da', a.grad), ('db', None if b is None else b.grad)):
        if got is not None:
            R.compare(capsys, MOD, tag, name, got, ref[F32][name], ref[F64][name], bad)
    for name, p in (('dw', m.weight), ('dbias', m.bias), ('dbranch', m.branch)):
        if p is not None and ref[F64][name] is not None:
            want32, want64 = _twice(pre, ref, name)
            R.compare(capsys, MOD, tag, f'{name} ({form}, two passes)', p.grad, want32, want64, bad)
    return lib, calls


def _assert_route(lib, calls, k, form, branch, direct):
    """The route by what was called: the direct kernel for few rows; partial rows reduced at once, or — arena, default switches —
    handed to the grouped column-sum launch of each backward pass, one entry per parameter."""
    nblk, np_ = lib.mbv_add_layernorm_bwd_blocks(k.rows, k.c), (3 if branch else 2)
    assert lib.mbv_add_layernorm_bwd_direct(k.rows, k.c) == (1 if direct else 0) and (nblk <= 64) == direct
    bwd = [args for name, args in calls if name == 'mbv_add_layernorm_bwd3']
    group = [args for name, args in calls if name == 'mbv_colsum_accum_group']
    assert len(bwd) == 2
    for args in bwd:
        assert bool(args[18].value) == branch                                     # np == 3: the column sums of dx as well
        assert args[17] == (0 if form == 'plain' else 1)                        # accumulate
        assert args[20] == (1 if form == 'arena' and not direct else 0)         # defer_reduce
    if form == 'arena' and not direct:
        assert len(group) == 2                                                  # one grouped launch per backward pass
        for args in group:
            n = args[6]
            assert n == np_ and list(args[2])[:n] == [nblk] * n and list(args[3])[:n] == [k.c] * n
            assert list(args[4])[:n] == [np_ * k.c] * n
    else:
        assert not group


@pytest.mark.parametrize('form', FORMS[:2])
@pytest.mark.parametrize('shape', FEW_ROWS, ids=_sid)
def test_few_rows_direct_backward_against_float64(device, capsys, shape, form):
    k, ref = _case(shape)
    bad = []
    lib, calls = _run(device, capsys, f'{_sid(shape)} {form}', k, ref, form, bad)
    _assert_route(lib, calls, k, form, False, direct=True)
    assert not bad, bad


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', MANY_ROWS, ids=_sid)
def test_many_rows_partial_rows_against_float64(device, capsys, shape, form):
    k, ref = _case(shape)
    bad = []
    lib, calls = _run(device, capsys, f'{_sid(shape)} {form}', k, ref, form, bad)
    _assert_route(lib, calls, k, form, False, direct=False)
    assert not bad, bad


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', BRANCH_SHAPES, ids=_sid)
def test_branch_bias_gradient_against_float64(device, capsys, shape, form):
    """branch_bias: the deferred bias gradient of the Linear that produced b — prefill + the row sums of dx, twice."""
    k, ref = _case(shape)
    bad = []
    lib, calls = _run(device, capsys, f'{_sid(shape)} branch {form}', k, ref, form, bad, branch=True)
    _assert_route(lib, calls, k, form, True, direct=shape[0] <= 512)
    assert not bad, bad


@pytest.mark.parametrize('shape', BRANCH_SHAPES, ids=_sid)
def test_branch_bias_with_only_the_residual_path(device, capsys, shape):
    """A loss on s alone: no LayerNorm backward runs, the branch bias receives colsum(gs) and a, b receive gs itself."""
    k, ref = _case(shape, gy_dts=())
    bad = []
    lib, calls = _run(device, capsys, f'{_sid(shape)} branch, residual path only', k, ref, 'arena', bad, branch=True)
    names = [name for name, _ in calls]
    assert names.count('mbv_add_layernorm_bwd3') == 0 and names.count('mbv_colsum_accum') == 2
    assert not bad, bad


@pytest.mark.parametrize('lo', LO, ids=[NAME[d] for d in LO])
@pytest.mark.parametrize('combo', ['f32+lo_to_lo', 'lo+lo_to_f32', 'f32_to_lo'])
@pytest.mark.parametrize('shape', STORAGE_SHAPES, ids=_sid)
def test_storage_types_against_float64(device, capsys, shape, combo, lo):
    """The storage types production uses, with the sum returned and its gradient in f32 and in the 16-bit type."""
    a_dt, b_dt, out_dt = {'f32+lo_to_lo': (F32, lo, lo), 'lo+lo_to_f32': (lo, lo, F32), 'f32_to_lo': (F32, None, lo)}[combo]
    from mask_bev_amd import ops
    bad = []
    for gs_dt in (F32, lo):
        k, ref = _case(shape, a_dt, b_dt, (out_dt,), gs_dt)
        tag = f'{_sid(shape)} {combo} {NAME[lo]} gs {NAME[gs_dt]}'
        a = k.a.clone().to(device).requires_grad_()
        b = None if k.b is None else k.b.clone().to(device).requires_grad_()
        w, bias = (t.clone().to(device).requires_grad_() for t in (k.w, k.bias))
        y, s = ops.add_layernorm(a, b, w, bias, R.EPS, out_dt, return_sum=True)
        assert y.dtype == out_dt and s.dtype == F32
        if b is None:
            assert s is a                                                           # a lone f32 input IS the sum
        else:
            assert torch.equal(s, a.detach().float() + b.detach().float())
        torch.autograd.backward([y, s], [k.gys[0].to(device), k.gs.to(device)])
        for name, got in (('y', y.detach()), ('da', a.grad), ('dw', w.grad), ('dbias', bias.grad)):
            R.compare(capsys, MOD, tag, name, got, ref[F32][name], ref[F64][name], bad)
        if combo == 'f32+lo_to_lo':
            assert torch.equal(b.grad, a.grad.to(lo))                               # the 16-bit copy: the f32 gradient rounded
        elif combo == 'lo+lo_to_f32':
            assert a.grad.dtype == lo and torch.equal(b.grad, a.grad)
    assert not bad, bad


@pytest.mark.parametrize('dt2', [F32] + list(LO), ids=lambda d: NAME[d])
@pytest.mark.parametrize('shape', FANOUT_SHAPES, ids=_sid)
def test_fanout_against_float64(device, capsys, shape, dt2):
    """``fanout``: y leaves twice (the second copy in ``branch_dtype``), the two gradients are added on load; either may be missing."""
    from mask_bev_amd import ops
    bad = []
    for which in ('both', 'first', 'second'):
        gy_dts = {'both': (F32, dt2), 'first': (F32,), 'second': (dt2,)}[which]
        k = R.ln_inputs(1200 + sum(shape), shape)
        gys = tuple(g.to(dt) for g, dt in zip((k.g1, k.g2), gy_dts))
        ref = R.ln_reference(k.a, k.b, k.w, k.bias, gys)
        a, b, w, bias = (t.clone().to(device).requires_grad_() for t in (k.a, k.b, k.w, k.bias))
        y, y2 = ops.add_layernorm(a, b, w, bias, R.EPS, F32, fanout=True, branch_dtype=None if dt2 == F32 else dt2)
        assert y.dtype == F32 and y2.dtype == dt2 and torch.equal(y2, y.to(dt2))
        assert (y.data_ptr() == y2.data_ptr()) == (dt2 == F32)
        outs = {'both': [y, y2], 'first': [y], 'second': [y2]}[which]
        torch.autograd.backward(outs, [g.to(device) for g in gys])
        tag = f'{_sid(shape)} fanout f32 + {NAME[dt2]}, {which}'
        for name, got in (('y', y.detach()), ('da', a.grad), ('db', b.grad), ('dw', w.grad), ('dbias', bias.grad)):
            R.compare(capsys, MOD, tag, name, got, ref[F32][name], ref[F64][name], bad)
    assert not bad, bad


@pytest.mark.parametrize('shape', [(3, 5, 7, 96), (2, 16, 24, 192)], ids=_sid)
def test_position_tokens_against_float64(device, capsys, shape):
    """ops.pos_tokens + the repeating ``b`` of the forward: the (1, C, rows, cols) embedding added inside the LayerNorm launch,
    its gradient the batch sum of dx transposed back — 105 rows (direct) and 768 rows (partial rows)."""
    from mask_bev_amd import _lib, ops
    bsz, h, w, c = shape
    k = R.ln_inputs(1200 + sum(shape), shape, b_dt=None)
    ape = torch.randn(1, c, w, h, generator=torch.Generator().manual_seed(5))       # (w, h) on purpose, as the model has it
    ref = R.ln_reference(k.a, ape, k.w, k.bias, (k.g1,), k.g3, b_map=R.pos_map(h, w, c))
    assert _lib.load().mbv_add_layernorm_bwd_direct(k.rows, c) == (1 if k.rows <= 512 else 0)
    x, p, gam, bet = (t.clone().to(device).requires_grad_() for t in (k.a, ape, k.w, k.bias))
    pos = ops.pos_tokens(p, bsz, h, w)
    assert pos.shape == x.shape and pos.stride(0) == 0
    y, s = ops.add_layernorm(x, pos, gam, bet, R.EPS, F32, return_sum=True)
    torch.autograd.backward([y, s], [k.g1.to(device), k.g3.to(device)])
    bad = []
    for name, got in (('y', y.detach()), ('s', s.detach()), ('da', x.grad), ('db', p.grad), ('dw', gam.grad), ('dbias', bet.grad)):
        R.compare(capsys, MOD, f'{_sid(shape)} position tokens', name.replace('db', 'd_ape') if name == 'db' else name, got,
                  ref[F32][name], ref[F64][name], bad)
    assert not bad, bad


@pytest.mark.parametrize('out_dt', [F32] + list(LO), ids=lambda d: NAME[d])
@pytest.mark.parametrize('shape', MERGE_SHAPES, ids=_sid)
def test_patch_merging_against_float64(device, capsys, shape, out_dt):
    """ops.merge_layernorm: LayerNorm_{4C} of the 2 x 2 neighbourhoods gathered from the channels-last map — 4C = 192 … 3072 (ITERS
    12), 1056 rows (partial rows); y and dy in f32 / bf16 / fp16; dx scattered back, finite everywhere."""
    from mask_bev_amd import ops
    bsz, h, w, c = shape
    g = torch.Generator().manual_seed(1200 + sum(shape))
    x = torch.randn(shape, generator=g) * 2 + 0.5
    wt, bias = torch.rand(4 * c, generator=g) + 0.5, torch.randn(4 * c, generator=g)
    gy = torch.randn(bsz, h // 2, w // 2, 4 * c, generator=g).to(out_dt)
    ref = R.merge_reference(x, wt, bias, gy)
    xd, wd, bd = (t.clone().to(device).requires_grad_() for t in (x, wt, bias))
    y = ops.merge_layernorm(xd, wd, bd, R.EPS, out_dt)
    assert y.dtype == out_dt and tuple(y.shape) == tuple(gy.shape)
    y.backward(gy.to(device))
    bad = []
    for name, got in (('y', y.detach()), ('dx', xd.grad), ('dw', wd.grad), ('dbias', bd.grad)):
        R.compare(capsys, MOD, f'{_sid(shape)} merge {NAME[out_dt]}', name, got, ref[F32][name], ref[F64][name], bad)
    assert not bad, bad


@pytest.mark.parametrize('c', [192, 768])
def test_values_against_float64(device, capsys, c):
    """Rows at 50 ± 1, a row of zeros and a row of constant 0.5 (exact sums: y must be beta), rows scaled by 2^-20 and by 2^10, all in
    one tensor."""
    from mask_bev_amd import ops
    k = R.ln_inputs(1200 + c, (64, c), b_dt=None)
    a0 = R.ln_value_rows(77 + c, c)
    ref = R.ln_reference(a0, None, k.w, k.bias, (k.g1,))
    a, w, bias = (t.clone().to(device).requires_grad_() for t in (a0, k.w, k.bias))
    y = ops.add_layernorm(a, None, w, bias, R.EPS, F32)
    y.backward(k.g1.to(device))
    bad = []
    for name, got in (('y', y.detach()), ('da', a.grad), ('dw', w.grad), ('dbias', bias.grad)):
        R.compare(capsys, MOD, f'64x{c} values', name, got, ref[F32][name], ref[F64][name], bad)
    for what, rows in R.VALUE_ROWS.items():                                            # each kind of row at its own scale
        R.compare(capsys, MOD, f'64x{c} values', f'y of the {what} rows', y.detach()[rows], ref[F32]['y'][rows], ref[F64]['y'][rows], bad)
    for row in (R.VALUE_ROWS['zeros'], R.VALUE_ROWS['half']):
        assert torch.equal(ref[F64]['y'][row], k.bias.double())                        # exact sums: the reference is beta itself
    assert not bad, bad


@pytest.mark.parametrize('rows', [40, 1032])
def test_absmax_record_of_dx(device, capsys, rows):
    """mbv_add_layernorm_bwd3 with a zeroed 64-word record: afterwards the largest word is exactly the bits of max|dx| — 5 blocks,
    and 129 blocks whose index wraps over the 64 words; dy = 0 without ds leaves the record zero.  ds arrives in bf16 here (the
    16-bit load of the residual gradient), and dx is compared with float64 as well."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    c = 192
    k, ref = _case((rows, c), gs_dt=torch.bfloat16)
    assert lib.mbv_add_layernorm_bwd_blocks(rows, c) == (rows + 7) // 8
    s64 = k.a.double() + k.b.double()
    mean = s64.mean(-1)
    rstd = ((s64 - mean[:, None]).square().mean(-1) + R.EPS).rsqrt()
    s, mean, rstd, w, gy, gs = (t.to(device) for t in (s64.float(), mean.float(), rstd.float(), k.w, k.gys[0], k.gs))
    bad = []
    for zero in (False, True):
        dy = torch.zeros_like(gy) if zero else gy
        dx = torch.full((rows, c), float('nan'), device=device)
        dgamma, dbeta = torch.empty(c, device=device), torch.empty(c, device=device)
        ws = torch.empty(lib.mbv_add_layernorm_bwd_blocks(rows, c) * 2 * c, device=device)
        rec = torch.zeros(64, dtype=torch.int32, device=device)
        ops.check(lib.mbv_add_layernorm_bwd3(ops._ptr(dy), 0, None, 0, None if zero else ops._ptr(gs), 0 if zero else 1, ops._ptr(s),
                                             ops._ptr(mean), ops._ptr(rstd), ops._ptr(w), rows, c, ops._ptr(dx), None, 0,
                                             ops._ptr(dgamma), ops._ptr(dbeta), 0, None, ops._ptr(ws), 0, ops._ptr(rec), ops._stream()),
                  'mbv_add_layernorm_bwd3')
        if zero:
            assert not rec.any() and not dx.any() and not dgamma.any() and not dbeta.any()
        else:
            assert int(rec.max()) == int(dx.abs().max().view(torch.int32)) and int(rec.min()) >= 0
            assert int((rec != 0).sum()) == min(64, (rows + 7) // 8)                  # every block recorded into its word
            for name, got in (('da', dx), ('dw', dgamma), ('dbias', dbeta)):
                R.compare(capsys, MOD, f'{rows}x{c} C ABI, ds bf16', name, got, ref[F32][name], ref[F64][name], bad)
    assert not bad, bad
