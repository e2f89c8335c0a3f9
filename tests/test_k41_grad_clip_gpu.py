"""K41 (csrc/optim_flat.hip): gradient clipping by global norm inside the flat optimizers.

The checker is torch on the CPU: ``torch.nn.utils.clip_grad_norm_`` followed by ``torch.optim.AdamW`` / ``SGD`` or by
``tests/optim_ref.lamb_step``, run in float64 from the same f32 inputs.  Parameters and optimizer state are held to the project's
f32 bar — max(4e-6, 4 x the error of the same reference run in f32 on the CPU), measured against the reference and never against
the kernel (tests/f64_bars.py).  Norms and coefficients are held to a relative 2^-23: the device accumulates in f64 (error about
n * 2^-53) and rounds the stored f32 once (2^-24); the bar is twice that rounding.

The toy arena has three segments with tensors of 1, 5, 63, 64, 65, 4096, 4097, 3 * 4096 + 17, (300, 257) and 257 * 4096 + 4
elements: the head segment is 276 chunks, so the coefficient pass's 256-strided loop runs more than once.  Per-step gradients
differ in magnitude by factors of 10 (Adam's direction is nearly invariant to a constant rescaling, so a constant clip would not
show in the parameters).  Their global norm is about 0.3 * sqrt(1.15e6) * mult >= 32, and MAX_NORM = 16 (exact in f32) keeps the
reference's coefficient below 1 on every step, which the reference run itself asserts.

Initial values and learning rates are chosen so that a parameter moves by at least a percent of its own size per step: the
half-ulp rounding of p that every f32 implementation makes then stays below the bar relative to the accumulated update
p_k - p_0 (SGD's lr of 0.5 is for that; its clipped gradient elements are about 0.015)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import f64_bars as B
from tests import optim_ref as R
from tests.util_cfg import random_gt, random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
MOD = 'k41'
STEPS = 6
MAX_NORM = 16.0
MULT = (1.0, 10.0, 0.1, 100.0, 1.0, 10.0)
NORM_BAR = 2.0 ** -23
BIG = 257 * 4096 + 4
SEGMENTS = ('encoder', 'backbone', 'head')
HP = dict(encoder=dict(lr=2e-2, weight_decay=0.01), backbone=dict(lr=2e-2, weight_decay=0.01),
          head=dict(lr=5e-3, weight_decay=0.0))
SGD_HP = dict(lr=0.5, weight_decay=1e-3)
STATE = dict(adamw=('exp_avg', 'exp_avg_sq'), adam=('exp_avg', 'exp_avg_sq'), lamb=('exp_avg', 'exp_avg_sq'),
             sgd=('momentum_buffer',))
INF = float('inf')


def _initial():
    g = torch.Generator().manual_seed(41)
    rnd = lambda *s: torch.randn(*s, generator=g)
    return dict(encoder=[rnd(1) * 0.1, rnd(5) * 0.1, rnd(63) * 0.1, rnd(64) * 0.1, rnd(65) * 0.1],
                backbone=[rnd(4096) * 0.02, rnd(4097) * 0.02, rnd(3 * 4096 + 17) * 0.02],
                head=[rnd(300, 257) * 0.01, rnd(BIG) * 0.01])


_CACHE = {}


def _gradients():
    if 'grads' not in _CACHE:
        g = torch.Generator(device='cpu').manual_seed(6)
        _CACHE['grads'] = [{s: [torch.randn(t.shape, generator=g) * (0.3 * MULT[step]) for t in ts]
                            for s, ts in _initial().items()} for step in range(STEPS)]
    return _CACHE['grads']


class _Seg(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        for name, ts in _initial().items():
            setattr(self, name, _Seg(ts))

    def named(self):
        return [((s, i), p) for s in SEGMENTS for i, p in enumerate(getattr(self, s).ps)]


def _toy(device):
    from mask_bev_amd.arena import ParameterArena
    toy = _Toy().to(device)
    arena = ParameterArena([(s, getattr(toy, s)) for s in SEGMENTS], shadow_dtype=torch.bfloat16)
    assert arena.intact()
    a, b = arena.segments['head']
    assert (b - a + 4095) // 4096 > 256
    return toy, arena


def _make(kind, arena, **kw):
    from mask_bev_amd.arena import FlatAdam, FlatLamb, FlatSGD
    groups = [dict(segment=s, **HP[s]) for s in SEGMENTS]
    if kind == 'sgd':
        return FlatSGD(arena, **SGD_HP, **kw)
    if kind == 'lamb':
        return FlatLamb(arena, groups, **kw)
    return FlatAdam(arena, groups, decoupled=(kind == 'adamw'), **kw)


def _feed(toy, grads, scale=1.0):
    for (s, i), q in toy.named():
        q.grad.copy_((grads[s][i] * scale).to(q.device))


def _flat_of(arena, flat, q):
    o = next(o for p, o in arena.layout if p is q)
    return flat[o:o + q.numel()].view(q.shape)


def _state(kind, arena, opt):
    extra = [opt.trust_ratio.clone()] if kind == 'lamb' else []
    return [arena.param.clone(), arena.shadow.clone()] + [getattr(opt, n).clone() for n in STATE[kind]] + extra


def _reference(kind, dtype):
    """clip_grad_norm_(MAX_NORM) then the optimizer of ``kind`` over the toy on the CPU at ``dtype``; per step the total norm,
    the coefficient, the norm of every segment and {key: (p, state...)}.  Computed once per setting and never modified."""
    key = (kind, dtype)
    if key in _CACHE:
        return _CACHE[key]
    init, grads = _initial(), _gradients()
    keys = [(s, i) for s in SEGMENTS for i in range(len(init[s]))]
    params = {k: torch.nn.Parameter(init[k[0]][k[1]].to(dtype)) for k in keys}
    if kind == 'adamw':
        opt = torch.optim.AdamW([dict(params=[params[k] for k in keys if k[0] == s], **HP[s]) for s in SEGMENTS],
                                betas=(0.9, 0.999), eps=1e-8)
    elif kind == 'sgd':
        opt = torch.optim.SGD([params[k] for k in keys], momentum=0.99, nesterov=True, **SGD_HP)
    else:
        assert kind == 'lamb'
        lamb = {k: (torch.zeros_like(params[k].data), torch.zeros_like(params[k].data)) for k in keys}
    out = []
    for step in range(STEPS):
        for k in keys:
            params[k].grad = grads[step][k[0]][k[1]].to(dtype, copy=True)      # clip_grad_norm_ scales it in place
        seg = {s: float(torch.cat([params[k].grad.reshape(-1) for k in keys if k[0] == s]).norm()) for s in SEGMENTS}
        total = float(torch.nn.utils.clip_grad_norm_([params[k] for k in keys], MAX_NORM))
        coef = min(1.0, MAX_NORM / (total + 1e-6))
        snap = {}
        if kind == 'lamb':
            with torch.no_grad():
                for k in keys:
                    p, m, v, _, _ = R.lamb_step(params[k].detach(), params[k].grad, lamb[k][0], lamb[k][1], step + 1,
                                                HP[k[0]]['lr'], weight_decay=HP[k[0]]['weight_decay'])
                    params[k].data = p
                    lamb[k] = (m, v)
                    snap[k] = (p.clone(), m.clone(), v.clone())
        else:
            opt.step()
            for k in keys:
                snap[k] = (params[k].detach().clone(),) + tuple(opt.state[params[k]][n].clone() for n in STATE[kind])
        out.append(dict(total=total, coef=coef, seg=seg, t=snap))
    if dtype == torch.float64:
        assert all(r['coef'] < 1.0 for r in out), [r['coef'] for r in out]      # the clip bites on EVERY step
        assert max(r['total'] for r in out) > 100.0 * min(r['total'] for r in out)
    _CACHE[key] = out
    return out


def _cmp(capsys, bad, tag, got, ref32, ref64):
    B.check(capsys, MOD, tag, B.err(got, ref64), B.f32_bar(ref32, ref64), bad)


def _cmp_scalar(capsys, bad, tag, got, want):
    B.check(capsys, MOD, tag, abs(float(got) - want) / abs(want), NORM_BAR, bad)


def _follow_reference(device, capsys, kind, tag, feed=1.0, scale=None, grad_scale=1.0, overflow_at=None):
    """STEPS steps of the flat optimizer of ``kind`` with max_grad_norm = MAX_NORM against the reference: gradients are fed
    multiplied by ``feed`` (what a loss scale ``scale`` or a data-parallel sum leave in the arena).  ``overflow_at`` = a step
    in front of which one overflowed step is taken: it must change nothing but the scale, and the steps after it still match."""
    from mask_bev_amd.arena import LossScaler
    toy, arena = _toy(device)
    sc = None
    if scale is not None:
        sc = LossScaler(device)
        sc.scale.fill_(scale)
    opt = _make(kind, arena, max_grad_norm=MAX_NORM, scaler=sc)
    opt.grad_scale = grad_scale
    assert opt.max_grad_norm == MAX_NORM
    grads = _gradients()
    ref64, ref32 = _reference(kind, torch.float64), _reference(kind, torch.float32)
    p0 = {k: q.detach().clone().cpu() for k, q in toy.named()}
    bad = []
    for step in range(STEPS):
        if overflow_at == step:
            before = _state(kind, arena, opt)
            _feed(toy, grads[step], feed)
            dict(toy.named())[('backbone', 1)].grad.view(-1)[4096] = INF          # the lone element of the second chunk
            opt.step()
            torch.cuda.synchronize()
            keep = 2 + len(STATE[kind])               # (LAMB's trust ratios are meaningless after a skipped step, and unused)
            for a, b in zip(before[:keep], _state(kind, arena, opt)[:keep]):
                assert torch.equal(a, b)
            assert float(arena.grad.abs().max()) == 0.0
            assert sc.get_scale() == scale / 2 and int(sc.applied_steps.item()) == step
            assert float(opt.grad_norm) == INF
            feed = feed / 2
        _feed(toy, grads[step], feed)
        opt.step()
        assert float(arena.grad.abs().max()) == 0.0
        assert torch.equal(arena.shadow, arena.param.to(torch.bfloat16))
        r64, r32 = ref64[step], ref32[step]
        _cmp_scalar(capsys, bad, f'{tag} step {step + 1} grad_norm', opt.grad_norm, r64['total'])
        _cmp_scalar(capsys, bad, f'{tag} step {step + 1} clip_coef', opt.clip_coef, r64['coef'])
        norms = opt.grad_norms()
        assert list(norms) == list(SEGMENTS)
        for s in SEGMENTS:
            _cmp_scalar(capsys, bad, f'{tag} step {step + 1} grad_norms[{s}]', norms[s], r64['seg'][s])
        assert 0.0 < float(opt.clip_coef) < 1.0
        for k, q in toy.named():
            t = f'{tag} step {step + 1} {k[0]}[{k[1]}]'
            _cmp(capsys, bad, t + ' update', q.detach().cpu().double() - p0[k].double(), r32['t'][k][0] - p0[k],
                 r64['t'][k][0] - p0[k].double())
            for j, name in enumerate(STATE[kind], 1):
                _cmp(capsys, bad, f'{t} {name}', _flat_of(arena, getattr(opt, name), q), r32['t'][k][j], r64['t'][k][j])
    if sc is not None:
        assert int(sc.applied_steps.item()) == STEPS
    assert not bad, bad


# ---- 1. the norm through the C ABI ---------------------------------------------------------------------------------------------
def _measure(lib, grad, ranges, max_norm=INF, grad_scale=1.0, loss_scale=None):
    """Both launches over ``ranges`` = [(start, len), ...] of ``grad``: (partials, rec) on the CPU."""
    starts, lens = [a for a, _ in ranges], [n for _, n in ranges]
    bounds = [0]
    for n in lens:
        bounds.append(bounds[-1] + (n + 4095) // 4096)
    partials = torch.full((max(1, bounds[-1]),), -1.0, dtype=torch.float64, device=grad.device)
    rec = torch.full((16,), -1.0, dtype=torch.float32, device=grad.device)
    st = torch.cuda.current_stream().cuda_stream
    LA = ctypes.c_int64 * len(ranges)
    assert lib.mbv_grad_norm_partials(grad.data_ptr(), grad.numel(), LA(*starts), LA(*lens), len(ranges), partials.data_ptr(),
                                      bounds[-1], st) == 0
    assert lib.mbv_grad_clip_coef(partials.data_ptr(), bounds[-1], (ctypes.c_int32 * len(bounds))(*bounds), len(ranges),
                                  max_norm, grad_scale, 0 if loss_scale is None else loss_scale.data_ptr(), rec.data_ptr(),
                                  st) == 0
    torch.cuda.synchronize()
    return partials[:bounds[-1]].cpu(), rec.cpu()


def _close(got, want):
    return abs(float(got) - want) <= NORM_BAR * abs(want)


@pytest.mark.parametrize('layout', ['one', 'three'])
@pytest.mark.parametrize('n', [4, 64, 4092, 4096, 4100, BIG])
def test_norm_through_the_c_abi(device, n, layout):
    """One range covering an arena of n elements, and three ranges of n elements whose starts are multiples of 64 but not of
    4096 inside a larger arena whose other elements are non-zero (they must not be summed).  Total and per-range norms against
    numpy float64 within 2^-23, every chunk's partial within 1e-12 of numpy's, two runs equal bit for bit."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(4100 + n)
    if layout == 'one':
        ranges, size = [(0, n)], n
    else:
        stride = (n + 63) // 64 * 64 + 64
        ranges = [(64 + r * stride, n) for r in range(3)]
        size = 64 + 3 * stride
        assert all(a % 64 == 0 and a % 4096 != 0 for a, _ in ranges)
    host = torch.randn(size, generator=gen) * 3.0
    grad = host.to(device)
    g64 = host.numpy().astype(np.float64)
    partials, rec = _measure(lib, grad, ranges)
    again = _measure(lib, grad, ranges)
    assert torch.equal(partials, again[0]) and torch.equal(rec, again[1])
    sums = [float((g64[a:a + m] ** 2).sum()) for a, m in ranges]
    assert _close(rec[1], math.sqrt(sum(sums))), (float(rec[1]), math.sqrt(sum(sums)))
    for r, s in enumerate(sums):
        assert _close(rec[3 + r], math.sqrt(s)), (r, float(rec[3 + r]), math.sqrt(s))
    assert float(rec[0]) == 1.0 and float(rec[2]) == 1.0 and float(rec[3 + len(ranges):].abs().max()) == 0.0
    want = np.array([(g64[a + c:min(a + c + 4096, a + m)] ** 2).sum() for a, m in ranges for c in range(0, m, 4096)])
    assert partials.numel() == want.size
    assert float(np.abs(partials.numpy() - want).max()) <= 1e-12 * float(want.max())


def test_norm_of_huge_and_zero_gradients(device):
    """Every element 1e30: its square overflows f32, the norm 1e30 * sqrt(n) does not — finite and right only if nothing
    accumulates in f32.  An all-zero gradient: norm 0, coefficient exactly 1."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    n = 4100
    grad = torch.full((n,), 1e30, dtype=torch.float32, device=device)
    _, rec = _measure(lib, grad, [(0, n)], max_norm=1.0)
    want = float(np.float32(1e30)) * math.sqrt(n)
    assert math.isfinite(float(rec[1])) and _close(rec[1], want) and _close(rec[3], want)
    assert _close(rec[2], 1.0 / (want + 1e-6)) and _close(rec[0], want + 1e-6)
    grad.zero_()
    partials, rec = _measure(lib, grad, [(0, 2048), (2048, n - 2048 - 4)], max_norm=1.0)
    assert float(partials.abs().max()) == 0.0
    assert rec.tolist() == [1.0, 0.0, 1.0] + [0.0] * 13


def test_k41_entry_points_refuse_bad_arguments(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    n = 8192
    grad = torch.ones(n, dtype=torch.float32, device=device)
    partials = torch.full((4,), -1.0, dtype=torch.float64, device=device)
    rec = torch.full((16,), -1.0, dtype=torch.float32, device=device)
    st = torch.cuda.current_stream().cuda_stream
    G, S, R_ = grad.data_ptr(), partials.data_ptr(), rec.data_ptr()
    L1, L9 = ctypes.c_int64 * 1, ctypes.c_int64 * 9
    part = lambda **k: lib.mbv_grad_norm_partials(k.get('g', G), k.get('n', n), k.get('start', L1(0)), k.get('len', L1(n)),
                                                  k.get('count', 1), k.get('s', S), k.get('np', 2), st)
    BAD, UNSUPPORTED = -1, -3
    assert part(g=0) == BAD and part(g=G + 4) == BAD and part(n=-1) == BAD and part(count=-1) == BAD
    assert part(start=None) == BAD and part(len=None) == BAD and part(s=0) == BAD and part(s=S + 4) == BAD
    assert part(start=L1(2), len=L1(4096), np=1) == BAD and part(len=L1(4098), np=2) == BAD        # not multiples of 4
    assert part(start=L1(-4)) == BAD and part(len=L1(-4)) == BAD
    assert part(start=L1(4096), len=L1(4100), np=2) == BAD and part(len=L1(n + 4), np=3) == BAD    # outside the arena
    assert part(np=1) == BAD and part(np=3) == BAD and part(np=-1) == BAD                         # != sum of ceil(len / 4096)
    assert part(start=L9(*range(0, 36, 4)), len=L9(*[4] * 9), count=9, np=9) == UNSUPPORTED
    assert part(n=0, start=None, len=None, count=0, np=0) == 0 and part(count=0, start=None, len=None, np=0) == 0
    assert part(len=L1(0), np=0) == 0
    C2 = ctypes.c_int32 * 2
    coef = lambda **k: lib.mbv_grad_clip_coef(k.get('s', S), k.get('np', 2), k.get('rc', C2(0, 2)), k.get('count', 1),
                                              k.get('max_norm', 1.0), 1.0, k.get('ls', 0), k.get('rec', R_), st)
    assert coef(rec=0) == BAD and coef(rec=R_ + 2) == BAD and coef(s=0) == BAD and coef(s=S + 4) == BAD
    assert coef(np=-1) == BAD and coef(count=-1) == BAD and coef(rc=None) == BAD and coef(ls=R_ + 2) == BAD
    assert coef(max_norm=0.0) == BAD and coef(max_norm=-1.0) == BAD and coef(max_norm=float('nan')) == BAD
    assert coef(rc=C2(0, 1)) == BAD and coef(rc=C2(1, 2)) == BAD and coef(rc=(ctypes.c_int32 * 3)(0, 3, 2), count=2) == BAD
    assert coef(rc=(ctypes.c_int32 * 10)(*range(10)), count=9, np=9) == UNSUPPORTED
    torch.cuda.synchronize()
    assert float(partials.max()) == -1.0 and float(rec.max()) == -1.0          # nothing ran
    # nothing to sum: MBV_OK, norm 0 and coefficient 1 are written
    assert coef(count=0, np=0, rc=None, s=0) == 0
    torch.cuda.synchronize()
    assert rec.tolist() == [1.0, 0.0, 1.0] + [0.0] * 13


# ---- 2. the coefficient's known answers ----------------------------------------------------------------------------------------
def test_coefficient_known_answers(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    g = torch.tensor([3.0, 4.0, 0.0, 0.0], device=device)
    scale = torch.full((1,), 1024.0, device=device)
    cases = [dict(grad=g, kw=dict(max_norm=1.0), total=5.0, L=1.0),
             dict(grad=g, kw=dict(max_norm=1.0, grad_scale=0.5), total=2.5, L=1.0),
             dict(grad=g * 1024.0, kw=dict(max_norm=1.0, loss_scale=scale), total=5.0, L=1024.0)]
    for c in cases:
        _, rec = _measure(lib, c['grad'], [(0, 4)], **c['kw'])
        coef = 1.0 / (c['total'] + 1e-6)
        assert _close(rec[1], c['total']) and _close(rec[3], c['total']), rec
        assert _close(rec[2], coef) and float(rec[2]) < 1.0, rec
        assert _close(rec[0], c['L'] / coef), rec
    _, rec = _measure(lib, g, [(0, 4)], max_norm=10.0)                        # does not bite: exactly 1
    assert float(rec[2]) == 1.0 and float(rec[0]) == 1.0 and float(rec[1]) == 5.0
    for kw, L in ((dict(), 1.0), (dict(loss_scale=scale), 1024.0)):
        _, rec = _measure(lib, g * L, [(0, 4)], max_norm=INF, **kw)
        assert float(rec[2]) == 1.0 and float(rec[0]) == L and float(rec[1]) == 5.0


# ---- 3. bit identity where the clip does not bite ------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adamw', 'adam', 'lamb', 'sgd'])
def test_a_clip_that_does_not_bite_changes_no_bit(device, kind):
    grads = [{s: [t.to(device) for t in ts] for s, ts in g.items()} for g in _gradients()[:3]]
    runs = {}
    for max_norm in (None, INF, 1e9):
        toy, arena = _toy(device)
        opt = _make(kind, arena, max_grad_norm=max_norm)
        for step in range(3):
            _feed(toy, grads[step])
            opt.step()
        torch.cuda.synchronize()
        runs[max_norm] = _state(kind, arena, opt)
        if max_norm is not None:
            assert float(opt.clip_coef) == 1.0 and 0.0 < float(opt.grad_norm) < 1e9
    assert float((runs[None][0] - _toy(device)[1].param).abs().max()) > 0.0
    for max_norm in (INF, 1e9):
        for a, b in zip(runs[None], runs[max_norm]):
            assert torch.equal(a, b), max_norm


def test_the_gradient_buffer_is_never_scaled_in_place(device):
    """zero_grad=False: after a step whose clip bites, p.grad still holds the un-clipped gradient."""
    toy, arena = _toy(device)
    opt = _make('sgd', arena, max_grad_norm=MAX_NORM, zero_grad=False)
    _feed(toy, _gradients()[0])
    g0 = arena.grad.clone()
    opt.step()
    assert float(opt.clip_coef) < 1.0 and torch.equal(arena.grad, g0)


# ---- 4. where it bites ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adamw', 'lamb', 'sgd'])
def test_clipped_steps_match_float64(device, capsys, kind):
    _follow_reference(device, capsys, kind, kind)


# ---- 5. with the loss scaler ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adamw', 'lamb', 'sgd'])
def test_clipped_steps_with_a_loss_scaler(device, capsys, kind):
    """Scale 1024, gradients fed multiplied by 1024: the reference of the plain run, under the same bar.  In front of step 4
    one step whose gradient holds an inf: parameters and state unchanged, the scale halves, applied_steps does not advance,
    grad_norm is inf; the clean steps after it (fed at the halved scale) match the reference."""
    _follow_reference(device, capsys, kind, kind + ' scaled', feed=1024.0, scale=1024.0, overflow_at=3)


# ---- 6. data-parallel arithmetic in one process --------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adamw', 'lamb', 'sgd'])
def test_clipped_steps_with_grad_scale(device, capsys, kind):
    """Gradients fed doubled (the sum over two ranks) with grad_scale = 0.5: the reference of the plain run — grad_norm is
    the norm of the MEAN gradient."""
    _follow_reference(device, capsys, kind, kind + ' mean of 2', feed=2.0, grad_scale=0.5)


# ---- 7. fused arms and the graphed step ----------------------------------------------------------------------------------------
def test_clipping_refuses_the_fused_arms(device):
    toy, arena = _toy(device)
    opt = _make('adamw', arena, max_grad_norm=1.0)
    w, b = toy.encoder.ps[3], toy.encoder.ps[3]
    assert opt.fuse_layernorm_affine(w, b) is False and not opt.k3_armed(w)
    assert opt.fuse_matrices([toy.head.ps[0]]) is False and opt.matrices_armed is False
    plain = _make('adamw', _toy(device)[1])
    assert plain.max_grad_norm is None


def _graphed(device, clip):
    from mask_bev_amd.graph import GraphedTrainStep
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(0)
    kw = dict(tiny_kwargs(nx=96, ny=96, q=8), compute_dtype='bf16', lr=5e-4, gradient_clip_val=clip)
    m = MaskBevModule(**kw).to(device).train()
    m.log_scalars = False
    m._panoptic_head._panoptic_head.num_points = 2000
    arena = m.flatten_parameters()
    opt = m.configure_optimizers()['optimizer']
    assert opt.max_grad_norm == clip
    scans = [x.to(device) for x in random_scans(kw, [3000, 2500], seed=0)]
    labels, gt = random_gt(kw, 2, 3, seed=10)
    batch = (scans, (labels.to(device), gt.to(device)))
    g = GraphedTrainStep(m, opt, batch)
    p0 = arena.param.clone()
    losses = [float(g.step(batch)) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(math.isfinite(x) for x in losses), losses
    assert float(arena.grad.abs().max()) == 0.0 and float((arena.param - p0).abs().max()) > 0.0
    return m, opt, g


def test_graphed_step_with_clipping_keeps_the_update_in_the_optimizer(device):
    from mask_bev_amd import switches
    m, opt, g = _graphed(device, 0.01)
    assert not g._k3_fused and g._mx_fused == [] and not opt.matrices_armed
    norm, coef = float(opt.grad_norm), float(opt.clip_coef)
    assert 0.0 < norm < INF and 0.0 < coef <= 1.0, (norm, coef)
    assert abs(coef - min(1.0, float(np.float32(0.01)) / (norm + 1e-6))) <= 2e-6 * coef
    seg = {k: float(v) for k, v in opt.grad_norms().items()}
    assert list(seg) == ['encoder', 'backbone', 'head']
    assert abs(math.sqrt(sum(v * v for v in seg.values())) - norm) <= 1e-6 * norm
    g.close()
    # without clipping the step arms what it arms today
    m, opt, g = _graphed(device, None)
    assert g._k3_fused and opt.k3_armed(m._encoder._layer_norm.weight)
    assert opt.matrices_armed == bool(switches.get('adam_in_wgrad'))
    assert bool(g._mx_fused) == bool(switches.get('adam_in_wgrad'))
    g.close()
