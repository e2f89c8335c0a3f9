"""K40 on the CPU: the LAMB rule's known answers, optimizers.Lamb against the restatement tests/optim_ref.py in float64, the SGD
restatement against torch.optim.SGD, what `optimiser_type: lamb` returns without an arena, and the C-ABI / work-model surface
of the four K40 entry points."""
import os
import re

import pytest
import torch

from tests import optim_ref as R
from tests.util_cfg import tiny_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K40 = ('mbv_lamb_moments', 'mbv_lamb_trust', 'mbv_lamb_apply', 'mbv_sgd_step')

# one tensor p = [3, 4], g = [1, -1] on both steps, lr 0.1, weight_decay 0.01, defaults otherwise; worked out in float64
KNOWN = [dict(wn=5.0, un=4.465197822680062, trust=1.1197712169892047, p=[2.642549133309, 4.349612468172]),
         dict(trust=0.8485437019396321, p=[2.279718453635, 4.706509993156])]


def test_lamb_known_answer_reference():
    p = torch.tensor([3.0, 4.0], dtype=torch.float64)
    g = torch.tensor([1.0, -1.0], dtype=torch.float64)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, want in enumerate(KNOWN, 1):
        wn = min(float(p.norm()), 10.0)
        p, m, v, trust, u = R.lamb_step(p, g, m, v, t, lr=0.1, weight_decay=0.01)
        if 'wn' in want:
            assert abs(wn - want['wn']) <= 1e-11 and abs(float(u.norm()) - want['un']) <= 1e-11
        assert abs(trust - want['trust']) <= 1e-11
        assert float((p - torch.tensor(want['p'], dtype=torch.float64)).abs().max()) <= 1e-11


def test_lamb_known_answer_optimizer():
    from mask_bev_amd.optimizers import Lamb
    p = torch.nn.Parameter(torch.tensor([3.0, 4.0], dtype=torch.float64))
    opt = Lamb([p], lr=0.1, weight_decay=0.01)
    assert opt.defaults['eps'] == 1e-6 and opt.defaults['betas'] == (0.9, 0.999)
    assert opt.clamp_value == 10.0 and opt.debias is False
    for want in KNOWN:
        p.grad = torch.tensor([1.0, -1.0], dtype=torch.float64)
        opt.step()
        assert float((p.detach() - torch.tensor(want['p'], dtype=torch.float64)).abs().max()) <= 1e-11
    st = opt.state[p]
    assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'} and st['step'] == 2


@pytest.mark.parametrize('debias', [False, True])
def test_lamb_matches_reference_f64(debias):
    """Sizes 1, 5, 300 x 7; an all-zero parameter (trust 1), a parameter whose gradient is zero in a group with weight_decay 0
    (trust 1), a parameter of norm 30 (the clamp bites) and one of norm 3; two groups with their own lr / weight_decay."""
    from mask_bev_amd.optimizers import Lamb
    gen = torch.Generator().manual_seed(40)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    unit = lambda t, norm: t / t.norm() * norm
    init = [rnd(1), rnd(5), unit(rnd(300, 7), 30.0), unit(rnd(5), 3.0), torch.zeros(5, dtype=torch.float64), rnd(5)]
    zero_grad = {5}                                          # the last tensor: gradient zero, in the weight_decay-0 group
    params = [torch.nn.Parameter(t.clone()) for t in init]
    hp = [dict(lr=3e-3, weight_decay=0.01), dict(lr=1e-2, weight_decay=0.0)]
    opt = Lamb([dict(params=params[:5], **hp[0]), dict(params=params[5:], **hp[1])], debias=debias)
    ref = [(t.clone(), torch.zeros_like(t), torch.zeros_like(t)) for t in init]
    for step in range(1, 6):
        grads = [torch.zeros_like(t) if i in zero_grad else rnd(*t.shape) for i, t in enumerate(init)]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()
        for i, g in enumerate(grads):
            h = hp[0] if i < 5 else hp[1]
            p, m, v, trust, u = R.lamb_step(ref[i][0], g, ref[i][1], ref[i][2], step, debias=debias, **h)
            ref[i] = (p, m, v)
            if i == 5 or (i == 4 and step == 1):             # ||u|| = 0 always; ||p|| = 0 until the first update moves it
                assert trust == 1.0
            if i == 2:                                       # norm 30: the clamp bites
                assert abs(trust - 10.0 / float(u.norm())) <= 1e-12
            assert float((params[i].detach() - p).abs().max()) <= 1e-12, (step, i)
            assert float((opt.state[params[i]]['exp_avg'] - m).abs().max()) <= 1e-12
            assert float((opt.state[params[i]]['exp_avg_sq'] - v).abs().max()) <= 1e-12
    assert torch.equal(params[5].detach(), init[5])          # zero gradient, no decay: it never moves


def test_sgd_reference_equals_torch_f64():
    gen = torch.Generator().manual_seed(41)
    init = [torch.randn(s, generator=gen, dtype=torch.float64) for s in ((1,), (5,), (300, 7))]
    params = [torch.nn.Parameter(t.clone()) for t in init]
    opt = torch.optim.SGD(params, lr=1e-2, momentum=0.99, nesterov=True, weight_decay=1e-3)
    ref = [(t.clone(), None) for t in init]
    for _ in range(4):
        for i, p in enumerate(params):
            g = torch.randn(p.shape, generator=gen, dtype=torch.float64)
            p.grad = g.clone()
            ref[i] = R.sgd_step(ref[i][0], g, ref[i][1], lr=1e-2, momentum=0.99, weight_decay=1e-3, nesterov=True)
        opt.step()
        for i, p in enumerate(params):
            assert torch.equal(p.detach(), ref[i][0]), i
            assert torch.equal(opt.state[p]['momentum_buffer'], ref[i][1]), i


def test_sgd_zero_buffer_equals_first_step_clone():
    """The flat kernel starts from a zero buffer where torch clones the gradient: the same bits with dampening 0."""
    gen = torch.Generator().manual_seed(42)
    p, g = torch.randn(50, generator=gen), torch.randn(50, generator=gen)
    a = R.sgd_step(p, g, None, lr=1e-2, weight_decay=1e-3)
    b = R.sgd_step(p, g, torch.zeros_like(p), lr=1e-2, weight_decay=1e-3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('differential', [False, True])
def test_module_returns_lamb_without_an_arena(differential):
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.optimizers import Lamb
    kw = dict(tiny_kwargs(), optimiser_type='lamb', lr=2e-4, weight_decay=1e-3, differential_lr=differential,
              differential_lr_scaling=0.1)
    m = MaskBevModule(**kw)
    out = m.configure_optimizers()
    assert set(out) == {'optimizer', 'lr_scheduler', 'monitor', 'interval'}
    opt = out['optimizer']
    assert type(opt) is Lamb
    assert out['lr_scheduler'].optimizer is opt
    assert opt.clamp_value == 10.0 and opt.debias is False
    for pg in opt.param_groups:
        assert pg['eps'] == 1e-6 and pg['betas'] == (0.9, 0.999) and pg['weight_decay'] == 1e-3
    if differential:
        assert [pg['lr'] for pg in opt.param_groups] == [2e-4 * 0.1, 2e-4 * 0.1, 2e-4]
        counts = [sum(1 for _ in mod.parameters()) for mod in (m._encoder, m._backbone, m._panoptic_head)]
        assert [len(pg['params']) for pg in opt.param_groups] == counts
    else:
        assert [pg['lr'] for pg in opt.param_groups] == [2e-4]
        assert len(opt.param_groups[0]['params']) == sum(1 for _ in m.parameters())
    # one step on the CPU moves a parameter that has a gradient
    p = next(m._panoptic_head.parameters())
    before = p.detach().clone()
    p.grad = torch.ones_like(p)
    opt.step()
    assert not torch.equal(p.detach(), before)


def test_k40_entry_points_are_declared_bound_and_priced():
    import ctypes
    from mask_bev_amd import _lib, build, workmodel as W
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    declared = set(re.findall(r'\b(mbv_[a-z0-9_]+)\s*\(', header))
    for name in K40:
        assert name in _lib.SIGNATURES and name in declared and name in W.MODELS, name
    assert _lib.ABI_VERSION == 59
    assert build.FILE_FLAGS['optim_flat.hip'] == ['-ffp-contract=off']
    # one unit for the optimizer passes (K11's AdamW with K40), one for the parameter-gradient kernels, on default flags
    assert 'pgrad.hip' in build.sources() and 'optim_flat.hip' in build.sources() and 'optim.hip' not in build.sources()
    assert 'pgrad.hip' not in build.FILE_FLAGS
    P = ctypes.c_void_p
    n = 3 * 4096 + 64                                        # one parameter: three full chunks and a 64-element one
    _lib.WORK_HINT.pop('lamb_elems', None)
    mom = (P(1), P(2), P(3), P(4), n, P(5), 4, 0, 4, P(6), 0.9, 0.999, 1e-6, 0.0, 1.0, None, None, None)
    app = (P(1), P(2), P(7), 1, n, P(5), 4, 0, 4, P(8), 1, 1e-3, 0.9, 0.999, 0, 1, None, None, None)
    # without the element count of the run every chunk is priced full
    assert W.MODELS['mbv_lamb_moments'](mom) == ('k_lamb_moments', 'hbm', 4 * 4096 * 28.0 + 4 * 8.0, 0.0)
    _lib.WORK_HINT['lamb_elems'] = {(0, 4): n}
    try:
        assert W.MODELS['mbv_lamb_moments'](mom) == ('k_lamb_moments', 'hbm', n * 28.0 + 4 * 8.0, 0.0)
        assert W.MODELS['mbv_lamb_apply'](app) == ('k_lamb_apply', 'hbm', n * 18.0, 0.0)
        assert W.MODELS['mbv_lamb_apply'](app[:2] + (None,) + app[3:])[2] == n * 16.0        # no shadow
    finally:
        _lib.WORK_HINT.pop('lamb_elems', None)
    assert W.MODELS['mbv_lamb_trust']((P(6), 4, P(9), 1, 10.0, P(8), None)) == ('k_lamb_trust', 'hbm', 4 * 8.0 + 12.0, 0.0)
    sgd = (P(1), P(2), P(3), P(7), 1, n, 1e-3, 0.99, 0.0, 0.0, 1, 1.0, 1, None, None, None)
    assert W.MODELS['mbv_sgd_step'](sgd) == ('k_sgd', 'hbm', n * 26.0, 0.0)
    assert W.MODELS['mbv_sgd_step'](sgd[:3] + (None,) + sgd[4:12] + (0,) + sgd[13:])[2] == n * 20.0
