"""K41 on the CPU: the C-ABI / work-model surface of the two gradient-clipping entry points, ``gradient_clip_val`` on the module,
``optimizers.clip_gradients`` against ``torch.nn.utils.clip_grad_norm_`` in float64, and what a flat optimizer with
``max_grad_norm`` does (and refuses) without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from tests.util_cfg import tiny_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K41 = ('mbv_grad_norm_partials', 'mbv_grad_clip_coef')


def test_k41_entry_points_are_declared_bound_and_priced():
    from mask_bev_amd import _lib, workmodel as W
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    declared = set(re.findall(r'\b(mbv_[a-z0-9_]+)\s*\(', header))
    for name in K41:
        assert name in _lib.SIGNATURES and name in declared and name in W.MODELS, name
    assert 'K41' in header
    assert len(_lib.SIGNATURES['mbv_grad_norm_partials'][1]) == 8 and len(_lib.SIGNATURES['mbv_grad_clip_coef'][1]) == 9
    P = ctypes.c_void_p
    lens = [4096 + 64, 3 * 4096, 8]                             # 2 + 3 + 1 chunks
    LA = ctypes.c_int64 * 3
    part = (P(1), sum(lens) + 640, LA(0, 8192, 32768), LA(*lens), 3, P(2), 6, None)
    assert W.MODELS['mbv_grad_norm_partials'](part) == ('k_grad_norm_partials', 'hbm', 4.0 * sum(lens) + 8.0 * 6, 0.0)
    assert W.MODELS['mbv_grad_norm_partials'](part[:4] + (0,) + part[5:6] + (0, None))[2] == 0.0
    coef = (P(2), 6, (ctypes.c_int32 * 4)(0, 2, 5, 6), 3, 0.01, 1.0, None, P(3), None)
    assert W.MODELS['mbv_grad_clip_coef'](coef) == ('k_grad_clip_coef', 'hbm', 8.0 * 6 + 64.0, 0.0)


def test_module_takes_gradient_clip_val_and_its_plain_optimizers_are_unchanged():
    from mask_bev_amd.mask_bev_module import MaskBevModule
    m = MaskBevModule(**tiny_kwargs(), gradient_clip_val=0.01)
    assert m._gradient_clip_val == 0.01 and m.hparams['gradient_clip_val'] == 0.01
    assert MaskBevModule(**tiny_kwargs())._gradient_clip_val is None
    out = m.configure_optimizers()                               # no arena: what it returns today
    assert set(out) == {'optimizer', 'lr_scheduler', 'monitor', 'interval'}
    plain = MaskBevModule(**tiny_kwargs()).configure_optimizers()['optimizer']
    assert type(out['optimizer']) is type(plain) and type(plain).__module__.startswith('torch.optim')
    assert not hasattr(out['optimizer'], 'max_grad_norm')
    strip = lambda pg: {k: v for k, v in pg.items() if k != 'params'}
    assert [strip(pg) for pg in out['optimizer'].param_groups] == [strip(pg) for pg in plain.param_groups]
    assert [len(pg['params']) for pg in out['optimizer'].param_groups] == [len(pg['params']) for pg in plain.param_groups]


def test_clip_gradients_equals_torch_in_float64():
    from mask_bev_amd.optimizers import clip_gradients
    gen = torch.Generator().manual_seed(41)
    shapes = [(1,), (5,), (300, 7), (4097,)]
    grads = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]

    def fresh():
        ps = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        return ps

    total = float(torch.cat([g.reshape(-1) for g in grads]).norm())
    for max_norm in (0.01, 0.5 * total, 2.0 * total):          # bites hard, bites, does not bite
        a, b = fresh(), fresh()
        got = clip_gradients(torch.optim.SGD(a, lr=0.1), a, max_norm)
        want = torch.nn.utils.clip_grad_norm_(b, max_norm)
        assert torch.equal(got, want) and abs(float(got) - total) <= 1e-12 * total
        for p, q, g in zip(a, b, grads):
            assert torch.equal(p.grad, q.grad)
            assert torch.allclose(p.grad, g * min(1.0, max_norm / (total + 1e-6)), rtol=1e-14, atol=0.0)
    a = fresh()
    assert clip_gradients(torch.optim.SGD(a, lr=0.1), a, None) is None
    for p, g in zip(a, grads):
        assert torch.equal(p.grad, g)                            # untouched


def test_flat_optimizer_with_clipping_on_a_cpu_arena():
    """Construction of FlatAdam works anywhere and step() raises as before; FlatLamb / FlatSGD raise at construction as before.
    clip_gradients leaves a flat optimizer alone; the readers raise when clipping is off; a bad threshold is refused."""
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.arena import FlatAdam, FlatLamb, FlatSGD, ParameterArena
    from mask_bev_amd.optimizers import clip_gradients
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4))
    arena = ParameterArena([('a', net[0]), ('b', net[1])])
    groups = [dict(segment='a'), dict(segment='b')]
    opt = FlatAdam(arena, groups, max_grad_norm=0.01)
    assert opt.max_grad_norm == 0.01
    with pytest.raises(AttributeError):
        opt.max_grad_norm = 1.0                                  # fixed for the optimizer's lifetime
    assert float(opt.grad_norm) == 0.0 and float(opt.clip_coef) == 1.0 and opt.grad_norm.dim() == 0
    assert list(opt.grad_norms()) == ['a', 'b'] and all(float(v) == 0.0 and v.dim() == 0 for v in opt.grad_norms().values())
    assert opt.fuse_layernorm_affine(net[0].weight, net[0].weight) is False
    assert opt.fuse_matrices([net[0].weight]) is False and opt.matrices_armed is False
    arena.grad.fill_(1.0)
    assert clip_gradients(opt, net.parameters(), 0.01) is None and float(arena.grad.min()) == 1.0
    with pytest.raises(MaskBevHipError, match='MI355X'):
        opt.step()
    off = FlatAdam(arena, groups)
    assert off.max_grad_norm is None and not hasattr(off, '_clip_rec')
    for read in (lambda: off.grad_norm, lambda: off.clip_coef, off.grad_norms):
        with pytest.raises(MaskBevHipError, match='max_grad_norm'):
            read()
    assert FlatAdam(arena, groups, max_grad_norm=float('inf')).max_grad_norm == float('inf')
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            FlatAdam(arena, groups, max_grad_norm=bad)
    with pytest.raises(MaskBevHipError):
        FlatLamb(arena, groups, max_grad_norm=0.01)
    with pytest.raises(MaskBevHipError):
        FlatSGD(arena, max_grad_norm=0.01)


def test_clip_stats_leave_skipped_steps_out_of_the_epoch_figures():
    """An overflowed fp16 step reports grad_norm = inf, clip_coef = 0: it is counted as skipped and enters neither the mean
    norm nor the clipped count."""
    from mask_bev_amd.optimizers import ClipStats
    stats = ClipStats()
    assert stats.line(0) == 'grad_norm 0 clipped 0/0'
    for norm, coef in ((2.0, 0.5), (float('inf'), 0.0), (4.0, 1.0), (float('nan'), float('nan'))):
        stats.add(torch.tensor(norm), torch.tensor(coef))
    assert stats.summary(4) == (3.0, 1, 2, 2)
    assert stats.line(4) == 'grad_norm 3 clipped 1/2 skipped 2'
    clean = ClipStats()
    clean.add(torch.tensor(0.5), torch.tensor(1.0))
    assert clean.line(1) == 'grad_norm 0.5 clipped 0/1'


def test_launcher_takes_gradient_clip_val():
    import train_mask_bev_amd as launcher
    args = launcher.build_parser().parse_args(['--config', 'x.yml', '--gradient-clip-val', '0.01'])
    assert args.gradient_clip_val == 0.01
    assert launcher.build_parser().parse_args(['--config', 'x.yml']).gradient_clip_val is None
