"""K43 on the CPU: known answers of the averaging rule, ``arena.WeightAverage`` over a CPU arena against the numpy restatement
bit for bit (skipped steps, ``every``, both modes), the swap, the checkpoint format, the C-ABI / work-model surface of the two
entry points, and the module and launcher settings."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.average_ref import AverageRef, run
from tests.util_cfg import tiny_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K43 = ('mbv_weight_average_update', 'mbv_weight_average_swap')
F = np.float32


def _toy(shadow=torch.bfloat16, seed=43):
    from mask_bev_amd.arena import ParameterArena
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 5))       # 5: a parameter that is no multiple of 4
    return net, ParameterArena([('a', net[0]), ('b', net[1])], shadow_dtype=shadow)


def _move(arena, gen):
    """What an optimizer step does to the live weights, as far as the average can tell."""
    with torch.no_grad():
        arena.param.add_(torch.randn(arena.numel, generator=gen) * 0.05)
    return arena.param.numpy().copy()


# ---- known answers -----------------------------------------------------------------------------------------------------------
def test_running_mean_of_1_2_3_is_exact():
    avgs, ref = run([7.0], [[1.0], [2.0], [3.0]], mode='mean')
    assert [float(a[0]) for a in avgs] == [1.0, 1.5, 2.0]              # f32(1/3) * 1.5 rounds to 0.5
    assert ref.updates == 3 and ref.weight == F(1) / F(3)
    from mask_bev_amd.arena import WeightAverage
    _, arena = _toy(shadow=None)
    arena.param.fill_(7.0)
    av = WeightAverage(arena, mode='mean')
    for k, want in enumerate((1.0, 1.5, 2.0)):
        arena.param.fill_(float(k + 1))
        av.update()
        assert torch.equal(av.avg, torch.full_like(av.avg, want))
    assert int(av.num_updates) == 3


def test_ema_warmup_weights_are_the_stated_ones():
    ref = AverageRef([0.0], mode='ema', decay=0.9999, warmup=True)
    assert ref.tick() == F(0.9)                                        # u = 0: d = 1 / 10
    ref.tick()
    assert ref.tick() == F(0.75)                                       # u = 2: d = 3 / 12
    floor = F(1) - F(0.9999)
    ref.updates = 80000
    assert ref.tick() > floor                                          # still warming up
    for u in (89990, 89991, 100000, 10 ** 7):                          # (1 + u) / (10 + u) >= 0.9999 from u = 89990 on
        ref.updates = u
        assert ref.tick() == floor
    assert (1 + 89990) / (10 + 89990) >= 0.9999 > (1 + 89989) / (10 + 89989)
    plain = AverageRef([0.0], mode='ema', decay=0.9999, warmup=False)
    assert plain.tick() == floor
    # the product's CPU form computes the same weights
    from mask_bev_amd.arena import WeightAverage
    _, arena = _toy(shadow=None)
    av = WeightAverage(arena, mode='ema', decay=0.9999, warmup=True)
    seen = []
    for _ in range(3):
        av.update()
        seen.append(float(av.last_weight))
    assert seen[0] == float(F(0.9)) and seen[2] == 0.75
    sd = av.state_dict()
    sd['updates'] = 89990
    av.load_state_dict(sd)
    av.update()
    assert float(av.last_weight) == float(floor) and int(av.num_updates) == 89991


def test_every_two_blends_on_even_applied_calls_only():
    ref = AverageRef([0.0], mode='mean', every=2)
    ws = [float(ref.tick()) for _ in range(6)]
    assert ws == [0.0, 1.0, 0.0, 0.5, 0.0, float(F(1) / F(3))] and ref.updates == 3 and ref.calls == 6


# ---- the CPU arena against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,warmup,every', [('ema', True, 1), ('ema', False, 1), ('ema', True, 3), ('ema', False, 3),
                                               ('mean', True, 1), ('mean', True, 3)])
def test_cpu_arena_average_equals_the_restatement(mode, warmup, every):
    from mask_bev_amd.arena import WeightAverage
    _, arena = _toy()
    gen = torch.Generator().manual_seed(1)
    av = WeightAverage(arena, mode=mode, decay=0.9, warmup=warmup, every=every)
    assert torch.equal(av.avg, arena.param) and av.avg.data_ptr() != arena.param.data_ptr()
    ref = AverageRef(arena.param.numpy(), mode=mode, decay=0.9, warmup=warmup, every=every)
    ref64 = AverageRef(arena.param.numpy(), mode=mode, decay=0.9, warmup=warmup, every=every, dtype=np.float64)
    shadow0 = arena.shadow.clone()
    for step in range(8):
        p = _move(arena, gen)
        av.update()
        want = ref.step(p)
        ref64.step(p)
        assert torch.equal(av.avg, torch.from_numpy(want)), step
        assert float(av.last_weight) == float(ref.weight) and int(av.num_updates) == ref.updates
        assert torch.equal(arena.param, torch.from_numpy(p))          # the live weights are read only
    assert ref.updates == 8 // every and int(av._rec[1]) == 8
    assert np.abs(ref.avg - ref64.avg).max() <= 8 * 3 * 2.0 ** -24 * np.abs(ref64.avg).max() + 1e-7     # sanity, not the bar
    assert torch.equal(arena.shadow, shadow0)                          # update() leaves the shadow alone


def test_skipped_steps_leave_the_average_and_its_counters_alone():
    from mask_bev_amd.arena import LossScaler, WeightAverage
    _, arena = _toy()
    gen = torch.Generator().manual_seed(2)
    sc = LossScaler('cpu')
    sc.applied_steps.fill_(5)                                          # steps applied before the average existed do not count
    av = WeightAverage(arena, mode='ema', decay=0.5, warmup=True, scaler=sc)
    ref = AverageRef(arena.param.numpy(), mode='ema', decay=0.5, warmup=True)
    applied = [True, True, False, True, False, True]
    for ok in applied:
        before = (av.avg.clone(), int(av.num_updates), int(av._rec[1]))
        p = _move(arena, gen) if ok else arena.param.numpy().copy()
        if ok:
            sc.applied_steps.add_(1)                                   # what mbv_loss_scale_update does on a clean step
        av.update()
        want = ref.step(p, ok)
        assert torch.equal(av.avg, torch.from_numpy(want))
        if not ok:
            assert torch.equal(av.avg, before[0]) and (int(av.num_updates), int(av._rec[1])) == before[1:]
            assert float(av.last_weight) == 0.0
    assert int(av.num_updates) == 4 == ref.updates
    # the step after a skipped one used the un-advanced u: weights 1 - (1 + u) / (10 + u) for u = 0 .. 3, nothing skipped over
    assert float(av.last_weight) == float(F(1) - F(4) / F(13))


# ---- swap --------------------------------------------------------------------------------------------------------------------
def test_swap_twice_is_the_identity_and_applied_restores_on_an_exception():
    from mask_bev_amd import ops
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.arena import WeightAverage
    net, arena = _toy()
    av = WeightAverage(arena, mode='ema', decay=0.5, warmup=False)
    _move(arena, torch.Generator().manual_seed(3))
    arena.refresh_shadow()
    av.update()
    p0, a0, s0 = arena.param.clone(), av.avg.clone(), arena.shadow.clone()
    assert not torch.equal(p0, a0)
    epoch = ops.PARAM_EPOCH[0]
    av.swap()
    assert av.is_applied and ops.PARAM_EPOCH[0] > epoch
    assert torch.equal(arena.param, a0) and torch.equal(av.avg, p0) and torch.equal(arena.shadow, a0.to(torch.bfloat16))
    assert torch.equal(net[0].weight.data.reshape(-1), a0[:net[0].weight.numel()])       # the module's views follow
    for call in (av.update, av.state_dict, av.reset):
        with pytest.raises(MaskBevHipError, match='swapped in'):
            call()
    av.swap()
    assert not av.is_applied
    assert torch.equal(arena.param, p0) and torch.equal(av.avg, a0) and torch.equal(arena.shadow, s0)
    with pytest.raises(RuntimeError, match='boom'):
        with av.applied():
            assert av.is_applied and torch.equal(arena.param, a0)
            raise RuntimeError('boom')
    assert not av.is_applied
    assert torch.equal(arena.param, p0) and torch.equal(av.avg, a0) and torch.equal(arena.shadow, s0)


# ---- state -------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trips_and_a_foreign_kind_is_refused(tmp_path):
    from mask_bev_amd.arena import FlatAdam, LossScaler, WeightAverage
    _, arena = _toy()
    gen = torch.Generator().manual_seed(4)
    sc = LossScaler('cpu')
    av = WeightAverage(arena, mode='ema', decay=0.75, warmup=False, every=2, scaler=sc)
    for _ in range(5):
        _move(arena, gen)
        sc.applied_steps.add_(1)
        av.update()
    sd = av.state_dict()
    assert sd['kind'] == 'weight_average' and (sd['updates'], sd['calls'], sd['seen']) == (2, 5, 5)
    assert (sd['mode'], sd['decay'], sd['warmup'], sd['every']) == ('ema', 0.75, False, 2)
    torch.save(sd, tmp_path / 'avg.pt')
    other = WeightAverage(arena, mode='mean', scaler=sc)
    other.load_state_dict(torch.load(tmp_path / 'avg.pt', weights_only=False))
    assert torch.equal(other.avg, av.avg) and torch.equal(other._rec[:3], av._rec[:3])
    assert (other.mode, other.decay, other.warmup, other.every) == ('ema', 0.75, False, 2)
    _move(arena, gen)
    sc.applied_steps.add_(1)
    av.update(), other.update()                                        # the sixth applied call blends (every = 2) in both
    assert torch.equal(other.avg, av.avg) and int(other.num_updates) == 3
    with pytest.raises(ValueError, match='adam'):
        av.load_state_dict(FlatAdam(arena, [dict(segment='a'), dict(segment='b')]).state_dict()['flat_state'])
    with pytest.raises(ValueError, match='kind'):
        av.load_state_dict({'avg': av.avg})


def test_reset_starts_over_from_the_live_weights():
    from mask_bev_amd.arena import LossScaler, WeightAverage
    _, arena = _toy()
    gen = torch.Generator().manual_seed(5)
    sc = LossScaler('cpu')
    av = WeightAverage(arena, mode='mean', scaler=sc)
    for _ in range(3):
        _move(arena, gen)
        sc.applied_steps.add_(1)
        av.update()
    assert not torch.equal(av.avg, arena.param)
    av.reset()
    assert torch.equal(av.avg, arena.param) and av._rec.tolist() == [0, 0, 3, 0]
    av.update()                                                        # no step was applied since the reset
    assert av._rec.tolist()[:3] == [0, 0, 3] and float(av.last_weight) == 0.0
    for bad in (dict(mode='swa'), dict(decay=1.0), dict(decay=-0.1), dict(decay=float('nan')), dict(every=0),
                dict(decay=0.99999999)):                               # rounds to 1.0f
        with pytest.raises(ValueError, match='weight average'):
            WeightAverage(arena, **bad)


# ---- surface -----------------------------------------------------------------------------------------------------------------
def test_k43_entry_points_are_declared_bound_and_priced():
    from mask_bev_amd import _lib, workmodel as W
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    declared = set(re.findall(r'\b(mbv_[a-z0-9_]+)\s*\(', header))
    for name in K43:
        assert name in _lib.SIGNATURES and name in declared and name in W.MODELS, name
    assert 'K43' in header and 'mbv_weight_average_state' in header
    assert len(_lib.SIGNATURES['mbv_weight_average_update'][1]) == 10 and len(_lib.SIGNATURES['mbv_weight_average_swap'][1]) == 6
    P = ctypes.c_void_p
    n = 4195333
    upd = (P(16), P(32), n, P(48), None, 0, 0.9999, 1, 1, None)
    assert W.MODELS['mbv_weight_average_update'](upd) == ('k_average_blend', 'hbm', n * 12.0, 0.0)
    swap = (P(16), P(32), P(64), 1, n, None)
    assert W.MODELS['mbv_weight_average_swap'](swap) == ('k_average_swap', 'hbm', n * 18.0, 0.0)
    assert W.MODELS['mbv_weight_average_swap'](swap[:2] + (None, 0) + swap[4:])[2] == n * 16.0


def test_module_and_launcher_settings_reach_the_average():
    import train_mask_bev_amd as launcher
    from mask_bev_amd.arena import WeightAverage
    from mask_bev_amd.mask_bev_module import MaskBevModule
    args = launcher.build_parser().parse_args(['--config', 'x.yml', '--weight-average', 'mean'])
    assert args.weight_average == 'mean'
    assert launcher.build_parser().parse_args(['--config', 'x.yml']).weight_average is None
    with pytest.raises(SystemExit):
        launcher.build_parser().parse_args(['--config', 'x.yml', '--weight-average', 'swa'])
    # the YAML keys are module keywords, as gradient_clip_val is
    m = MaskBevModule(**tiny_kwargs(), weight_average='ema', weight_average_decay=0.99, weight_average_warmup=False,
                      weight_average_every=4, weight_average_start_epoch=2)
    assert m.hparams['weight_average'] == 'ema' and m.hparams['weight_average_start_epoch'] == 2
    assert m.make_weight_average() is None                              # no arena yet
    m.flatten_parameters()
    av = m.make_weight_average()
    assert isinstance(av, WeightAverage) and av.arena is m._arena and av.scaler is None
    assert (av.mode, av.decay, av.warmup, av.every) == ('ema', 0.99, False, 4)
    assert torch.equal(av.avg, m._arena.param)
    with pytest.raises(ValueError, match='weight_average'):
        MaskBevModule(**tiny_kwargs(), weight_average='swa')


def test_a_config_without_the_key_builds_no_average():
    from mask_bev_amd.mask_bev_module import MaskBevModule
    m = MaskBevModule(**tiny_kwargs())
    assert 'weight_average' not in m.hparams
    m.flatten_parameters()
    assert m.make_weight_average() is None
