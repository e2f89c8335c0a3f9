"""K43 (csrc/optim_flat.hip): EMA / running-mean weight averaging over the parameter arena.

The checker is ``tests/average_ref.py``: the tick and the element rule in numpy float32, one rounding per operation.  Nothing
here has a tolerance: every comparison is ``torch.equal``, against that restatement or between two runs of the product.

The C-ABI sizes are 1, 3, 4, 5 (ragged tails around one float4), 1027 and 2051 (more than one block, with a tail) and
4195333 = kMaxBlocks * 256 * 4 + 1029, where a kernel under the arena frame's usual cap of 4096 blocks takes a second
grid-stride trip.  K43's two streams were measured faster under a cap of 65536 blocks (csrc/optim_flat.hip), so their second
trip and tail are exercised once more at BIG = 65536 * 256 * 4 + 1029 elements, with one update and one swap."""
import re

import numpy as np
import pytest
import torch
import yaml

from tests.average_ref import AverageRef
from tests.util_cfg import random_gt, random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
SIZES = (1, 3, 4, 5, 1027, 2051, 4195333)
BIG = 65536 * 256 * 4 + 1029                  # one float4 trip past kAverageMaxBlocks blocks, and a ragged tail
PAD = 64                                      # canary elements behind every buffer
EMA, MEAN = 0, 1


def _lib_stream(device):
    from mask_bev_amd import _lib
    return _lib.load(), torch.cuda.current_stream(device).cuda_stream


def _buffers(n, device, seed):
    """(param, avg) views of n elements in front of PAD canary elements, and their hosts."""
    g = torch.Generator().manual_seed(seed)
    hosts = []
    for k in range(2):
        h = torch.full((n + PAD,), 12345.0 + k)
        h[:n] = torch.randn(n, generator=g) * (0.1 if k == 0 else 0.3)
        hosts.append(h.to(device))
    return hosts[0][:n], hosts[1][:n], hosts


def _canaries_intact(hosts, n):
    return all(torch.equal(h[n:], torch.full((PAD,), 12345.0 + k, device=h.device)) for k, h in enumerate(hosts))


def _rec(device, updates=0, calls=0, seen=0):
    return torch.tensor([updates, calls, seen, 0], dtype=torch.int32, device=device)


def _weight(rec):
    return float(rec.view(torch.float32)[3])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_update_through_the_c_abi(device, n):
    lib, st = _lib_stream(device)
    p, avg, hosts = _buffers(n, device, seed=n)
    p0, a0 = p.clone(), avg.clone()
    # a skipped step: the applied-step count has not moved since the last call -> w = 0, nothing is touched
    applied = torch.tensor([7], dtype=torch.int32, device=device)
    rec = _rec(device, updates=3, calls=3, seen=7)
    assert lib.mbv_weight_average_update(p.data_ptr(), avg.data_ptr(), n, rec.data_ptr(), applied.data_ptr(), EMA, 0.9, 1, 1,
                                         st) == 0
    torch.cuda.synchronize()
    assert rec.tolist()[:3] == [3, 3, 7] and _weight(rec) == 0.0
    assert torch.equal(avg, a0) and torch.equal(p, p0) and _canaries_intact(hosts, n)
    # w = 1: the first update of a mean takes param itself
    rec = _rec(device)
    assert lib.mbv_weight_average_update(p.data_ptr(), avg.data_ptr(), n, rec.data_ptr(), 0, MEAN, 0.0, 0, 1, st) == 0
    torch.cuda.synchronize()
    assert rec.tolist()[:3] == [1, 1, 0] and _weight(rec) == 1.0
    assert torch.equal(avg, p0) and torch.equal(p, p0) and _canaries_intact(hosts, n)
    # generic weights: an EMA in its warm-up from u = 3 with the step counted through the applied-step count, twice
    avg.copy_(a0)
    ref = AverageRef(a0.cpu().numpy(), mode='ema', decay=0.9, warmup=True)
    ref.updates = ref.calls = 3
    rec = _rec(device, updates=3, calls=3, seen=7)
    for k in range(2):
        applied.add_(1)
        assert lib.mbv_weight_average_update(p.data_ptr(), avg.data_ptr(), n, rec.data_ptr(), applied.data_ptr(), EMA, 0.9, 1,
                                             1, st) == 0
        want = ref.step(p0.cpu().numpy())
        torch.cuda.synchronize()
        assert rec.tolist()[:3] == [4 + k, 4 + k, 8 + k] and _weight(rec) == float(ref.weight) and 0.0 < _weight(rec) < 1.0
        assert torch.equal(avg.cpu(), torch.from_numpy(want))
    assert torch.equal(p, p0) and _canaries_intact(hosts, n)
    # `every`: the call between two blends costs a launch and changes nothing but the call count
    rec = _rec(device, updates=2, calls=2)
    before = avg.clone()
    assert lib.mbv_weight_average_update(p.data_ptr(), avg.data_ptr(), n, rec.data_ptr(), 0, EMA, 0.5, 0, 2, st) == 0
    torch.cuda.synchronize()
    assert rec.tolist()[:3] == [2, 3, 0] and _weight(rec) == 0.0 and torch.equal(avg, before)
    assert lib.mbv_weight_average_update(p.data_ptr(), avg.data_ptr(), n, rec.data_ptr(), 0, EMA, 0.5, 0, 2, st) == 0
    torch.cuda.synchronize()
    assert rec.tolist()[:3] == [3, 4, 0] and _weight(rec) == 0.5
    half = AverageRef(before.cpu().numpy(), mode='ema', decay=0.5, warmup=False).step(p0.cpu().numpy())
    assert torch.equal(avg.cpu(), torch.from_numpy(half)) and _canaries_intact(hosts, n)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('shadow_dtype', [torch.bfloat16, torch.float16, None])
def test_swap_through_the_c_abi(device, n, shadow_dtype):
    lib, st = _lib_stream(device)
    p, avg, hosts = _buffers(n, device, seed=100 + n)
    special = torch.tensor([-0.0, float('inf'), 1e30, 1e-6, float('nan'), -float('inf')])[:min(n, 6)]
    avg[:special.numel()] = special.to(device)
    if n >= 12:
        p[-special.numel():] = special.flip(0).to(device)
    bits = lambda t: t.view(torch.int32).clone()
    p0, a0 = bits(p), bits(avg)
    shadow = sh_host = None
    if shadow_dtype is not None:
        sh_host = torch.full((n + PAD,), 7.0, dtype=shadow_dtype, device=device)
        shadow = sh_host[:n]
    flag = 0 if shadow is None else (2 if shadow_dtype == torch.float16 else 1)
    swap = lambda: lib.mbv_weight_average_swap(p.data_ptr(), avg.data_ptr(), 0 if shadow is None else shadow.data_ptr(), flag,
                                               n, st)
    assert swap() == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(p), a0) and torch.equal(bits(avg), p0) and _canaries_intact(hosts, n)      # bits moved, NaN included
    if shadow is not None:
        ok = ~torch.isnan(p)
        assert torch.equal(shadow[ok].cpu(), p[ok].cpu().to(shadow_dtype))                           # RNE of the new param
        assert torch.isnan(shadow[~ok].float()).all()
        assert torch.equal(sh_host[n:], torch.full((PAD,), 7.0, dtype=shadow_dtype, device=device))
        s1 = shadow.clone()
    assert swap() == 0 and swap() == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(p), a0) and torch.equal(bits(avg), p0) and _canaries_intact(hosts, n)      # three swaps = one
    if shadow is not None:
        assert torch.equal(shadow.view(torch.int16), s1.view(torch.int16))
        assert torch.equal(sh_host[n:], torch.full((PAD,), 7.0, dtype=shadow_dtype, device=device))


def test_grid_stride_beyond_the_block_cap(device):
    """BIG elements: more float4 items than the capped grid has threads, so the loop takes a second trip; then the tail."""
    lib, st = _lib_stream(device)
    n = BIG
    g = torch.Generator(device=device).manual_seed(43)
    hosts = [torch.full((n + PAD,), 12345.0 + k, device=device) for k in range(2)]
    p, avg = hosts[0][:n], hosts[1][:n]
    p.copy_(torch.randn(n, generator=g, device=device) * 0.1)
    avg.copy_(torch.randn(n, generator=g, device=device) * 0.3)
    p0, a0 = p.clone(), avg.clone()
    rec = _rec(device, updates=5, calls=5)
    assert lib.mbv_weight_average_update(p.data_ptr(), avg.data_ptr(), n, rec.data_ptr(), 0, EMA, 0.9, 0, 1, st) == 0
    ref = AverageRef(a0.cpu().numpy(), mode='ema', decay=0.9, warmup=False)
    want = torch.from_numpy(ref.step(p0.cpu().numpy()))
    torch.cuda.synchronize()
    assert _weight(rec) == float(ref.weight) and rec.tolist()[:3] == [6, 6, 0]
    assert torch.equal(avg.cpu(), want) and torch.equal(p, p0) and _canaries_intact(hosts, n)
    # the last elements are the ones the second trip and the tail write
    assert not torch.equal(avg[-1029:], a0[-1029:])
    blended = avg.clone()
    sh_host = torch.full((n + PAD,), 7.0, dtype=torch.bfloat16, device=device)
    assert lib.mbv_weight_average_swap(p.data_ptr(), avg.data_ptr(), sh_host.data_ptr(), 1, n, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(p, blended) and torch.equal(avg, p0) and _canaries_intact(hosts, n)
    assert torch.equal(sh_host[:n], blended.to(torch.bfloat16))
    assert torch.equal(sh_host[n:], torch.full((PAD,), 7.0, dtype=torch.bfloat16, device=device))


def test_bad_arguments_are_refused_and_an_empty_arena_is_accepted(device):
    lib, st = _lib_stream(device)
    n = 1024
    p, avg, _ = _buffers(n, device, seed=9)
    rec = _rec(device)
    sh = torch.zeros(n + 8, dtype=torch.bfloat16, device=device)
    P, A, R, S = p.data_ptr(), avg.data_ptr(), rec.data_ptr(), sh.data_ptr()
    good = dict(param=P, avg=A, n=n, state=R, applied=0, mode=EMA, decay=0.9, warmup=1, every=1)
    upd = lambda **kw: lib.mbv_weight_average_update(*{**good, **kw}.values(), st)
    a0 = avg.clone()
    for bad in (dict(param=0), dict(avg=0), dict(state=0), dict(param=P + 4), dict(avg=A + 8), dict(avg=P), dict(state=R + 2),
                dict(applied=R + 1), dict(n=-1), dict(decay=1.0), dict(decay=-0.01), dict(decay=float('nan')), dict(decay=1.5),
                dict(every=0), dict(every=-3), dict(mode=2), dict(mode=-1)):
        assert upd(**bad) == -1, bad
    assert upd(n=0) == 0
    swp = lambda param=P, avg=A, shadow=S, dtype=1, n=n: lib.mbv_weight_average_swap(param, avg, shadow, dtype, n, st)
    for bad in (dict(param=0), dict(avg=0), dict(param=P + 4), dict(avg=A + 12), dict(avg=P), dict(n=-1), dict(shadow=S + 2),
                dict(dtype=0), dict(dtype=3)):
        assert swp(**bad) == -1, bad
    assert swp(n=0) == 0
    torch.cuda.synchronize()
    assert rec.tolist() == [0, 0, 0, 0] and torch.equal(avg, a0)      # nothing ran: the record did not advance
    assert upd(decay=0.0) == 0                                        # decay 0 is in range: d = min(0, 1 / 10), so w = 1
    torch.cuda.synchronize()
    assert _weight(rec) == 1.0 and torch.equal(avg, p)


# ---- behind the flat optimizers ----------------------------------------------------------------------------------------------
SHAPES = [(1,), (5,), (63,), (64, 3), (4097,), (300, 257)]
STEPS = 6


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(43)
        self.a = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g) * 0.1) for s in SHAPES[:3]])
        self.b = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g) * 0.1) for s in SHAPES[3:]])


def _toy(device):
    from mask_bev_amd.arena import ParameterArena
    toy = _Toy().to(device)
    return toy, ParameterArena([('a', toy.a), ('b', toy.b)], shadow_dtype=torch.bfloat16)


_GRADS = {}


def _gradients():
    if not _GRADS:
        g = torch.Generator().manual_seed(6)
        _GRADS['g'] = [[torch.randn(s, generator=g) * 0.3 for s in SHAPES] for _ in range(STEPS)]
    return _GRADS['g']


def _feed(toy, grads, scale=None, poison=False):
    for q, g in zip(toy.parameters(), grads):
        q.grad.copy_(g.to(q.device))
        if scale is not None:
            q.grad.mul_(scale.view(()))
    if poison:
        next(iter(toy.parameters())).grad.view(-1)[0] = float('inf')


def _optimizer(kind, arena, scaler=None):
    from mask_bev_amd.arena import FlatAdam, FlatSGD
    if kind == 'sgd':
        return FlatSGD(arena, lr=0.05, momentum=0.9, weight_decay=1e-3, scaler=scaler)
    return FlatAdam(arena, [dict(segment='a', lr=2e-2), dict(segment='b', lr=5e-3)], weight_decay=0.01, scaler=scaler)


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
@pytest.mark.parametrize('scaled', [False, True])
def test_average_follows_a_flat_optimizer(device, kind, scaled):
    """Six steps; avg equals the restatement applied to the snapshots of arena.param.  With a loss scaler, an inf in the
    gradient of step 3 makes the optimizer skip that step, and the average with it."""
    from mask_bev_amd.arena import LossScaler, WeightAverage
    toy, arena = _toy(device)
    sc = LossScaler(device) if scaled else None
    opt = _optimizer(kind, arena, sc)
    av = WeightAverage(arena, mode='ema', decay=0.9, warmup=True, scaler=sc)
    ref = AverageRef(arena.param.cpu().numpy(), mode='ema', decay=0.9, warmup=True)
    prev = arena.param.clone()
    for step, grads in enumerate(_gradients()):
        skipped = scaled and step == 2
        _feed(toy, grads, None if sc is None else sc.scale, poison=skipped)
        opt.step()
        av.update()
        assert torch.equal(arena.param, prev) == skipped
        want = ref.step(arena.param.cpu().numpy(), not skipped)
        assert torch.equal(av.avg.cpu(), torch.from_numpy(want)), step
        assert float(av.last_weight) == float(ref.weight)
        prev = arena.param.clone()
    assert int(av.num_updates) == (5 if scaled else 6) == ref.updates
    assert av.num_updates.dim() == 0 and av.num_updates.is_cuda and av.last_weight.dtype == torch.float32


def test_captured_step_and_update_replay_like_eager_ones(device):
    """opt.step(); avg.update() captured once and replayed five times against five eager steps: the warm-up weight is different
    on every replay, which only the device-side counter can produce."""
    from mask_bev_amd.arena import WeightAverage
    grads = _gradients()

    def fresh():
        toy, arena = _toy(device)
        return toy, arena, _optimizer('sgd', arena), WeightAverage(arena, mode='ema', decay=0.9999, warmup=True)

    toy, arena, opt, av = fresh()
    for g in grads:
        _feed(toy, g)
        opt.step()
        av.update()
    torch.cuda.synchronize()
    eager = [arena.param.clone(), av.avg.clone(), arena.shadow.clone(), av._rec.clone()]
    toy, arena, opt, av = fresh()
    side = torch.cuda.Stream(device=device)
    _feed(toy, grads[0])
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                                        # warm-up = step 1
        av.update()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
        av.update()
    weights = []
    for g in grads[1:]:
        _feed(toy, g)
        graph.replay()
        weights.append(float(av.last_weight))
    torch.cuda.synchronize()
    for a, b, name in zip(eager, [arena.param, av.avg, arena.shadow, av._rec], ('param', 'avg', 'shadow', 'record')):
        assert torch.equal(a, b), name
    assert len(set(weights)) == 5 and int(av.num_updates) == 6
    assert weights == [float(np.float32(1) - np.float32(1 + u) / np.float32(10 + u)) for u in range(1, 6)]


# ---- the module --------------------------------------------------------------------------------------------------------------
def _module(device, dtype='bf16', **extra):
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(0)
    kw = dict(tiny_kwargs(nx=96, ny=96, q=8), compute_dtype=dtype, lr=5e-4, **extra)
    m = MaskBevModule(**kw).to(device).train()
    m.log_scalars = False
    m._panoptic_head._panoptic_head.num_points = 2000
    m.flatten_parameters()
    return kw, m


def _batch(kw, device, seed=0):
    scans = [x.to(device) for x in random_scans(kw, [3000, 2500], seed=seed)]
    labels, gt = random_gt(kw, 2, 3, seed=10 + seed)
    return scans, (labels.to(device), gt.to(device))


def test_graphed_train_step_updates_the_average(device):
    """GraphedTrainStep(average=) with the fused arms as they come (AdamW, one GPU: K3's and K17's updates happen inside the
    backward): the update behind opt.step() sees every parameter's new value."""
    from mask_bev_amd.arena import WeightAverage
    from mask_bev_amd.graph import GraphedTrainStep
    kw, m = _module(device, weight_average='ema', weight_average_decay=0.9)
    arena = m._arena
    opt = m.configure_optimizers()['optimizer']
    av = m.make_weight_average()
    assert isinstance(av, WeightAverage) and (av.mode, av.decay, av.warmup, av.every) == ('ema', 0.9, True, 1)
    batch = _batch(kw, device)
    g = GraphedTrainStep(m, opt, batch, average=av)
    assert g._k3_fused                                                  # nothing was disarmed for the average
    assert torch.equal(av.avg, arena.param)
    ref = AverageRef(arena.param.cpu().numpy(), mode='ema', decay=0.9, warmup=True)
    for it in range(3):
        before = arena.param.clone()
        g.step(batch)
        for seg in ('encoder', 'backbone', 'head'):
            a, b = arena.segments[seg]
            assert not torch.equal(arena.param[a:b], before[a:b])
        want = ref.step(arena.param.cpu().numpy())
        assert torch.equal(av.avg.cpu(), torch.from_numpy(want)), it
    assert int(av.num_updates) == 3
    g.close()


def _assert_same(a, b):
    """tests/test_predict_gpu.py's comparison of a replay with eager predict, at its strictest setting."""
    from tests.test_predict_gpu import assert_same
    assert_same(a, b)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_predictions_under_the_average(device, dtype):
    """Inside applied() the module predicts what a second module holding the averaged weights predicts — eagerly, and from a
    graph captured before the swap (the 16-bit shadow and the cached weight records follow the exchange); afterwards it predicts
    what it did before."""
    from mask_bev_amd.arena import WeightAverage
    from mask_bev_amd.predict import GraphedPredictStep
    kw, m = _module(device, dtype)
    opt = m.configure_optimizers()['optimizer']
    av = WeightAverage(m._arena, mode='ema', decay=0.5, warmup=False)
    batch = _batch(kw, device, seed=4)
    scans = batch[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                 # eager backward off the default stream (graph.py)
        for _ in range(3):
            opt.zero_grad()
            m.scale_loss(m.training_step(batch, 0)).backward()
            opt.step()
            av.update()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not torch.equal(av.avg, m._arena.param)
    _, other = _module(device, dtype)
    other.load_state_dict(m.state_dict())         # the live buffers (they are not averaged) ...
    with torch.no_grad():
        other._arena.param.copy_(av.avg)          # ... and the averaged parameters
    other._arena.refresh_shadow()
    want = other.predict(scans)
    graphed = GraphedPredictStep(m, scans)
    before = graphed.step(scans).clone()
    _assert_same(before, m.predict(scans))
    with av.applied():
        got = m.predict(scans)
        _assert_same(got, want)
        replay = graphed.step(scans).clone()
        _assert_same(replay, got)
    assert not torch.equal(want.scores, before.scores)                 # the averaged weights do predict something else
    after = m.predict(scans)
    _assert_same(after, before)
    _assert_same(graphed.step(scans).clone(), before)
    graphed.close()


def test_launcher_trains_validates_and_tests_with_an_average(tmp_path, capsys):
    import train_mask_bev_amd as launcher
    from mask_bev_amd import synthetic
    kw = dict(synthetic.module_kwargs('smoke_96', 2, compute_dtype='bf16'), dataset='synthetic', synthetic_points=6000,
              limit_val_batches=0.0, x_range=[-12, 12], y_range=[-12, 12], z_range=[-3, 1], weight_average='ema',
              weight_average_decay=0.99)
    cfg = tmp_path / 'smoke_96.yml'
    cfg.write_text(yaml.safe_dump(kw))
    ck = tmp_path / 'ckpt'
    rc = launcher.main(['--config', str(cfg), '--train', '--synthetic', '--max-epochs', '2', '--steps-per-epoch', '2',
                        '--checkpoint-root', str(ck)])
    assert rc == 0
    capsys.readouterr()
    sd = torch.load(ck / 'smoke_96' / 'last.ckpt', weights_only=False)
    wa = sd['weight_average']
    assert wa['kind'] == 'weight_average' and (wa['mode'], wa['decay'], wa['updates'], wa['calls']) == ('ema', 0.99, 4, 4)
    assert torch.isfinite(wa['avg']).all() and float(wa['avg'].abs().max()) > 0
    # 'state_dict' is still the LIVE weights, the ones the optimizer state belongs to: laid out in an arena they are not the average
    from mask_bev_amd.mask_bev_module import MaskBevModule
    live = MaskBevModule(**sd['hyper_parameters'])
    live.load_state_dict(sd['state_dict'])
    flat = live.flatten_parameters().param
    assert flat.shape == wa['avg'].shape and not torch.equal(flat, wa['avg'].cpu())
    assert float((flat - wa['avg'].cpu()).abs().max()) < 0.1          # ... but four steps away from it
    rc = launcher.main(['--config', str(cfg), '--test', '--synthetic', '--checkpoint-root', str(ck)])
    out = capsys.readouterr().out
    assert rc == 0 and 'Testing from' in out
    found = re.search(r'^weight average: ema, decay 0\.99, (\d+) updates$', out, re.M)
    assert found and int(found.group(1)) in (2, 4), out
