"""AdamW in the epilogue of K17's grouped weight-gradient product (csrc/gemm.hip: k_gemm16_tn_group with AdamEpi;
mbv_gemm16_tn_group_adam, mbv_adam_args_write; FlatAdam.fuse_matrices; GraphedTrainStep).

The fused update runs adam_one (csrc/adam.hpp) — the one definition k_adamw runs — on the gradient in the product's
accumulators, so every comparison with "grouped product into a zeroed gradient, then mbv_adamw_step" below is BIT FOR BIT
(torch.equal), not a tolerance: 0 + g == g, g * 1.0f == g, and the bias corrections come from one host helper."""
import ctypes
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from mask_bev_amd import switches

pytestmark = pytest.mark.gpu

BF16, F16 = 1, 2          # MBV_DT_BF16 / MBV_DT_F16 (maskbev_hip.h)
SHADOW = {BF16: torch.bfloat16, F16: torch.float16}

# (m, n, k) of one launch: ragged tiles below one depth; exactly one depth; splits == 2 (must come back unfused); a plain entry
ENTRIES = [(96, 200, 136), (4096, 256, 128), (4100, 128, 128), (64, 128, 128)]
ARMED = [True, True, True, False]
EXPECT_FUSED = [True, True, False, False]


def _rand(shape, dt, seed, device, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt).to(device)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Arena:
    """Five flat buffers laid out like a parameter arena: every entry's (n, k) weight at a 64-element boundary."""

    def __init__(self, shapes, shadow_kind, device, seed=0):
        self.offsets, off = [], 0
        for _, n, k in shapes:
            self.offsets.append(off)
            off += (n * k + 63) // 64 * 64
        self.numel = off
        self.param = _rand((off,), torch.float32, seed + 1, device)
        self.exp_avg = _rand((off,), torch.float32, seed + 2, device, 0.1)
        self.exp_avg_sq = _rand((off,), torch.float32, seed + 3, device, 0.1).square()
        self.grad = torch.zeros(off, dtype=torch.float32, device=device)
        self.shadow = self.param.to(SHADOW[shadow_kind])
        self.shadow_kind = shadow_kind
        self.shapes = shapes

    def clone(self):
        c = object.__new__(_Arena)
        c.__dict__.update(self.__dict__)
        for name in ('param', 'exp_avg', 'exp_avg_sq', 'grad', 'shadow'):
            setattr(c, name, getattr(self, name).clone())
        return c

    def dw(self, i):
        _, n, k = self.shapes[i]
        return self.grad[self.offsets[i]:self.offsets[i] + n * k].view(n, k)

    def as_optimizer(self):
        """What ops.gemm16_tn_group reads of a FlatAdam."""
        return SimpleNamespace(arena=SimpleNamespace(grad=self.grad, param=self.param, shadow=self.shadow, numel=self.numel),
                               exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq)

    def adamw(self, i, hp, step):
        """mbv_adamw_step over entry i's range (the unfused reference), leaving the gradient as it is."""
        from mask_bev_amd import _lib
        _, n, k = self.shapes[i]
        o = self.offsets[i]
        _lib.check(_lib.load().mbv_adamw_step(
            self.param.data_ptr() + 4 * o, self.grad.data_ptr() + 4 * o, self.exp_avg.data_ptr() + 4 * o,
            self.exp_avg_sq.data_ptr() + 4 * o, self.shadow.data_ptr() + 2 * o, self.shadow_kind, n * k, hp['lr'], hp['b1'],
            hp['b2'], hp['eps'], hp['wd'], step, 1.0, hp['decoupled'], 0, None, None, None, _stream()), 'mbv_adamw_step')


def _write_block(block, hp, step, shadow_kind):
    from mask_bev_amd import _lib
    _lib.check(_lib.load().mbv_adam_args_write(block.data_ptr(), hp['lr'], hp['b1'], hp['b2'], hp['eps'], hp['wd'], step,
                                               hp['decoupled'], shadow_kind, _stream()), 'mbv_adam_args_write')


def _operands(dt, device):
    return [(_rand((m, n), dt, 10 + i, device, 0.5), _rand((m, k), dt, 20 + i, device, 0.5)) for i, (m, n, k) in enumerate(ENTRIES)]


@pytest.mark.parametrize('shadow_kind', [BF16, F16])
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
def test_fused_entries_equal_product_then_adamw_bit_for_bit(device, dt, shadow_kind):
    """One launch of four entries (ENTRIES) against mbv_gemm16_tn_group into a zeroed dw + mbv_adamw_step over the same ranges,
    for weight_decay 0 / 1e-2, decoupled on / off and steps 1 / 7: param, exp_avg, exp_avg_sq and shadow of the fused entries
    torch.equal; their gradient keeps what it held; the splits == 2 entry and the plain entry get their gradient, keep their
    param / moments, and are reported unfused."""
    from mask_bev_amd import ops
    gx = _operands(dt, device)
    base = _Arena(ENTRIES, shadow_kind, device)
    block = torch.zeros(16, dtype=torch.float32, device=device)
    fused_idx = [i for i, f in enumerate(EXPECT_FUSED) if f]
    for wd in (0.0, 1e-2):
        for decoupled in (1, 0):
            for step in (1, 7):
                hp = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=wd, decoupled=decoupled)
                ref, got = base.clone(), base.clone()
                ops.gemm16_tn_group([(g, x, ref.dw(i)) for i, (g, x) in enumerate(gx)])
                for i in fused_idx:
                    ref.adamw(i, hp, step)
                for i in fused_idx:
                    got.dw(i).fill_(7.0)                 # a fused entry neither reads nor writes its gradient
                _write_block(block, hp, step, shadow_kind)
                flags = ops.gemm16_tn_group([(g, x, got.dw(i)) for i, (g, x) in enumerate(gx)],
                                            [block.data_ptr() if a else 0 for a in ARMED], got.as_optimizer())
                assert flags == EXPECT_FUSED
                tag = f'wd {wd} decoupled {decoupled} step {step}'
                for name in ('param', 'exp_avg', 'exp_avg_sq', 'shadow'):
                    assert torch.equal(getattr(got, name), getattr(ref, name)), f'{name}: {tag}'
                for i, (m, n, k) in enumerate(ENTRIES):
                    o = base.offsets[i]
                    if EXPECT_FUSED[i]:
                        assert bool((got.dw(i) == 7.0).all()), f'gradient of fused entry {i} touched: {tag}'
                        assert not torch.equal(got.param[o:o + n * k], base.param[o:o + n * k])
                    else:
                        assert torch.equal(got.dw(i), ref.dw(i)) and float(got.dw(i).abs().max()) > 0
                        for name in ('param', 'exp_avg', 'exp_avg_sq', 'shadow'):
                            assert torch.equal(getattr(got, name)[o:o + n * k], getattr(base, name)[o:o + n * k]), (name, i, tag)


def test_old_entry_and_null_blocks_stay_plain(device):
    """mbv_gemm16_tn_group_adam with no block anywhere is mbv_gemm16_tn_group; a destination outside the arena or off the
    8-element grid is refused, nothing launched."""
    from mask_bev_amd import _lib, ops
    gx = _operands(torch.bfloat16, device)
    a, b = _Arena(ENTRIES, BF16, device), _Arena(ENTRIES, BF16, device)
    ops.gemm16_tn_group([(g, x, a.dw(i)) for i, (g, x) in enumerate(gx)])
    assert ops.gemm16_tn_group([(g, x, b.dw(i)) for i, (g, x) in enumerate(gx)], [0] * 4, b.as_optimizer()) == [False] * 4
    assert torch.equal(a.grad, b.grad) and torch.equal(a.param, b.param)
    block = torch.zeros(16, dtype=torch.float32, device=device)
    _write_block(block, dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=1), 1, BF16)
    g, x = gx[3]
    outside = torch.zeros(128, 128, dtype=torch.float32, device=device)
    before = b.param.clone()
    with pytest.raises(_lib.MaskBevHipError):
        ops.gemm16_tn_group([(g, x, outside)], [block.data_ptr()], b.as_optimizer())
    torch.cuda.synchronize()
    assert torch.equal(b.param, before)


def test_replay_follows_hyper_parameters_written_before_it(device):
    """One fused launch captured in a graph, replayed three times with mbv_adam_args_write(another lr, the next step) in front
    of each replay, against three eager rounds of product + mbv_adamw_step with the same hyper-parameters: bit for bit.  Fails
    if the learning rate or a bias correction were baked in at capture."""
    from mask_bev_amd import ops
    dt, kind = torch.bfloat16, BF16
    gx = _operands(dt, device)
    ref, got = _Arena(ENTRIES, kind, device), _Arena(ENTRIES, kind, device)
    block = torch.zeros(16, dtype=torch.float32, device=device)
    hps = [dict(lr=lr, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, decoupled=1) for lr in (3e-3, 1e-3, 7e-4)]
    fused_idx = [i for i, f in enumerate(EXPECT_FUSED) if f]
    items = [(g, x, got.dw(i)) for i, (g, x) in enumerate(gx)]
    blocks = [block.data_ptr() if a else 0 for a in ARMED]
    _write_block(block, hps[0], 1, kind)
    ops.gemm16_tn_group(items, [0] * 4, got.as_optimizer())        # workspace of the split entry allocated before capture
    got.grad.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        flags = ops.gemm16_tn_group(items, blocks, got.as_optimizer())
    assert flags == EXPECT_FUSED
    for step, hp in enumerate(hps, start=1):
        _write_block(block, hp, step, kind)
        graph.replay()
        ref.grad.zero_()
        ops.gemm16_tn_group([(g, x, ref.dw(i)) for i, (g, x) in enumerate(gx)])
        for i in fused_idx:
            ref.adamw(i, hp, step)
    torch.cuda.synchronize()
    for name in ('param', 'exp_avg', 'exp_avg_sq', 'shadow'):
        assert torch.equal(getattr(got, name), getattr(ref, name)), name
    for i in fused_idx:
        assert float(got.dw(i).abs().max()) == 0.0


def test_adamw_over_many_short_ranges_equals_one_launch_per_range(device):
    """mbv_adamw_step_ranges (what FlatAdam._launch issues for the short runs the fused matrices leave between them) against
    mbv_adamw_step per range: 70 ranges (two launches of 64), lengths from 4 elements to three blocks' worth, bit for bit;
    the elements between the ranges are untouched; an overflowed step (skip flag) only clears the ranges' gradient."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    lens = [4, 64, 4096, 4100, 3 * 4096 + 8] + [64 * (1 + i % 5) for i in range(65)]
    ranges, off = [], 8
    for ln in lens:
        ranges.append((off, ln))
        off += ln + 4 * (len(ranges) % 3)                 # gaps of 0 / 4 / 8 elements
    n = off + 8
    mk = lambda seed, scale=1.0: _rand((n,), torch.float32, seed, device, scale)
    hp = dict(lr=2e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)

    def state():
        return dict(param=mk(1), grad=mk(2, 0.1), m=mk(3, 0.1), v=mk(4, 0.1).square(), shadow=mk(1).to(torch.bfloat16))

    def call(fn, st, *mid, skip=None):
        _lib.check(fn(st['param'].data_ptr() + mid[0] * 4, st['grad'].data_ptr() + mid[0] * 4, st['m'].data_ptr() + mid[0] * 4,
                      st['v'].data_ptr() + mid[0] * 4, st['shadow'].data_ptr() + mid[0] * 2, BF16, *mid[1:], hp['lr'], hp['b1'],
                      hp['b2'], hp['eps'], hp['wd'], 3, 1.0, 1, 1, None, None if skip is None else skip.data_ptr(), None,
                      _stream()), 'adamw')

    LA = ctypes.c_int64 * len(ranges)
    for skip in (None, torch.ones(1, dtype=torch.int32, device=device)):
        ref, got, base = state(), state(), state()
        for a, ln in ranges:
            call(lib.mbv_adamw_step, ref, a, ln, skip=skip)
        call(lib.mbv_adamw_step_ranges, got, 0, n, LA(*[a for a, _ in ranges]), LA(*[ln for _, ln in ranges]), len(ranges),
             skip=skip)
        torch.cuda.synchronize()
        for k in ref:
            assert torch.equal(ref[k], got[k]), (k, skip is not None)
        inside = torch.zeros(n, dtype=torch.bool, device=device)
        for a, ln in ranges:
            inside[a:a + ln] = True
        assert torch.equal(got['param'][~inside], base['param'][~inside]) and torch.equal(got['grad'][~inside], base['grad'][~inside])
        assert float(got['grad'][inside].abs().max()) == 0.0
        assert torch.equal(got['param'], base['param']) == (skip is not None)
    with pytest.raises(_lib.MaskBevHipError):                 # a range that leaves the arena is refused, nothing launched
        call(lib.mbv_adamw_step_ranges, got, 0, n, LA(*([n - 4] * len(ranges))), LA(*([8] * len(ranges))), len(ranges))


# ---- optimizer ------------------------------------------------------------------------------------------------------------
class _Two(nn.Module):
    """Two Linears (no biases: their column sums end in f32 atomics, whose order is free) around a per-channel scale that
    autograd differentiates — a parameter the fused path never touches."""

    def __init__(self):
        super().__init__()
        self.a = nn.Linear(64, 128, bias=False)
        self.scale = nn.Parameter(torch.ones(128))
        self.b = nn.Linear(128, 64, bias=False)


def _two_step(m, x):
    from mask_bev_amd import ops
    with torch.autocast('cuda', dtype=torch.bfloat16):
        h = ops.linear(x, m.a.weight) * m.scale.to(torch.bfloat16)
        y = ops.linear(h, m.b.weight)
    return y.float().square().mean()


def _two(device, **opt_kw):
    from mask_bev_amd.arena import FlatAdam, ParameterArena
    torch.manual_seed(5)
    m = _Two().to(device)
    arena = ParameterArena([('all', m)], shadow_dtype=torch.bfloat16)
    opt = FlatAdam(arena, [dict(segment='all')], lr=2e-3, weight_decay=1e-2, **opt_kw)
    return m, arena, opt


def test_armed_optimizer_equals_unarmed_bit_for_bit(device):
    """Three steps of a two-Linear arena (bf16 activations, 256 tokens) with FlatAdam.fuse_matrices armed against the plain
    optimizer: parameters, moments, shadow and the step count agree exactly; the armed gradient ranges stay zero."""
    x = _rand((256, 64), torch.bfloat16, 1, device)
    out = []
    for armed in (False, True):
        m, arena, opt = _two(device)
        assert opt.fuse_matrices([m.a.weight, m.b.weight] if armed else None) == armed
        off = {id(p): o for p, o in arena.layout}
        for it in range(3):
            opt.param_groups[0]['lr'] = 2e-3 / (it + 1)            # a schedule: the block is rewritten every pass
            loss = _two_step(m, x)
            loss.backward()
            if armed:
                for w in (m.a.weight, m.b.weight):
                    o = off[id(w)]
                    assert float(arena.grad[o:o + w.numel()].abs().max()) == 0.0
                assert float(m.scale.grad.abs().max()) > 0
            opt.step()
            assert float(arena.grad.abs().max()) == 0.0
        torch.cuda.synchronize()
        out.append((arena.param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), arena.shadow.clone(),
                    opt.state_dict()['flat_state']['steps'], float(loss.detach())))
        opt.fuse_matrices(None)
        assert not hasattr(m.a.weight.grad, '_mbv_adam')
    for a, b, name in zip(out[0][:4], out[1][:4], ('param', 'exp_avg', 'exp_avg_sq', 'shadow')):
        assert torch.equal(a, b), name
    assert out[0][4] == out[1][4] == 3 and out[0][5] == out[1][5]
    assert not torch.equal(out[1][0], _two(device)[1].param)       # ... and they moved


def test_arming_is_refused_where_the_update_cannot_be_fused(device):
    from mask_bev_amd.arena import LossScaler
    m, arena, opt = _two(device, scaler=LossScaler(device))
    assert not opt.fuse_matrices([m.a.weight, m.b.weight]) and not opt.matrices_armed
    m, arena, opt = _two(device)
    opt.grad_scale = 0.5
    assert not opt.fuse_matrices([m.a.weight, m.b.weight])
    m, arena, opt = _two(device, zero_grad=False)
    assert not opt.fuse_matrices([m.a.weight, m.b.weight])
    m, arena, opt = _two(device)                                    # armed, then a data-parallel scale: nothing is claimed
    assert opt.fuse_matrices([m.a.weight, m.b.weight])
    opt.grad_scale = 0.5
    _two_step(m, _rand((256, 64), torch.bfloat16, 1, device)).backward()
    assert float(m.a.weight.grad.abs().max()) > 0 and not opt._mx_applied


def test_a_weight_meeting_itself_in_one_pass_raises(device):
    from mask_bev_amd import ops
    from mask_bev_amd.arena import FlatAdam, ParameterArena
    torch.manual_seed(6)
    lin = nn.Linear(64, 64, bias=False).to(device)
    arena = ParameterArena([('all', lin)], shadow_dtype=torch.bfloat16)
    opt = FlatAdam(arena, [dict(segment='all')], lr=1e-3)
    assert opt.fuse_matrices([lin.weight])
    before = arena.param.clone()
    x = _rand((256, 64), torch.bfloat16, 2, device)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = ops.linear(ops.linear(x, lin.weight), lin.weight)
    with pytest.raises(Exception, match='two products for one destination'):
        y.float().square().mean().backward()
    torch.cuda.synchronize()
    assert torch.equal(arena.param, before)                         # a tied weight was not updated at all


def test_two_backward_passes_before_step_raise(device):
    m, arena, opt = _two(device)
    assert opt.fuse_matrices([m.a.weight, m.b.weight])
    x = _rand((256, 64), torch.bfloat16, 1, device)
    _two_step(m, x).backward()
    with pytest.raises(Exception, match='second weight-gradient product before step'):
        _two_step(m, x).backward()
    opt.step()
    _two_step(m, x).backward()                                      # the step re-opened the arm
    opt.step()
    torch.cuda.synchronize()


# ---- whole step -------------------------------------------------------------------------------------------------------------
def _graph_run(device, fused: bool, steps: int = 4):
    from mask_bev_amd import synthetic
    from mask_bev_amd.graph import GraphedTrainStep
    from mask_bev_amd.mask_bev_module import MaskBevModule
    with switches.override(adam_in_wgrad=fused):
        torch.manual_seed(420)
        m = MaskBevModule(**synthetic.module_kwargs('smoke_96', 2, compute_dtype='bf16')).to(device).train()
        m.log_scalars = False
        m.flatten_parameters()
        opt = m.configure_optimizers()['optimizer']
        data = [synthetic.make_batch('smoke_96', 2, 0, s, device) for s in range(2)]
        torch.manual_seed(7)
        g = GraphedTrainStep(m, opt, data[0])
        assert bool(g._mx_fused) == fused
        armed = [p for p in g._swin_matrices() if getattr(p.grad, '_mbv_adam', None) is not None]
        assert bool(armed) == fused
        losses = [float(g.step(data[i % 2])) for i in range(steps)]
        torch.cuda.synchronize()
        state = {k: v.clone() for k, v in m.state_dict().items() if v.is_floating_point()}
        g.close()
    return m, opt, g, data, armed, losses, state


def _max_diff(a, b):
    la, sa = a
    lb, sb = b
    d = max(abs(x - y) for x, y in zip(la, lb))
    return max([d] + [float((sa[k].double() - sb[k].double()).abs().max()) for k in sa])


def test_graph_step_with_the_switch_on_equals_the_switch_off(device):
    """smoke_96 through GraphedTrainStep, 4 steps, fixed seeds: off, off, on.  Losses of every step and every floating tensor of
    state_dict(): equal bit for bit if the two unfused runs are; else within twice their largest difference (the step's f32
    atomics reorder freely).  After close() an eager step runs and k_adamw moves every parameter that was armed."""
    from mask_bev_amd import _lib
    off1 = _graph_run(device, False)
    off2 = _graph_run(device, False)
    m, opt, g, data, armed, losses, state = _graph_run(device, True)
    assert armed and len(g._mx_fused) > 0
    noise = _max_diff((off1[5], off1[6]), (off2[5], off2[6]))
    d = max(_max_diff((losses, state), (o[5], o[6])) for o in (off1, off2))
    print(f'unfused vs unfused {noise:.3e}, fused vs unfused {d:.3e}, fused matrices {len(g._mx_fused)}')
    assert d <= 2.0 * noise, (d, noise)
    # close() disarmed: the graphs refuse to replay, an eager step takes the plain path for every parameter
    assert not opt.matrices_armed
    with pytest.raises(_lib.MaskBevHipError):
        g.step(data[0])
    before = [p.detach().clone() for p in armed]
    lib, calls = _lib.load(), []
    lib.hook = lambda name, fn, args: (calls.append(name), fn(*args))[1]
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.training_step(data[0], 0).backward()
            opt.step()
        torch.cuda.current_stream().wait_stream(side)
    finally:
        lib.hook = None
    torch.cuda.synchronize()
    assert 'mbv_adamw_step' in calls and 'mbv_gemm16_tn_group_adam' not in calls
    assert all(not torch.equal(p.detach(), b) for p, b in zip(armed, before))
