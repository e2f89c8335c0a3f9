"""K40 (csrc/optim_flat.hip): FlatLamb and FlatSGD over a toy arena against tests/optim_ref.py run in float64 from the same f32
inputs, under the project's f32 bar — max(4e-6, 4 x the error of the same restatement run in f32 on the CPU), measured against
the reference and never against the kernel (tests/f64_bars.py).  What is compared is the ACCUMULATED UPDATE p_k - p_0 (and both
moments, and the trust ratios), so the bar is relative to how far a parameter moved, not to its size.

The toy's parameter sizes are those at which chunking (4096), padding (64) and the per-parameter reduction can go wrong: 1, 5,
63, 64, 65, 4096, 4097, 3 * 4096 + 17, a (300, 257) matrix (19 chunks), an all-zero tensor (trust 1 on its first step), a tensor
of norm 30 (the clamp at 10 bites; the other norms stay away from 10), and a tensor whose gradient is zero in a group without
weight decay (trust 1, never moves).  Three segments, two learning rates.  The learning rates (2e-2, 5e-3) are LAMB-sized on
purpose: a parameter then moves by percents of its own size in six steps, so that the half-ulp roundings of p itself, which
every f32 implementation makes, stay well below the bar relative to the update."""
import pytest
import torch

from tests import f64_bars as B
from tests import optim_ref as R
from tests.util_cfg import random_gt, random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
MOD = 'k40'
STEPS = 6
SEGMENTS = ('encoder', 'backbone', 'head')
HP = dict(encoder=dict(lr=2e-2, weight_decay=0.01), backbone=dict(lr=2e-2, weight_decay=0.01),
          head=dict(lr=5e-3, weight_decay=0.0))
ZERO_PARAM, CLAMPED, ZERO_GRAD = ('backbone', 3), ('head', 1), ('head', 2)


def _initial():
    g = torch.Generator().manual_seed(40)
    rnd = lambda *s: torch.randn(*s, generator=g)
    big = rnd(500)
    return dict(encoder=[rnd(1), rnd(5), rnd(63), rnd(64), rnd(65)],
                backbone=[rnd(4096) * 0.02, rnd(4097) * 0.02, rnd(3 * 4096 + 17) * 0.02, torch.zeros(100)],
                head=[rnd(300, 257) * 0.01, big / big.norm() * 30.0, rnd(70)])


def _gradients(steps=STEPS):
    g = torch.Generator(device='cpu').manual_seed(5)
    return [{s: [torch.zeros_like(t) if (s, i) == ZERO_GRAD else torch.randn(t.shape, generator=g) * 0.3
                 for i, t in enumerate(ts)] for s, ts in _initial().items()} for _ in range(steps)]


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


def _toy(device, shadow=torch.bfloat16):
    from mask_bev_amd.arena import ParameterArena
    toy = _Toy().to(device)
    arena = ParameterArena([(s, getattr(toy, s)) for s in SEGMENTS], shadow_dtype=shadow)
    assert arena.intact()
    return toy, arena


def _lamb(arena, **kw):
    from mask_bev_amd.arena import FlatLamb
    return FlatLamb(arena, [dict(segment=s, **HP[s]) for s in SEGMENTS], **kw)


def _feed(toy, grads, scale=1.0):
    for (s, i), q in toy.named():
        q.grad.copy_((grads[s][i] * scale).to(q.device))


def _lr_at(step, seg):
    """The schedule of the main LAMB run: from step 4 on the head's lr is a tenth (what ReduceLROnPlateau does), from step 5 on
    the backbone's differs from the encoder's (their shared launch splits)."""
    lr = HP[seg]['lr']
    if seg == 'head' and step >= 4:
        lr *= 0.1
    if seg == 'backbone' and step >= 5:
        lr *= 0.5
    return lr


_REF = {}


def _lamb_ref(dtype, debias=False, schedule=True, grad_mul=1.0, steps=STEPS):
    """optim_ref.lamb_step over the toy on the CPU at ``dtype``: per step {key: (p, m, v, trust)}.  Computed once per setting."""
    key = ('lamb', dtype, debias, schedule, grad_mul, steps)
    if key not in _REF:
        grads = _gradients(steps)
        state = {(s, i): (t.to(dtype), torch.zeros_like(t, dtype=dtype), torch.zeros_like(t, dtype=dtype))
                 for s, ts in _initial().items() for i, t in enumerate(ts)}
        out = []
        for step in range(1, steps + 1):
            cur = {}
            for (s, i), (p, m, v) in state.items():
                g = (grads[step - 1][s][i] * grad_mul).to(dtype)
                lr = _lr_at(step, s) if schedule else HP[s]['lr']
                p, m, v, trust, _ = R.lamb_step(p, g, m, v, step, lr, weight_decay=HP[s]['weight_decay'], debias=debias)
                state[(s, i)] = (p, m, v)
                cur[(s, i)] = (p, m, v, trust)
            out.append(cur)
        _REF[key] = out
    return _REF[key]


def _sgd_ref(dtype, grad_mul=1.0, steps=STEPS, lr=1e-2, wd=1e-3):
    key = ('sgd', dtype, grad_mul, steps)
    if key not in _REF:
        grads = _gradients(steps)
        state = {(s, i): (t.to(dtype), None) for s, ts in _initial().items() for i, t in enumerate(ts)}
        out = []
        for step in range(steps):
            for (s, i), (p, buf) in state.items():
                state[(s, i)] = R.sgd_step(p, (grads[step][s][i] * grad_mul).to(dtype), buf, lr, momentum=0.99,
                                           weight_decay=wd, nesterov=True)
            out.append(dict(state))
        _REF[key] = out
    return _REF[key]


def _cmp(capsys, bad, tag, got, ref32, ref64):
    """err(got, ref64) under f32_bar(ref32, ref64); a reference that is zero everywhere demands exact zeros."""
    if float(ref64.abs().max()) == 0.0:
        if float(got.abs().max()) != 0.0:
            bad.append(f'{tag}: expected exact zeros')
        return
    B.check(capsys, MOD, tag, B.err(got, ref64), B.f32_bar(ref32, ref64), bad)


def _padding_mask(arena):
    pad = torch.ones(arena.numel, dtype=torch.bool, device=arena.device)
    for p, o in arena.layout:
        pad[o:o + p.numel()] = False
    return pad


def _assert_padding_zero(arena, *buffers):
    pad = _padding_mask(arena)
    assert int(pad.sum()) > 0
    for b in (arena.param, arena.grad, arena.shadow) + buffers:
        assert float(b[pad].float().abs().max()) == 0.0


def _flat_of(arena, flat, q):
    o = next(o for p, o in arena.layout if p is q)
    return flat[o:o + q.numel()].view(q.shape)


@pytest.mark.parametrize('shadow', [torch.bfloat16, torch.float16])
def test_flat_lamb_matches_float64(device, capsys, shadow):
    toy, arena = _toy(device, shadow)
    opt = _lamb(arena)
    assert opt.zero_grad_in_step is True and opt.grad_scale == 1.0 and not hasattr(opt, 'fuse_layernorm_affine')
    assert opt.trust_ratio.shape == (len(arena.layout),) and opt.trust_ratio.dtype == torch.float32
    keys = [k for k, _ in toy.named()]
    p0 = {k: q.detach().clone().cpu() for k, q in toy.named()}
    grads = _gradients()
    ref64, ref32 = _lamb_ref(torch.float64), _lamb_ref(torch.float32)
    bad = []
    for step in range(1, STEPS + 1):
        for pg in opt.param_groups:
            pg['lr'] = _lr_at(step, pg['segment'])
        _feed(toy, grads[step - 1])
        opt.step()
        assert float(arena.grad.abs().max()) == 0.0                       # cleared by the apply pass
        assert torch.equal(arena.shadow, arena.param.to(shadow))           # shadow = RNE 16-bit of the new value
        trust = opt.trust_ratio.cpu()
        for n, (k, q) in enumerate(toy.named()):
            r64, r32 = ref64[step - 1][k], ref32[step - 1][k]
            tag = f'{B.NAME[shadow]} step {step} {k[0]}[{k[1]}] {tuple(q.shape)}'
            _cmp(capsys, bad, tag + ' update', q.detach().cpu().double() - p0[k].double(), r32[0] - p0[k], r64[0] - p0[k].double())
            _cmp(capsys, bad, tag + ' exp_avg', _flat_of(arena, opt.exp_avg, q), r32[1], r64[1])
            _cmp(capsys, bad, tag + ' exp_avg_sq', _flat_of(arena, opt.exp_avg_sq, q), r32[2], r64[2])
            _cmp(capsys, bad, tag + ' trust', trust[n:n + 1], torch.tensor([r32[3]]), torch.tensor([r64[3]], dtype=torch.float64))
            assert torch.equal(q._mbv_shadow, q.detach().to(shadow))
        # branches: exact ones, and the clamp
        n_of = {k: n for n, k in enumerate(keys)}
        assert float(trust[n_of[ZERO_GRAD]]) == 1.0
        if step == 1:
            assert float(trust[n_of[ZERO_PARAM]]) == 1.0
        assert float(ref64[step - 1][CLAMPED][0].norm()) > 20.0            # the clamp at 10 bites (its ratio: the next test)
    assert torch.equal(dict(toy.named())[ZERO_GRAD].detach().cpu(), p0[ZERO_GRAD])
    _assert_padding_zero(arena, opt.exp_avg, opt.exp_avg_sq)
    assert not bad, bad


def test_flat_lamb_clamp_and_debias(device, capsys):
    """The clamped parameter's ratio is 10 / ||u|| (||u|| from the float64 reference); debias=True follows the reference."""
    toy, arena = _toy(device)
    opt = _lamb(arena, debias=True)
    p0 = {k: q.detach().clone().cpu() for k, q in toy.named()}
    grads = _gradients(3)
    ref64 = _lamb_ref(torch.float64, debias=True, schedule=False, steps=3)
    ref32 = _lamb_ref(torch.float32, debias=True, schedule=False, steps=3)
    bad = []
    keys = [k for k, _ in toy.named()]
    for step in range(1, 4):
        _feed(toy, grads[step - 1])
        opt.step()
        for n, (k, q) in enumerate(toy.named()):
            r64, r32 = ref64[step - 1][k], ref32[step - 1][k]
            _cmp(capsys, bad, f'debias step {step} {k} update', q.detach().cpu().double() - p0[k].double(), r32[0] - p0[k],
                 r64[0] - p0[k].double())
    # 10 / un, un recomputed from the float64 state of the last step
    prev, g = ref64[1][CLAMPED], grads[2][CLAMPED[0]][CLAMPED[1]].double()
    prev32 = ref32[1][CLAMPED]
    u64 = R.lamb_step(prev[0], g, prev[1], prev[2], 3, HP['head']['lr'], debias=True)[4]
    u32 = R.lamb_step(prev32[0], g.float(), prev32[1], prev32[2], 3, HP['head']['lr'], debias=True)[4]
    assert float(prev[0].norm()) > 10.0
    got = opt.trust_ratio[keys.index(CLAMPED)].cpu().view(1)
    _cmp(capsys, bad, 'clamped trust = 10 / un', got, 10.0 / u32.norm().view(1), 10.0 / u64.norm().view(1))
    assert not bad, bad


def _state(arena, opt):
    return [arena.param.clone(), arena.shadow.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.trust_ratio.clone()]


def test_flat_lamb_is_reproducible_and_replays_from_a_graph(device):
    """Equal state + equal gradients -> equal bits (no float atomics anywhere), eager against eager and eager against a
    captured step replayed from a graph (captured on a private side stream after one warm-up step, as GraphedTrainStep does)."""
    grads = _gradients(3)
    runs = []
    for _ in range(2):
        toy, arena = _toy(device)
        opt = _lamb(arena)
        for step in range(3):
            _feed(toy, grads[step])
            opt.step()
        torch.cuda.synchronize()
        runs.append(_state(arena, opt))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    toy, arena = _toy(device)
    opt = _lamb(arena)
    side = torch.cuda.Stream(device=device)
    _feed(toy, grads[0])
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                                        # warm-up = step 1
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for step in (1, 2):
        _feed(toy, grads[step])
        graph.replay()
    torch.cuda.synchronize()
    assert float(arena.grad.abs().max()) == 0.0
    for a, b, name in zip(runs[0], _state(arena, opt), ('param', 'shadow', 'exp_avg', 'exp_avg_sq', 'trust_ratio')):
        assert torch.equal(a, b), name


def test_flat_lamb_loss_scaler_and_grad_scale(device, capsys):
    """fp16 loss scaling (the scale is a power of two, so un-scaling is exact and a clean scaled step must equal the unscaled one
    BIT FOR BIT): an overflowed step changes nothing but the gradient (cleared) and the scale (halved) and does not count; the
    clean step after it is step 1 of an unscaled optimizer, which is itself held to the float64 reference.  debias=True makes
    the step count matter (read on the device from LossScaler.applied_steps).  grad_scale = 0.25 equals feeding g / 4."""
    from mask_bev_amd.arena import LossScaler
    grads = _gradients(2)
    toy, arena = _toy(device)
    sc = LossScaler(device)
    opt = _lamb(arena, debias=True, scaler=sc)
    twin_toy, twin_arena = _toy(device)
    twin = _lamb(twin_arena, debias=True)
    before = _state(arena, opt)[:4]
    _feed(toy, grads[0], scale=65536.0)
    dict(toy.named())[('backbone', 1)].grad.view(-1)[4096] = float('inf')      # the lone element of the second chunk
    opt.step()
    torch.cuda.synchronize()
    for a, b, name in zip(before, _state(arena, opt)[:4], ('param', 'shadow', 'exp_avg', 'exp_avg_sq')):
        assert torch.equal(a, b), name
    assert float(arena.grad.abs().max()) == 0.0
    assert sc.get_scale() == 32768.0 and int(sc.applied_steps.item()) == 0
    # clean steps at the halved scale == unscaled steps
    bad = []
    p0 = {k: q.detach().clone().cpu() for k, q in twin_toy.named()}
    ref64 = _lamb_ref(torch.float64, debias=True, schedule=False, steps=3)
    ref32 = _lamb_ref(torch.float32, debias=True, schedule=False, steps=3)
    for step in range(2):
        _feed(toy, grads[step], scale=32768.0)
        _feed(twin_toy, grads[step])
        opt.step()
        twin.step()
        for a, b, name in zip(_state(arena, opt), _state(twin_arena, twin), ('param', 'shadow', 'exp_avg', 'exp_avg_sq', 'trust')):
            assert torch.equal(a, b), (step, name)
        for k, q in twin_toy.named():
            _cmp(capsys, bad, f'scaled step {step + 1} {k} update', q.detach().cpu().double() - p0[k].double(),
                 ref32[step][k][0] - p0[k], ref64[step][k][0] - p0[k].double())
    assert int(sc.applied_steps.item()) == 2 and opt.state_dict()['flat_state']['steps'] == 2
    assert opt.state_dict()['flat_state']['kind'] == 'lamb'
    # data-parallel mean folded into the kernel
    toy, arena = _toy(device)
    opt = _lamb(arena)
    opt.grad_scale = 0.25
    twin_toy, twin_arena = _toy(device)
    twin = _lamb(twin_arena)
    _feed(toy, grads[0])
    _feed(twin_toy, grads[0], scale=0.25)
    opt.step()
    twin.step()
    for a, b in zip(_state(arena, opt), _state(twin_arena, twin)):
        assert torch.equal(a, b)
    r64 = _lamb_ref(torch.float64, schedule=False, grad_mul=0.25, steps=1)[0]
    r32 = _lamb_ref(torch.float32, schedule=False, grad_mul=0.25, steps=1)[0]
    for k, q in toy.named():
        _cmp(capsys, bad, f'grad_scale 0.25 {k} update', q.detach().cpu().double() - p0[k].double(), r32[k][0] - p0[k],
             r64[k][0] - p0[k].double())
    assert not bad, bad


def test_flat_lamb_state_dict_round_trip_and_per_parameter_state(device):
    from mask_bev_amd.optimizers import Lamb
    grads = _gradients(2)
    toy, arena = _toy(device)
    opt = _lamb(arena)
    _feed(toy, grads[0])
    opt.step()
    sd = opt.state_dict()
    assert set(sd['flat_state']) == {'exp_avg', 'exp_avg_sq', 'steps', 'kind'} and sd['flat_state']['steps'] == 1
    toy2, arena2 = _toy(device)
    opt2 = _lamb(arena2)
    opt2.load_state_dict(sd)
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq) and opt2.steps == 1
    # a per-tensor Lamb's state maps through the layout
    plain = _Toy().to(device)
    per = Lamb([p for _, p in plain.named()], lr=1e-2)
    for (s, i), p in plain.named():
        p.grad = grads[0][s][i].to(device)
    per.step()
    opt3 = _lamb(_toy(device)[1])
    opt3.load_state_dict(per.state_dict())
    assert opt3.steps == 1
    for (k, p), (p3, o) in zip(plain.named(), opt3.arena.layout):
        assert torch.equal(opt3.exp_avg[o:o + p.numel()].view(p.shape), per.state[p]['exp_avg'])
        assert torch.equal(opt3.exp_avg_sq[o:o + p.numel()].view(p.shape), per.state[p]['exp_avg_sq'])


@pytest.mark.parametrize('shadow', [torch.bfloat16, torch.float16])
def test_flat_sgd_matches_torch_and_float64(device, capsys, shadow):
    from mask_bev_amd.arena import FlatSGD
    toy, arena = _toy(device, shadow)
    opt = FlatSGD(arena, lr=1e-2, weight_decay=1e-3)
    assert opt.zero_grad_in_step is True and opt.grad_scale == 1.0 and not hasattr(opt, 'fuse_layernorm_affine')
    assert len(opt.param_groups) == 1 and opt.param_groups[0]['momentum'] == 0.99 and opt.param_groups[0]['nesterov'] is True
    plain = _Toy().to(device)
    topt = torch.optim.SGD([p for _, p in plain.named()], lr=1e-2, momentum=0.99, nesterov=True, weight_decay=1e-3)
    p0 = {k: q.detach().clone().cpu() for k, q in toy.named()}
    grads = _gradients()
    ref64, ref32 = _sgd_ref(torch.float64), _sgd_ref(torch.float32)
    bad = []
    for step in range(STEPS):
        _feed(toy, grads[step])
        for (s, i), p in plain.named():
            p.grad = grads[step][s][i].to(device)
        opt.step()
        topt.step()
        assert float(arena.grad.abs().max()) == 0.0
        assert torch.equal(arena.shadow, arena.param.to(shadow))
        for (k, q), (_, p) in zip(toy.named(), plain.named()):
            assert torch.allclose(p, q, rtol=2e-6, atol=2e-7), (step, k, float((p - q).abs().max()))
            tag = f'sgd {B.NAME[shadow]} step {step + 1} {k[0]}[{k[1]}]'
            _cmp(capsys, bad, tag + ' update', q.detach().cpu().double() - p0[k].double(), ref32[step][k][0] - p0[k],
                 ref64[step][k][0] - p0[k].double())
            _cmp(capsys, bad, tag + ' buffer', _flat_of(arena, opt.momentum_buffer, q), ref32[step][k][1], ref64[step][k][1])
    _assert_padding_zero(arena, opt.momentum_buffer)
    assert not bad, bad
    # state: own format, and a torch.optim.SGD state through the layout
    sd = opt.state_dict()
    assert set(sd['flat_state']) == {'momentum_buffer', 'kind'} and sd['flat_state']['kind'] == 'sgd'
    opt2 = FlatSGD(_toy(device)[1], lr=1e-2)
    opt2.load_state_dict(topt.state_dict())
    for (_, p), (q, o) in zip(plain.named(), opt2.arena.layout):
        assert torch.equal(opt2.momentum_buffer[o:o + p.numel()].view(p.shape), topt.state[p]['momentum_buffer'])


def test_flat_sgd_loss_scaler_and_grad_scale(device):
    from mask_bev_amd.arena import FlatSGD, LossScaler
    grads = _gradients(2)
    toy, arena = _toy(device)
    sc = LossScaler(device)
    opt = FlatSGD(arena, lr=1e-2, weight_decay=1e-3, scaler=sc)
    twin_toy, twin_arena = _toy(device)
    twin = FlatSGD(twin_arena, lr=1e-2, weight_decay=1e-3)
    state = lambda ar, o: [ar.param.clone(), ar.shadow.clone(), o.momentum_buffer.clone()]
    before = state(arena, opt)
    _feed(toy, grads[0], scale=65536.0)
    dict(toy.named())[('head', 0)].grad.view(-1)[77000] = float('nan')
    opt.step()
    torch.cuda.synchronize()
    for a, b in zip(before, state(arena, opt)):
        assert torch.equal(a, b)
    assert float(arena.grad.abs().max()) == 0.0 and sc.get_scale() == 32768.0 and int(sc.applied_steps.item()) == 0
    for step in range(2):
        _feed(toy, grads[step], scale=32768.0)
        _feed(twin_toy, grads[step])
        opt.step()
        twin.step()
        for a, b in zip(state(arena, opt), state(twin_arena, twin)):
            assert torch.equal(a, b)
    toy, arena = _toy(device)
    opt = FlatSGD(arena, lr=1e-2, weight_decay=1e-3)
    opt.grad_scale = 0.25
    twin_toy, twin_arena = _toy(device)
    twin = FlatSGD(twin_arena, lr=1e-2, weight_decay=1e-3)
    _feed(toy, grads[0])
    _feed(twin_toy, grads[0], scale=0.25)
    opt.step()
    twin.step()
    for a, b in zip(state(arena, opt), state(twin_arena, twin)):
        assert torch.equal(a, b)
    # zero_grad=False leaves the gradient for the caller
    toy, arena = _toy(device)
    opt = FlatSGD(arena, lr=1e-2, zero_grad=False)
    _feed(toy, grads[0])
    g0 = arena.grad.clone()
    opt.step()
    assert torch.equal(arena.grad, g0)
    opt.zero_grad()
    assert float(arena.grad.abs().max()) == 0.0


def test_k40_entry_points_refuse_bad_arguments(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    toy, arena = _toy(device)
    opt = _lamb(arena)
    st = torch.cuda.current_stream().cuda_stream
    P, G, M, V = arena.param.data_ptr(), arena.grad.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr()
    C, S, T, PC = opt._chunks.data_ptr(), opt._partials.data_ptr(), opt.trust_ratio.data_ptr(), opt._param_chunks.data_ptr()
    nc, npar, n = opt.n_chunks, opt.n_params, arena.numel
    mom = lambda **k: lib.mbv_lamb_moments(k.get('p', P), G, M, V, n, k.get('c', C), nc, k.get('c0', 0), k.get('c1', nc), S,
                                           0.9, 0.999, 1e-6, 0.0, 1.0, 0, 0, st)
    app = lambda **k: lib.mbv_lamb_apply(k.get('p', P), G, k.get('sh', arena.shadow.data_ptr()), k.get('dt', 1), n, C, nc,
                                         k.get('c0', 0), k.get('c1', nc), T, npar, 1e-3, 0.9, 0.999, 0, k.get('step', 1), 0, 0, st)
    sgd = lambda **k: lib.mbv_sgd_step(k.get('p', P), G, M, k.get('sh', arena.shadow.data_ptr()), k.get('dt', 1), k.get('n', n),
                                       1e-3, 0.99, 0.0, 0.0, 1, 1.0, 1, 0, 0, st)
    BAD = -1
    assert mom(p=0) == BAD and mom(p=P + 4) == BAD and mom(c=0) == BAD and mom(c0=2, c1=1) == BAD and mom(c1=nc + 1) == BAD
    assert mom(c0=-1) == BAD and mom(c0=3, c1=3) == 0
    assert app(p=0) == BAD and app(p=P + 4) == BAD and app(dt=0) == BAD and app(dt=3) == BAD and app(c0=2, c1=1) == BAD
    assert app(sh=arena.shadow.data_ptr() + 2) == BAD and app(step=0) == BAD and app(c0=3, c1=3) == 0
    assert lib.mbv_lamb_trust(0, nc, PC, npar, 10.0, T, st) == BAD and lib.mbv_lamb_trust(S, nc, 0, npar, 10.0, T, st) == BAD
    assert lib.mbv_lamb_trust(S, nc, PC, -1, 10.0, T, st) == BAD and lib.mbv_lamb_trust(S, nc, PC, 0, 10.0, T, st) == 0
    assert sgd(p=0) == BAD and sgd(p=P + 4) == BAD and sgd(dt=0) == BAD and sgd(n=-1) == BAD and sgd(n=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(arena.param, _toy(device)[1].param)               # nothing ran


def test_flat_optimizers_refuse_frozen_parameters_and_cpu_arenas(device):
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.arena import FlatLamb, FlatSGD, ParameterArena
    toy, arena = _toy(device)
    next(toy.encoder.parameters()).requires_grad_(False)
    with pytest.raises(ValueError, match='frozen'):
        _lamb(arena)
    with pytest.raises(ValueError, match='frozen'):
        FlatSGD(arena)
    cpu = _Toy()
    cpu_arena = ParameterArena([(s, getattr(cpu, s)) for s in SEGMENTS])
    with pytest.raises(MaskBevHipError):
        FlatLamb(cpu_arena, [dict(segment=s) for s in SEGMENTS])
    with pytest.raises(MaskBevHipError):
        FlatSGD(cpu_arena)


def _adam(arena, **kw):
    from mask_bev_amd.arena import FlatAdam
    return FlatAdam(arena, [dict(segment=s, **HP[s]) for s in SEGMENTS], **kw)


def test_flat_state_carries_its_kind_and_is_refused_by_the_other_optimizers(device):
    """One checkpoint format for the three flat optimizers: each writes its own ``kind``, each refuses the other two, and a
    state without the key (what FlatAdam wrote before it existed) still loads into FlatAdam and FlatLamb."""
    from mask_bev_amd.arena import FlatSGD
    make = dict(adam=lambda: _adam(_toy(device)[1]), lamb=lambda: _lamb(_toy(device)[1]),
                sgd=lambda: FlatSGD(_toy(device)[1], lr=1e-2))
    toy, arena = _toy(device)
    stepped = _adam(arena)
    _feed(toy, _gradients(1)[0])
    stepped.step()
    sds = {k: f().state_dict() for k, f in make.items()}
    sds['adam'] = stepped.state_dict()
    for k, sd in sds.items():
        assert sd['flat_state']['kind'] == k
    assert set(sds['adam']['flat_state']) == {'exp_avg', 'exp_avg_sq', 'steps', 'kind'}
    for k, f in make.items():
        for other, sd in sds.items():
            if other != k:
                with pytest.raises(ValueError, match=f"kind '{other}' cannot be loaded into Flat"):
                    f().load_state_dict(sd)
    legacy = dict(sds['adam'], flat_state={k: v for k, v in sds['adam']['flat_state'].items() if k != 'kind'})
    assert float(stepped.exp_avg.abs().max()) > 0.0
    for k in ('adam', 'lamb'):
        opt = make[k]()
        opt.load_state_dict(legacy)
        assert torch.equal(opt.exp_avg, stepped.exp_avg) and torch.equal(opt.exp_avg_sq, stepped.exp_avg_sq)
        assert opt.steps == 1


def test_flat_adam_resumes_from_its_state_dict_bit_for_bit(device):
    """Two steps, state_dict, a fresh FlatAdam over a fresh arena holding the saved parameters, one more step == three steps
    without the interruption, in every bit of param, exp_avg, exp_avg_sq and the 16-bit shadow."""
    grads = _gradients(3)

    def run(toy, arena, opt, steps):
        for s in steps:
            _feed(toy, grads[s])
            opt.step()
        return opt

    toy_a, arena_a = _toy(device)
    a = run(toy_a, arena_a, _adam(arena_a), range(3))
    toy_b, arena_b = _toy(device)
    b = run(toy_b, arena_b, _adam(arena_b), range(2))
    toy_c, arena_c = _toy(device)
    c = _adam(arena_c)
    c.load_state_dict(b.state_dict())
    arena_c.param.copy_(arena_b.param)
    arena_c.refresh_shadow()
    assert c.steps == 2
    run(toy_c, arena_c, c, [2])
    torch.cuda.synchronize()
    for x, y, name in ((arena_a.param, arena_c.param, 'param'), (a.exp_avg, c.exp_avg, 'exp_avg'),
                       (a.exp_avg_sq, c.exp_avg_sq, 'exp_avg_sq'), (arena_a.shadow, arena_c.shadow, 'shadow')):
        assert torch.equal(x, y), name
    assert float((arena_a.param - _toy(device)[1].param).abs().max()) > 0.0


@pytest.mark.parametrize('entry', ['adamw', 'sgd'])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, 2051])
def test_streaming_helpers_at_vector_and_tail_boundaries(device, entry, n):
    """mbv_adamw_step / mbv_sgd_step through the C ABI at the sizes where the shared streaming frame can go wrong: below one
    float4 (1, 3), exactly one (4), one plus a tail (5), a full block of vectors plus a tail (1027) and two blocks plus a tail
    (2051).  With the overflow flag clear the result EQUALS tests/optim_ref.py's one-rounding-per-operation f32 restatement
    (the kernels pin contraction off and use correctly rounded divide / sqrt, so there is nothing to tolerate), the shadow is
    the RNE bf16 of the new parameter and the gradient is cleared; with the flag set parameters, state and shadow are
    untouched and the gradient is cleared all the same, ragged tail included."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(1000 + n)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.3
    m0, v0 = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01
    st = torch.cuda.current_stream().cuda_stream
    scale = torch.ones(1, device=device)
    if entry == 'adamw':
        hp = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
        want = R.adamw_step_unfused(p0, g0, m0, v0, 2, **hp)
        state0 = (m0, v0)
    else:
        hp = dict(lr=1e-2, momentum=0.99, weight_decay=1e-3)
        want = R.sgd_step_unfused(p0, g0, m0, nesterov=True, **hp)
        state0 = (m0,)
    for skip in (1, 0):
        p, g = p0.to(device), g0.to(device)
        state = [s.to(device) for s in state0]
        shadow = torch.full((n,), 7.0, dtype=torch.bfloat16, device=device)
        flag = torch.full((1,), skip, dtype=torch.int32, device=device)
        if entry == 'adamw':
            rc = lib.mbv_adamw_step(p.data_ptr(), g.data_ptr(), state[0].data_ptr(), state[1].data_ptr(), shadow.data_ptr(), 1,
                                    n, hp['lr'], hp['betas'][0], hp['betas'][1], hp['eps'], hp['weight_decay'], 2, 1.0, 1, 1,
                                    scale.data_ptr(), flag.data_ptr(), 0, st)
        else:
            rc = lib.mbv_sgd_step(p.data_ptr(), g.data_ptr(), state[0].data_ptr(), shadow.data_ptr(), 1, n, hp['lr'],
                                  hp['momentum'], 0.0, hp['weight_decay'], 1, 1.0, 1, scale.data_ptr(), flag.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        assert float(g.abs().max()) == 0.0, skip
        got = [p.cpu()] + [s.cpu() for s in state]
        expect = [p0, *state0] if skip else list(want)
        for i, (x, y) in enumerate(zip(got, expect)):
            assert torch.equal(x, y), (skip, i, float((x - y).abs().max()))
        assert torch.equal(shadow.cpu(), torch.full((n,), 7.0, dtype=torch.bfloat16) if skip else want[0].to(torch.bfloat16))


@pytest.mark.parametrize('kind', ['lamb', 'sgd'])
def test_module_trains_with_flat_lamb_and_sgd(device, kind):
    """The whole module under `optimiser_type: lamb | sgd` with bf16 compute, flattened, six captured steps: the flat optimizer
    is what configure_optimizers returns, both eager- and graph-owned segments move, and the 16-bit shadow the GEMMs read follows
    the f32 masters (with torch.optim.SGD over an arena it stayed at the weights of step 0; `lamb` used to raise)."""
    from mask_bev_amd.arena import FlatLamb, FlatSGD
    from mask_bev_amd.graph import GraphedTrainStep
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(0)
    kw = dict(tiny_kwargs(nx=96, ny=96, q=8), compute_dtype='bf16', lr=5e-4, optimiser_type=kind)
    m = MaskBevModule(**kw).to(device).train()
    m.log_scalars = False
    m._panoptic_head._panoptic_head.num_points = 2000
    arena = m.flatten_parameters()
    out = m.configure_optimizers()
    opt = out['optimizer']
    assert type(opt) is (FlatLamb if kind == 'lamb' else FlatSGD)
    assert out['lr_scheduler'].optimizer is opt
    if kind == 'lamb':
        assert [pg['segment'] for pg in opt.param_groups] == ['encoder', 'backbone', 'head']
        assert all(pg['eps'] == 1e-6 for pg in opt.param_groups)
    scans = [x.to(device) for x in random_scans(kw, [3000, 2500], seed=0)]
    labels, gt = random_gt(kw, 2, 3, seed=10)
    batch = (scans, (labels.to(device), gt.to(device)))
    g = GraphedTrainStep(m, opt, batch)
    p0 = arena.param.clone()
    losses = []
    for it in range(6):
        losses.append(float(g.step(batch)))
        assert float(arena.grad.abs().max()) == 0.0
    torch.cuda.synchronize()
    assert arena.intact()
    assert all(l == l and abs(l) != float('inf') for l in losses), losses
    for seg in ('encoder', 'head'):
        a, b = arena.segments[seg]
        assert float((arena.param[a:b] - p0[a:b]).abs().max()) > 0
    w = m._backbone._backbone.stages[0].blocks[0].ffn.layers[0][0].weight
    assert not torch.equal(w, _flat_of(arena, p0, w))
    assert torch.equal(w._mbv_shadow, w.detach().to(torch.bfloat16))
    assert torch.equal(arena.shadow, arena.param.to(torch.bfloat16))
    g.close()
