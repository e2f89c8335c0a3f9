"""K18 (GroupNorm of NCHW maps + the FPN up-sampled add / ReLU / output cast, csrc/groupnorm.hip) against float64 on the paths
production takes.

The reference is torch on the CPU with autograd — F.group_norm, F.interpolate(bilinear, align_corners=False), relu — on the
inputs as their dtype holds them, in float64 (the reference) and in float32 (its error sets the bar, f64_bars.f32_bar; no bar
may exceed 1e-5); the upstream gradient is created in the output's type.  f32-stored tensors take the bar, 16-bit stored ones
may add one rounding of the type.  Compared: y, dx, d gamma, d beta, d(add); ``accumulate = 1`` into pre-filled arena gradients,
twice; the saved mean / rstd through the C ABI.  Every comparison prints ``err … bar …``.

Shapes (tests/norm_ref.py GN_CASES): at most one float4 per thread; W % 4 != 0; ``splits`` 8 in k_gn_stats with a ragged
two-load loop and ``chunks`` 2 in the apply / dx kernels; the batch sum of d gamma / d beta; one channel per group; one group.
Inputs N(0.3, 1.5²) and N(50, 1) — the variance is E[x²] − mean², summed in float64 from the first add.  ReLU cases: the seeds
leave no element within f32 rounding of a flipped gate (asserted; test_norm_ref_cpu.py asserts it without a GPU).  ReLU over
the sum with an added map is refused by the op (its backward gates on GroupNorm(x) alone); layers.ConvGN takes its torch path.
Measured: DESIGN.md §2."""
import functools

import pytest
import torch

from tests import norm_ref as R
from tests.f64_bars import LO, NAME, check, err, f32_bar
from tests.norm_ref import BF16, F32, F64

pytestmark = pytest.mark.gpu
MOD = 'k18-paths'
PARAMS = [(ci, dist, dts) for ci in range(len(R.GN_CASES)) for dist in R.GN_DISTS for dts in R.GN_DTYPES]
PIDS = [f'{R.GN_IDS[ci]}-{dist}-x_{NAME[dts[0]]}-y_{NAME[dts[1]]}' for ci, dist, dts in PARAMS]


def _bar(ref, name):
    bar = R.bar(ref[F32][name], ref[F64][name])
    assert bar <= R.BAR_CAP, (name, bar)
    return bar


def _cmp(capsys, tag, name, got, ref, bad):
    R.compare(capsys, MOD, tag, name, got, ref[F32][name], ref[F64][name], bad)


def _run(ops, device, k, add, relu, out_dt):
    x, w, bias = (t.clone().to(device).requires_grad_() for t in (k.x, k.w, k.bias))
    a = None if add is None else add.clone().to(device).requires_grad_()
    y = ops.group_norm(x, w, bias, k.groups, R.EPS, relu=relu, add_upsampled=a, out_dtype=out_dt)
    assert y.dtype == out_dt and tuple(y.shape) == k.shape
    y.backward(k.gy.to(device))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, dbias=bias.grad, dadd=None if a is None else a.grad)


@pytest.mark.parametrize('ci,dist,dts', PARAMS, ids=PIDS)
def test_group_norm_against_float64(device, capsys, ci, dist, dts):
    from mask_bev_amd import ops
    x_dt, out_dt = dts
    k = R.gn_inputs(ci, dist, x_dt, out_dt)
    lo = x_dt if x_dt in LO else BF16                      # the 16-bit type of the added map
    modes = [('plain', None, False)]
    if dist == 'n0.3':                                     # ReLU: N(0.3, 1.5²) only
        assert R.relu_band(k.x, k.w, k.bias, k.groups) == 0, 'an element within rounding of a flipped gate: pick another seed'
        modes.append(('relu', None, True))
    for kind in k.adds:
        modes += [(f'add-{kind}-{NAME[dt]}', k.adds[kind].to(dt), False) for dt in (F32, lo)]
    bad = []
    for mode, add, relu in modes:
        ref = R.gn_reference(k.x, k.w, k.bias, k.groups, k.gy, add, relu)
        got = _run(ops, device, k, add, relu, out_dt)
        for name in ('y', 'dx', 'dw', 'dbias') + (('dadd',) if add is not None else ()):
            _cmp(capsys, f'{PIDS[PARAMS.index((ci, dist, dts))]} {mode}', name, got[name], ref, bad)
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _plain_reference(ci, dist):
    k = R.gn_inputs(ci, dist, F32, F32)
    return R.gn_reference(k.x, k.w, k.bias, k.groups, k.gy)


@pytest.mark.parametrize('dist', list(R.GN_DISTS))
@pytest.mark.parametrize('ci', [0, 2, 3], ids=[R.GN_IDS[i] for i in (0, 2, 3)])
def test_group_norm_accumulates_into_arena_gradients(device, capsys, ci, dist):
    """accumulate = 1: arena-resident gamma / beta with pre-filled gradients, two backward passes add twice the gradient."""
    from mask_bev_amd import ops
    from mask_bev_amd.arena import ParameterArena
    k = R.gn_inputs(ci, dist, F32, F32)
    ref = _plain_reference(ci, dist)
    gn = torch.nn.GroupNorm(k.groups, k.shape[1]).to(device)
    with torch.no_grad():
        gn.weight.copy_(k.w)
        gn.bias.copy_(k.bias)
    ParameterArena([('gn', gn)], shadow_dtype=None)
    g = torch.Generator().manual_seed(9)
    pre = dict(dw=torch.randn(k.shape[1], generator=g), dbias=torch.randn(k.shape[1], generator=g))
    with torch.no_grad():
        gn.weight.grad.copy_(pre['dw'])
        gn.bias.grad.copy_(pre['dbias'])
    ptrs = (gn.weight.grad.data_ptr(), gn.bias.grad.data_ptr())
    bad = []
    for _ in range(2):
        x = k.x.clone().to(device).requires_grad_()
        ops.group_norm(x, gn.weight, gn.bias, k.groups, R.EPS).backward(k.gy.to(device))
    assert ptrs == (gn.weight.grad.data_ptr(), gn.bias.grad.data_ptr())            # accumulated in place
    tag = f'{R.GN_IDS[ci]}-{dist} accumulate x 2'
    for name, got in (('dw', gn.weight.grad), ('dbias', gn.bias.grad)):
        want64, want32 = pre[name].double() + 2 * ref[F64][name], (pre[name] + ref[F32][name]) + ref[F32][name]
        bar = R.bar(want32, want64)
        assert bar <= R.BAR_CAP
        check(capsys, MOD, f'{tag} {name}', err(got, want64), bar, bad)
    check(capsys, MOD, f'{tag} dx', err(x.grad, ref[F64]['dx']), _bar(ref, 'dx'), bad)
    assert not bad, bad


@pytest.mark.parametrize('dist', list(R.GN_DISTS))
@pytest.mark.parametrize('ci', [2, 4], ids=[R.GN_IDS[i] for i in (2, 4)])
def test_saved_statistics_against_float64(device, capsys, ci, dist):
    """mbv_groupnorm_fwd through the C ABI: the mean / rstd the backward reads, against float64 (bar: torch's float32
    native_group_norm on the CPU) — eight splits of a group, and a group of 96 elements."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    k = R.gn_inputs(ci, dist, F32, F32)
    b, c, h, w = k.shape
    nbytes = lib.mbv_groupnorm_workspace_bytes(b, c, k.groups, h, w)
    assert nbytes == b * k.groups * (8 if ci == 2 else 1) * 16                      # splits of k_gn_stats
    x, wt, bias = (t.to(device) for t in (k.x, k.w, k.bias))
    y = torch.full(k.shape, float('nan'), device=device)
    mean, rstd = (torch.full((b * k.groups,), float('nan'), device=device) for _ in range(2))
    ws = ops._workspace(nbytes, device)
    ops.check(lib.mbv_groupnorm_fwd(ops._ptr(x), 0, b, c, h, w, k.groups, ops._ptr(wt), ops._ptr(bias), R.EPS, None, 0, 0, 0, 0,
                                    ops._ptr(y), 0, ops._ptr(mean), ops._ptr(rstd), ops._ptr(ws), int(nbytes), ops._stream()),
              'mbv_groupnorm_fwd')
    mean64, rstd64 = R.gn_stats(k.x, k.groups)
    _, mean32, rstd32 = torch.native_group_norm(k.x, k.w, k.bias, b, c, h * w, k.groups, R.EPS)
    bad = []
    for name, got, r32, r64 in (('mean', mean, mean32.reshape(-1), mean64), ('rstd', rstd, rstd32.reshape(-1), rstd64)):
        bar = f32_bar(r32, r64)
        assert bar <= R.BAR_CAP
        check(capsys, MOD, f'{R.GN_IDS[ci]}-{dist} saved {name}', err(got, r64), bar, bad)
    ref = _plain_reference(ci, dist)
    check(capsys, MOD, f'{R.GN_IDS[ci]}-{dist} C ABI y', err(y, ref[F64]['y']), _bar(ref, 'y'), bad)
    assert not bad, bad


def test_relu_with_added_map_is_refused(device):
    """The backward rebuilds the gate from GroupNorm(x) alone, so the op refuses ReLU over the sum (C ABI: UNSUPPORTED)."""
    from mask_bev_amd import _lib, ops
    from mask_bev_amd._lib import MaskBevHipError
    lib = _lib.load()
    k = R.gn_inputs(0, 'n0.3', F32, F32)
    b, c, h, w = k.shape
    x, wt, bias, add = (t.to(device) for t in (k.x, k.w, k.bias, k.adds['half']))
    with pytest.raises(MaskBevHipError):
        ops.group_norm(x, wt, bias, k.groups, R.EPS, relu=True, add_upsampled=add)
    nbytes = lib.mbv_groupnorm_workspace_bytes(b, c, k.groups, h, w)
    ws = ops._workspace(nbytes, device)
    y, mean, rstd = torch.empty_like(x), torch.empty(b * k.groups, device=device), torch.empty(b * k.groups, device=device)
    args = [ops._ptr(x), 0, b, c, h, w, k.groups, ops._ptr(wt), ops._ptr(bias), R.EPS, ops._ptr(add), 0, h // 2, w // 2, 1,
            ops._ptr(y), 0, ops._ptr(mean), ops._ptr(rstd), ops._ptr(ws), int(nbytes), ops._stream()]
    assert lib.mbv_groupnorm_fwd(*args) == -3                                       # MBV_ERR_UNSUPPORTED
    args[14] = 0
    assert lib.mbv_groupnorm_fwd(*args) == 0                                        # either of the two alone is served


def test_conv_gn_relu_with_added_map_against_float64(device, capsys):
    """layers.ConvGN(48, 64, 1, bias=False, relu=True)(x, add_upsampled=add): the combination K18 refuses goes through the torch
    path — y and the gradients of x, the convolution weight, gamma, beta and the added map against float64."""
    from mask_bev_amd.layers import ConvGN
    k = R.conv_gn_inputs()
    ref = R.conv_gn_reference(k)
    assert R.relu_band(ref[F64]['z'], k.w, k.bias, k.groups,
                       add=torch.nn.functional.interpolate(k.add.double(), size=(24, 16), mode='bilinear', align_corners=False)) == 0
    m = ConvGN(48, 64, 1, bias=False, relu=True).to(device)
    with torch.no_grad():
        m.conv.weight.copy_(k.cw)
        m.gn.weight.copy_(k.w)
        m.gn.bias.copy_(k.bias)
    x, add = (t.clone().to(device).requires_grad_() for t in (k.x, k.add))
    y = m(x, add_upsampled=add)
    y.backward(k.gy.to(device))
    bad = []
    for name, got in (('y', y), ('dx', x.grad), ('dcw', m.conv.weight.grad), ('dw', m.gn.weight.grad),
                      ('dbias', m.gn.bias.grad), ('dadd', add.grad)):
        _cmp(capsys, 'ConvGN relu + add', name, got.detach().float(), ref, bad)
    assert not bad, bad
