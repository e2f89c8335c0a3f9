"""Case builders and CPU references shared by the float64 suites of the two normalisation kernels (test_k12_paths_gpu.py —
fused add + LayerNorm, csrc/layernorm.hip — and test_k18_paths_gpu.py — GroupNorm + FPN add, csrc/groupnorm.hip), checked
on their own by test_norm_ref_cpu.py.

Every reference is torch on the CPU with autograd — F.layer_norm / F.group_norm / F.interpolate(bilinear, align_corners=False)
/ F.unfold — on the inputs AS THEIR DTYPE HOLDS THEM, run in float64 (the reference) and in float32 (its error against float64
sets the bar, f64_bars.f32_bar); upstream gradients are created in the dtype the kernel receives."""
import functools
import math
import types

import torch
import torch.nn.functional as F

from tests.f64_bars import check, err, err_beyond_one_rounding, f32_bar

F64, F32, BF16, FP16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
EPS = 1e-5
BAR_CAP = 1e-5                        # no bar of these suites may exceed it (asserted where the bar is used)


def bar(ref32, ref64) -> float:
    """f64_bars.f32_bar, held at the cap.  The cap binds for one tensor: d gamma of GroupNorm at N(50, 1).  torch's float32 CPU
    backward forms it as (sum dy x - mean sum dy) rstd, which cancels at that offset (its own error there: 6e-6 ... 8e-5, so four
    times it would be a bar of up to 3e-4); the kernels sum dy (x - mean) rstd and are held to 1e-5 instead.  Everywhere else
    the float32 reference's error leaves the bar under the cap (test_norm_ref_cpu.py)."""
    return min(f32_bar(ref32, ref64), BAR_CAP)


def compare(capsys, mod, tag, name, got, ref32, ref64, bad):
    """One tensor against float64, printed: stored in f32 -> its error; stored in 16 bits -> what it adds beyond one rounding of
    the reference to that type.  The bar comes from the float32 reference and is asserted to respect the cap."""
    assert torch.isfinite(got).all(), f'{tag} {name}'
    b = bar(ref32, ref64)
    assert b <= BAR_CAP, (tag, name, b)
    if got.dtype == F32:
        check(capsys, mod, f'{tag} {name}', err(got, ref64), b, bad)
    else:
        check(capsys, mod, f'{tag} {name} beyond one rounding', err_beyond_one_rounding(got, ref64, got.dtype), b, bad)


def _leaf(t, dt):
    return None if t is None else t.to(dt).clone().requires_grad_()


# ------------------------------------------------------------------------------------------------------------------
# K12: y = LayerNorm_C(a + b), optionally with the sum s = a + b as a second output
# ------------------------------------------------------------------------------------------------------------------
def ln_inputs(seed, shape, a_dt=F32, b_dt=F32, offset=0.5, scale=2.0):
    """a (scale N(0,1) + offset), b (N(0,1), or None), gamma in [0.5, 1.5), beta N(0,1) and three upstream gradients (f32;
    the tests round them to what the kernel receives) — CPU tensors, the activations already in their storage type."""
    g = torch.Generator().manual_seed(seed)
    c = shape[-1]
    a = (torch.randn(shape, generator=g) * scale + offset).to(a_dt)
    b = None if b_dt is None else torch.randn(shape, generator=g).to(b_dt)
    w, bias = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    g1, g2, g3 = (torch.randn(shape, generator=g) for _ in range(3))
    return types.SimpleNamespace(a=a, b=b, w=w, bias=bias, g1=g1, g2=g2, g3=g3, shape=tuple(shape), c=c, rows=a.numel() // c)


def ln_reference(a, b, w, bias, gys=(), gs=None, b_map=None, eps=EPS):
    """{float64 | float32: dict(y, s, da, db, dw, dbias, dbranch)}.  ``gys``: the upstream gradients of y (their sum arrives:
    a LayerNorm output with two consumers), ``gs``: that of the sum (None: no such path); ``b_map``: how the leaf ``b``
    becomes the addend (the position embedding's transposed view).  ``dbranch`` = the row sum of d(a + b): the bias gradient
    of the Linear that produced the residual branch."""
    res = {}
    for dt in (F64, F32):
        al, bl, wl, biasl = (_leaf(t, dt) for t in (a, b, w, bias))
        s = al if bl is None else al + (bl if b_map is None else b_map(bl))
        y = F.layer_norm(s, (s.shape[-1],), wl, biasl, eps)
        outs, gos = [], []
        if len(gys):
            go = gys[0].to(dt)
            for t in gys[1:]:
                go = go + t.to(dt)
            outs.append(y)
            gos.append(go)
        if gs is not None:
            outs.append(s)
            gos.append(gs.to(dt))
        if outs:
            torch.autograd.backward(outs, gos)
        res[dt] = dict(y=y.detach(), s=s.detach(), da=al.grad, db=None if bl is None else bl.grad, dw=wl.grad, dbias=biasl.grad,
                       dbranch=None if al.grad is None else al.grad.reshape(-1, al.shape[-1]).sum(0))
    return res


def unfold2x2(x):
    """nn.Unfold(2, stride 2) of a channels-last map: (B, H, W, C) -> (B, H/2, W/2, 4C), channel order c*4 + kh*2 + kw."""
    b, h, w, c = x.shape
    return F.unfold(x.permute(0, 3, 1, 2), kernel_size=2, stride=2).transpose(1, 2).reshape(b, h // 2, w // 2, 4 * c)


def merge_reference(x, w, bias, gy, eps=EPS):
    """{float64 | float32: dict(y, dx, dw, dbias)} of LayerNorm_{4C}(unfold2x2(x))."""
    res = {}
    for dt in (F64, F32):
        xl, wl, biasl = (_leaf(t, dt) for t in (x, w, bias))
        y = F.layer_norm(unfold2x2(xl), (4 * x.shape[-1],), wl, biasl, eps)
        y.backward(gy.to(dt))
        res[dt] = dict(y=y.detach(), dx=xl.grad, dw=wl.grad, dbias=biasl.grad)
    return res


def pos_map(h, w, c):
    """(1, C, rows, cols) embedding -> (1, h, w, C) tokens (rows * cols == h * w, flattened row-major)."""
    return lambda ape: ape.flatten(2).transpose(1, 2).reshape(1, h, w, c)


VALUE_ROWS = dict(offset=slice(0, 16), zeros=16, half=17, tiny=slice(18, 34), big=slice(34, 50))


def ln_value_rows(seed, c, rows=64):
    """(rows, c) f32: rows at 50 ± 1, a row of zeros and a row of constant 0.5 (exact sums: y is beta), rows scaled by 2^-20
    and by 2^10, the rest N(0, 1) — all in one tensor."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(rows, c, generator=g)
    a[VALUE_ROWS['offset']] += 50.0
    a[VALUE_ROWS['zeros']] = 0.0
    a[VALUE_ROWS['half']] = 0.5
    a[VALUE_ROWS['tiny']] *= 2.0 ** -20
    a[VALUE_ROWS['big']] *= 2.0 ** 10
    return a


# ------------------------------------------------------------------------------------------------------------------
# K18: y = relu?(GroupNorm_G(x) + bilinear-upsampled add) on NCHW maps
# ------------------------------------------------------------------------------------------------------------------
# B, C, H, W, G
GN_CASES = [
    (2, 64, 16, 16, 32),       # at most one float4 per thread
    (1, 96, 10, 6, 8),         # 15 float4 per plane; W % 4 != 0: no add
    (1, 8, 92, 92, 2),         # splits 8 of 1058 float4 (ragged two-load loop + single tail); chunks 2, ragged
    (3, 32, 64, 64, 4),        # splits 8, batch sum of d gamma / d beta
    (2, 16, 8, 12, 16),        # one channel per group
    (2, 16, 8, 12, 1),         # one group
]
GN_IDS = ['x'.join(map(str, c[:4])) + f'g{c[4]}' for c in GN_CASES]
GN_DISTS = {'n0.3': (0.3, 1.5), 'n50': (50.0, 1.0)}
GN_DTYPES = [(F32, F32), (BF16, BF16), (BF16, F32), (FP16, FP16)]
GN_ADDS = ('half', 'third', 'one', 'same')
GN_SEED = 1800


def gn_add_size(kind, h, w):
    return {'half': (h // 2, w // 2), 'third': (math.ceil(h / 3), w // 4), 'one': (1, 1), 'same': (h, w)}[kind]


@functools.lru_cache(maxsize=8)
def gn_inputs(ci, dist, x_dt, out_dt):
    """x ~ N(dist) stored in x_dt, gamma in [0.5, 1.5), beta 0.5 N(0, 1), the upstream gradient in out_dt and the four coarse
    maps (f32) of the add mode."""
    b, c, h, w, groups = GN_CASES[ci]
    mu, sigma = GN_DISTS[dist]
    g = torch.Generator().manual_seed(GN_SEED + 16 * ci + list(GN_DISTS).index(dist))
    x = (torch.randn(b, c, h, w, generator=g) * sigma + mu).to(x_dt)
    wt, bias = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5
    gy = torch.randn(b, c, h, w, generator=g).to(out_dt)
    adds = {k: torch.randn((b, c) + gn_add_size(k, h, w), generator=g) for k in GN_ADDS} if w % 4 == 0 else {}
    return types.SimpleNamespace(x=x, w=wt, bias=bias, gy=gy, adds=adds, groups=groups, shape=(b, c, h, w))


def gn_reference(x, w, bias, groups, gy, add=None, relu=False, eps=EPS):
    """{float64 | float32: dict(y, dx, dw, dbias, dadd)} of relu?(GroupNorm(x) + interpolate(add))."""
    res = {}
    for dt in (F64, F32):
        xl, wl, biasl, addl = (_leaf(t, dt) for t in (x, w, bias, add))
        y = F.group_norm(xl, groups, wl, biasl, eps)
        if addl is not None:
            y = y + F.interpolate(addl, size=x.shape[-2:], mode='bilinear', align_corners=False)
        if relu:
            y = F.relu(y)
        y.backward(gy.to(dt))
        res[dt] = dict(y=y.detach(), dx=xl.grad, dw=wl.grad, dbias=biasl.grad, dadd=None if addl is None else addl.grad)
    return res


def gn_stats(x, groups, eps=EPS, dt=F64):
    """(mean, rstd) of every (sample, group) — biased variance, as GroupNorm."""
    xg = x.to(dt).reshape(x.shape[0], groups, -1)
    mean = xg.mean(-1)
    var = (xg - mean[..., None]).square().mean(-1)
    return mean.reshape(-1), (var + eps).rsqrt().reshape(-1)


def relu_band(x, w, bias, groups, eps=EPS, add=None):
    """How many elements of GN(x) [+ add, already up-sampled] lie so close to zero that f32 arithmetic may flip the ReLU gate:
    |y64| <= 4 * 2^-24 * (|x gamma rstd| + |beta - mean gamma rstd|).  A flipped gate moves d gamma / d beta by a whole element, so
    the suites use seeds whose band is empty."""
    b, c = x.shape[:2]
    mean, rstd = gn_stats(x, groups, eps)
    ga = w.double().view(1, c, 1, 1) * rstd.view(b, groups, 1).repeat_interleave(c // groups, 1).view(b, c, 1, 1)
    be = bias.double().view(1, c, 1, 1) - mean.view(b, groups, 1).repeat_interleave(c // groups, 1).view(b, c, 1, 1) * ga
    t = x.double() * ga
    y = t + be + (0 if add is None else add.double())
    return int((y.abs() <= 4 * 2.0 ** -24 * (t.abs() + be.abs())).sum())


def conv_gn_inputs():
    """The ConvGN(48, 64, 1, bias=False, relu=True) case with an added coarser map: x, conv weight, gamma, beta, add, gy."""
    g = torch.Generator().manual_seed(GN_SEED + 500)
    x = torch.randn(2, 48, 24, 16, generator=g)
    cw = torch.randn(64, 48, 1, 1, generator=g) / 48 ** 0.5
    wt, bias = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.5
    add = torch.randn(2, 64, 12, 8, generator=g)
    gy = torch.randn(2, 64, 24, 16, generator=g)
    return types.SimpleNamespace(x=x, cw=cw, w=wt, bias=bias, add=add, gy=gy, groups=32)


def conv_gn_reference(k, eps=EPS):
    """{float64 | float32: dict(y, dx, dcw, dw, dbias, dadd)} of relu(GroupNorm(conv1x1(x)) + interpolate(add))."""
    res = {}
    for dt in (F64, F32):
        xl, cwl, wl, biasl, addl = (_leaf(t, dt) for t in (k.x, k.cw, k.w, k.bias, k.add))
        z = F.conv2d(xl, cwl)
        y = F.relu(F.group_norm(z, k.groups, wl, biasl, eps)
                   + F.interpolate(addl, size=z.shape[-2:], mode='bilinear', align_corners=False))
        y.backward(k.gy.to(dt))
        res[dt] = dict(y=y.detach(), dx=xl.grad, dcw=cwl.grad, dw=wl.grad, dbias=biasl.grad, dadd=addl.grad, z=z.detach())
    return res
