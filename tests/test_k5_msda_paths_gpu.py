"""K5 multi-scale deformable attention, K16 and the fused query-side node on the paths production takes, against
float64 references evaluated on the CPU (autograd for the gradients).

Every comparison prints ``max|got - ref64| / max|ref64|`` and its bar.  Bars:

* f32 arithmetic (f32 entry points, and K5 kernels on 16-bit value maps — the value maps here are exactly representable in
  bf16 AND fp16, so the float64 reference of the f32 map is the reference of the rounded map too): ``max(4e-6, 4 x e32)``,
  e32 the error of the same reference evaluated in float32 on the CPU, per case and per tensor.  4x covers summation order
  and FMA differences; a wrong tap, channel, level or axis errs by 1e-2 or more.
* d(location) is not compared at coordinates within 1e-4 px of an integer (bilinear interpolation has no derivative there;
  f32 position rounding reaches ~1e-5 px on a 136-px level).  The share left out is asserted to stay <= 1e-3.
* 16-bit outputs of K16: one rounding of the dtype (half an ulp of the float64 value) plus the f32 bar.
* The 16-bit node: twice the error of the upstream layer under autocast (emulated on the CPU: the Linears' inputs, weights,
  outputs and gradients rounded to the dtype, the rest in float64) against float64.
* The packed value gradient keeps its documented bound: 1e-4 * max|g| (3e-4 above 8 192 queries) plus one output rounding.

Worst values measured on MI355X (error vs bar), per class — also in DESIGN.md §2:
  f32 K5 paths: bench 3.5e-7 (bar 4e-6), waymo 2.9e-7 (bar 4.1e-6), kitti 2.8e-6 (bar 1.1e-5), 136² 6.1e-6 (bar 2.4e-5);
  node f32 (bench) 3.4e-6 (bar 1.3e-5), chain 1.3e-6 (bar 4.3e-6);
  node bf16: bench 1.4e-2 (bar 2.8e-2), 136² level 1.8e-2 (d of the weight bias, bar 1.8e-2: the closest margin);
  node fp16: bench 1.9e-3 (bar 3.8e-3), 136² level 2.2e-3 (bar 4.1e-3).
The f32 node runs with the f64-accumulator value gradient (switches.msda_packed_f32 off): the packed form it takes by
default is held to its documented bound against float64 by test_k5_packed_value_gradient_against_float64.
"""
import ctypes
import math
from types import SimpleNamespace

import pytest
import torch

from oracle import maskbev_oracle as O

pytestmark = pytest.mark.gpu

F32_BAR = 4e-6          # the project's f32 bar (test_k20, test_k6, test_k4)
KINK_PX = 1e-4          # d(location) is left out this close to an integer pixel coordinate
KINK_SHARE_CAP = 1e-3
LO = (torch.bfloat16, torch.float16)


def _err(got, ref, mask=None) -> float:
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if mask is not None:
        got, ref = got[mask], ref[mask]
    return float((got - ref).abs().max() / ref.abs().max())


def _report(capsys, tag, err, bar):
    with capsys.disabled():
        print(f'\n[k5-paths] {tag}: err {err:.3e} bar {bar:.3e}', end='')


def _pd_levels(workload):
    """The pixel decoder's level shapes (coarsest first, the order its token map concatenates them) of a named workload:
    BEV grid (ny, nx) -> patch embedding (corner padding) -> one patch merging per later stage (padded to the stride)."""
    from mask_bev_amd import synthetic
    cfg = O.make_cfg(**synthetic.module_kwargs(workload, 1))
    h, w = math.ceil(cfg.ny / cfg.patch_size), math.ceil(cfg.nx / cfg.patch_size)
    hw = [(h, w)]
    for s in cfg.strides[1:]:
        h, w = math.ceil(h / s), math.ceil(w / s)
        hw.append((h, w))
    return hw[::-1][:cfg.pd_levels]


def _spec(name):
    """(B, H, D, shapes, P, nq) of a case; nq None = the self-attention token map (nq == nv)."""
    small = [(9, 13), (24, 40)]
    return {
        'bench': (2, 8, 32, _pd_levels('semantic_kitti_512'), 4, None),
        'waymo': (1, 8, 32, _pd_levels('waymo_1024'), 4, None),
        'kitti': (2, 8, 32, _pd_levels('kitti_496x432'), 4, None),
        'levels4': (1, 8, 32, [(6, 10), (12, 20), (24, 40), (48, 80)], 4, None),
        'pixel1': (2, 8, 32, [(1, 1), (7, 5), (40, 24)], 4, None),
        'side136': (1, 2, 32, [(136, 136), (36, 36)], 4, None),
        'p2': (2, 8, 32, small, 2, None),
        'unaligned': (2, 8, 32, small, 4, None),
        'dim2': (2, 8, 2, small, 4, None),
        'noshape': (2, 8, 32, small, 4, None),
        'nq': (2, 8, 32, [(9, 13), (72, 72)], 4, 700),      # a level over 4 096 pixels: not the split form
    }[name]


def _edge_samples(h, w):
    """(x, y) locations of the deliberate edge set of one level (None: keep the random coordinate)."""
    cx = lambda c: (c + 0.5) / w          # noqa: E731  pixel-space coordinate c -> normalised location
    cy = lambda c: (c + 0.5) / h          # noqa: E731
    s = [(cx(c), None) for c in (-1, 0, w - 1, w)] + [(None, cy(c)) for c in (-1, 0, h - 1, h)]
    s += [(cx(0), cy(0)), (cx(w - 1), cy(h - 1)), (cx(-1), cy(h))]                 # map corners, one just outside
    s += [(cx(w // 2), cy(h // 3)), (cx(w - 1 - w // 3), cy(h // 2))]               # exact pixel centres
    s += [(3.0, 0.5), (-3.0, -3.0), (0.5, 3.1)]                                     # far outside
    return s


def _inputs(name, seed):
    B, H, D, shapes, P, nq = _spec(name)
    L = len(shapes)
    nv = sum(h * w for h, w in shapes)
    nq = nv if nq is None else nq
    g = torch.Generator().manual_seed(seed)
    # exactly representable in bf16 and fp16: one float64 reference serves the f32 and both 16-bit value maps
    value = torch.randn(B, nv, H, D, generator=g).to(torch.bfloat16).float()
    value[value.abs() < 2.0 ** -14] = 0.0
    loc = torch.rand(B, nq, H, L, P, 2, generator=g) * 1.3 - 0.15
    attn = torch.rand(B, nq, H, L, P, generator=g).flatten(-2).softmax(-1).view(B, nq, H, L, P)
    attn[torch.rand(B, nq, H, L, P, generator=g) < 0.01] = 0.0
    # the edge set twice: first batch / head / queries and last batch / head / queries (batch and head offsets)
    for b, hd, qsign in ((0, 0, 1), (B - 1, H - 1, -1)):
        for l, (h, w) in enumerate(shapes):
            for j, (x, y) in enumerate(_edge_samples(h, w)):
                q = j // P if qsign > 0 else nq - 1 - j // P
                p = j % P
                if x is not None:
                    loc[b, q, hd, l, p, 0] = x
                if y is not None:
                    loc[b, q, hd, l, p, 1] = y
        attn[b, nq // 2 if qsign > 0 else nq // 3, hd] = 0.0                        # a whole (query, head) weightless
    go = torch.randn(B, nq, H * D, generator=g)
    return SimpleNamespace(B=B, H=H, D=D, shapes=shapes, P=P, L=L, nv=nv, nq=nq, value=value, loc=loc, attn=attn, go=go)


def _k5_reference(c, dtype):
    v, l, a = (t.to(dtype, copy=True).requires_grad_() for t in (c.value, c.loc, c.attn))
    out = O.ms_deform_attn_core(v, c.shapes, l, a)
    out.backward(c.go.to(dtype))
    return dict(out=out.detach(), d_value=v.grad, d_loc=l.grad, d_attn=a.grad)


_CACHE = {}


def _case(name):
    """Inputs, the float64 reference, the float32 reference's error against it per tensor, and the d(location) mask."""
    if name not in _CACHE:
        c = _inputs(name, seed=len(_CACHE) + 11)
        c.ref = _k5_reference(c, torch.float64)
        r32 = _k5_reference(c, torch.float32)
        wh = torch.tensor([[w, h] for h, w in c.shapes], dtype=torch.float64).view(1, 1, 1, c.L, 1, 2)
        pix = c.loc.double() * wh - 0.5
        c.loc_mask = (pix - pix.round()).abs() >= KINK_PX
        c.kink_share = 1.0 - float(c.loc_mask.double().mean())
        c.e32 = {k: _err(r32[k], c.ref[k], c.loc_mask if k == 'd_loc' else None) for k in c.ref}
        _CACHE[name] = c
    return _CACHE[name]


def _bar(c, key):
    return max(F32_BAR, 4.0 * c.e32[key])


def _check(capsys, c, tag, key, got):
    mask = c.loc_mask if key == 'd_loc' else None
    err, bar = _err(got, c.ref[key], mask), _bar(c, key)
    _report(capsys, f'{tag} {key}', err, bar)
    assert err <= bar, f'{tag} {key}: {err:.3e} > {bar:.3e}'


def _level_start(shapes, device):
    starts = [0]
    for h, w in shapes[:-1]:
        starts.append(starts[-1] + h * w)
    return torch.tensor(starts, dtype=torch.int64, device=device)


def _host(shapes):
    return (ctypes.c_int64 * (2 * len(shapes)))(*[int(v) for hw in shapes for v in hw])


def _at_offset(t, device, bytes_off=4):
    """``t`` on the device as a view whose data starts ``bytes_off`` bytes past a 16-byte boundary."""
    k = bytes_off // t.element_size()
    big = torch.zeros(t.numel() + k, dtype=t.dtype, device=device)
    v = big[k:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == bytes_off and v.is_contiguous()
    return v


def test_level_shapes_of_the_reference_configurations():
    assert _pd_levels('semantic_kitti_512') == [(16, 16), (32, 32), (64, 64)]
    assert _pd_levels('waymo_1024') == [(32, 32), (64, 64), (128, 128)]
    kitti = _pd_levels('kitti_496x432')
    assert any(h != w for h, w in kitti) and any(h % 2 or w % 2 for h, w in kitti)


# ------------------------------------------------------------------------------------------------------------------
# 1. K5 entry points, path by path
# ------------------------------------------------------------------------------------------------------------------
# name -> (forward kernel, backward form) as mbv_ms_deform_attn_fwd / _bwd select them for these inputs
_F32_PATHS = {
    'bench': ('p4', 'split'), 'kitti': ('p4', 'split'), 'levels4': ('p4', 'split'), 'pixel1': ('p4', 'split'),
    'p2': ('v4', 'split'), 'waymo': ('p4', 'banded'), 'side136': ('p4', 'banded'), 'unaligned': ('v4', 'banded'),
    'dim2': ('scalar', 'banded'), 'noshape': ('p4', 'generic'), 'nq': ('p4', 'generic'),
}


@pytest.mark.parametrize('name', list(_F32_PATHS))
def test_k5_f32_paths_against_float64(device, capsys, name):
    """ops.ms_deform_attn forward (k_msda_fwd_p4 / k_msda_fwd_v4 / k_msda_fwd) and its mode-3 backward (split: k_msda_bwd_value
    <4> or <0> + k_msda_bwd_locattn[_p4]; banded k_msda_bwd_banded; generic atomic k_msda_bwd) against float64."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    c = _case(name)
    fwd, bwd = _F32_PATHS[name]
    assert c.kink_share <= KINK_SHARE_CAP, c.kink_share
    host = _host(c.shapes)
    split = lib.mbv_ms_deform_attn_bwd_split(c.D, c.L, None if name == 'noshape' else host) == 1
    assert split == (bwd == 'split' or name == 'unaligned')     # 'unaligned': the split form also wants 16-byte pointers
    if bwd == 'banded':
        assert c.nq == c.nv and (name == 'unaligned' or not split)
    if bwd == 'generic':
        assert name == 'noshape' or c.nq != c.nv
    assert (fwd == 'scalar') == (c.D % 4 != 0) and (fwd == 'p4') == (c.P == 4 and name != 'unaligned' and c.D % 4 == 0)
    v_d = c.value.to(device).requires_grad_()
    if name == 'unaligned':
        l_d, a_d = _at_offset(c.loc, device).requires_grad_(), _at_offset(c.attn, device).requires_grad_()
    else:
        l_d, a_d = c.loc.to(device).requires_grad_(), c.attn.to(device).requires_grad_()
    shapes_t = torch.tensor(c.shapes, dtype=torch.int64, device=device)
    out = ops.ms_deform_attn(v_d, None if name == 'noshape' else c.shapes, shapes_t, _level_start(c.shapes, device),
                             l_d, a_d)
    out.backward(c.go.to(device))
    torch.cuda.synchronize()
    _check(capsys, c, f'f32 {name} fwd:{fwd}', 'out', out)
    for key, got in (('d_value', v_d.grad), ('d_loc', l_d.grad), ('d_attn', a_d.grad)):
        _check(capsys, c, f'f32 {name} bwd:{bwd}', key, got)


_V16_NAMES = ['bench', 'waymo', 'kitti', 'levels4', 'pixel1', 'side136', 'p2', 'unaligned']


@pytest.mark.parametrize('dt', LO)
@pytest.mark.parametrize('name', _V16_NAMES)
def test_k5_16bit_forward_against_float64(device, capsys, name, dt):
    """mbv_ms_deform_attn_fwd_v on a bf16 / fp16 value map: k_msda_fwd_p4<VK> (P = 4, aligned) and k_msda_fwd_v4<VK>
    (P = 2, or P = 4 with locations / weights at an offset of 4 bytes)."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    c = _case(name)
    val = c.value.to(device).to(dt)
    assert torch.equal(val.float().cpu(), c.value)                  # the map holds exactly the reference's values
    if name == 'unaligned':
        loc, attn = _at_offset(c.loc, device), _at_offset(c.attn, device)
    else:
        loc, attn = c.loc.to(device), c.attn.to(device)
    shapes_t = torch.tensor(c.shapes, dtype=torch.int64, device=device)
    ls = _level_start(c.shapes, device)
    out = torch.empty(c.B, c.nq, c.H * c.D, device=device)
    ops.check(lib.mbv_ms_deform_attn_fwd_v(ops._ptr(val), ops._dt_flag(dt), ops._ptr(shapes_t), ops._ptr(ls), ops._ptr(loc),
                                           ops._ptr(attn), c.B, c.nv, c.H, c.D, c.L, c.nq, c.P, ops._ptr(out), ops._stream()),
              'mbv_ms_deform_attn_fwd_v')
    torch.cuda.synchronize()
    form = 'p4' if (c.P == 4 and name != 'unaligned') else 'v4'
    _check(capsys, c, f'{str(dt)[6:]} {name} fwd_v:{form}', 'out', out)


@pytest.mark.parametrize('dt', (torch.float32,) + LO)
@pytest.mark.parametrize('name', _V16_NAMES)
def test_k5_location_weight_gradient_against_float64(device, capsys, name, dt):
    """mbv_ms_deform_attn_bwd_locattn (k_msda_bwd_locattn_p4<VK> for P = 4 with 16-byte aligned locations / weights,
    k_msda_bwd_locattn<VK> otherwise) on an f32 / bf16 / fp16 value map, called as _MSDAQuerySide calls it."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    c = _case(name)
    assert c.kink_share <= KINK_SHARE_CAP, c.kink_share
    val = c.value.to(device).to(dt)
    if name == 'unaligned':
        loc, attn = _at_offset(c.loc, device), _at_offset(c.attn, device)
    else:
        loc, attn = c.loc.to(device), c.attn.to(device)
    go = c.go.to(device)
    shapes_t = torch.tensor(c.shapes, dtype=torch.int64, device=device)
    ls = _level_start(c.shapes, device)
    g_loc = torch.full((c.B, c.nq, c.H, c.L, c.P, 2), float('nan'), device=device)
    g_attn = torch.full((c.B, c.nq, c.H, c.L, c.P), float('nan'), device=device)
    ops.check(lib.mbv_ms_deform_attn_bwd_locattn(ops._ptr(go), ops._ptr(val), ops._dt_flag(dt), ops._ptr(shapes_t),
                                                 ops._ptr(ls), ops._ptr(loc), ops._ptr(attn), c.B, c.nv, c.H, c.D, c.L, c.nq,
                                                 c.P, ops._ptr(g_loc), ops._ptr(g_attn), ops._stream()),
              'mbv_ms_deform_attn_bwd_locattn')
    torch.cuda.synchronize()
    form = 'p4' if (c.P == 4 and name != 'unaligned') else 'generic'
    assert bool(torch.isfinite(g_loc).all()) and bool(torch.isfinite(g_attn).all())      # every element written
    _check(capsys, c, f'{str(dt)[6:]} {name} locattn:{form}', 'd_loc', g_loc)
    _check(capsys, c, f'{str(dt)[6:]} {name} locattn:{form}', 'd_attn', g_attn)


@pytest.mark.parametrize('dt', (torch.float32,) + LO)
@pytest.mark.parametrize('name', ['bench', 'waymo', 'kitti', 'levels4', 'pixel1'])
def test_k5_packed_value_gradient_against_float64(device, capsys, name, dt):
    """mbv_ms_deform_attn_bwd_value_packed against float64 (not against the f64-accumulator kernel): its documented bound,
    1e-4 * max|g| (3e-4 above 8 192 queries) plus one output rounding, per element."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    c = _case(name)
    host = _host(c.shapes)
    assert lib.mbv_ms_deform_attn_bwd_value_packed_supported(c.D, c.L, c.P, c.nq, host) == 1
    go, loc, attn = c.go.to(device), c.loc.to(device), c.attn.to(device)
    ld = c.H * c.D
    out = torch.full((c.B * c.nv, ld), 7.0, dtype=dt, device=device)
    ws = torch.empty(lib.mbv_ms_deform_attn_bwd_value_packed_workspace_bytes(c.B, c.H, c.L, c.nq), dtype=torch.uint8,
                     device=device)
    ops.check(lib.mbv_ms_deform_attn_bwd_value_packed(ops._ptr(go), ops._ptr(loc), ops._ptr(attn), c.B, c.nv, c.H, c.D, c.L,
                                                      c.nq, c.P, host, ops._ptr(out), ops._dt_flag(dt), ld, ops._ptr(ws),
                                                      ws.numel(), ops._stream()), 'mbv_ms_deform_attn_bwd_value_packed')
    torch.cuda.synchronize()
    got = out.double().cpu().view(c.B, c.nv, c.H, c.D)
    ref = c.ref['d_value']
    gmax = float(c.go.abs().max())
    rnd = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dt]
    lim = (1e-4 if c.nq <= 8192 else 3e-4) * gmax + rnd * ref.abs()
    excess = float(((got - ref).abs() - lim).max())
    _report(capsys, f'{str(dt)[6:]} {name} packed d_value (max err - bound, abs)', excess, 0.0)
    assert excess <= 0.0


# ------------------------------------------------------------------------------------------------------------------
# 2. K16's strided forms
# ------------------------------------------------------------------------------------------------------------------
def _half_ulp(x, dt):
    """Half an ulp of |x| (float64) in ``dt`` — one rounding (a value within 2^-20 of it may sit in the next binade)."""
    mant, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dt]
    a = (x.abs() * (1 + 2.0 ** -20)).clamp_min(2.0 ** emin)
    return torch.exp2(torch.floor(torch.log2(a)) - mant) / 2


@pytest.mark.parametrize('dt', (torch.float32,) + LO)
@pytest.mark.parametrize('workload,points', [('semantic_kitti_512', 4), ('kitti_496x432', 4), ('kitti_496x432', 3)])
def test_k16_strided_forms_against_float64(device, capsys, workload, points, dt):
    """mbv_msda_prepare_fwd_ld / _bwd_ld with offsets and logits as column blocks of one wider matrix (row stride, f32
    biases), as _MSDAQuerySide passes them.  P = 3 takes the scalar (L*P % 4 != 0) form."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    shapes = _pd_levels(workload)
    B, N, E, H, L, P = 2, 700, 256, 8, len(shapes), points
    lo, la = H * L * P * 2, H * L * P
    width = E + lo + la + 8
    g = torch.Generator().manual_seed(5 + points)
    mat = (torch.randn(B * N, width, generator=g) * 2.0).to(dt)
    b_o = torch.randn(lo, generator=g) * 2.0
    b_a = torch.randn(la, generator=g)
    ref_pts = torch.rand(N, 2, generator=g)
    esz = mat.element_size()
    m_d, bo_d, ba_d, r_d = mat.to(device), b_o.to(device), b_a.to(device), ref_pts.to(device)
    loc = torch.empty(B, N, H, L, P, 2, device=device)
    attn = torch.empty(B, N, H, L, P, device=device)
    host = _host(shapes)
    ops.check(lib.mbv_msda_prepare_fwd_ld(ctypes.c_void_p(m_d.data_ptr() + E * esz), width,
                                          ctypes.c_void_p(m_d.data_ptr() + (E + lo) * esz), width, ops._ptr(bo_d),
                                          ops._ptr(ba_d), ops._dt_flag(dt), ops._ptr(r_d), host, B, N, H, L, P, ops._ptr(loc),
                                          ops._ptr(attn), ops._stream()), 'mbv_msda_prepare_fwd_ld')
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).view(1, 1, 1, L, 1, 2)

    def forward_ref(fdt):
        off = mat[:, E:E + lo].to(fdt).view(B, N, H, L, P, 2) + b_o.to(fdt).view(H, L, P, 2)
        quot = off / wh.to(fdt)
        logit = mat[:, E + lo:E + lo + la].to(fdt).view(B, N, H, L * P) + b_a.to(fdt).view(H, L * P)
        return ref_pts.to(fdt).view(1, N, 1, 1, 1, 2) + quot, logit.softmax(-1).view(B, N, H, L, P), quot

    loc64, attn64, quot64 = forward_ref(torch.float64)
    loc32, attn32, _ = forward_ref(torch.float32)
    torch.cuda.synchronize()
    bar_a = max(F32_BAR, 4 * _err(attn32, attn64))
    err_a = _err(attn, attn64)
    _report(capsys, f'k16 {workload} P{P} {str(dt)[6:]} attn', err_a, bar_a)
    assert err_a <= bar_a
    bar_l = max(F32_BAR, 4 * _err(loc32, loc64))
    if dt == torch.float32:
        err_l = _err(loc, loc64)
        _report(capsys, f'k16 {workload} P{P} f32 loc', err_l, bar_l)
        assert err_l <= bar_l
    else:
        # the quotient offset / (w, h) is a 16-bit value (msda_prepare.hip: rounding follows the torch composition under
        # autocast, where it is a tensor of the projection's dtype): one rounding of it, plus the f32 bar
        lim = _half_ulp(quot64, dt) + bar_l * float(loc64.abs().max())
        excess = float(((loc.double().cpu() - loc64).abs() - lim).max())
        _report(capsys, f'k16 {workload} P{P} {str(dt)[6:]} loc (max err - one rounding, abs)', excess, 0.0)
        assert excess <= 0.0

    # backward: both blocks into a sentinel-filled matrix of the same layout
    g_loc = torch.randn(B, N, H, L, P, 2, generator=g)
    g_attn = torch.randn(B, N, H, L, P, generator=g)
    a_cpu = attn.cpu()
    sentinel = -7.0
    gm = torch.full((B * N, width), sentinel, dtype=dt, device=device)
    gl_d, ga_d = g_loc.to(device), g_attn.to(device)
    ops.check(lib.mbv_msda_prepare_bwd_ld(ops._ptr(gl_d), ops._ptr(ga_d), ops._ptr(attn), host, B, N,
                                          H, L, P, ops._dt_flag(dt), ctypes.c_void_p(gm.data_ptr() + E * esz), width,
                                          ctypes.c_void_p(gm.data_ptr() + (E + lo) * esz), width, ops._stream()),
              'mbv_msda_prepare_bwd_ld')
    torch.cuda.synchronize()
    gm = gm.cpu()
    assert bool((gm[:, :E] == sentinel).all()) and bool((gm[:, E + lo + la:] == sentinel).all())

    def backward_ref(fdt, gl):
        a, ga = a_cpu.to(fdt).view(B, N, H, L * P), g_attn.to(fdt).view(B, N, H, L * P)
        g_logit = a * (ga - (a * ga).sum(-1, keepdim=True))
        return (gl.to(fdt) / wh.to(fdt)).reshape(B * N, lo), g_logit.reshape(B * N, la)

    # a 16-bit quotient's incoming gradient is a 16-bit value before the division's backward (autograd of the torch
    # composition; msda_prepare.hip): the reference divides that value
    gl_in = g_loc if dt == torch.float32 else g_loc.to(dt).float()
    goff64, glog64 = backward_ref(torch.float64, gl_in)
    goff32, glog32 = backward_ref(torch.float32, gl_in)
    for tag, got, r64, r32 in (('d_off', gm[:, E:E + lo], goff64, goff32), ('d_logit', gm[:, E + lo:E + lo + la], glog64,
                                                                             glog32)):
        bar = max(F32_BAR, 4 * _err(r32, r64))
        if dt == torch.float32:
            err = _err(got, r64)
            _report(capsys, f'k16 {workload} P{P} f32 {tag}', err, bar)
            assert err <= bar
        else:
            lim = _half_ulp(r64, dt) + bar * float(r64.abs().max())
            excess = float(((got.double() - r64).abs() - lim).max())
            _report(capsys, f'k16 {workload} P{P} {str(dt)[6:]} {tag} (max err - one rounding, abs)', excess, 0.0)
            assert excess <= 0.0


# ------------------------------------------------------------------------------------------------------------------
# 3. The fused query-side node
# ------------------------------------------------------------------------------------------------------------------
def _rd(t, dt):
    return t.to(dt).to(t.dtype)


class _AutocastLinear(torch.autograd.Function):
    """nn.Linear under autocast, in float64 with the roundings of the dtype: inputs, weight, bias, output and the
    gradients (incoming, and the three outgoing ones) rounded to ``dt``."""

    @staticmethod
    def forward(ctx, x, w, b, dt):
        xr, wr = _rd(x, dt), _rd(w, dt)
        ctx.save_for_backward(xr, wr)
        ctx.dt = dt
        return _rd(xr @ wr.t() + _rd(b, dt), dt)

    @staticmethod
    def backward(ctx, gy):
        xr, wr = ctx.saved_tensors
        dt = ctx.dt
        gy = _rd(gy, dt)
        return _rd(gy @ wr, dt), _rd(gy.t() @ xr, dt), _rd(gy.sum(0), dt), None


def _node_reference(x, pos, ref_pts, layers, shapes, H, P, go, mode):
    """mmcv's MultiScaleDeformableAttention up to output_proj, a chain of ``len(layers)`` of them (each one's output is the
    next one's query), on the CPU.  mode: 'f64', 'f32' (plain arithmetic of that type) or 'bf16' / 'fp16' (autocast)."""
    cdt = torch.float32 if mode == 'f32' else torch.float64
    lo = {'bf16': torch.bfloat16, 'fp16': torch.float16}.get(mode)
    B, N, E = x.shape
    L = len(shapes)
    xs, ps = x.detach().to(cdt, copy=True).requires_grad_(), pos.detach().to(cdt, copy=True).requires_grad_()
    prm = [[p.detach().cpu().to(cdt, copy=True).requires_grad_() for p in lay] for lay in layers]

    def lin(t, w, b):
        return _AutocastLinear.apply(t, w, b, lo) if lo is not None else torch.nn.functional.linear(t, w, b)

    norm = torch.tensor([[w, h] for h, w in shapes], dtype=cdt).view(1, 1, 1, L, 1, 2)
    r = ref_pts.to(cdt).view(1, N, 1, 1, 1, 2)
    cur = xs
    for wv, bv, wo, bo, wa, ba in prm:
        value = lin(cur.reshape(B * N, E), wv, bv).view(B, N, H, E // H)
        q = (cur + ps).reshape(B * N, E)
        off = lin(q, wo, bo).view(B, N, H, L, P, 2)
        aw = lin(q, wa, ba).view(B, N, H, L * P).softmax(-1).view(B, N, H, L, P)
        cur = O.ms_deform_attn_core(value, shapes, r + off / norm, aw)
    cur.backward(go.to(cdt))
    return [cur.detach(), xs.grad, ps.grad] + [p.grad for lay in prm for p in lay]


_NODE_KEYS = ['out', 'd_x', 'd_pos', 'd_wv', 'd_bv', 'd_wo', 'd_bo', 'd_wa', 'd_ba']


def _node_inputs(name):
    """(B, shapes, layers) of a node case; E 256, 8 heads (head dim 32), 4 points, pos (1, N, E)."""
    return {
        'bench': (2, _pd_levels('semantic_kitti_512'), 1),
        'side136': (1, [(136, 136), (36, 36)], 1),
        'chain': (3, [(16, 16), (8, 8), (4, 4)], 3),
    }[name]


_NODE_CACHE = {}


def _node_case(name):
    if name in _NODE_CACHE:
        return _NODE_CACHE[name]
    B, shapes, nlay = _node_inputs(name)
    E, H, L, P = 256, 8, len(shapes), 4
    N = sum(h * w for h, w in shapes)
    g = torch.Generator().manual_seed(23 + nlay)
    x = torch.randn(B, N, E, generator=g)
    pos = torch.randn(1, N, E, generator=g)
    # Sampling positions kept >= 0.3 px from integer pixel coordinates, where bilinear interpolation has no derivative: a
    # 16-bit rounding of an offset (~1e-2 px) that carries a sample across one changes its location gradient by O(1) and
    # would make every d(location)-borne gradient (x, pos, offsets) a count of such crossings instead of a rounding error.
    # Reference points on a grid G that divides every level's side (ref * side - 0.5 is a half-integer on every level),
    # offset biases whole pixels, and the query-dependent part of the offsets small (std ~0.03 px).
    gx, gy = math.gcd(*[w for _, w in shapes]), math.gcd(*[h for h, _ in shapes])
    ref_pts = torch.stack([torch.randint(0, gx + 1, (N,), generator=g) / gx,
                           torch.randint(0, gy + 1, (N,), generator=g) / gy], -1).float()
    layers = []
    for _ in range(nlay):
        layers.append([torch.randn(E, E, generator=g) * E ** -0.5, torch.randn(E, generator=g) * 0.1,
                       torch.randn(H * L * P * 2, E, generator=g) * 1.3e-3,
                       torch.randint(-3, 4, (H * L * P * 2,), generator=g).float(),
                       torch.randn(H * L * P, E, generator=g) * 0.05, torch.randn(H * L * P, generator=g) * 0.5])
    go = torch.randn(B, N, E, generator=g)
    c = SimpleNamespace(B=B, N=N, E=E, H=H, L=L, P=P, shapes=shapes, x=x, pos=pos, ref_pts=ref_pts, layers=layers, go=go,
                        refs={})
    c.refs['f64'] = _node_reference(x, pos, ref_pts, layers, shapes, H, P, go, 'f64')
    _NODE_CACHE[name] = c
    return c


def _node_ref(c, mode):
    if mode not in c.refs:
        c.refs[mode] = _node_reference(c.x, c.pos, c.ref_pts, c.layers, c.shapes, c.H, c.P, c.go, mode)
    return c.refs[mode]


def _run_node(device, c, dt, arena, share=False, wcat_from_stacks=False):
    """The node (a chain of them for several layers) on the GPU → [out, d_x, d_pos, 6 gradients per layer]."""
    from mask_bev_amd import ops
    x = c.x.to(device).requires_grad_()
    pos = c.pos.to(device).requires_grad_()
    ref_pts = c.ref_pts.to(device)
    mods = []
    for lay in c.layers:
        ps = [p.to(device).requires_grad_() for p in lay]
        if arena:
            for p in ps:
                p._mbv_arena = True
                p.grad = torch.ones_like(p)
        mods.append((SimpleNamespace(weight=ps[0], bias=ps[1]), SimpleNamespace(weight=ps[2], bias=ps[3]),
                     SimpleNamespace(weight=ps[4], bias=ps[5]), ps))
    shapes_t = torch.tensor(c.shapes, dtype=torch.int64, device=device)
    ls = _level_start(c.shapes, device)
    pshare = ops.PosGradShare(len(mods)) if share else None
    stacks = None
    if wcat_from_stacks:
        stacks = ops.msda_weight_stacks([SimpleNamespace(value_proj=m[0], sampling_offsets=m[1], attention_weights=m[2])
                                         for m in mods], dt)
        assert stacks is not None
    cur, saved = x, []
    with torch.autocast('cuda', dtype=dt, enabled=dt != torch.float32):
        for j, (vp, so, aw, _) in enumerate(mods):
            cur = ops.msda_query_side(cur, pos, ref_pts, vp, so, aw, c.H, c.L, c.P, c.shapes, shapes_t, ls,
                                      pos_share=pshare, pos_share_index=j, wcat=None if stacks is None else stacks[j])
            saved.append(cur.grad_fn.saved_tensors[2].dtype)          # the value map K5 reads (16-bit or f32)
    from mask_bev_amd import switches
    # f32 compute: the f64-accumulator value gradient, so that the node is f32 arithmetic throughout and takes the f32 bar;
    # the packed form it would otherwise use (switches.msda_packed_f32) is held to its own bound against float64 above
    with switches.override(msda_packed_f32=dt != torch.float32):
        cur.backward(c.go.to(device))
    ops.flush_deferred_grads()
    torch.cuda.synchronize()
    off = 1.0 if arena else 0.0
    res = [cur.detach(), x.grad, pos.grad]
    for *_, ps in mods:
        res += [p.grad - off for p in ps]
    return res, saved, stacks, mods


def _node_bars(c, dt, arena):
    ref64 = c.refs['f64']
    if dt == torch.float32:
        r32 = _node_ref(c, 'f32')
        bars = [max(F32_BAR, 4 * _err(a, b)) for a, b in zip(r32, ref64)]
    else:
        emu = _node_ref(c, 'bf16' if dt == torch.bfloat16 else 'fp16')
        bars = [2 * _err(a, b) for a, b in zip(emu, ref64)]
    if arena:
        # an arena gradient is 1.0 + g stored in f32: one f32 rounding of that sum (2^-24 of |1 + g|) on top
        bars = [bar + (2.0 ** -24 * (1.0 + float(r.abs().max())) / float(r.abs().max()) if i >= 3 else 0.0)
                for i, (bar, r) in enumerate(zip(bars, ref64))]
    return bars


def _node_compare(capsys, c, tag, got, dt, arena):
    ref64 = c.refs['f64']
    bars = _node_bars(c, dt, arena)
    nl = len(c.layers)
    keys = _NODE_KEYS[:3] + [f'{k}[{j}]' for j in range(nl) for k in _NODE_KEYS[3:]]
    bad = []
    for k, a, r, bar in zip(keys, got, ref64, bars):
        err = _err(a, r)
        _report(capsys, f'{tag} {k}', err, bar)
        if not err <= bar:
            bad.append(f'{k}: {err:.3e} > {bar:.3e}')
    assert not bad, bad


@pytest.mark.parametrize('arena', [False, True])
@pytest.mark.parametrize('dt', (torch.float32,) + LO)
def test_msda_query_side_against_float64(device, capsys, dt, arena):
    """ops.msda_query_side (one autograd node: projections, K16 _ld forms, K5 forward / backward — the packed value gradient
    in the 16-bit modes —, the [d value | d offsets | d logits] matrix, bias column sums, weight gradients) at the bench class against the
    float64 composition of mmcv's layer up to output_proj: output, d(x), d(pos), the six parameter gradients.  Arena
    parameters accumulate into gradients pre-filled with 1.0 (bias sums through the deferred grouped launch)."""
    from mask_bev_amd import _lib
    c = _node_case('bench')
    host = _host(c.shapes)
    assert _lib.load().mbv_ms_deform_attn_bwd_value_packed_supported(32, c.L, c.P, c.N, host) == 1
    got, saved, _, _ = _run_node(device, c, dt, arena)
    assert saved == [torch.float32 if dt == torch.float32 else dt]          # 16-bit modes keep the map in 16 bits
    _node_compare(capsys, c, f'node bench {str(dt)[6:]} arena={arena}', got, dt, arena)


@pytest.mark.parametrize('dt', LO)
def test_msda_query_side_level_beyond_the_packed_form(device, capsys, dt):
    """A 136 x 136 level (18 496 pixels): the packed value gradient is unsupported, so the 16-bit node keeps an f32 value
    map and takes the banded f64 backward — against float64."""
    from mask_bev_amd import _lib
    c = _node_case('side136')
    lib = _lib.load()
    host = _host(c.shapes)
    assert lib.mbv_ms_deform_attn_bwd_value_packed_supported(32, c.L, c.P, c.N, host) == 0
    assert lib.mbv_ms_deform_attn_bwd_split(32, c.L, host) == 0
    got, saved, _, _ = _run_node(device, c, dt, False)
    assert saved == [torch.float32]
    _node_compare(capsys, c, f'node side136 {str(dt)[6:]}', got, dt, False)


@pytest.mark.parametrize('dt', (torch.float32, torch.bfloat16))
def test_msda_query_side_chain_with_shared_pos_gradient(device, capsys, dt):
    """Three nodes in a chain sharing one PosGradShare (only the first layer returns d(pos): the three layers' batch sums
    times the stacked weights), B = 3 with pos (1, N, E) — the row-modulo read of mbv_msda_query_inputs — against the float64
    chain, whose d(pos) is the sum of the three layers' contributions."""
    c = _node_case('chain')
    got, saved, _, _ = _run_node(device, c, dt, False, share=True)
    assert saved == [torch.float32 if dt == torch.float32 else dt] * 3
    _node_compare(capsys, c, f'node chain {str(dt)[6:]}', got, dt, False)


@pytest.mark.parametrize('dt', (torch.float32,) + LO)
def test_msda_weight_stacks_equal_concatenation(device, dt):
    """msda_weight_stacks (one mbv_copy_group launch): each stack is torch.cat of the three casts, and the node given the
    stacks as ``wcat`` is bit-identical to the node that concatenates for itself (gradients reduced with float atomics:
    up to summation order)."""
    c = _node_case('chain')
    a, _, stacks, mods = _run_node(device, c, dt, False, share=True, wcat_from_stacks=True)
    for st, (vp, so, aw, _) in zip(stacks, mods):
        assert st.dtype == dt
        assert torch.equal(st, torch.cat([vp.weight.to(dt), so.weight.to(dt), aw.weight.to(dt)], 0))
    b, _, _, _ = _run_node(device, c, dt, False, share=True)
    # the output is bit-identical; the gradients too, except where the node itself is not run-to-run reproducible (column
    # sums with float atomics): those may differ by summation order alone, within the f32 bar
    assert torch.equal(a[0], b[0])
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y) or _err(x, y) <= F32_BAR, (i, _err(x, y))
