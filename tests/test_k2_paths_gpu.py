"""K2 (PillarFeatureNet: K2a decoration, K2b per-pillar kernels, K2c Linears) against float64, on the paths production takes.

References are plain torch on the CPU (tests/pfn_ref.py and the dense steps below), run twice: in float64 — the reference —
and in float32, whose own error against float64 sets the bar (f64_bars.f32_bar: max(4e-6, 4 x that error)).  Every
comparison prints ``err … bar …``; error = max|got - ref64| / max|ref64| per tensor.

(a) the whole forward through ops.pfn_layers with ``row_pillar`` ('stream', the default: one call, the pillar term inside the
    Linear, streamed statistics; 'walk': one call, per-pillar statistics; 'layers': one C-ABI call per kernel), train and
    eval: output and both running buffers of every layer.  The forward is continuous — no element is left out.
(b) the kernels of one layer through the C ABI, as the backward issues them, on GIVEN f32 inputs: mbv_pfn_stats +
    mbv_pfn_bn_finalize + mbv_pfn_apply_max, mbv_pfn_bwd_route, mbv_pfn_bwd_bn.  The float64 step is the DENSE definition
    (V, P, U): a pillar's P - n unused slots all hold its padded row, the statistics run over V·P rows, torch.max picks the
    first maximal slot, the padded slots' gradient is returned summed.  Gates are decided by z = scale·y + shift in float64; an
    element is fragile if |z| < 4·2^-24·(|scale·y| + |shift|), a pillar-channel pair if it holds a fragile element or if its
    winner and runner-up among distinct candidates (bit-identical rows — the P - n copies of the padded row, duplicate
    points — are ONE candidate: first-index rule, no margin) are closer than that.  Fragile pairs are left out of dz, dz_pad,
    dy, dy_pad and dt; d gamma / d beta get Σ_fragile |dm|·(1 + |x̂|).  A case may leave out at most 1e-5 of its elements
    (asserted; the seeds here leave out none).  Exact: a pair whose rows are all gated off carries no gradient; a pillar of
    duplicate points gives the reference's per-pillar sums.
(c) the products of the backward — _wgrad, dy.mm(w) of a Fourier front end, the three _pfn_mm data gradients — on dy, dy_pad,
    dt of the float64 step rounded to f32, against float64 products; below and above the 8 192-row threshold of K2c / split-K.
(d) K2a at production ranges (x 0 … 70.4 m, y ±40 m), full pillars, 3 and 4 point channels.

Shapes: units [32,32,32], [64,128], [128,128,128] (4-channel lane kernels), [48,96] (lane = channel walk at <= 64 and > 64
units; library Linears, one call per kernel) and [96,96] (the one-call forward whose statistics fall back to the walk:
256 % (96 / 4) != 0); 10 and 11 input features; P 4, 8, 32; V 1, 3, 257 (one past kStatPadBlocks), 700; K below and above
kStatRowBlocks = 512; pillars all full (the padded row must stay out of the max), all of one point, mixed, and one pillar of
duplicate points; rows decorated at production ranges, and one case with absolute coordinates in the rows (the BatchNorm
sums cancel).  Measured errors: DESIGN.md §2."""
import functools
import types

import pytest
import torch

from tests import pfn_ref as R
from tests.f64_bars import check, err, f32_bar

pytestmark = pytest.mark.gpu
MOD = 'k2-paths'
VOXEL, RANGE = (0.16, 0.16, 4.0), (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)      # 440 x 500 x 1 cells
GX, GY = 440, 500
CAP = 1e-5                                                                # share of a case's elements the fragile set may take
F64, F32 = torch.float64, torch.float32


# ---------------------------------------------------------------------------------------------------------------------------
# inputs (CPU, seeded)
# ---------------------------------------------------------------------------------------------------------------------------
def _num_points(v, p, occ, g):
    if occ == 'full':
        return torch.full((v,), p, dtype=torch.int32)
    if occ == 'one':
        return torch.ones(v, dtype=torch.int32)
    n = torch.randint(1, p + 1, (v,), generator=g, dtype=torch.int32)          # 'mixed', 'dup'
    edge = [p, 1, min(p, 9), max(1, p - 1), min(p, 17), min(p, 8)]              # full, single, around the 8-row chunks
    for i in range(min(v, len(edge))):
        n[(i * 7) % v] = edge[i]
    if v == 1:
        n[0] = max(1, p - 3)
    if occ == 'dup':
        n[v // 2] = max(2, p - 2)
    return n


@functools.lru_cache(maxsize=None)
def _pillars(v, p, occ, pc_dim, seed, raw=False):
    """Pillars at production ranges → f32 compact decorated rows (K, pc_dim + 7), num_points, the dup pillar (or -1).
    raw: channels 0-2 keep the ABSOLUTE coordinates (metres) instead of the centre offset."""
    g = torch.Generator().manual_seed(seed)
    n = _num_points(v, p, occ, g)
    cells = torch.randperm(GX * GY, generator=g)[:v]
    coors = torch.stack([torch.zeros_like(cells), torch.zeros_like(cells), cells // GX, cells % GX], 1).to(torch.int32)
    u = torch.rand(v, p, pc_dim, generator=g)
    vox = u.clone()
    vox[..., 0] = RANGE[0] + (coors[:, 3:4] + 0.05 + 0.9 * u[..., 0]) * VOXEL[0]
    vox[..., 1] = RANGE[1] + (coors[:, 2:3] + 0.05 + 0.9 * u[..., 1]) * VOXEL[1]
    vox[..., 2] = RANGE[2] + u[..., 2] * VOXEL[2]
    dup = v // 2 if occ == 'dup' else -1
    if dup >= 0:
        vox[dup] = vox[dup, :1]
    vox = vox * (torch.arange(p).view(1, -1) < n.view(-1, 1)).unsqueeze(-1)
    dense = R.decorate(vox, n, coors, VOXEL, RANGE)
    if raw:
        dense = torch.cat([vox[..., :3], dense[..., 3:]], -1)
    return R.compact_rows(dense, n).contiguous(), n, dup


def _layers(units, cin, seed, full):
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for u in units:
        w = torch.randn(u, cin, generator=g) / cin ** 0.5
        gamma = 1 + 0.1 * torch.randn(u, generator=g)
        # all pillars full: a positive beta lifts relu(bn(y_pad)) above the rows of every pillar whose y are all below y_pad
        beta = torch.full((u,), 1.0) if full else 0.1 * torch.randn(u, generator=g)
        out.append((w, gamma, beta, 0.1 * torch.randn(u, generator=g), torch.rand(u, generator=g) + 0.5))
        cin = 2 * u
    return out


def _index(n):
    row_start = torch.zeros(n.shape[0] + 1, dtype=torch.int32)
    row_start[1:] = torch.cumsum(n, 0)
    return row_start, torch.repeat_interleave(torch.arange(n.shape[0]), n.long())


def _dev_pillars(n, p, device):
    row_start, row_pillar = _index(n)
    pil = types.SimpleNamespace(row_start=row_start.to(device), num_points=n.to(device), num_pillars=int(n.shape[0]),
                                max_points=p)
    return pil, row_pillar.to(device)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the whole forward
# ---------------------------------------------------------------------------------------------------------------------------
# units, pc_dim (10 / 11 input features), P, V, occupancy, rows hold absolute coordinates
FWD_CASES = [
    ((32, 32, 32), 4, 8, 700, 'mixed', False),
    ((64, 128), 3, 4, 257, 'full', False),           # K = 1 028: above kStatRowBlocks and no multiple of it
    ((128, 128, 128), 4, 32, 257, 'mixed', False),
    ((48, 96), 3, 8, 257, 'dup', False),
    ((96, 96), 4, 4, 700, 'one', False),
    ((32, 32, 32), 3, 8, 1, 'mixed', False),
    ((64, 128), 4, 32, 3, 'mixed', False),
    ((128, 128, 128), 3, 4, 700, 'full', False),
    ((64, 128), 4, 8, 257, 'mixed', True),
]


@functools.lru_cache(maxsize=None)
def _fwd_reference(ci, training):
    units, pc_dim, p, v, occ, raw = FWD_CASES[ci]
    rows, n, _ = _pillars(v, p, occ, pc_dim, 11 + ci, raw)
    layers = _layers(units, pc_dim + 7, ci, occ == 'full')
    res = {}
    for dt in (F64, F32):
        out, zs, bufs = R.pfn_ref(R.dense_rows(rows.to(dt), n, p), [tuple(t.to(dt) for t in l) for l in layers], training)
        res[dt] = (out, bufs, zs)
    hazard = 0
    if occ == 'full':                                  # how often a padded row — there is none — would win layer 0's max
        w, gamma, beta = (t.double() for t in layers[0][:3])
        y = (R.dense_rows(rows.double(), n, p) @ w.t()).reshape(v * p, -1)
        mean, var = (y.mean(0), ((y - y.mean(0)) ** 2).mean(0)) if training else (layers[0][3].double(), layers[0][4].double())
        zpad = beta - mean * gamma / torch.sqrt(var + R.EPS)
        hazard = int((torch.relu(zpad) > torch.relu(res[F64][2][0]).amax(1)).sum())
    return rows, n, layers, res, hazard


@pytest.mark.parametrize('path', ['stream', 'walk', 'layers'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('ci', range(len(FWD_CASES)), ids=[f'{"-".join(map(str, c[0]))}_f{c[1] + 7}_P{c[2]}_V{c[3]}_{c[4]}{"_raw" if c[5] else ""}'
                                                           for c in FWD_CASES])
def test_pfn_forward_against_float64(device, capsys, monkeypatch, ci, training, path):
    from mask_bev_amd import ops, switches
    units, pc_dim, p, v, occ, raw = FWD_CASES[ci]
    rows, n, layers, res, hazard = _fwd_reference(ci, training)
    if occ == 'full':
        assert hazard > 0, 'the case must be one in which a padded row taking part in the max would be seen'
    switches.patch(monkeypatch, pfn_stream_stats=(path == 'stream'), pfn_one_call=(path != 'layers'))
    pil, row_pillar = _dev_pillars(n, p, device)
    dev_layers = [tuple(t.clone().to(device) for t in l) + (R.EPS, R.MOMENTUM) for l in layers]
    out = ops.pfn_layers(rows.to(device), pil, dev_layers, training, row_pillar)
    (o64, b64, _), (o32, b32, _) = res[F64], res[F32]
    tag = f'{path} {"train" if training else "eval"} case {ci}'
    bad = []
    assert out.shape == o64.shape and torch.isfinite(out).all()
    check(capsys, MOD, f'{tag} out', err(out, o64), f32_bar(o32, o64), bad)
    for i, l in enumerate(dev_layers):
        check(capsys, MOD, f'{tag} running_mean[{i}]', err(l[3], b64[i][0]), f32_bar(b32[i][0], b64[i][0]), bad)
        check(capsys, MOD, f'{tag} running_var[{i}]', err(l[4], b64[i][1]), f32_bar(b32[i][1], b64[i][1]), bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# (b) one layer's kernels on given inputs: the dense steps (any dtype)
# ---------------------------------------------------------------------------------------------------------------------------
def _dense(rows, pad, n, p):
    """(V, P, U): the real rows, then the padded row in every unused slot; the mask of the real slots."""
    mask = (torch.arange(p).view(1, -1) < n.long().view(-1, 1)).unsqueeze(-1)
    return torch.where(mask, R.dense_rows(rows, n, p), pad.unsqueeze(1)), mask


def _spread(total, n, p):
    """A padded row's summed quantity, one share per copy (the maps are linear: any split with that sum gives the same result)."""
    mult = (p - n.long()).view(-1, 1).to(total.dtype)
    return torch.where(mult > 0, total / mult.clamp_min(1), torch.zeros_like(total))


def step_forward(y0, ypad0, t, gamma, beta, rm, rv, n, p, training, dt):
    cast = lambda x: None if x is None else x.to(dt)
    y0, ypad0, t, gamma, beta, rm, rv = map(cast, (y0, ypad0, t, gamma, beta, rm, rv))
    _, row_pillar = _index(n)
    y, ypad = (y0, ypad0) if t is None else (y0 + t[row_pillar], ypad0 + t)
    yd, mask = _dense(y, ypad, n, p)
    flat = yd.reshape(-1, yd.shape[-1])
    sums = torch.cat([flat.sum(0), (flat * flat).sum(0)])
    z, rm2, rv2 = R.batch_norm(flat, gamma, beta, rm, rv, training)
    mean, var = (flat.mean(0), ((flat - flat.mean(0)) ** 2).mean(0)) if training else (rm, rv)
    rstd = 1 / torch.sqrt(var + R.EPS)
    a = torch.relu(z).view(yd.shape)
    return dict(y=y, y_pad=ypad, sums=sums, mean=mean, rstd=rstd, scale=gamma * rstd, shift=beta - mean * gamma * rstd,
                running_mean=rm2, running_var=rv2, a=a[mask.expand_as(a)].view(-1, a.shape[-1]),
                a_pad=a[:, -1] * (n.view(-1, 1) < p), m=a.amax(1))


def step_route(y, ypad, scale, shift, mean, rstd, da, sapad, dm, n, p, dt):
    cast = lambda x: None if x is None else x.to(dt)
    y, ypad, scale, shift, mean, rstd, da, sapad, dm = map(cast, (y, ypad, scale, shift, mean, rstd, da, sapad, dm))
    yd, mask = _dense(y, ypad, n, p)
    z = yd * scale + shift
    arg = torch.relu(z).max(dim=1, keepdim=True)[1]                                     # the first maximal slot
    g = torch.zeros_like(yd) if da is None else _dense(da, _spread(torch.zeros_like(ypad) if sapad is None else sapad, n, p), n, p)[0]
    g = g.scatter_add(1, arg, dm.unsqueeze(1))
    dzd = torch.where(z > 0, g, torch.zeros_like(g))
    xhat = (yd - mean) * rstd
    return dict(dz=dzd[mask.expand_as(dzd)].view(-1, dzd.shape[-1]), dz_pad=(dzd * ~mask).sum(1),
                d_beta=dzd.sum((0, 1)), d_gamma=(dzd * xhat).sum((0, 1)))


def step_bn(y, ypad, dz, dzpad, mean, rstd, gamma, sums, count, training, n, p, dt):
    y, ypad, dz, dzpad, mean, rstd, gamma, sums = (x.to(dt) for x in (y, ypad, dz, dzpad, mean, rstd, gamma, sums))
    yd, mask = _dense(y, ypad, n, p)
    dzd, _ = _dense(dz, _spread(dzpad, n, p), n, p)
    u = yd.shape[-1]
    c1, c2 = (sums[:u] / count, sums[u:] / count) if training else (torch.zeros_like(mean), torch.zeros_like(mean))
    dyd = gamma * rstd * (dzd - c1 - (yd - mean) * rstd * c2)
    return dict(dy=dyd[mask.expand_as(dyd)].view(-1, u), dy_pad=(dyd * ~mask).sum(1), dt=dyd.sum(1))


def fragile_pairs(y, ypad, scale, shift, n, p):
    """(V, U) bool — the pillar-channel pairs whose gate or max is decided by less than 4·2^-24·(|scale·y| + |shift|) —
    and the dense z (float64)."""
    yd, _ = _dense(y.double(), ypad.double(), n, p)
    sy, sh = yd * scale.double(), shift.double()
    z = sy + sh
    margin = 4 * 2.0 ** -24 * (sy.abs() + sh.abs())
    gate = (z.abs() < margin).any(1)
    a = torch.relu(z)
    a1 = a.amax(1, keepdim=True)
    a2 = torch.where(a == a1, torch.full_like(a, -1.0), a).amax(1)                      # the best DISTINCT other candidate
    close = (a1.squeeze(1) > 0) & (a2 >= 0) & (a1.squeeze(1) - a2 < margin.amax(1))
    return gate | close, z


U_CASES = [      # units, P, V, occupancy
    (32, 8, 700, 'mixed'), (64, 4, 257, 'full'), (128, 32, 257, 'mixed'), (48, 8, 257, 'dup'), (96, 32, 3, 'mixed'),
    (64, 8, 1, 'mixed'), (128, 4, 700, 'one'), (32, 32, 257, 'dup'), (96, 8, 700, 'mixed'),
]
U_IDS = [f'U{c[0]}_P{c[1]}_V{c[2]}_{c[3]}' for c in U_CASES]


@functools.lru_cache(maxsize=None)
def _given(ki):
    """The f32 inputs of one layer's kernels and the float64 / float32 steps on them."""
    u, p, v, occ = U_CASES[ki]
    g = torch.Generator().manual_seed(500 + ki)
    n = _num_points(v, p, occ, g)
    row_start, row_pillar = _index(n)
    k = int(n.sum())
    r = lambda *s: torch.randn(*s, generator=g)
    off = r(u)                                                          # channel means up to ~2 sigma: the sums cancel
    y0, ypad0, t = 1.5 * r(k, u) + off, 1.5 * r(v, u) + off, 0.5 * r(v, u)
    dup = v // 2 if occ == 'dup' else -1
    if dup >= 0:
        y0[row_start[dup]:row_start[dup + 1]] = y0[row_start[dup]]
    gamma, beta = 1 + 0.1 * r(u), 0.1 * r(u)
    beta[::7] = -40.0                                                   # every row of these channels is gated off
    if occ == 'full':
        ypad0 += 10.0                                                   # would win every max if it took part
    rm, rv = 0.1 * r(u), torch.rand(u, generator=g) + 0.5
    fwd = {(tr, ht, dt): step_forward(y0, ypad0, t if ht else None, gamma, beta, rm, rv, n, p, tr, dt)
           for tr in (True, False) for ht in (True, False) for dt in (F64, F32)}
    # the backward's given inputs: the f32 roundings of the float64 forward (training, with the pillar term)
    f = fwd[(True, True, F64)]
    y, ypad, scale, shift, mean, rstd = (f[key].float() for key in ('y', 'y_pad', 'scale', 'shift', 'mean', 'rstd'))
    dm, da = r(v, u), r(k, u)
    sapad = r(v, u) * (n.view(-1, 1) < p)                               # a full pillar has no padded slot to hand a gradient on
    frag, z = fragile_pairs(y, ypad, scale, shift, n, p)
    route = {(hd, dt): step_route(y, ypad, scale, shift, mean, rstd, da if hd else None, sapad if hd else None, dm, n, p, dt)
             for hd in (True, False) for dt in (F64, F32)}
    dz, dzpad = route[(True, F64)]['dz'].float(), route[(True, F64)]['dz_pad'].float()
    dzd, _ = _dense(dz.double(), _spread(dzpad.double(), n, p), n, p)
    xhat = (_dense(y.double(), ypad.double(), n, p)[0] - mean.double()) * rstd.double()
    sums = torch.cat([dzd.sum((0, 1)), (dzd * xhat).sum((0, 1))])        # of the dz handed over, in float64
    bn = {(tr, dt): step_bn(y, ypad, dz, dzpad, mean, rstd, gamma, sums, float(v * p), tr, n, p, dt)
          for tr in (True, False) for dt in (F64, F32)}
    return types.SimpleNamespace(u=u, p=p, v=v, k=k, n=n, row_start=row_start, row_pillar=row_pillar, dup=dup, y0=y0, ypad0=ypad0,
                                 t=t, gamma=gamma, beta=beta, rm=rm, rv=rv, fwd=fwd, y=y, ypad=ypad, scale=scale, shift=shift,
                                 mean=mean, rstd=rstd, dm=dm, da=da, sapad=sapad, frag=frag, z=z, xhat=xhat, route=route, dz=dz,
                                 dzpad=dzpad, sums=sums, bn=bn)


def _left_out(c):
    """Row mask (K, U) and pillar mask (V, U) of the fragile pairs; asserts the cap."""
    rows = c.frag[c.row_pillar]
    share = (int(rows.sum()) + int(c.frag.sum())) / float((c.k + c.v) * c.u)
    assert share <= CAP, f'{share:.2e} of the elements sit in fragile pillar-channel pairs: choose another seed'
    return rows, c.frag


def _cmp(capsys, tag, got, ref64, ref32, bad, out=None):
    """One printed comparison against the f32 bar, the fragile positions ``out`` left out; a reference that is zero throughout
    (the padded row's gradients when every pillar is full) asks for exact zeros."""
    got, ref64 = got.detach().double().cpu(), ref64.double()
    if out is not None:
        got, ref64, ref32 = got.masked_fill(out, 0.0), ref64.masked_fill(out, 0.0), ref32.masked_fill(out, 0.0)
    if float(ref64.abs().max()) == 0.0:
        check(capsys, MOD, tag + ' (exact zeros)', float(got.abs().max()), 0.0, bad)
    else:
        check(capsys, MOD, tag, err(got, ref64), f32_bar(ref32, ref64), bad)


def _ptrs(ops, *ts):
    return [ops._ptr(t) for t in ts]


@pytest.mark.parametrize('with_t', [True, False], ids=['t', 'first-layer'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('ki', range(len(U_CASES)), ids=U_IDS)
def test_stats_finalize_apply_max_against_float64(device, capsys, ki, training, with_t):
    """mbv_pfn_stats (adds t to y and y_pad in place, Σ y and Σ y² with the padded row P - n times) + mbv_pfn_bn_finalize +
    mbv_pfn_apply_max.  with_t = False is the first layer's form: no pillar term, y_pad = W·0 = 0."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    c = _given(ki)
    ypad0 = c.ypad0 if with_t else torch.zeros_like(c.ypad0)
    if with_t:
        r64, r32 = c.fwd[(training, True, F64)], c.fwd[(training, True, F32)]
    else:
        r64, r32 = (step_forward(c.y0, ypad0, None, c.gamma, c.beta, c.rm, c.rv, c.n, c.p, training, dt) for dt in (F64, F32))
    y, ypad, gamma, beta, rm, rv = (x.clone().to(device) for x in (c.y0, ypad0, c.gamma, c.beta, c.rm, c.rv))
    t = c.t.to(device) if with_t else None
    rs, nump = c.row_start.to(device), c.n.to(device)
    sums = torch.full((2 * c.u,), float('nan'), dtype=F64, device=device)
    scale, shift, mean, rstd = (torch.full((c.u,), float('nan'), device=device) for _ in range(4))
    a, apad, m = (torch.full(s, float('nan'), device=device) for s in ((c.k, c.u), (c.v, c.u), (c.v, c.u)))
    st = ops._stream()
    ops.check(lib.mbv_pfn_stats(*_ptrs(ops, y, t, ypad, rs, nump), c.v, c.u, c.p, ops._ptr(sums), st), 'mbv_pfn_stats')
    ops.check(lib.mbv_pfn_bn_finalize(ops._ptr(sums), float(c.v * c.p), *_ptrs(ops, gamma, beta), R.EPS, R.MOMENTUM,
                                      1 if training else 0, *_ptrs(ops, rm, rv), c.u, *_ptrs(ops, scale, shift, mean, rstd), st),
              'mbv_pfn_bn_finalize')
    ops.check(lib.mbv_pfn_apply_max(*_ptrs(ops, y, ypad, scale, shift, rs, nump), c.v, c.u, c.p, *_ptrs(ops, a, apad, m), st),
              'mbv_pfn_apply_max')
    has_pad = (c.n.view(-1, 1) < c.p).to(device)
    got = dict(y=y, y_pad=ypad, sums=sums, mean=mean, rstd=rstd, scale=scale, shift=shift, running_mean=rm, running_var=rv, a=a,
               a_pad=apad * has_pad, m=m)
    bad = []
    tag = f'{U_IDS[ki]} {"train" if training else "eval"} {"t" if with_t else "first-layer"}'
    for key, val in got.items():
        assert torch.isfinite(val).all(), key
        if key == 'y_pad' and not with_t:
            assert float(val.abs().max()) == 0.0
            continue
        _cmp(capsys, f'{tag} {key}', val, r64[key], r32[key], bad)
    assert not bad, bad


@pytest.mark.parametrize('has_da', [True, False], ids=['dA', 'last-layer'])
@pytest.mark.parametrize('ki', range(len(U_CASES)), ids=U_IDS)
def test_bwd_route_against_float64(device, capsys, ki, has_da):
    """mbv_pfn_bwd_route: dM through the max (first maximal slot, padded copies behind the real rows), + dA, relu', the
    BatchNorm-backward sums (d beta, d gamma)."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    c = _given(ki)
    r64, r32 = c.route[(has_da, F64)], c.route[(has_da, F32)]
    out_rows, out_pairs = _left_out(c)
    y, ypad, scale, shift, mean, rstd, dm, rs, nump = (x.to(device) for x in (c.y, c.ypad, c.scale, c.shift, c.mean, c.rstd, c.dm,
                                                                              c.row_start, c.n))
    dz = c.da.clone().to(device) if has_da else torch.full((c.k, c.u), float('nan'), device=device)
    sapad = c.sapad.to(device) if has_da else None
    dzpad = torch.full((c.v, c.u), float('nan'), device=device)
    sums = torch.full((2 * c.u,), float('nan'), dtype=F64, device=device)
    ops.check(lib.mbv_pfn_bwd_route(*_ptrs(ops, y, ypad, scale, shift, mean, rstd, dz), 1 if has_da else 0,
                                    *_ptrs(ops, sapad, dm, rs, nump), c.v, c.u, c.p, *_ptrs(ops, dzpad, sums), ops._stream()),
              'mbv_pfn_bwd_route')
    assert torch.isfinite(dz).all() and torch.isfinite(dzpad).all() and torch.isfinite(sums).all()
    dz, dzpad, sums = dz.cpu(), dzpad.cpu(), sums.cpu()
    bad = []
    tag = f'{U_IDS[ki]} {"dA" if has_da else "last-layer"}'
    _cmp(capsys, f'{tag} dz', dz, r64['dz'], r32['dz'], bad, out_rows)
    _cmp(capsys, f'{tag} dz_pad', dzpad, r64['dz_pad'], r32['dz_pad'], bad, out_pairs)
    # the channel sums: what the fragile pairs may move
    fr = out_pairs.unsqueeze(1).double()
    allow = (fr * c.dm.double().abs().unsqueeze(1) * (1 + c.xhat.abs())).amax(1).sum(0)          # (U,) one slot per pair takes dM
    for key, got in (('d_beta', sums[:c.u]), ('d_gamma', sums[c.u:])):
        e = float(((got - r64[key]).abs() - allow).max() / r64[key].abs().max())
        check(capsys, MOD, f'{tag} {key}', e, f32_bar(r32[key], r64[key]), bad)
    # exact: a pair whose slots are all gated off (z <= 0 everywhere, a tie at 0) carries no gradient
    dead = (c.z <= 0).all(1)
    assert int(dead.sum()) >= c.v * ((c.u + 6) // 7) * 0.9
    assert float(dz[dead[c.row_pillar]].abs().max()) == 0.0 and float(dzpad[dead].abs().max()) == 0.0
    # a pillar of duplicate points: the parameter side sees the pillar's sums — whichever copy won
    if c.dup >= 0:
        lo, hi = int(c.row_start[c.dup]), int(c.row_start[c.dup + 1])
        assert hi - lo >= 2 and torch.equal(c.y[lo:hi], c.y[lo:lo + 1].expand(hi - lo, -1))
        want = r64['dz'][lo:hi].sum(0)
        assert float(c.dm[c.dup].abs().min()) > 0 and float(want.abs().max()) > 0
        check(capsys, MOD, f'{tag} duplicate pillar Σ dz', err(dz[lo:hi].double().sum(0), want),
              f32_bar(r32['dz'][lo:hi].sum(0), want), bad)
    assert not bad, bad


@pytest.mark.parametrize('with_dt', [True, False], ids=['dt', 'first-layer'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('ki', range(len(U_CASES)), ids=U_IDS)
def test_bwd_bn_against_float64(device, capsys, ki, training, with_dt):
    """mbv_pfn_bwd_bn: the BatchNorm backward per row in place, the padded row's gradient summed over its P - n copies,
    dt[v] = Σ over all P slots (null for the first layer)."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    c = _given(ki)
    r64, r32 = c.bn[(training, F64)], c.bn[(training, F32)]
    out_rows, out_pairs = _left_out(c)
    y, ypad, dz, dzpad, mean, rstd, gamma, sums, rs, nump = (x.clone().to(device) for x in (
        c.y, c.ypad, c.dz, c.dzpad, c.mean, c.rstd, c.gamma, c.sums, c.row_start, c.n))
    dt = torch.full((c.v, c.u), float('nan'), device=device) if with_dt else None
    ops.check(lib.mbv_pfn_bwd_bn(*_ptrs(ops, y, ypad, dz, dzpad, mean, rstd, gamma, sums), float(c.v * c.p), 1 if training else 0,
                                 *_ptrs(ops, rs, nump), c.v, c.u, c.p, ops._ptr(dt), ops._stream()), 'mbv_pfn_bwd_bn')
    bad = []
    tag = f'{U_IDS[ki]} {"train" if training else "eval"}'
    got = dict(dy=(dz, out_rows), dy_pad=(dzpad, out_pairs))
    if with_dt:
        got['dt'] = (dt, out_pairs)
    for key, (val, out) in got.items():
        assert torch.isfinite(val).all(), key
        if key == 'dt' and training and c.v == 1:
            # one pillar IS the batch: dt = Σ over the batch of the BatchNorm backward, which is 0 but for the rounding of the
            # given mean (1e-7 of its terms in float64).  Such a sum is judged against the terms it adds — max over the
            # channels of Σ |dy| — not against its own size; the f32 step sets the bar in the same measure.
            terms = float((r64['dy'].abs().sum(0) + r64['dy_pad'].abs().sum(0)).max())
            assert float(r64['dt'].abs().max()) <= 1e-6 * terms
            check(capsys, MOD, f'{tag} dt (one pillar: against Σ|dy|)', float((val.double().cpu() - r64['dt']).abs().max()) / terms,
                  max(4e-6, 4 * float((r32['dt'].double() - r64['dt']).abs().max()) / terms), bad)
            continue
        _cmp(capsys, f'{tag} {key}', val, r64[key], r32[key], bad, out)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the products of the backward
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big_step():
    """A layer of 64 units over more than 8 192 rows (K2c and the split-K weight gradient start there): dy, dy_pad, dt."""
    g = torch.Generator().manual_seed(77)
    u, p, v = 64, 32, 700
    n = _num_points(v, p, 'mixed', g)
    k = int(n.sum())
    assert k > 8192
    r = lambda *s: torch.randn(*s, generator=g)
    y, ypad, dz = r(k, u), r(v, u), r(k, u)
    dzpad = r(v, u) * (n.view(-1, 1) < p)
    mean, rstd, gamma = 0.1 * r(u), 1 + 0.1 * torch.rand(u, generator=g), 1 + 0.1 * r(u)
    dzd, _ = _dense(dz.double(), _spread(dzpad.double(), n, p), n, p)
    xhat = (_dense(y.double(), ypad.double(), n, p)[0] - mean.double()) * rstd.double()
    sums = torch.cat([dzd.sum((0, 1)), (dzd * xhat).sum((0, 1))])
    return step_bn(y, ypad, dz, dzpad, mean, rstd, gamma, sums, float(v * p), True, n, p, F64), k, v, u


@pytest.mark.parametrize('which', ['U32_P8_V700', 'U128_P32_V257', 'U48_P8_V257', 'rows>8192'])
def test_backward_products_against_float64(device, capsys, which):
    """_wgrad (dy^T a_prev, dy_pad^T a_pad_prev, dt^T m_prev), d_rows = dy.mm(w) for a Fourier front end and the three _pfn_mm
    data gradients (dy·W_a, dy_pad·W_a, dt·W_b with W_a, W_b column blocks of one weight)."""
    from mask_bev_amd import ops
    if which == 'rows>8192':
        step, k, v, u = _big_step()
    else:
        c = _given({'U32_P8_V700': 0, 'U128_P32_V257': 2, 'U48_P8_V257': 3}[which])
        step, k, v, u = c.bn[(True, F64)], c.k, c.v, c.u
    dy, dypad, dt = (step[key].float() for key in ('dy', 'dy_pad', 'dt'))
    g = torch.Generator().manual_seed(k)
    cp = u                                                                # the previous layer's units
    a_prev, apad_prev, m_prev = (torch.relu(torch.randn(r, cp, generator=g)) for r in (k, v, v))
    w = torch.randn(u, 2 * cp, generator=g) / (2 * cp) ** 0.5
    rows0, w0 = torch.randn(k, 11, generator=g), torch.randn(u, 11, generator=g)
    D = lambda x: x.to(device)
    dyd, dypadd, dtd, wd = D(dy), D(dypad), D(dt), D(w)
    products = {
        'wgrad rows': (lambda: ops._wgrad(dyd, D(a_prev)), lambda f: f(dy).t() @ f(a_prev)),
        'wgrad padded': (lambda: ops._wgrad(dypadd, D(apad_prev)), lambda f: f(dypad).t() @ f(apad_prev)),
        'wgrad pillar term': (lambda: ops._wgrad(dtd, D(m_prev)), lambda f: f(dt).t() @ f(m_prev)),
        'wgrad first layer': (lambda: ops._wgrad(dyd, D(rows0)), lambda f: f(dy).t() @ f(rows0)),
        'd_rows': (lambda: dyd.mm(D(w0)), lambda f: f(dy) @ f(w0)),
        'dA': (lambda: ops._pfn_mm(dyd, wd[:, :cp], False), lambda f: f(dy) @ f(w[:, :cp])),
        'Σ dA_pad': (lambda: ops._pfn_mm(dypadd, wd[:, :cp], False), lambda f: f(dypad) @ f(w[:, :cp])),
        'dM': (lambda: ops._pfn_mm(dtd, wd[:, cp:], False), lambda f: f(dt) @ f(w[:, cp:])),
    }
    bad = []
    for name, (run, ref) in products.items():
        got, r64, r32 = run(), ref(lambda x: x.double()), ref(lambda x: x)
        assert got.dtype == F32 and got.shape == r64.shape
        check(capsys, MOD, f'{which} {name}', err(got, r64), f32_bar(r32, r64), bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# (d) K2a decoration at production ranges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pc_dim', [3, 4])
def test_decorate_at_production_ranges_against_float64(device, capsys, pc_dim):
    from mask_bev_amd import ops
    p, v, per_cell = 4, 600, 6
    g = torch.Generator().manual_seed(pc_dim)
    cells = torch.randperm(GX * GY, generator=g)[:v]
    cells = torch.cat([cells, torch.tensor([0, GX - 1, GX * (GY - 1), GX * GY - 1])]).unique()      # and the four corners
    cx, cy = (cells % GX).view(-1, 1), (cells // GX).view(-1, 1)
    u = torch.rand(cells.shape[0], per_cell, pc_dim, generator=g)
    pts = u.clone()
    pts[..., 0] = RANGE[0] + (cx + 0.05 + 0.9 * u[..., 0]) * VOXEL[0]
    pts[..., 1] = RANGE[1] + (cy + 0.05 + 0.9 * u[..., 1]) * VOXEL[1]
    pts[..., 2] = RANGE[2] + (0.05 + 0.9 * u[..., 2]) * VOXEL[2]
    pts = pts.reshape(-1, pc_dim)
    scans = [pts[torch.randperm(pts.shape[0], generator=g)], pts[torch.randperm(pts.shape[0], generator=g)][: pts.shape[0] // 2]]
    geom = ops.VoxelGeometry.from_ranges(RANGE, VOXEL)
    assert list(geom.grid) == [GX, GY, 1]
    pil = ops.voxelize([s.to(device) for s in scans], geom, p, 100000)
    rows, row_pillar = ops.pfn_decorate(pil, VOXEL, RANGE)
    n, coors = pil.num_points.cpu(), pil.coors.cpu()
    assert pil.num_pillars >= cells.shape[0] and int((n == p).sum()) >= cells.shape[0]            # the first scan: full pillars
    ref = {}
    for dt in (F64, F32):
        vox = R.dense_voxels(pil.points.cpu().to(dt), pil.pillar_points.cpu())
        ref[dt] = R.compact_rows(R.decorate(vox, n, coors, VOXEL, RANGE), n)
    assert rows.shape == ref[F64].shape == (pil.num_rows, pc_dim + 7)
    assert torch.equal(row_pillar.cpu(), _index(n)[1])
    bad = []
    check(capsys, MOD, f'decorate {pc_dim} channels', err(rows, ref[F64]), f32_bar(ref[F32], ref[F64]), bad)
    assert not bad, bad
