"""K3 (scatter + LayerNorm([C, ny, nx], eps 1e-3), csrc/scatter_layernorm.hip) against float64 on the paths production takes.

The reference is the dense definition on the CPU — a zero canvas, the pillar rows written into their cells, F.layer_norm — with
autograd, run in float64 (the reference) and in float32 (its error against float64 sets the bar, f64_bars.f32_bar).  Compared:
the forward, d feats, d weight, d bias of the f32 NCHW form; the bf16 / fp16 patch-token form with the upstream gradient in
the 16-bit type (its forward must be the rounding of the f32 map of the same kernel family and stay within one rounding of
float64 beyond the f32 bar; its gradients are f32 and take the f32 bars); ``accumulate = 1`` into a pre-filled gradient,
twice; d feats of the AdamW-fused backward.  Every comparison prints ``err … bar …``.

Shapes: C = 48 and 40 (one full 32-channel tile and a partial one; NCHW only); nx = 130 (scalar path, three x-tiles, tail of 2),
260 and 300 (vector path, two tiles with a tail); ny = 1; a batch whose scans are empty, a single pillar and every cell
occupied; features with a mean far from zero (50 ± 1: E[x²] - mean² in the kernel's float64 sums).  Measured: DESIGN.md §2."""
import functools
import types

import pytest
import torch

from tests.f64_bars import LO, NAME, check, err, err_beyond_one_rounding, f32_bar

pytestmark = pytest.mark.gpu
MOD = 'k3-paths'
EPS = 1e-3
F64, F32 = torch.float64, torch.float32

# C, ny, nx, scans ('empty' / 'single' / 'full' / a pillar count), feature offset
CASES = [
    (48, 5, 130, ('empty', 'single', 'full'), 0.0),
    (40, 3, 260, ('full', 25), 0.0),
    (32, 1, 300, (100, 'single'), 0.0),
    (64, 4, 300, ('full', 'empty', 77), 0.0),
    (32, 8, 260, (150, 'single'), 0.0),
    (48, 5, 130, (300, 'full'), 50.0),
    (32, 4, 260, (400, 90), 50.0),
]
IDS = [f'C{c[0]}_{c[1]}x{c[2]}_{"-".join(map(str, c[3]))}{"_offset" if c[4] else ""}' for c in CASES]
PATCH_CASES = [3, 4, 6]


def _dense_ln(feats, w, b, cells, batch, ny, nx):
    """feats (V, C) written into a zero canvas at ``cells`` = (scan of every pillar, cell of every pillar), then LayerNorm."""
    c = feats.shape[1]
    canvas = feats.new_zeros((batch, ny * nx, c)).index_put(cells, feats)
    return torch.nn.functional.layer_norm(canvas.permute(0, 2, 1).reshape(batch, c, ny, nx), [c, ny, nx], w, b, EPS)


@functools.lru_cache(maxsize=None)
def _case(ci):
    c, ny, nx, scans, offset = CASES[ci]
    g = torch.Generator().manual_seed(40 + ci)
    batch, cells_n = len(scans), ny * nx
    c2p = torch.full((batch, cells_n), -1, dtype=torch.int32)
    starts, scan_of, cell_of = [0], [], []
    for s, occ in enumerate(scans):
        count = {'empty': 0, 'single': 1, 'full': cells_n}.get(occ, occ)
        cells = torch.randperm(cells_n, generator=g)[:count]                  # pillar order is the voxeliser's business: any
        c2p[s, cells] = torch.arange(starts[-1], starts[-1] + count, dtype=torch.int32)
        starts.append(starts[-1] + count)
        scan_of.append(torch.full((count,), s, dtype=torch.long))
        cell_of.append(cells)
    v = starts[-1]
    feats = offset + torch.randn(v, c, generator=g)
    w, b = 1 + 0.1 * torch.randn(c, ny, nx, generator=g), 0.1 * torch.randn(c, ny, nx, generator=g)
    go = torch.randn(batch, c, ny, nx, generator=g)
    return types.SimpleNamespace(c=c, ny=ny, nx=nx, batch=batch, v=v, c2p=c2p, pbs=torch.tensor(starts, dtype=torch.int32),
                                 cells=(torch.cat(scan_of), torch.cat(cell_of)), feats=feats, w=w, b=b, go=go)


@functools.lru_cache(maxsize=None)
def _reference(ci, go_dtype=None):
    """{dtype: (out, d feats, d weight, d bias)} in float64 and float32; the upstream gradient rounded to ``go_dtype`` first."""
    k = _case(ci)
    go = k.go if go_dtype is None else k.go.to(go_dtype).float()
    res = {}
    for dt in (F64, F32):
        f, w, b = (t.to(dt).clone().requires_grad_() for t in (k.feats, k.w, k.b))
        out = _dense_ln(f, w, b, k.cells, k.batch, k.ny, k.nx)
        out.backward(go.to(dt))
        res[dt] = (out.detach(), f.grad, w.grad, b.grad)
    return res


def _pillars(k, device):
    return types.SimpleNamespace(cell_to_pillar=k.c2p.to(device), pillar_batch_start=k.pbs.to(device))


def _compare(capsys, tag, got, res, bad, names=('out', 'd_feats', 'd_weight', 'd_bias')):
    for i, name in enumerate(('out', 'd_feats', 'd_weight', 'd_bias')):
        if name in names:
            assert torch.isfinite(got[name]).all(), name
            check(capsys, MOD, f'{tag} {name}', err(got[name], res[F64][i]), f32_bar(res[F32][i], res[F64][i]), bad)


@pytest.mark.parametrize('ci', range(len(CASES)), ids=IDS)
def test_scatter_layernorm_f32_against_float64(device, capsys, ci):
    from mask_bev_amd import ops
    k = _case(ci)
    if k.c % 32:
        assert not ops.patch_layout_supported(k.c, 4 * k.ny, 4 * k.nx, 4)       # a partial channel tile: NCHW only
    f, w, b = (t.clone().to(device).requires_grad_() for t in (k.feats, k.w, k.b))
    out = ops.scatter_layernorm(f, w, b, _pillars(k, device), k.batch, k.ny, k.nx, EPS)
    assert out.dtype == F32 and tuple(out.shape) == (k.batch, k.c, k.ny, k.nx)
    out.backward(k.go.to(device))
    bad = []
    _compare(capsys, IDS[ci], dict(out=out, d_feats=f.grad, d_weight=w.grad, d_bias=b.grad), _reference(ci), bad)
    assert not bad, bad


@pytest.mark.parametrize('lo', LO, ids=[NAME[d] for d in LO])
@pytest.mark.parametrize('ci', PATCH_CASES, ids=[IDS[i] for i in PATCH_CASES])
def test_scatter_layernorm_patch_tokens_against_float64(device, capsys, ci, lo):
    from mask_bev_amd import ops
    k = _case(ci)
    assert ops.patch_layout_supported(k.c, k.ny, k.nx, 4)
    res = _reference(ci, lo)
    pil = _pillars(k, device)
    f, w, b = (t.clone().to(device).requires_grad_() for t in (k.feats, k.w, k.b))
    with torch.autocast('cuda', dtype=lo):
        tok = ops.scatter_layernorm(f, w, b, pil, k.batch, k.ny, k.nx, EPS, patch=4)
    assert tok.rows.dtype == lo and tuple(tok.rows.shape) == (k.batch, k.ny // 4, k.nx // 4, 16 * k.c)
    with torch.no_grad():
        img32 = ops.scatter_layernorm(f, w, b, pil, k.batch, k.ny, k.nx, EPS)
    assert torch.equal(tok.to_image(), img32.to(lo))                              # the rounding of the f32 map
    go = k.go.to(lo)
    go_rows = go.view(k.batch, k.c, k.ny // 4, 4, k.nx // 4, 4).permute(0, 2, 4, 3, 1, 5).reshape(tok.rows.shape)
    tok.rows.backward(go_rows.contiguous().to(device))
    bad = []
    tag = f'{IDS[ci]} patch {NAME[lo]}'
    check(capsys, MOD, f'{tag} out beyond one rounding', err_beyond_one_rounding(tok.to_image(), res[F64][0], lo),
          f32_bar(res[F32][0], res[F64][0]), bad)
    _compare(capsys, tag, dict(d_feats=f.grad, d_weight=w.grad, d_bias=b.grad), res, bad, ('d_feats', 'd_weight', 'd_bias'))
    assert not bad, bad


def _raw_forward(lib, ops, k, f, w, b, device):
    """mbv_scatter_layernorm_fwd2 through the C ABI: the f32 map and the (mean, rstd) of every scan the backward reads."""
    out = torch.full((k.batch, k.c, k.ny, k.nx), float('nan'), device=device)
    stats = torch.full((k.batch, 2), float('nan'), device=device)
    ws = ops._workspace(lib.mbv_scatter_layernorm_workspace_bytes(k.batch), device)
    pbs, c2p = k.pbs.to(device), k.c2p.to(device)
    ops.check(lib.mbv_scatter_layernorm_fwd2(ops._ptr(f), ops._ptr(pbs), ops._ptr(c2p), ops._ptr(w), ops._ptr(b), k.batch, k.c, k.ny,
                                             k.nx, EPS, 0, 0, ops._ptr(out), ops._ptr(stats), ops._ptr(ws), ws.numel(), None,
                                             ops._stream(), None, None), 'mbv_scatter_layernorm_fwd2')
    return out, stats, ws, pbs, c2p


@pytest.mark.parametrize('ci', [0, 1], ids=[IDS[0], IDS[1]])
def test_scatter_layernorm_backward_accumulates_against_float64(device, capsys, ci):
    """accumulate = 1 (what the arena's direct gradients use): two backward calls add twice the gradient to what d weight and
    d bias held; d feats is written, not accumulated."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    k = _case(ci)
    res = _reference(ci)
    f, w, b, go = (t.to(device) for t in (k.feats, k.w, k.b, k.go))
    _, stats, ws, pbs, c2p = _raw_forward(lib, ops, k, f, w, b, device)
    g = torch.Generator().manual_seed(9)
    pre_w, pre_b = torch.randn(k.w.shape, generator=g), torch.randn(k.b.shape, generator=g)
    g_w, g_b = pre_w.clone().to(device), pre_b.clone().to(device)
    g_f = torch.full((k.v, k.c), float('nan'), device=device)
    for _ in range(2):
        ops.check(lib.mbv_scatter_layernorm_bwd(ops._ptr(go), 0, 0, ops._ptr(f), ops._ptr(pbs), ops._ptr(c2p), ops._ptr(w),
                                                ops._ptr(stats), k.batch, k.c, k.ny, k.nx, k.v, ops._ptr(g_f), ops._ptr(g_w),
                                                ops._ptr(g_b), 1, ops._ptr(ws), ws.numel(), ops._stream(), None, None),
                  'mbv_scatter_layernorm_bwd')
    bad = []
    for name, got, pre, i in (('d_weight', g_w, pre_w, 2), ('d_bias', g_b, pre_b, 3)):
        want64, want32 = pre.double() + 2 * res[F64][i], (pre + res[F32][i]) + res[F32][i]
        check(capsys, MOD, f'{IDS[ci]} accumulate x 2 {name}', err(got, want64), f32_bar(want32, want64), bad)
    check(capsys, MOD, f'{IDS[ci]} accumulate x 2 d_feats', err(g_f, res[F64][1]), f32_bar(res[F32][1], res[F64][1]), bad)
    assert not bad, bad


def test_adamw_fused_backward_d_feats_against_float64(device, capsys):
    """mbv_scatter_layernorm_bwd_adamw (bit-identical to the plain path on parameters and moments, test_k11_arena_gpu.py):
    its d feats against float64 at C = 48, nx = 130 — with the weight it read BEFORE updating it."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    k = _case(0)
    res = _reference(0)
    f, w, b, go = (t.clone().to(device) for t in (k.feats, k.w, k.b, k.go))
    _, stats, ws, pbs, c2p = _raw_forward(lib, ops, k, f, w, b, device)
    m_w, v_w, m_b, v_b = (torch.zeros(k.w.shape, device=device) for _ in range(4))
    g_f = torch.full((k.v, k.c), float('nan'), device=device)
    ops.check(lib.mbv_scatter_layernorm_bwd_adamw(ops._ptr(go), 0, 0, ops._ptr(f), ops._ptr(pbs), ops._ptr(c2p), ops._ptr(w), ops._ptr(b),
                                                  ops._ptr(stats), k.batch, k.c, k.ny, k.nx, k.v, ops._ptr(g_f), ops._ptr(m_w),
                                                  ops._ptr(v_w), ops._ptr(m_b), ops._ptr(v_b), None, None, 0, 1e-3, 0.9, 0.999, 1e-8,
                                                  0.01, 1, 1, ops._ptr(ws), ws.numel(), ops._stream(), None, None),
              'mbv_scatter_layernorm_bwd_adamw')
    assert not torch.equal(w.cpu(), k.w) and not torch.equal(b.cpu(), k.b)         # the update happened in this launch
    bad = []
    check(capsys, MOD, f'{IDS[0]} AdamW-fused d_feats', err(g_f, res[F64][1]), f32_bar(res[F32][1], res[F64][1]), bad)
    assert not bad, bad
