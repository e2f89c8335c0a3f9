"""K17 (csrc/gemm.hip, the 16-bit MFMA GEMM family) against float64 on the routes production takes.  This module holds the bars;
tests/test_k17_gemm_gpu.py keeps the workload's shapes at looser ones.

Operands are drawn on the CPU with a seeded generator and rounded to the 16-bit type; every comparison is made on the CPU in
float64 and prints ``max|got - ref64| / max|ref64|`` and its bar through f64_bars.check; misses are collected and asserted
at the end of each test.  Bars (tests/f64_bars.py, no number of this module's own):

* f32 stores, f32 accumulations and column sums: ``f32_bar = max(4e-6, 4 x e32)``, e32 the error of the float32 CPU evaluation
  of the same expression, per case and tensor.
* 16-bit stores: the error beyond one rounding of the float64 value to the type, at that same bar.
* Accumulating products: the destination is pre-filled with N(0, 1) and the reference is ``acc0 + product``; the owner-adds
  route of gemm16_tn_acc and the grouped launch run twice into the same destination.

Rounding boundaries: GELU to a 16-bit output is applied by the kernel to its own rounded pre-activation, so ``pre`` is held
to one rounding of x w^T + b and ``out`` to one rounding of gelu(pre as returned); GELU to f32 is gelu(ref64); ReLU commutes
with rounding; for EPI_DRELU / EPI_DGELU ``aux`` is an input and the reference (g w) act'(aux) uses the exact erf form; column
sums are the sums of the STORED values, so they are referenced on the returned ``out``.

Routes: every case states the block tile it expects (128 | 256 rows) and the test asserts that gemm_ref.tile_rows — the
restatement of gemm16_pick_shape, itself checked against the library through mbv_gemm16_nn_part_rows — agrees; the split of an
accumulating product, the finish of its parts and the parts of a grouped entry are restated and asserted the same way; where a
Python wrapper chooses between entry points they are counted through ``lib.hook``.  Measured errors: DESIGN.md §2."""
import functools

import pytest
import torch

from tests import gemm_ref as R
from tests.f64_bars import LO, NAME, check, err, err_beyond_one_rounding, f32_bar
from tests.gemm_ref import F32, F64, SENTINEL

MOD = 'k17-paths'
gpu = pytest.mark.gpu

# ---- cases: (expected tile rows, shape) ---------------------------------------------------------------------------------
# NT (M, N, K): the ring — nk = 1, 1, 2 ragged, 2, 3, 4 ragged, 4, 9 ragged K-steps of 32 in 3 slots —, the edges, the 256-row
# tile: (32641, 8, 8) is 128 row tiles whose last holds 129 rows (wave row 2 one row, wave row 3 none), (4096, 1000, 40) has a
# column tail of 104
NT_CASES = ([(128, (129, 128, k)) for k in (8, 32, 40, 64, 96, 104, 128, 264)]
            + [(128, (33, 8, 8)), (128, (131, 200, 72)), (128, (257, 136, 40))]
            + [(256, (32641, 8, 8)), (256, (3969, 1024, 72)), (256, (4096, 1000, 40))])
NT_BLOCK_CASES = [(128, (131, 200, 72)), (256, (3969, 1024, 72))]             # x a column block of a wider matrix (ld 1152)
# NN (M, n, K): output M x K, contraction n; the third entry: aux passed as a column block (ldaux != K)
NN_CASES = ([(128, (129, n, 128), False) for n in (8, 40, 96, 264)]
            + [(128, (131, 72, 200), True), (256, (32641, 8, 8), False), (256, (3969, 40, 1024), True)])
# TN accumulate (route, parts, (m, n, k), contiguous acc, runs into the same destination)
TN_ACC_CASES = [('owner', 4, (1032, 136, 72), True, 2),             # 2 x 1 tiles, the split capped at the 256-deep parts
                ('atomic-finish', 32, (8192, 64, 64), True, 1),     # 32 parts of fewer than 65 536 elements: gridDim.y == 2
                ('atomics', 1, (70, 768, 192), True, 1),            # one part: the GEMM's own atomics
                ('atomics', 4, (1032, 136, 72), False, 1),          # acc a column block (lddw > k): no parts
                ('atomics', 1, (31, 136, 72), True, 1),             # one ragged K-step
                ('owner', 15, (4099, 200, 72), True, 1)]            # the last part: 3 K-steps, the last of 3 rows
# TN store, batched (B, m, n, k): output (B, n, k)
TN_STORE_CASES = [(128, (3, 100, 256, 1032)), (256, (2, 40, 256, 8192))]      # 256: 1 x 64 x 2 = 128 tiles, the class of dF
# NT split-K (parts, (B, M, N, K))
NT_ACC_CASES = [(4, (2, 33, 48, 1032)), (1, (1, 130, 256, 264))]
# 3 x 3 convolution ((B, C, cout, H, W), tile of the forward, tile of the data gradient)
CONV_CASES = [((2, 32, 64, 24, 23), 128, 128), ((1, 32, 256, 126, 126), 256, 128), ((1, 256, 32, 126, 126), 128, 256)]
# fused FFN (rows, C, tile of fc1 forward and of the fused data gradient); hidden width 4 C
FFN_CASES = [(4100, 96, 128), (8200, 192, 256)]

GROUP_NAMED = [((400, 256, 256), 1), ((4096, 128, 128), 1), ((4097, 136, 72), 2), ((8200, 200, 40), 3), ((31, 8, 8), 1),
               ((777, 72, 136), 1), ((0, 64, 40), 0)]              # ((m, n, k), parts); entry 5: g a column block; entry 6: skipped
GROUP_BLOCK, GROUP_EMPTY = 5, 6
GROUP_SHAPES = [s for s, _ in GROUP_NAMED] + [(33 + 37 * i, 8 * (1 + i % 6), 8 * (1 + (i * 5) % 7)) for i in range(45)]


def _sid(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


def _ids(cases, at=1):
    return [f'{c[0]}-{_sid(c[at])}' for c in cases]


def _tile_users():
    """(gm, gn, work units) of every STORE product of this module."""
    out = [(m, n, 1) for _, (m, n, _) in NT_CASES] + [(m, k, 1) for _, (m, _, k), _ in NN_CASES]
    out += [(n, k, b) for _, (b, _, n, k) in TN_STORE_CASES]
    for (b, c, cout, h, w), _, _ in CONV_CASES:
        out += [(b * (h + 2) * (w + 2), cout, 1), (b * (h + 2) * (w + 2), c, 1)]
    out += [(rows, 4 * c, 1) for rows, c, _ in FFN_CASES]
    return out


class _Routes:
    """Counts the calls of the library's entry points (through the proxy's hook) and of the named torch functions."""

    def __init__(self, monkeypatch, torch_fns=()):
        from mask_bev_amd import _lib
        self.n = {}
        lib = _lib.load()

        def hook(name, fn, args):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*args)

        monkeypatch.setattr(lib, 'hook', hook)
        for owner, attr in torch_fns:
            monkeypatch.setattr(owner, attr, self._counted(f'torch.{attr}', getattr(owner, attr)))

    def _counted(self, name, fn):
        def run(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*a, **k)
        return run

    def of(self, *names):
        return {k: self.n.get(k, 0) for k in names}


def _cmp(capsys, tag, got, ref, bad):
    """``got`` against ``ref`` = (float64, float32) evaluations: an f32 tensor at the f32 bar, a 16-bit one beyond one rounding."""
    r64, r32 = ref
    bar = f32_bar(r32, r64)
    got = got.detach().cpu()
    if got.dtype == F32:
        check(capsys, MOD, tag, err(got, r64), bar, bad)
    else:
        check(capsys, MOD, f'{tag} (beyond one rounding)', err_beyond_one_rounding(got, r64, got.dtype), bar, bad)


def _filled(device, *shape):
    """An f32 tensor whose every word is the sentinel."""
    t = torch.empty(shape, dtype=F32, device=device)
    t.view(torch.int32).fill_(SENTINEL)
    return t


def _is_sentinel(t):
    return t.view(torch.int32) == SENTINEL


# ---- host checks (no device) ----------------------------------------------------------------------------------------------
def test_tile_rule_restatement_equals_the_library():
    """gemm_ref.tile_rows against gemm16_pick_shape through the NN layout, which exposes it: part rows = (BM / 64) x row tiles x
    batch — for every (gm, gn, batch) of this module and a sweep around the 128-tile threshold and the 0.9 efficiency ratio."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    sweep = [(256 * t + d, 128 * c - e, b) for t in (31, 32, 42, 43, 63, 64, 127, 128) for d in (-255, -129, -128, -1, 0)
             for c, b in ((1, 1), (1, 2), (1, 4), (2, 1), (3, 1), (4, 1)) for e in (0, 8, 120)]
    sweep += [(m, 128, 128) for m in (1, 128, 129, 256, 257, 384, 385, 512, 513, 640, 641, 1024, 1025, 1152, 1153, 1280, 1281)]
    seen = set()
    for gm, gn, batch in _tile_users() + sweep:
        bm = R.tile_rows(0, gm, gn, batch)
        seen.add(bm)
        assert lib.mbv_gemm16_nn_part_rows(gm, gn, batch) == (bm // 64) * R.ceil_div(gm, bm) * batch, (gm, gn, batch, bm)
    assert seen == {128, 256}
    # the sweep crosses the 0.9 ratio: 384 / 512 and 640 / 768 rows of tiles lose, 512 / 512 wins, 1152 / 1280 is the ratio itself
    assert [R.tile_rows(0, m, 128, 128) for m in (257, 384, 385, 513, 640, 641)] == [128, 128, 256, 128, 128, 256]


def test_nn_part_rows_and_workspace():
    """mbv_gemm16_nn_part_rows / mbv_gemm16_nn_workspace_bytes at the wave-row and tile edges: the restated counts, and the
    workspace holds the rows."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    for m in (1, 64, 65, 129, 256, 257, 32641):
        for k in (8, 200, 1024):
            for batch in (1, 3):
                rows = lib.mbv_gemm16_nn_part_rows(m, k, batch)
                nbytes = lib.mbv_gemm16_nn_workspace_bytes(m, k, batch)
                assert rows == R.nn_part_rows(m, k, batch) and nbytes == R.nn_workspace_bytes(m, k, batch), (m, k, batch)
                assert R.ceil_div(m, 64) * batch <= rows and rows * k * 4 <= nbytes, (m, k, batch)
    assert R.nn_dead_part_rows(32641, 8) == [511] and R.nn_dead_part_rows(129, 128) == [3] and R.nn_dead_part_rows(1, 8) == [1]
    assert lib.mbv_gemm16_nn_part_rows(0, 8, 1) == 0


def test_cases_take_the_route_they_name():
    """Every case's stated tile, split and finish against the restated rules (the GPU tests assert them again where they run)."""
    for tile, (m, n, _) in NT_CASES + NT_BLOCK_CASES:
        assert R.tile_rows(0, m, n, 1) == tile, (m, n)
    for tile, (m, _, k), _ in NN_CASES:
        assert R.tile_rows(0, m, k, 1) == tile, (m, k)
    for tile, (b, _, n, k) in TN_STORE_CASES:
        assert R.tile_rows(0, n, k, b) == tile, (b, n, k)
    for (b, c, cout, h, w), fwd, dgrad in CONV_CASES:
        mp = b * (h + 2) * (w + 2)
        assert (R.tile_rows(0, mp, cout, 1), R.tile_rows(0, mp, c, 1)) == (fwd, dgrad), (b, c, cout, h, w)
    for rows, c, tile in FFN_CASES:
        assert R.tile_rows(0, rows, 4 * c, 1) == tile, (rows, c)
    for route, parts, (m, n, k), contiguous, _ in TN_ACC_CASES:
        assert R.tn_acc_route(m, n, k, contiguous) == (route, parts), (m, n, k)
        assert R.tn_workspace_bytes(m, n, k) >= parts * n * k * 4
    for parts, (b, m, n, k) in NT_ACC_CASES:
        assert R.split(k, R.ceil_div(m, 128) * R.ceil_div(n, 128) * b)[0] == parts, (b, m, n, k)
    for (m, _, _), parts in GROUP_NAMED:
        assert (R.tn_group_parts(m) if m else 0) == parts, m
    assert len(GROUP_SHAPES) > R.TN_GROUP and R.tn_group_parts(4096) == 1 and R.tn_group_parts(4097) == 2
    assert [R.ring_steps(k) for k in (8, 32, 40, 64, 96, 104, 128, 264)] == [
        (1, True), (1, False), (2, True), (2, False), (3, False), (4, True), (4, False), (9, True)]


# ---- NT store -----------------------------------------------------------------------------------------------------------
def _nt_operands(shape, dt):
    m, n, k = shape
    seed = 1000 + m + 3 * n + 7 * k
    x, w = R.randn(seed, (m, k), dt), R.randn(seed + 1, (n, k), dt, k ** -0.5)
    b = R.randn(seed + 2, (n,), F32)
    x[m - 1] = 0                                              # a zero row, in the last (partly filled) row tile
    return x, w, b


def _nt_variants(device, capsys, tag, x, w, b, x_d, bad):
    from mask_bev_amd import ops
    w_d, b_d = w.to(device), b.to(device)
    plain = R.both(lambda x, w: x @ w.t(), x, w)
    pre = R.both(lambda x, w, b: x @ w.t() + b, x, w, b)
    dt = x.dtype
    out = ops.gemm16_nt(x_d, w_d)
    assert out.dtype == dt
    _cmp(capsys, f'{tag} plain', out, plain, bad)
    out32 = ops.gemm16_nt(x_d, w_d, b_d, out_dtype=F32)
    assert out32.dtype == F32
    _cmp(capsys, f'{tag} bias f32', out32, pre, bad)
    assert torch.equal(out32[-1].cpu(), b)                    # the zero row returns the bias exactly
    out = ops.gemm16_nt(x_d, w_d, b_d, act='relu')
    _cmp(capsys, f'{tag} relu', out, tuple(torch.relu(p) for p in pre), bad)
    out, got_pre = ops.gemm16_nt(x_d, w_d, b_d, act='gelu', want_pre=True)
    assert out.dtype == dt and got_pre.dtype == dt
    _cmp(capsys, f'{tag} gelu pre', got_pre, pre, bad)
    _cmp(capsys, f'{tag} gelu of the returned pre', out, R.both(R.gelu, got_pre.cpu()), bad)
    out32 = ops.gemm16_nt(x_d, w_d, b_d, act='gelu', out_dtype=F32)
    _cmp(capsys, f'{tag} gelu f32', out32, tuple(R.gelu(p) for p in pre), bad)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
@pytest.mark.parametrize('tile,shape', NT_CASES, ids=_ids(NT_CASES))
def test_nt_store_against_float64(device, capsys, tile, shape, dt):
    """ops.gemm16_nt: no bias to the 16-bit type; f32 bias to f32 (the MSDA value projection); ReLU and GELU (with the
    pre-activation) to the 16-bit type; GELU to f32."""
    assert R.tile_rows(0, shape[0], shape[1], 1) == tile
    x, w, b = _nt_operands(shape, dt)
    bad = []
    _nt_variants(device, capsys, f'nt {NAME[dt]} {shape} tile {tile}', x, w, b, x.to(device), bad)
    assert not bad, bad


@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
@pytest.mark.parametrize('tile,shape', NT_BLOCK_CASES, ids=_ids(NT_BLOCK_CASES))
def test_nt_store_of_a_column_block(device, capsys, tile, shape, dt):
    """The same with x as columns 384 : 384 + K of a 1152-wide matrix (ldx != K)."""
    assert R.tile_rows(0, shape[0], shape[1], 1) == tile
    x, w, b = _nt_operands(shape, dt)
    x_d = R.column_block(x, 1152, 384).to(device)[:, 384:384 + shape[2]]
    assert x_d.stride(0) == 1152 and not x_d.is_contiguous()
    bad = []
    _nt_variants(device, capsys, f'nt {NAME[dt]} {shape} tile {tile} ld 1152', x, w, b, x_d, bad)
    assert not bad, bad


# ---- NN store -----------------------------------------------------------------------------------------------------------
def _check_parts(capsys, tag, parts, rows, shape, out, bad):
    """The partial column-sum rows of one NN launch: all written, dead wave rows exactly zero, their float64 sum the column sums
    of the stored ``out``."""
    m, _, k = shape
    words = parts.flatten()
    assert rows == R.nn_part_rows(m, k)
    assert not bool(_is_sentinel(words[:rows * k]).any()), f'{tag}: a partial row was not written'
    assert bool(_is_sentinel(words[rows * k:]).all()), f'{tag}: written beyond the partial rows'
    p = words[:rows * k].view(rows, k).cpu()
    dead = R.nn_dead_part_rows(m, k)
    assert all(bool((p[r] == 0).all()) for r in dead), f'{tag}: dead wave rows {dead}'
    o = out.detach().cpu()
    r64, r32 = o.double().sum(0), o.float().sum(0)
    check(capsys, MOD, f'{tag} sum of the partial rows', err(p.double().sum(0), r64), f32_bar(r32, r64), bad)


@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
@pytest.mark.parametrize('tile,shape,aux_block', NN_CASES, ids=_ids(NN_CASES))
def test_nn_store_against_float64(device, monkeypatch, capsys, tile, shape, aux_block, dt):
    """ops.gemm16_nn: plain to the 16-bit type and to f32; EPI_DRELU / EPI_DGELU against (g w) act'(aux); the column sums of the
    stored result through k_sum_rows into a pre-filled vector, and as partial rows (wrapper with a sink; C ABI into a
    sentinel-filled tensor)."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    m, n, k = shape
    assert R.tile_rows(0, m, k, 1) == tile
    seed = 2000 + m + 3 * n + 7 * k
    g, w, aux = R.randn(seed, (m, n), dt), R.randn(seed + 1, (n, k), dt, n ** -0.5), R.randn(seed + 2, (m, k), dt)
    cs0 = R.randn(seed + 3, (k,), F32)
    g_d, w_d = g.to(device), w.to(device)
    aux_d = R.column_block(aux, 1152, 64).to(device)[:, 64:64 + k] if aux_block else aux.to(device)
    assert aux_d.stride(0) == (1152 if aux_block else k)
    tag = f'nn {NAME[dt]} {shape} tile {tile}'
    bad = []
    prod = R.both(lambda g, w: g @ w, g, w)
    ref = {a: R.both(lambda g, w, z, a=a: (g @ w) * R.dact(a, z), g, w, aux) for a in ('relu', 'gelu')}
    with monkeypatch.context() as patch:
        routes = _Routes(patch)
        _cmp(capsys, f'{tag} plain', ops.gemm16_nn(g_d, w_d), prod, bad)
        _cmp(capsys, f'{tag} plain f32', ops.gemm16_nn(g_d, w_d, out_dtype=F32), prod, bad)
        for a in ('relu', 'gelu'):
            out = ops.gemm16_nn(g_d, w_d, act=a, aux=aux_d)
            assert out.dtype == dt
            _cmp(capsys, f'{tag} d{a}', out, ref[a], bad)
        assert routes.of('mbv_gemm16_nn', 'mbv_gemm16_nn_parts') == {'mbv_gemm16_nn': 4, 'mbv_gemm16_nn_parts': 0}
        # column sums through k_sum_rows: of the 16-bit stored values (fused GELU backward), of the f32 stored values (plain)
        for a, od in (('gelu', dt), (None, F32)):
            cs = cs0.to(device)
            out = ops.gemm16_nn(g_d, w_d, act=a, aux=aux_d if a else None, colsum=cs, out_dtype=od)
            form = f'd{a}' if a else 'plain'
            _cmp(capsys, f'{tag} {form} {NAME[od]} with column sums', out, ref[a] if a else prod, bad)
            o = out.cpu()
            _cmp(capsys, f'{tag} {form} {NAME[od]} column sums of the stored values', cs,
                 (cs0.double() + o.double().sum(0), cs0 + o.float().sum(0)), bad)
        assert routes.of('mbv_gemm16_nn', 'mbv_gemm16_nn_parts') == {'mbv_gemm16_nn': 6, 'mbv_gemm16_nn_parts': 0}
        # the wrapper with a sink: mbv_gemm16_nn_parts, the rows handed on
        seen = []
        cs = cs0.to(device)
        out = ops.gemm16_nn(g_d, w_d, act='relu', aux=aux_d, colsum=cs, colsum_sink=lambda *a: seen.append(a))
        assert routes.of('mbv_gemm16_nn', 'mbv_gemm16_nn_parts') == {'mbv_gemm16_nn': 6, 'mbv_gemm16_nn_parts': 1}
    (parts, cs_seen, rows, n_seen, ld_seen), = seen
    assert cs_seen is cs and (rows, n_seen, ld_seen) == (R.nn_part_rows(m, k), k, k) and torch.equal(cs.cpu(), cs0)
    _cmp(capsys, f'{tag} drelu through the sink', out, ref['relu'], bad)
    o = out.cpu()
    p = parts[:rows * k].view(rows, k).cpu()
    check(capsys, MOD, f'{tag} drelu sum of the sink rows', err(p.double().sum(0), o.double().sum(0)),
          f32_bar(o.float().sum(0), o.double().sum(0)), bad)
    # the C ABI into a sentinel-filled parts tensor
    for a, od in (('gelu', dt), (None, F32)):
        words = int(lib.mbv_gemm16_nn_workspace_bytes(m, k, 1)) // 4
        parts = _filled(device, words)
        out = torch.empty((m, k), dtype=od, device=device)
        ops.check(lib.mbv_gemm16_nn_parts(ops._ptr(g_d), ops._ptr(w_d), ops._ptr(out), ops._ptr(aux_d if a else None),
                                          ops._ptr(parts), words * 4, m, n, k, n, k, k, aux_d.stride(0) if a else 0,
                                          ops._GEMM16_DT[dt], int(od == F32), ops._ACT[a], 1, 0, 0, 0, ops._stream()),
                  'mbv_gemm16_nn_parts')
        torch.cuda.synchronize()
        form = f'd{a}' if a else 'plain'
        _cmp(capsys, f'{tag} {form} {NAME[od]} (C ABI)', out, ref[a] if a else prod, bad)
        _check_parts(capsys, f'{tag} {form} {NAME[od]}', parts, int(lib.mbv_gemm16_nn_part_rows(m, k, 1)), shape, out, bad)
    assert not bad, bad


# ---- TN accumulate --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
@pytest.mark.parametrize('route,parts,shape,contiguous,runs', TN_ACC_CASES,
                         ids=[f'{c[0]}-{c[1]}-{_sid(c[2])}-{"c" if c[3] else "block"}' for c in TN_ACC_CASES])
def test_tn_accumulate_against_float64(device, monkeypatch, capsys, route, parts, shape, contiguous, runs, dt):
    """ops.gemm16_tn_acc with splits = 0 into a pre-filled destination: stored parts + owner adds (twice into the same
    destination), stored parts + k_add_parts ending in atomics (gridDim.y > 1), the GEMM's own atomics (one part; a destination
    that is a column block), ragged contraction tails."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    m, n, k = shape
    assert R.tn_acc_route(m, n, k, contiguous) == (route, parts)
    assert lib.mbv_gemm16_tn_workspace_bytes(m, n, k) == R.tn_workspace_bytes(m, n, k) >= parts * n * k * 4
    seed = 3000 + m + 3 * n + 7 * k
    g, x, acc0 = R.randn(seed, (m, n), dt), R.randn(seed + 1, (m, k), dt), R.randn(seed + 2, (n, k), F32)
    g_d, x_d = g.to(device), x.to(device)
    if contiguous:
        acc = acc0.to(device)
    else:
        wide = R.column_block(acc0, k + 8, 0).to(device)
        acc = wide[:, :k]
        assert not acc.is_contiguous()
    with monkeypatch.context() as patch:
        routes = _Routes(patch)
        for _ in range(runs):
            ops.gemm16_tn_acc(acc, g_d, x_d)
        assert routes.of('mbv_gemm16_tn', 'mbv_gemm16_tn_group') == {'mbv_gemm16_tn': runs, 'mbv_gemm16_tn_group': 0}
    torch.cuda.synchronize()
    bad = []
    _cmp(capsys, f'tn acc {NAME[dt]} {shape} {route} parts {parts} x{runs}', acc,
         R.both(lambda a, g, x: a + runs * (g.t() @ x), acc0, g, x), bad)
    if not contiguous:
        assert bool((wide[:, k:] == 3.0).all())               # the columns beside the block are untouched
    assert not bad, bad


# ---- TN grouped -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _group_case(dt):
    """(g, x, acc0) per entry on the CPU and the (float64, float32) references of acc0 + 2 x product."""
    ops, refs = [], []
    for i, (m, n, k) in enumerate(GROUP_SHAPES):
        g, x, acc0 = R.randn(4000 + 3 * i, (m, n), dt), R.randn(4001 + 3 * i, (m, k), dt), R.randn(4002 + 3 * i, (n, k), F32)
        ops.append((g, x, acc0))
        refs.append(R.both(lambda a, g, x: a + 2 * (g.t() @ x), acc0, g, x))
    return ops, refs


def _group_items(device, dt):
    items = []
    for i, (g, x, acc0) in enumerate(_group_case(dt)[0]):
        n = g.shape[1]
        g_d = R.column_block(g, n + 16, 8).to(device)[:, 8:8 + n] if i == GROUP_BLOCK else g.to(device)
        items.append((g_d, x.to(device), acc0.to(device)))
    assert items[GROUP_BLOCK][0].stride(0) == GROUP_SHAPES[GROUP_BLOCK][1] + 16
    return items


@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
def test_tn_group_against_float64(device, monkeypatch, capsys, dt):
    """ops.gemm16_tn_group on 52 entries (two launches of 48), twice into the same pre-filled destinations: single-part entries
    (``acc_out``: the few-token class, the depth limit 4096), multi-part entries (4097: the second part one row), a strided g,
    an empty entry (skipped, destination untouched), ragged fillers.  No atomics: a second pair of runs is bit-equal."""
    from mask_bev_amd import ops
    operands, refs = _group_case(dt)
    for (shape, parts) in GROUP_NAMED:
        assert (R.tn_group_parts(shape[0]) if shape[0] else 0) == parts
    bad = []
    runs = []
    for _ in range(2):
        items = _group_items(device, dt)
        with monkeypatch.context() as patch:
            routes = _Routes(patch)
            ops.gemm16_tn_group(items)
            ops.gemm16_tn_group(items)
            assert routes.of('mbv_gemm16_tn_group', 'mbv_gemm16_tn') == {'mbv_gemm16_tn_group': 2, 'mbv_gemm16_tn': 0}
        torch.cuda.synchronize()
        runs.append([acc.cpu() for _, _, acc in items])
    for i, (shape, acc, ref) in enumerate(zip(GROUP_SHAPES, runs[0], refs)):
        if i == GROUP_EMPTY:
            assert torch.equal(acc, operands[i][2])
            continue
        _cmp(capsys, f'tn group {NAME[dt]} {shape} parts {R.tn_group_parts(shape[0])} x2', acc, ref, bad)
    assert all(torch.equal(a, b) for a, b in zip(*runs)), 'the grouped launch is not bit-reproducible'
    assert not bad, bad


@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
def test_tn_group_with_a_repeated_destination(device, monkeypatch, capsys, dt):
    """ops.launch_tn_group with two products on ONE destination, a single-part and a three-part entry: the launcher separates
    them into successive launches (_distinct_destination_waves), and both arrive."""
    from mask_bev_amd import ops
    n, k = 136, 72
    acc0 = R.randn(4500, (n, k), F32)
    acc = acc0.to(device)
    cpu = [(R.randn(4501 + 2 * i, (m, n), dt), R.randn(4502 + 2 * i, (m, k), dt)) for i, m in enumerate((400, 8200))]
    assert [R.tn_group_parts(g.shape[0]) for g, _ in cpu] == [1, 3]
    items = [(g.to(device), x.to(device), acc) for g, x in cpu]
    other = (items[0][0], items[0][1], torch.zeros_like(acc))
    assert [len(w) for w in ops._distinct_destination_waves(items + [other])] == [2, 1]
    with monkeypatch.context() as patch:
        routes = _Routes(patch)
        ops.launch_tn_group(items)
        assert routes.of('mbv_gemm16_tn_group') == {'mbv_gemm16_tn_group': 2}
    torch.cuda.synchronize()
    bad = []
    _cmp(capsys, f'tn group {NAME[dt]} two products on one ({n}, {k}) destination', acc,
         R.both(lambda a, g0, x0, g1, x1: a + g0.t() @ x0 + g1.t() @ x1, acc0, *cpu[0], *cpu[1]), bad)
    assert not bad, bad


# ---- TN store, batched ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
@pytest.mark.parametrize('tile,shape', TN_STORE_CASES, ids=_ids(TN_STORE_CASES))
def test_tn_store_batched_against_float64(device, capsys, tile, shape, dt):
    """ops.gemm16_tn (both operands as transposed reads, stored once per tile) to the 16-bit type and to f32."""
    from mask_bev_amd import ops
    b, m, n, k = shape
    assert R.tile_rows(0, n, k, b) == tile
    g, x = R.randn(5000 + m + k, (b, m, n), dt), R.randn(5001 + m + k, (b, m, k), dt)
    ref = R.both(lambda g, x: g.transpose(1, 2) @ x, g, x)
    g_d, x_d = g.to(device), x.to(device)
    bad = []
    tag = f'tn store {NAME[dt]} {shape} tile {tile}'
    out = ops.gemm16_tn(g_d, x_d)
    assert out.dtype == dt and out.shape == (b, n, k)
    _cmp(capsys, tag, out, ref, bad)
    _cmp(capsys, f'{tag} f32', ops.gemm16_tn(g_d, x_d, out_dtype=F32), ref, bad)
    assert not bad, bad


# ---- NT split-K -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
@pytest.mark.parametrize('parts,shape', NT_ACC_CASES, ids=_ids(NT_ACC_CASES))
def test_nt_split_k_against_float64(device, capsys, parts, shape, dt):
    """ops.gemm16_nt_acc (the wrapper zeroes the result) and one direct mbv_gemm16_nt_acc into a pre-filled ``acc``: the ABI
    accumulates."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    b, m, n, k = shape
    assert R.split(k, R.ceil_div(m, 128) * R.ceil_div(n, 128) * b)[0] == parts
    x, w = R.randn(6000 + m + k, (b, m, k), dt), R.randn(6001 + m + k, (b, n, k), dt)
    acc0 = R.randn(6002 + m + k, (b, m, n), F32)
    x_d, w_d = x.to(device), w.to(device)
    bad = []
    tag = f'nt split-K {NAME[dt]} {shape} parts {parts}'
    out = ops.gemm16_nt_acc(x_d, w_d)
    assert out.dtype == F32
    _cmp(capsys, tag, out, R.both(lambda x, w: x @ w.transpose(1, 2), x, w), bad)
    acc = acc0.to(device)
    ops.check(lib.mbv_gemm16_nt_acc(ops._ptr(x_d), ops._ptr(w_d), ops._ptr(acc), m, n, k, k, k, n, ops._GEMM16_DT[dt], 0, b,
                                    m * k, n * k, m * n, ops._stream()), 'mbv_gemm16_nt_acc')
    torch.cuda.synchronize()
    _cmp(capsys, f'{tag} into a pre-filled acc (C ABI)', acc, R.both(lambda a, x, w: a + x @ w.transpose(1, 2), acc0, x, w), bad)
    assert not bad, bad


@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
def test_mask_logits_backward_against_float64(device, monkeypatch, capsys, dt):
    """ops.mask_logits_backward end to end on (B 2, R 130, C 48, P 1032): d_embed by split-K NT (f32), d_feature by the batched TN
    store (16-bit); dL exactly representable in both 16-bit types."""
    from mask_bev_amd import ops
    b, r, c, p = 2, 130, 48, 1032
    dl = R.exact16(R.randn(6100, (b, r, p), F32)).to(dt)
    e, f = R.randn(6101, (b, r, c), dt, c ** -0.5), R.randn(6102, (b, c, p), dt)
    with monkeypatch.context() as patch:
        routes = _Routes(patch, [(torch, 'bmm')])
        d_e, d_f = ops.mask_logits_backward(dl.to(device), e.to(device), f.to(device))
        names = ('mbv_gemm16_nt_acc', 'mbv_gemm16_tn', 'torch.bmm')
        assert routes.of(*names) == dict(zip(names, (1, 1, 0)))
    torch.cuda.synchronize()
    assert d_e.dtype == F32 and d_f.dtype == dt
    bad = []
    tag = f'mask-logit backward {NAME[dt]} {(b, r, c, p)}'
    _cmp(capsys, f'{tag} d_embed', d_e, R.both(lambda dl, f: dl @ f.transpose(1, 2), dl, f), bad)
    _cmp(capsys, f'{tag} d_feature', d_f, R.both(lambda e, dl: e.transpose(1, 2) @ dl, e, dl), bad)
    assert not bad, bad


# ---- 3 x 3 convolution ------------------------------------------------------------------------------------------------------
def _conv_case(shape, dt):
    """Operands as ``dt`` holds them (float32 tensors) and the float64 / float32 conv2d with autograd."""
    b, c, cout, h, w = shape
    seed = 7000 + c + h
    x, wt = R.randn(seed, (b, c, h, w), dt).float(), R.randn(seed + 1, (cout, c, 3, 3), dt, (9 * c) ** -0.5).float()
    gy = R.randn(seed + 2, (b, cout, h, w), dt).float()
    res = []
    for fdt in (F64, F32):
        xd, wd = x.to(fdt).clone().requires_grad_(), wt.to(fdt).clone().requires_grad_()
        y = torch.nn.functional.conv2d(xd, wd, padding=1)
        y.backward(gy.to(fdt))
        res.append((y.detach(), xd.grad, wd.grad))
    return x, wt, gy, tuple(zip(*res))


@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
@pytest.mark.parametrize('shape,fwd,dgrad', CONV_CASES, ids=[_sid(c[0]) for c in CONV_CASES])
def test_conv3x3_against_float64(device, monkeypatch, capsys, shape, fwd, dgrad, dt):
    """ops.conv3x3_16 (EPI_CONV forward and data gradient, nine grouped TN entries for the weight gradient) against the float64
    conv2d of the same 16-bit operands; the pixels on the map's edge — whose taps read the zero border of the padded rows —
    are compared on their own as well."""
    from mask_bev_amd import ops
    b, c, cout, h, w = shape
    mp = b * (h + 2) * (w + 2)
    assert (R.tile_rows(0, mp, cout, 1), R.tile_rows(0, mp, c, 1)) == (fwd, dgrad)
    x, wt, gy, (ry, rgx, rgw) = _conv_case(shape, dt)
    x_d = x.to(device=device, dtype=dt).requires_grad_()
    w_d = wt.to(device).requires_grad_()
    with monkeypatch.context() as patch:
        routes = _Routes(patch)
        y = ops.conv3x3_16(x_d, w_d)
        y.backward(gy.to(device=device, dtype=dt))
        names = ('mbv_conv3x3_gemm16', 'mbv_gemm16_tn_group')
        assert routes.of(*names) == dict(zip(names, (2, 1)))
    torch.cuda.synchronize()
    assert y.dtype == dt and x_d.grad.dtype == dt and w_d.grad.dtype == F32
    bad = []
    tag = f'conv3x3 {NAME[dt]} {shape} tiles {fwd}/{dgrad}'
    _cmp(capsys, f'{tag} y', y, ry, bad)
    _cmp(capsys, f'{tag} d x', x_d.grad, rgx, bad)
    _cmp(capsys, f'{tag} d w', w_d.grad, rgw, bad)

    def edge(t):
        return torch.cat([t[..., 0, :].flatten(), t[..., -1, :].flatten(), t[..., :, 0].flatten(), t[..., :, -1].flatten()])
    _cmp(capsys, f'{tag} y on the edge', edge(y.detach().cpu()), tuple(edge(r) for r in ry), bad)
    _cmp(capsys, f'{tag} d x on the edge', edge(x_d.grad.cpu()), tuple(edge(r) for r in rgx), bad)
    assert not bad, bad


# ---- the fused FFN as production runs it ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dt', LO, ids=NAME.get)
@pytest.mark.parametrize('kind', ['gelu', 'relu'])
@pytest.mark.parametrize('rows,c,tile', FFN_CASES, ids=[f'{c[0]}x{c[1]}-tile{c[2]}' for c in FFN_CASES])
def test_fused_ffn_equals_its_building_blocks(device, monkeypatch, capsys, rows, c, tile, kind, dt):
    """layers.FFN under policy ``auto`` with arena parameters and 16-bit autocast, forward and backward into a pre-filled arena
    gradient, against the same chain issued from the building blocks on the same operands — gemm16_nt(act, want_pre), the
    library linear for fc2, gemm16_nn(act, aux, colsum, colsum_sink), the two weight gradients through the grouped launch, the
    library product for d x: the entry points are counted, and y, d x, d W1, d W2 are bit-equal.  d b1 is not: on this route its
    partial rows are reduced by k_colsum_group (mbv_colsum_accum_group), whose row slices finish with f32 atomics, so it is held to
    the f32 bar.  Each block's result is then held against float64 given the RETURNED output of the block before it."""
    from mask_bev_amd import layers, ops, switches
    from mask_bev_amd.arena import ParameterArena
    f = 4 * c
    assert R.tile_rows(0, rows, f, 1) == tile and switches.get('gemm16') == 'auto' and rows >= switches.get('k17_fused_min')
    seed = 8000 + rows + c
    x = R.randn(seed, (rows, c), F32)
    g0 = R.randn(seed + 1, (rows, c), dt)
    mod = layers.FFN(c, f, act=kind).to(device)
    fc1, fc2 = mod.layers[0][0], mod.layers[1]
    with torch.no_grad():
        fc1.weight.copy_(R.randn(seed + 2, (f, c), F32, c ** -0.5))
        fc1.bias.copy_(R.randn(seed + 3, (f,), F32, 0.5))
        fc2.weight.copy_(R.randn(seed + 4, (c, f), F32, f ** -0.5))
        fc2.bias.copy_(R.randn(seed + 5, (c,), F32, 0.5))
    arena = ParameterArena([('ffn', mod)], dt)
    fill = R.randn(seed + 6, tuple(arena.grad.shape), F32).to(device)
    arena.grad.copy_(fill)
    acc0 = {k: p.grad.detach().clone() for k, p in (('w1', fc1.weight), ('b1', fc1.bias), ('w2', fc2.weight))}
    x_d, g_d = x.to(device).requires_grad_(), g0.to(device)
    k17 = ('mbv_gemm16_nt', 'mbv_gemm16_nn', 'mbv_gemm16_nn_parts', 'mbv_gemm16_tn', 'mbv_gemm16_tn_group',
           'torch.linear', 'torch.mm')
    want = dict(zip(k17, (1, 0, 1, 0, 1, 1, 1)))
    torch_fns = [(torch.nn.functional, 'linear'), (torch, 'mm')]
    # -- the module
    with monkeypatch.context() as patch:
        routes = _Routes(patch, torch_fns)
        with torch.autocast('cuda', dtype=dt):
            assert ops.ffn_fused_ok(x_d, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
            y = mod(x_d, add_identity=False)
        y.backward(g_d)
        ops.flush_deferred_grads()
        assert routes.of(*k17) == want, routes.n
    torch.cuda.synchronize()
    got = dict(y=y.detach(), dx=x_d.grad, w1=fc1.weight.grad.clone(), b1=fc1.bias.grad.clone(), w2=fc2.weight.grad.clone())
    assert got['y'].dtype == dt and got['dx'].dtype == F32
    # -- the building blocks, same operands
    w1c, w2c, b2c = (ops._compute_copy(p, dt).detach() for p in (fc1.weight, fc2.weight, fc2.bias))
    assert w1c.dtype == dt and b2c.dtype == dt
    b1 = fc1.bias.detach()
    x2 = x_d.detach().to(dt)
    blk = {k: v.clone() for k, v in acc0.items()}
    with monkeypatch.context() as patch:
        routes = _Routes(patch, torch_fns)
        if kind == 'gelu':
            a, h = ops.gemm16_nt(x2, w1c, b1, act='gelu', want_pre=True)
        else:
            a, h = ops.gemm16_nt(x2, w1c, b1, act='relu'), None
        blk['y'] = torch.nn.functional.linear(a, w2c, b2c)
        aux = a if h is None else h
        dh = ops.gemm16_nn(g_d, w2c, act=kind, aux=aux, colsum=blk['b1'], colsum_sink=ops.accumulate_colsum)
        ops.launch_tn_group([(g_d, a, blk['w2']), (dh, x2, blk['w1'])])
        blk['dx'] = torch.mm(dh, w1c, out_dtype=F32)
        assert routes.of(*k17) == want, routes.n
    torch.cuda.synchronize()
    for k in ('y', 'dx', 'w1', 'w2'):
        assert torch.equal(got[k].view(blk[k].shape), blk[k]), f'{k}: the module and its building blocks differ'
    # -- each block against float64, given the returned output of the block before it
    bad = []
    tag = f'ffn {NAME[dt]} {kind} rows {rows} C {c} tile {tile}'
    xc, w1, w2, b2, gc = x2.cpu(), w1c.cpu(), w2c.cpu(), b2c.cpu(), g0
    ac, dhc, auxc, b1c = a.cpu(), dh.cpu(), aux.cpu(), b1.cpu()
    pre = R.both(lambda x, w, b: x @ w.t() + b, xc, w1, b1c)
    if kind == 'gelu':
        _cmp(capsys, f'{tag} fc1 pre', h, pre, bad)
        _cmp(capsys, f'{tag} fc1 gelu of the returned pre', a, R.both(R.gelu, h.cpu()), bad)
    else:
        _cmp(capsys, f'{tag} fc1 relu', a, tuple(torch.relu(p) for p in pre), bad)
    _cmp(capsys, f'{tag} y (library fc2 of the returned activation)', got['y'], R.both(lambda a, w, b: a @ w.t() + b, ac, w2, b2), bad)
    _cmp(capsys, f'{tag} d hidden', dh, R.both(lambda g, w, z: (g @ w) * R.dact(kind, z), gc, w2, auxc), bad)
    sums = (acc0['b1'].cpu().double() + dhc.double().sum(0), acc0['b1'].cpu() + dhc.float().sum(0))
    _cmp(capsys, f'{tag} d b1 (module; atomic finish of k_colsum_group)', got['b1'], sums, bad)
    _cmp(capsys, f'{tag} d b1 (building blocks)', blk['b1'], sums, bad)
    _cmp(capsys, f'{tag} d W2', got['w2'], R.both(lambda a0, g, a: a0 + g.t() @ a, acc0['w2'].cpu(), gc, ac), bad)
    _cmp(capsys, f'{tag} d W1', got['w1'], R.both(lambda a0, d, x: a0 + d.t() @ x, acc0['w1'].cpu(), dhc, xc), bad)
    _cmp(capsys, f'{tag} d x (library product of the returned d hidden)', got['dx'], R.both(lambda d, w: d @ w, dhc, w1), bad)
    assert not bad, bad
