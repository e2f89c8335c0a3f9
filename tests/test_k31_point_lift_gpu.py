"""K31 (lift of the predicted instances to the points, csrc/point_lift.hip) and K26b (3-D overlap of oriented boxes,
csrc/rotate_iou.hip) through the C ABI, and what is built on them: ``Predictions.lift`` / ``boxes3d``, the ``3d`` metric of
``kitti_eval`` and the launcher's ``kitti_3d`` key.

K31: labels, counts and all four z columns EQUAL to the numpy restatement (tests/point_lift_ref.py), no point and no query
excluded, into poisoned output buffers; agreement with K1's own cells; two runs bit-equal; the degenerate calls.
K26b: exactly 0 where the float64 oracle is exactly 0, otherwise within K26's bar, max(4e-6, 4 x the float32 oracle's own
error) relative to the largest reference value.  The protocol: tp / fp / fn sums exact, thresholds, precision and AP to 1e-6
against the values recorded from the reference's own functions (tests/golden/kitti_eval_3d.npz)."""
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

from tests import f64_bars
from tests import kitti_eval_ref as R
from tests import point_lift_ref as L
from tests.test_kitti_eval_cpu import golden, golden_frames
from tests.test_point_lift_cpu import MIN_OVERLAPS, golden_3d, golden_3d_frames
from tests.util_cfg import tiny_kwargs

pytestmark = pytest.mark.gpu
MODULE = 'test_k31_point_lift_gpu'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, 'tests', 'golden', 'kitti_object_sample')

# a non-square grid, 20 (x) by 12 (y) by 2 (z) cells of 0.5 m x 0.75 m x 2 m: a transposed map read cannot pass
RANGE, VOXEL, GRID = [-5.0, -4.5, -2.0, 5.0, 4.5, 2.0], [0.5, 0.75, 2.0], [20, 12, 2]
SIZES = (0, 1, 257, 1000)                 # an empty scan, and both sides of the 256-thread block
POISON = 0x5a5a5a5a


def _scans(dim, seed):
    """Four scans of SIZES points around the range, the two large ones with planted points: on cell borders, on every range
    limit, outside z, NaN and inf."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(RANGE[:3]), np.array(RANGE[3:])
    nan, inf = np.nan, np.inf
    planted = [[-5.0 + 0.5 * 7, 0.1, 0.3], [0.2, -4.5 + 0.75 * 5, -0.3], [-5.0 + 0.5 * 19, -4.5 + 0.75 * 11, 0.0],   # borders
               [-5.0, 0.1, 0.1], [5.0, 0.1, 0.1], [0.1, -4.5, 0.1], [0.1, 4.5, 0.1], [0.1, 0.1, -2.0], [0.1, 0.1, 2.0],  # limits
               [0.1, 0.1, 2.5], [0.1, 0.1, -2.5], [5.5, 0.1, 0.0], [0.1, -5.0, 0.0],                                    # outside
               [nan, 0.1, 0.0], [0.1, nan, 0.0], [0.1, 0.1, nan], [inf, 0.1, 0.0], [0.1, -inf, 0.0], [0.1, 0.1, inf],
               [0.1, 0.1, -inf]]
    out = []
    for n in SIZES:
        pts = rng.uniform(0, 1, (n, dim))
        pts[:, :3] = (lo + hi) / 2 + (pts[:, :3] * 2 - 1) * (hi - lo) / 2 * 1.1
        if n >= len(planted):
            where = rng.choice(n, len(planted), replace=False)      # spread over the blocks
            pts[where, :3] = planted
        out.append(pts.astype(np.float32))
    return out


def _instance_map(q, seed):
    """(4, 12, 20) int32: queries, -1, one entry of num_queries, one far outside; query q - 2 (if any) owns no cell; query 0
    owns a 6 x 3 patch, enough points for more than one block of the large scan."""
    rng = np.random.default_rng(seed)
    m = rng.integers(-1, q, (len(SIZES), GRID[1], GRID[0])).astype(np.int32)
    if q >= 3:
        m[m == q - 2] = -1                                           # a query without a point
    m[:, 8:11, 10:16] = 0
    m[:, 0, 3] = q                                                   # values the kernel must never index with
    m[:, 5, 0] = 2 ** 30
    m[:, 7, 9] = -5
    m[:, 2, 2] = -1
    return m


def _raw_lift(lib, device, scans, imap, q, z_bins, quantiles, prefilter, dim):
    """mbv_lift_instances into poisoned buffers (outputs and workspace) → (rc, point_query, counts, z_extent) on the host."""
    from mask_bev_amd.ops_core import _ptr, _stream
    n = sum(s.shape[0] for s in scans)
    batch = len(scans)
    pts = torch.from_numpy(np.concatenate(scans).reshape(n, dim)).to(device)
    offs = torch.tensor(np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]), dtype=torch.int32, device=device)
    tm = torch.from_numpy(imap).to(device)
    pq = torch.full((n,), POISON, dtype=torch.int32, device=device)
    counts = torch.full((batch, q), POISON, dtype=torch.int32, device=device)
    ext = torch.full((batch, q, 4), POISON, dtype=torch.int32, device=device).view(torch.float32)
    nbytes = lib.mbv_lift_instances_workspace_bytes(batch, q, z_bins)
    ws = torch.full((max(nbytes, 256),), 0x5a, dtype=torch.uint8, device=device)
    rc = lib.mbv_lift_instances(_ptr(pts), dim, n, _ptr(offs), batch, *RANGE, *VOXEL, *GRID, 1 if prefilter else 0, _ptr(tm), q,
                                z_bins, quantiles[0], quantiles[1], _ptr(pq), _ptr(counts), _ptr(ext), _ptr(ws), ws.numel(),
                                _stream())
    torch.cuda.synchronize()
    return rc, pq.cpu(), counts.cpu(), ext.cpu()


@pytest.mark.parametrize('prefilter', [True, False])
@pytest.mark.parametrize('z_bins', [1, 64])
@pytest.mark.parametrize('q', [1, 7, 1024])
@pytest.mark.parametrize('dim', [3, 4])
def test_k31_labels_counts_and_extents_equal_the_reference(device, dim, q, z_bins, prefilter):
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    scans, imap, quantiles = _scans(dim, 31 + dim), _instance_map(q, q), (0.1, 0.9)
    ref = L.lift(scans, imap, RANGE, VOXEL, GRID, q, z_bins, quantiles, prefilter)
    # the cases are there: labelled and unlabelled points, a query without a point, one fed by two blocks of one scan
    big = ref['point_query'][-SIZES[3]:]
    assert (ref['point_query'] >= 0).sum() >= 100 and (ref['point_query'] < 0).sum() >= 100
    assert (ref['counts'] == 0).any() if q > 1 else True
    assert len(set(np.flatnonzero(big == 0) // 256)) >= 2
    rc, pq, counts, ext = _raw_lift(lib, device, scans, imap, q, z_bins, quantiles, prefilter, dim)
    assert rc == 0
    assert torch.equal(pq, torch.from_numpy(ref['point_query']))
    assert torch.equal(counts, torch.from_numpy(ref['counts']))
    assert torch.equal(ext, torch.from_numpy(ref['z_extent'])), np.abs(ext.numpy() - ref['z_extent']).max()
    assert int(counts.sum()) == int((pq >= 0).sum())
    # the wrapper: the same, split per scan
    geom = ops.VoxelGeometry(RANGE, VOXEL, GRID)
    out = ops.lift_instances([torch.from_numpy(s).to(device) for s in scans], torch.from_numpy(imap).to(device), geom, q,
                             z_bins=z_bins, quantiles=quantiles, prefilter=prefilter)
    assert torch.equal(out.point_query.cpu(), pq) and torch.equal(out.counts.cpu(), counts)
    assert torch.equal(torch.stack([out.z_min, out.z_max, out.z_lo, out.z_hi], -1).cpu(), ext)
    per = out.per_scan()
    assert [p.shape[0] for p in per] == list(SIZES) and out.scan_offsets.cpu().tolist() == [0, 0, 1, 258, 1258]
    assert torch.equal(torch.cat(per).cpu(), pq)


@pytest.mark.parametrize('prefilter', [True, False])
def test_k31_agrees_with_k1(device, prefilter):
    """Every point K1 keeps carries the query of the cell K1 put it in; every point K1 rejected carries -1."""
    from mask_bev_amd import ops
    q = 7
    scans = [torch.from_numpy(s).to(device) for s in _scans(4, 5)]
    imap = torch.from_numpy(np.random.default_rng(3).integers(-1, q, (4, GRID[1], GRID[0])).astype(np.int32)).to(device)
    geom = ops.VoxelGeometry(RANGE, VOXEL, GRID)
    p = ops.voxelize(scans, geom, max_points=1300, max_voxels=5000, prefilter=prefilter)      # nothing is dropped
    out = ops.lift_instances(scans, imap, geom, q, prefilter=prefilter)
    coors, slots = p.coors.cpu().long(), p.pillar_points.cpu().long()
    want = torch.full((sum(SIZES),), -1, dtype=torch.int32)
    cell_query = imap.cpu()[coors[:, 0], coors[:, 2], coors[:, 3]]
    for v in range(slots.shape[0]):
        idx = slots[v][slots[v] >= 0]
        want[idx] = cell_query[v]
    kept = int((slots >= 0).sum())
    assert kept == int(p.num_points.sum()) and 400 < kept < sum(SIZES)
    assert torch.equal(out.point_query.cpu(), want)


def test_k31_is_deterministic(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    scans, imap = _scans(4, 9), _instance_map(7, 1)
    a = _raw_lift(lib, device, scans, imap, 7, 64, (0.05, 0.95), True, 4)
    b = _raw_lift(lib, device, scans, imap, 7, 64, (0.05, 0.95), True, 4)
    assert a[0] == b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_k31_degenerate_calls_and_error_codes(device):
    from mask_bev_amd import _lib
    from mask_bev_amd.ops_core import _ptr, _stream
    lib = _lib.load()
    scans, imap = _scans(4, 2), _instance_map(7, 2)
    # no query: every point unlabelled
    rc, pq, counts, ext = _raw_lift(lib, device, scans, imap, 0, 8, (0.0, 1.0), True, 4)
    assert rc == 0 and pq.shape[0] == sum(SIZES) and bool((pq == -1).all()) and counts.numel() == 0
    # no point: counts and extents zero
    rc, pq, counts, ext = _raw_lift(lib, device, [s[:0] for s in scans], imap, 7, 8, (0.0, 1.0), True, 4)
    assert rc == 0 and pq.numel() == 0 and not counts.any() and not ext.view(torch.int32).any()
    pts = torch.from_numpy(np.concatenate(scans)).to(device)
    offs = torch.tensor([0, 0, 1, 258, 1258], dtype=torch.int32, device=device)
    tm = torch.from_numpy(imap).to(device)
    n = pts.shape[0]

    def call(points=pts, dim=4, q=7, z_bins=8, q_lo=0.0, q_hi=1.0, ws_bytes=None, m=tm, gx=GRID[0]):
        pq = torch.empty((n,), dtype=torch.int32, device=device)
        counts = torch.empty((4, max(q, 1)), dtype=torch.int32, device=device)
        ext = torch.empty((4, max(q, 1), 4), dtype=torch.float32, device=device)
        ws = torch.empty((1 << 20,), dtype=torch.uint8, device=device)
        rc = lib.mbv_lift_instances(_ptr(points), dim, n, _ptr(offs), 4, *RANGE, *VOXEL, gx, GRID[1], GRID[2], 1, _ptr(m), q,
                                    z_bins, q_lo, q_hi, _ptr(pq), _ptr(counts), _ptr(ext), _ptr(ws),
                                    ws.numel() if ws_bytes is None else ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc

    BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
    assert call() == 0
    assert call(points=None) == BAD_ARG and call(m=None) == BAD_ARG
    assert call(dim=5) == BAD_ARG and call(dim=2) == BAD_ARG
    assert call(q=1025) == UNSUPPORTED
    assert call(z_bins=0) == BAD_ARG and call(z_bins=257) == BAD_ARG
    assert call(q_lo=0.6, q_hi=0.4) == BAD_ARG and call(q_lo=-0.1) == BAD_ARG and call(q_hi=1.5) == BAD_ARG
    assert call(q_lo=float('nan')) == BAD_ARG
    assert call(gx=0) == BAD_ARG
    assert call(ws_bytes=16) == WORKSPACE
    assert lib.mbv_lift_instances_workspace_bytes(4, 1025, 8) == 0 and lib.mbv_lift_instances_workspace_bytes(4, 7, 0) == 0
    assert lib.mbv_lift_instances_workspace_bytes(4, 7, 8) >= 4 * 7 * (8 + 2) * 4


# ------------------------------------------------------------------------------------------------ K26b
def _k26b_tables():
    rng = np.random.default_rng(262)
    sizes = [(8, 12), (0, 5), (10, 10)]                                # 96 + 0 + 100 pairs; a frame with no boxes

    def rand(n):
        return np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-2, 0, n), rng.uniform(1, 6, n),
                         rng.uniform(1, 6, n), rng.uniform(0.5, 3, n), rng.uniform(-np.pi, np.pi, n)], axis=1).reshape(n, 7)

    a, b = [rand(n) for n, _ in sizes], [rand(k) for _, k in sizes]
    for f in (0, 2):                                                   # dense enough to overlap
        n, k = sizes[f]
        for j in range(k):
            b[f][j, :3] = a[f][j % n, :3] + rng.uniform(-1.5, 1.5, 3) * [1, 1, 0.5]
    box = np.array([2.5, -3.25, -1.0, 4.5, 1.75, 1.5, 0.4])
    a[2][0], b[2][0] = box, box                                                       # identical
    a[2][1], b[2][1] = box, box + [0.25, 0.5, 1.5, 0, 0, 0, 0.1]                      # its bottom on the other's top
    a[2][2], b[2][2] = box + [0, 0, 1.5, 0, 0, 0.5, 0], box + [0.1, 0, 0, 0, 0, 0, 0]  # the same, the other way round
    a[2][3], b[2][3] = box, box + [0, 0, 0.75, 0, 0, 0, 0]                            # half the height in common
    a[2][4], b[2][4] = box, box + [30, 0, 0, 0, 0, 0, 0]                              # apart in BEV
    return sizes, [x.astype(np.float32) for x in a], [x.astype(np.float32) for x in b]


@pytest.fixture(scope='module')
def k26b_refs():
    sizes, a, b = _k26b_tables()
    inter64 = [L.intersection_3d(x, y, np.float64) for x, y in zip(a, b)]
    inter32 = [L.intersection_3d(x, y, np.float32) for x, y in zip(a, b)]
    return sizes, a, b, inter64, inter32


def test_k26b_rotate_iou_3d(device, capsys, k26b_refs):
    from mask_bev_amd import kitti_eval as KE, ops
    sizes, a, b, inter64, inter32 = k26b_refs
    ta, tb = torch.from_numpy(np.concatenate(a)).to(device), torch.from_numpy(np.concatenate(b)).to(device)
    off_a = np.concatenate([[0], np.cumsum([n for n, _ in sizes])])
    off_b = np.concatenate([[0], np.cumsum([k for _, k in sizes])])
    bad, offsets = [], None
    for criterion in (-1, 0, 1, 2):
        got, offsets = ops.rotate_iou_3d(ta, tb, off_a, off_b, criterion=criterion, offsets=offsets)
        assert got.dtype == torch.float32 and got.numel() == sum(n * k for n, k in sizes) == offsets.total == 196
        ref64 = np.concatenate([L.overlap_from_intersection_3d(i, x, y, criterion).reshape(-1) for i, x, y in zip(inter64, a, b)])
        ref32 = np.concatenate([L.overlap_from_intersection_3d(i, x, y, criterion).reshape(-1) for i, x, y in zip(inter32, a, b)])
        g = got.cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(g))
        zero = ref64 == 0
        assert (~zero).sum() >= 20 and zero.sum() >= 100 and np.all(g[zero] == 0), (criterion, np.flatnonzero(zero & (g != 0))[:5])
        bar = f64_bars.f32_bar(torch.from_numpy(ref32.astype(np.float64)), torch.from_numpy(ref64))
        f64_bars.check(capsys, MODULE, f'K26b criterion {criterion}', f64_bars.err(torch.from_numpy(g), torch.from_numpy(ref64)),
                       bar, bad)
        last = g[offsets.pairs[2]:].reshape(10, 10)
        assert last[1, 1] == 0 and last[2, 2] == 0 and last[4, 4] == 0                     # touching in z, apart in BEV
        scale = np.abs(ref64).max()
        if criterion == -1:
            assert abs(last[0, 0] - 1.0) <= bar * scale and abs(last[3, 3] - 1.0 / 3.0) <= bar * scale
        if criterion == 2:
            assert abs(last[0, 0] - 4.5 * 1.75 * 1.5) <= bar * scale
    assert not bad, bad
    # one frame through kitti_eval.d3_box_overlap; an empty table; the BEV kernel is untouched by the height columns
    one = KE.d3_box_overlap(a[0], b[0])
    assert one.shape == (8, 12) and np.array_equal(one.reshape(-1), ops.rotate_iou_3d(ta[:8], tb[:12])[0].cpu().numpy())
    got, o = ops.rotate_iou_3d(ta[:0], tb[:5])
    assert got.numel() == 0 and o.total == 0
    bev, _ = ops.rotate_iou(ta[:8, L.BEV].contiguous(), tb[:12, L.BEV].contiguous(), criterion=2)
    vol, _ = ops.rotate_iou_3d(ta[:8], tb[:12], criterion=2)
    dz = torch.from_numpy(L.z_overlap(a[0], b[0], np.float32).reshape(-1)).to(device)
    want = torch.where(dz > 0, bev * dz, torch.zeros_like(bev))
    assert torch.equal(vol == 0, want == 0) and float((vol - want).abs().max()) <= f64_bars.F32_BAR * float(want.max())
    with pytest.raises(ValueError):
        ops.rotate_iou_3d(ta, tb, [0, 3], off_b)


# ------------------------------------------------------------------------------------------------ the protocol, 3-D
def _product_inputs(frames, device):
    labels = [gt for gt, _ in frames]
    preds = [dict(boxes=torch.from_numpy(dt['boxes']).float().to(device), boxes3d=torch.from_numpy(dt['boxes3d']).float().to(device),
                  score=torch.from_numpy(dt['score']).float().to(device), type=torch.from_numpy(dt['type'])) for _, dt in frames]
    return labels, preds


def test_eval_class_3d_equals_the_reference(device):
    from mask_bev_amd import kitti_eval as KE
    g = golden_3d()
    frames = golden_3d_frames(g)
    labels, preds = _product_inputs(frames, device)
    got = KE.eval_class(labels, preds, [0], (0, 1, 2), metric='3d')
    assert got['min_overlaps'].reshape(-1).tolist() == list(MIN_OVERLAPS)                 # the reference's table, Car
    assert got['precision'].shape == (1, 3, 2, 41) and np.array_equal(got['num_valid_gt'][0], g['num_valid_gt'])
    assert np.array_equal(got['num_thresholds'][0], g['num_thresholds'])
    assert np.array_equal(got['stats'][0], g['stats'])                                    # tp / fp / fn sums: exact
    assert np.abs(got['thresholds'][0] - g['thresholds']).max() <= 1e-6
    assert np.abs(got['precision'][0] - g['precision']).max() <= 1e-6
    assert np.abs(KE.get_mAP(got['precision'])[0] - g['ap']).max() <= 1e-6
    # the text: a `3d   AP:` line after every `bev  AP:` line, formatted as the reference prints it
    text = KE.eval_kitti(labels, preds)
    lines = text.splitlines()
    assert len(lines) == 6 and lines[0] == 'Car AP(Average Precision)@0.70:' and lines[3] == 'Car AP(Average Precision)@0.50:'
    assert lines[1].startswith('bev  AP:') and lines[4].startswith('bev  AP:')
    assert lines[2] == '3d   AP:' + ', '.join(f'{v:.2f}' for v in g['ap'][:, 0])
    assert lines[5] == '3d   AP:' + ', '.join(f'{v:.2f}' for v in g['ap'][:, 1])
    assert set(text.metrics['Car']) == {'bev_ap@0.70', 'bev_ap@0.50', '3d_ap@0.70', '3d_ap@0.50'}
    assert text.metrics['Car']['3d_ap@0.50']['hard'] == pytest.approx(g['ap'][2, 1], abs=1e-6)
    assert np.array_equal(text.raw['3d']['stats'][0], g['stats']) and 'precision' in text.raw
    # one dictionary without boxes3d: the BEV text alone, as before
    fewer = [dict(p) for p in preds]
    del fewer[4]['boxes3d']
    bev_only = KE.eval_kitti(labels, fewer)
    assert bev_only.splitlines() == [lines[0], lines[1], lines[3], lines[4]] and '3d' not in bev_only.raw
    assert set(bev_only.metrics['Car']) == {'bev_ap@0.70', 'bev_ap@0.50'}
    with pytest.raises(ValueError):
        KE.eval_class(labels, fewer, [0], (0, 1, 2), metric='3d')


def test_eval_kitti_text_without_boxes3d_is_unchanged(device):
    """The BEV fixture through ``eval_kitti``: the string built from tests/golden/kitti_eval.npz, byte for byte, and no key
    beyond the two BEV ones."""
    from mask_bev_amd import kitti_eval as KE
    g = golden()
    frames = golden_frames(g)
    labels = [gt for gt, _ in frames]
    preds = [dict(boxes=torch.from_numpy(dt['boxes']).float().to(device), score=torch.from_numpy(dt['score']).float().to(device),
                  type=torch.from_numpy(dt['type'])) for _, dt in frames]
    text = KE.eval_kitti(labels, preds)
    want = ''
    for k, mo in enumerate((0.7, 0.5)):
        want += f'Car AP(Average Precision)@{mo:.2f}:\n' + 'bev  AP:' + ', '.join(f'{v:.2f}' for v in g['ap'][:, k]) + '\n'
    assert str(text) == want
    assert set(text.metrics['Car']) == {'bev_ap@0.70', 'bev_ap@0.50'} and '3d' not in text.raw
    assert set(text.raw) == {'precision', 'thresholds', 'num_thresholds', 'stats', 'num_valid_gt', 'min_overlaps'}


# ------------------------------------------------------------------------------------------------ end to end, tiny
X_RANGE, Y_RANGE, Z_RANGE, VS = (0.0, 16.0), (-6.0, 6.0), (-3.0, 5.0), 0.25          # a 64 (x) by 48 (y) grid
BOXES = np.array([[4.0, -2.5, -1.75, 4.0, 1.75, 1.5, 0.3],
                  [10.5, 2.0, -1.5, 4.5, 2.0, 1.625, -1.1],
                  [6.0, 3.5, -1.875, 3.5, 1.75, 1.375, 2.4]])


def _e2e_points(owner):
    """Per box 300 points inside the middle half of its footprint and inside [z, z + h], one at its exact bottom and one at its exact top;
    ground clutter in the cells no box owns (``owner``: the (48, 64) host copy of the map); one outlier 3 m above box 1."""
    rng = np.random.default_rng(7)
    pts = []
    for x, y, z, l, w, h, yaw in BOXES:
        u, v = rng.uniform(-0.25, 0.25, 300) * l, rng.uniform(-0.25, 0.25, 300) * w
        px, py = x + u * np.cos(yaw) - v * np.sin(yaw), y + u * np.sin(yaw) + v * np.cos(yaw)
        pz = z + rng.uniform(0.0, 1.0, 300) * h
        pts.append(np.stack([px, py, pz], 1))
        pts.append(np.array([[x, y, z], [x, y, z + h]]))
    clutter = np.stack([rng.uniform(0.1, 15.9, 600), rng.uniform(-5.9, 5.9, 600), rng.uniform(-2.2, -1.9, 600)], 1)
    cx, cy = ((clutter[:, 0] - X_RANGE[0]) / VS).astype(int), ((clutter[:, 1] - Y_RANGE[0]) / VS).astype(int)
    pts.append(clutter[owner[cy, cx] < 0])
    pts.append(np.array([[BOXES[1, 0], BOXES[1, 1], BOXES[1, 2] + BOXES[1, 5] + 3.0]]))
    pts = np.concatenate(pts)
    pts = pts[rng.permutation(pts.shape[0])]
    return np.concatenate([pts, rng.uniform(0, 1, (pts.shape[0], 1))], 1).astype(np.float32)


def test_end_to_end_boxes3d_and_3d_ap(device):
    from mask_bev_amd import batch as B, kitti_eval as KE, ops, rasterize
    from mask_bev_amd.predict import Predictions
    q = 6
    rz = rasterize.KittiRasterizer(X_RANGE, Y_RANGE, Z_RANGE, VS, device=device)
    assert (rz.nx, rz.ny) == (64, 48)
    maps = rz.rasterize_batch([BOXES])                                             # (1, nx, ny), ids 1 .. 3
    labels, pm = B.instance_targets(maps, q, packed=True)
    imap = (maps.permute(0, 2, 1).to(torch.int32) - 1).contiguous()                # (1, ny, nx): query = id - 1, -1 = none
    owner = imap[0].cpu().numpy()
    assert sorted(set(owner.reshape(-1).tolist())) == [-1, 0, 1, 2]
    scores = torch.tensor([[0.9, 0.8, 0.7, 0.0, 0.0, 0.0]], device=device)
    p = Predictions(labels.to(torch.int32), scores, labels > 0, pm, None, None, imap, (48, 64))
    geom = ops.VoxelGeometry.from_ranges([X_RANGE[0], Y_RANGE[0], Z_RANGE[0], X_RANGE[1], Y_RANGE[1], Z_RANGE[1]],
                                         [VS, VS, Z_RANGE[1] - Z_RANGE[0]])
    assert list(geom.grid) == [64, 48, 1]
    pts = _e2e_points(owner)
    ref = L.lift([pts], owner[None], geom.pc_range, geom.voxel_size, geom.grid, q)
    assert ref['counts'][0, :3].tolist() == [302, 303, 302] and not ref['counts'][0, 3:].any()      # every planted point lands
    scans = [torch.from_numpy(pts).to(device)]
    lifted = p.lift(scans, geom)
    assert torch.equal(lifted.point_query.cpu(), torch.from_numpy(ref['point_query']))
    out = p.boxes3d(scans, geom, rz)
    f = np.float32
    assert out['points'].cpu().tolist() == [302, 303, 302] and out['query'].cpu().tolist() == [0, 1, 2]
    b3 = out['boxes3d'].cpu().numpy()
    assert b3.dtype == np.float32 and b3.shape == (3, 7)
    want_z = BOXES[:, 2].astype(f)
    want_top = (BOXES[:, 2] + BOXES[:, 5]).astype(f)
    want_top[1] = f(BOXES[1, 2] + BOXES[1, 5] + 3.0)                                # the outlier stretches box 1
    assert np.array_equal(b3[:, 2], want_z) and np.array_equal(b3[:, 5], want_top - want_z)
    assert np.array_equal(b3[:, [0, 1, 3, 4, 6]], p.boxes(rz)['boxes'].cpu().numpy())
    # the quantile extent brings box 1 back to within one histogram bin (8 m / 64) of the planted height
    bw = (Z_RANGE[1] - Z_RANGE[0]) / 64
    robust = p.boxes3d(scans, geom, rz, extent=(0.02, 0.98))['boxes3d'].cpu().numpy()
    assert np.all(np.abs(robust[:, 5] - BOXES[:, 5]) <= bw) and np.all(np.abs(robust[:, 2] - BOXES[:, 2]) <= bw)
    assert abs(b3[1, 5] - BOXES[1, 5]) > 2.9
    # min_points drops rows; a mask without a return has no box
    assert p.boxes3d(scans, geom, rz, min_points=303)['query'].cpu().tolist() == [1]
    none = p.boxes3d([scans[0][:0]], geom, rz)
    assert none['boxes3d'].shape == (0, 7) and none['points'].numel() == 0
    # eval_kitti on these predictions against the float64 protocol oracle on the same boxes
    lab = dict(boxes=BOXES, type=np.zeros(3, dtype=np.int64), occluded=np.zeros(3, dtype=np.int64), truncated=np.zeros(3),
               bbox=np.array([[0.0, 0.0, 50.0, 80.0]] * 3))
    preds = p.kitti_predictions(rz, scans=scans, module=geom, extent=(0.02, 0.98))
    assert len(preds) == 1 and np.array_equal(preds[0]['boxes3d'].cpu().numpy(), robust)
    assert torch.equal(preds[0]['boxes'], preds[0]['boxes3d'][:, [0, 1, 3, 4, 6]])
    assert set(p.kitti_predictions(rz)[0]) == {'boxes', 'score', 'type'}
    text = KE.eval_kitti([lab], preds)
    dt = dict(type=np.zeros(3, dtype=np.int64), score=preds[0]['score'].double().cpu().numpy())
    ov = [L.rotate_iou_3d(robust.astype(np.float64), BOXES)]
    assert np.abs(ov[0] - 0.5).min() > 1e-3 and np.abs(ov[0] - 0.7).min() > 1e-3 and ov[0].max() > 0.5
    res = R.eval_class([(lab, dt)], ov, 0, (0, 1, 2), MIN_OVERLAPS)
    want_ap = R.get_map(res['precision'])                                          # (3, 2)
    lines = text.splitlines()
    assert len(lines) == 6 and lines[2].startswith('3d   AP:') and lines[5].startswith('3d   AP:')
    for k, mo in enumerate(('0.70', '0.50')):
        got = [text.metrics['Car'][f'3d_ap@{mo}'][d] for d in ('easy', 'moderate', 'hard')]
        assert np.abs(np.array(got) - want_ap[:, k]).max() <= 1e-6
        assert lines[2 + 3 * k] == '3d   AP:' + ', '.join(f'{v:.2f}' for v in want_ap[:, k])


# ------------------------------------------------------------------------------------------------ the launcher
def test_launcher_writes_point_labels(device, tmp_path):
    """``write_point_labels`` (behind ``--write-labels``): one ``.label`` per scan under sequences/SS/predictions, holding the
    lifted queries of that scan as SemanticKITTI packs them."""
    from mask_bev_amd.evaluate import write_point_labels
    from mask_bev_amd import batch as B
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from tests.util_cfg import random_scans
    kw = tiny_kwargs()
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    d = tmp_path / 'data' / 'sequences' / '08' / 'velodyne'
    d.mkdir(parents=True)
    scans = random_scans(kw, [1500, 1201, 900], seed=3)
    files = []
    for i, s in enumerate(scans):
        s.numpy().tofile(d / f'{i:06d}.bin')
        files.append((d / f'{i:06d}.bin', None))
    out = tmp_path / 'out'
    paths = write_point_labels(model, dict(kw, batch_size=2), device, files, out)
    assert [p.relative_to(out).as_posix() for p in paths] == [f'sequences/08/predictions/{i:06d}.label' for i in range(3)]
    labelled, wants = 0, []
    for start in (0, 2):                                                # the batches the launcher made
        part = [s.to(device) for s in scans[start:start + 2]]
        wants += [w.cpu().numpy().astype(np.int64) for w in model.predict(part).lift(part, model).per_scan()]
    for s, p, want in zip(scans, paths, wants):
        sem, inst = B.read_semantic_kitti_label(p)
        assert inst.shape[0] == s.shape[0] and np.array_equal(inst.astype(np.int64), want + 1)
        assert np.array_equal(sem, np.where(want >= 0, 10, 0))
        labelled += int((want >= 0).sum())
    assert labelled > 0


def test_launcher_kitti_3d_lines(device, tmp_path, capsys):
    """``--test`` on ``dataset: kitti`` over a tree holding the committed sample frame: with ``kitti_3d: true`` every
    ``bev  AP:`` line is followed by a ``3d   AP:`` line; without the key the output has none."""
    import train_mask_bev_amd as launcher
    from mask_bev_amd.mask_bev_module import MaskBevModule
    rng = np.random.default_rng(2)
    for k in ('velodyne', 'label_2', 'calib'):
        d = tmp_path / f'data_object_{k}' / 'training' / k
        d.mkdir(parents=True)
        for frame in (0, 1):
            if k == 'velodyne':
                rng.uniform([0, -10, -3, 0], [20, 10, 1, 1], (2000 + frame, 4)).astype(np.float32).tofile(d / f'{frame:06d}.bin')
            else:
                shutil.copy(os.path.join(SAMPLE, k, '000000.txt'), d / f'{frame:06d}.txt')
    (tmp_path / 'val.txt').write_text('000000\n000001\n')
    (tmp_path / 'train.txt').write_text('000000\n000001\n')
    kw = dict(tiny_kwargs(), x_range=[0, 20], y_range=[-10, 10], z_range=[-3, 1], dataset='kitti', batch_size=1)
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    ck = tmp_path / 'ckpt'
    for name, extra in (('plain', {}), ('lifted', {'kitti_3d': True, 'kitti_3d_extent': [0.02, 0.98]})):
        (ck / name).mkdir(parents=True)
        launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'],
                                 ck / name / f'{name}-epoch=00-val_loss=1.000000.ckpt', 0, 'val_loss', 1.0)
        cfg = tmp_path / f'{name}.yml'
        cfg.write_text(yaml.safe_dump(dict(kw, **extra)))
        rc = launcher.main(['--config', str(cfg), '--test', '--data-root', str(tmp_path), '--checkpoint-root', str(ck)])
        assert rc == 0
        lines = capsys.readouterr().out.splitlines()
        bev = [i for i, l in enumerate(lines) if l.startswith('bev  AP:')]
        d3 = [i for i, l in enumerate(lines) if l.startswith('3d   AP:')]
        assert len(bev) == 2
        if extra:
            assert d3 == [i + 1 for i in bev] and all(len(lines[i].split(',')) == 3 for i in d3)
        else:
            assert d3 == []
