"""K31 / K26b on the host: the numpy restatement (tests/point_lift_ref.py) on hand-worked cases, the 3-D overlap oracle against
closed forms and against the values recorded from the reference's own ``d3_box_overlap`` and protocol
(tests/golden/kitti_eval_3d.npz), the SemanticKITTI label writer against the reader, and the refusal of CPU tensors."""
import os

import numpy as np
import pytest
import torch

from tests import kitti_eval_ref as R
from tests import point_lift_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_OVERLAPS = (0.7, 0.5)
# a 4 (x) by 3 (y) by 1 (z) grid of 1 m x 1 m x 2 m cells
RANGE, VOXEL, GRID = [0.0, 0.0, -1.0, 4.0, 3.0, 1.0], [1.0, 1.0, 2.0], [4, 3, 1]


def golden_3d():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'kitti_eval_3d.npz'))


def golden_3d_frames(g):
    """Per frame (gt dict, dt dict): the oracle's and — ``boxes`` (n, 7) / ``boxes3d`` (k, 7) — the product's inputs."""
    frames = []
    for f in range(len(g['gt_offsets']) - 1):
        a, b = int(g['gt_offsets'][f]), int(g['gt_offsets'][f + 1])
        c, d = int(g['dt_offsets'][f]), int(g['dt_offsets'][f + 1])
        n = b - a
        gt = dict(type=g['gt_types'][a:b], occluded=g['gt_occluded'][a:b], truncated=g['gt_truncated'][a:b],
                  bbox=np.stack([np.zeros(n), np.zeros(n), np.full(n, 50.0), g['gt_heights'][a:b]], axis=1).reshape(n, 4),
                  boxes=g['gt_boxes'][a:b])
        dt = dict(type=g['dt_types'][c:d], score=g['dt_scores'][c:d], boxes3d=g['dt_boxes'][c:d],
                  boxes=g['dt_boxes'][c:d][:, L.BEV])
        frames.append((gt, dt))
    return frames


# ------------------------------------------------------------------------------------------------ K31: the cell rule
def _labels(points, imap, q, prefilter):
    return L.lift([np.array(points, dtype=np.float32)], np.array(imap)[None], RANGE, VOXEL, GRID, q, prefilter=prefilter)


IMAP = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, -1, 11]]            # imap[cy][cx]


def test_reference_cell_rule_on_hand_worked_points():
    # interior points: the map is read at [cy][cx] — x = 2.5, y = 0.5 is column 2 of row 0
    assert _labels([[2.5, 0.5, 0.0], [0.5, 2.5, 0.0], [2.5, 2.5, 0.0]], IMAP, 12, True)['point_query'].tolist() == [2, 8, -1]
    # a point exactly on a cell border belongs to the upper cell: floor(2.0) = 2
    assert _labels([[2.0, 1.0, 0.0]], IMAP, 12, True)['point_query'].tolist() == [6]
    # the lower limits: cell 0 without the pre-filter, dropped by its strict compare
    lower = [[0.0, 0.5, 0.0], [0.5, 0.0, 0.0], [0.5, 0.5, -1.0]]
    assert _labels(lower, IMAP, 12, False)['point_query'].tolist() == [0, 0, 0]
    assert _labels(lower, IMAP, 12, True)['point_query'].tolist() == [-1, -1, -1]
    # the upper limits: cell index == grid, dropped either way; so is a point outside z
    upper = [[4.0, 0.5, 0.0], [0.5, 3.0, 0.0], [0.5, 0.5, 1.0], [0.5, 0.5, 1.5], [0.5, 0.5, -1.5], [-0.5, 0.5, 0.0]]
    for prefilter in (False, True):
        assert _labels(upper, IMAP, 12, prefilter)['point_query'].tolist() == [-1] * 6
    # NaN and inf coordinates, on any axis
    nan, inf = float('nan'), float('inf')
    bad = [[nan, 0.5, 0.0], [0.5, nan, 0.0], [0.5, 0.5, nan], [inf, 0.5, 0.0], [0.5, -inf, 0.0], [0.5, 0.5, inf]]
    for prefilter in (False, True):
        out = _labels(bad + [[1.5, 1.5, 0.0]], IMAP, 12, prefilter)
        assert out['point_query'].tolist() == [-1] * 6 + [5] and out['counts'][0].tolist() == [0] * 5 + [1] + [0] * 6
    # a map value >= num_queries (and one below -1) counts as -1
    out = _labels([[3.5, 2.5, 0.0], [3.5, 1.5, 0.0], [0.5, 0.5, 0.0]], [[-7, 1, 2, 3], [4, 5, 6, 7], [8, 9, -1, 11]], 8, True)
    assert out['point_query'].tolist() == [-1, 7, -1] and out['counts'].sum() == 1
    # the quotient is formed in float32: the cell of x = 0.3f at 0.1f cells is floor(0.3f / 0.1f) as float32 rounds it, and
    # the float32 just below 0.3f stays in cell 2
    ok, cx, _ = L.point_cells(np.array([[0.3, 0.05, 0.0], [np.nextafter(np.float32(0.3), np.float32(0)), 0.05, 0.0]]),
                              [0, 0, -1, 1, 1, 1], [0.1, 0.1, 2.0], [10, 10, 1], True)
    want = np.floor((np.float32(0.3) - np.float32(0)) / np.float32(0.1))
    assert ok.all() and cx[0] == int(want) and cx[1] == 2


def test_reference_extent_and_histogram_edges_on_hand_worked_points():
    pts = [[0.5, 0.5, z] for z in (-0.9, -0.6, 0.1, 0.8)] + [[1.5, 0.5, 0.25]]
    f = np.float32
    out = L.lift([np.array(pts, dtype=f)], np.array(IMAP)[None], RANGE, VOXEL, GRID, 3, z_bins=4, quantiles=(0.0, 1.0))
    assert out['counts'][0].tolist() == [4, 1, 0]
    # 4 bins of 0.5 over [-1, 1]: ranks 0 and 3 sit in bins 0 and 3, whose outer edges -1 and 1 are clamped to the points
    assert out['z_extent'][0, 0].tolist() == [f(-0.9), f(0.8), f(-0.9), f(0.8)]
    assert out['z_extent'][0, 1].tolist() == [f(0.25)] * 4 and not out['z_extent'][0, 2].any()
    # quantiles 0.5 and 0.75 of 4 points: ranks floor(1.5) = 1 and floor(2.25) = 2 -> bins 0 and 2: edges -1 (clamped) and 0.5
    out = L.lift([np.array(pts, dtype=f)], np.array(IMAP)[None], RANGE, VOXEL, GRID, 3, z_bins=4, quantiles=(0.5, 0.75))
    assert out['z_extent'][0, 0].tolist() == [f(-0.9), f(0.8), f(-0.9), f(0.5)]
    # quantile 1 / 3 picks rank floor(f32(1 / 3) * 3) = 1: -0.6 is in bin 0; with 64 bins its lower edge is -1 + 12 / 32
    out = L.lift([np.array(pts, dtype=f)], np.array(IMAP)[None], RANGE, VOXEL, GRID, 3, z_bins=64, quantiles=(1 / 3, 1 / 3))
    assert out['z_extent'][0, 0, 2] == f(-1 + 12 * 2 / 64) and out['z_extent'][0, 0, 3] == f(-1 + 13 * 2 / 64)
    # one bin: both edges are the range limits, clamped to the points
    out = L.lift([np.array(pts, dtype=f)], np.array(IMAP)[None], RANGE, VOXEL, GRID, 3, z_bins=1, quantiles=(0.2, 0.8))
    assert out['z_extent'][0, 0].tolist() == [f(-0.9), f(0.8), f(-0.9), f(0.8)]


# ------------------------------------------------------------------------------------------------ K26b: the oracle
def test_oracle_3d_overlap_closed_forms():
    a = [1.0, 2.0, -1.0, 4.0, 2.0, 1.5, 0.3]
    assert L.rotate_iou_3d([a], [a])[0, 0] == pytest.approx(1.0, abs=1e-12)
    assert L.rotate_iou_3d([a], [a], 2)[0, 0] == pytest.approx(12.0, abs=1e-12)
    above = [1.0, 2.0, 0.5, 4.0, 2.0, 1.5, 0.3]                                  # its bottom is the other's top: touching
    assert L.rotate_iou_3d([a], [above])[0, 0] == 0.0 and L.rotate_iou_3d([a], [above], 2)[0, 0] == 0.0
    half = [1.0, 2.0, -0.25, 4.0, 2.0, 1.5, 0.3]                                 # shifted up by half the height
    assert L.rotate_iou_3d([a], [half], 2)[0, 0] == pytest.approx(6.0, abs=1e-12)
    assert L.rotate_iou_3d([a], [half])[0, 0] == pytest.approx(6.0 / 18.0, abs=1e-12)
    inner = [1.0, 2.0, -0.5, 2.0, 1.0, 0.5, 0.3]
    assert L.rotate_iou_3d([inner], [a], 0)[0, 0] == pytest.approx(1.0, abs=1e-12)
    assert L.rotate_iou_3d([inner], [a], 1)[0, 0] == pytest.approx(1.0 / 12.0, abs=1e-12)
    far = [30.0, 2.0, -1.0, 4.0, 2.0, 1.5, 0.3]
    assert L.rotate_iou_3d([a], [far])[0, 0] == 0.0


def test_oracle_equals_the_reference_recorded_in_the_fixture():
    g = golden_3d()
    frames = golden_3d_frames(g)
    overlaps = [L.rotate_iou_3d(dt['boxes3d'], gt['boxes']) for gt, dt in frames]
    allov = np.concatenate([ov.reshape(-1) for ov in overlaps])
    assert np.abs(allov - g['overlaps']).max() <= 1e-12                                   # the reference's d3_box_overlap
    assert np.abs(allov - 0.5).min() > 1e-3 and np.abs(allov - 0.7).min() > 1e-3          # the margin
    bev = np.concatenate([R.rotate_iou(dt['boxes'], gt['boxes'][:, L.BEV]).reshape(-1) for gt, dt in frames])
    assert ((bev > 0.3) & (allov == 0)).sum() >= 3                                        # pairs that meet in BEV only
    res = R.eval_class(frames, overlaps, 0, (0, 1, 2), MIN_OVERLAPS)
    assert np.array_equal(res['num_thresholds'], g['num_thresholds']) and np.array_equal(res['num_valid_gt'], g['num_valid_gt'])
    assert np.abs(res['thresholds'] - g['thresholds']).max() <= 1e-12
    assert np.abs(res['precision'] - g['precision']).max() <= 1e-12
    assert np.abs(R.get_map(res['precision']) - g['ap']).max() <= 1e-12
    for (d, k), pr in res['stats'].items():
        assert np.array_equal(pr, g['stats'][d, k, :len(pr)])


# ------------------------------------------------------------------------------------------------ host functions
def test_label_writer_round_trip(tmp_path):
    from mask_bev_amd import batch as B
    from mask_bev_amd.predict import write_semantic_kitti_labels
    q = np.array([-1, 0, 1, 65534, -1, 7], dtype=np.int32)
    path = tmp_path / '000000.label'
    write_semantic_kitti_labels(path, torch.from_numpy(q))
    raw = np.fromfile(path, dtype='<u4')
    assert raw.tolist() == [0, (1 << 16) | 10, (2 << 16) | 10, (65535 << 16) | 10, 0, (8 << 16) | 10]
    sem, inst = B.read_semantic_kitti_label(path)
    assert inst.tolist() == [0, 1, 2, 65535, 0, 8] and sem.tolist() == [0, 10, 10, 10, 0, 10]
    write_semantic_kitti_labels(path, q, semantic_id=252)                       # an array, another class
    sem, inst = B.read_semantic_kitti_label(path)
    assert sem.tolist() == [0, 252, 252, 252, 0, 252] and inst.tolist() == [0, 1, 2, 65535, 0, 8]
    write_semantic_kitti_labels(path, np.zeros((0,), dtype=np.int32))
    assert os.path.getsize(path) == 0
    for bad in ([65535], [-2]):
        with pytest.raises(ValueError):
            write_semantic_kitti_labels(path, np.array(bad))


def test_new_entry_points_are_declared_and_cpu_tensors_refused():
    from mask_bev_amd import _lib, kitti_eval as KE, ops
    from mask_bev_amd._lib import MaskBevHipError
    import importlib
    for name in ('mbv_lift_instances', 'mbv_lift_instances_workspace_bytes', 'mbv_rotate_iou_3d'):
        assert name in _lib.SIGNATURES
    assert importlib.import_module('mask_bev.evaluation.kitti_eval').d3_box_overlap is KE.d3_box_overlap
    geom = ops.VoxelGeometry.from_ranges(RANGE, VOXEL)
    assert list(geom.grid) == GRID
    with pytest.raises(MaskBevHipError):
        ops.lift_instances([torch.zeros(5, 4)], torch.zeros((1, 3, 4), dtype=torch.int32), geom, 4)
    with pytest.raises(MaskBevHipError):
        ops.rotate_iou_3d(torch.zeros(2, 7), torch.zeros(3, 7))
    with pytest.raises(ValueError):
        KE.eval_class([{}], [{}], metric='aos')
