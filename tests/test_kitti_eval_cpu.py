"""KITTI BEV evaluation on the host: the numpy oracle (tests/kitti_eval_ref.py) against the values recorded from the
reference's own protocol functions (tests/golden/kitti_eval.npz) and against closed forms, the product's host functions
(``clean_data``, ``get_thresholds``, ``get_mAP``, the cells → metres mapping) against the same, the alias modules with the
reference's import paths, and the refusal of CPU tensors."""
import os

import numpy as np
import pytest
import torch

from tests import kitti_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_OVERLAPS = (0.7, 0.5)


def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'kitti_eval.npz'))


def golden_frames(g):
    """Per frame (gt dict, dt dict): the oracle's and — with ``boxes`` (n, 7) / (k, 5) — the product's inputs."""
    frames = []
    for f in range(len(g['gt_offsets']) - 1):
        a, b = int(g['gt_offsets'][f]), int(g['gt_offsets'][f + 1])
        c, d = int(g['dt_offsets'][f]), int(g['dt_offsets'][f + 1])
        n = b - a
        bev = g['gt_boxes'][a:b]
        boxes7 = np.stack([bev[:, 0], bev[:, 1], np.zeros(n), bev[:, 2], bev[:, 3], np.zeros(n), bev[:, 4]], axis=1).reshape(n, 7)
        gt = dict(type=g['gt_types'][a:b], occluded=g['gt_occluded'][a:b], truncated=g['gt_truncated'][a:b],
                  bbox=np.stack([np.zeros(n), np.zeros(n), np.full(n, 50.0), g['gt_heights'][a:b]], axis=1).reshape(n, 4),
                  boxes=boxes7, bev=bev)
        dt = dict(type=g['dt_types'][c:d], score=g['dt_scores'][c:d], boxes=g['dt_boxes'][c:d])
        frames.append((gt, dt))
    return frames


@pytest.fixture(scope='module')
def oracle_eval():
    g = golden()
    frames = golden_frames(g)
    overlaps = [R.rotate_iou(dt['boxes'], gt['bev']) for gt, dt in frames]
    return g, frames, overlaps, R.eval_class(frames, overlaps, 0, (0, 1, 2), MIN_OVERLAPS)


def test_fixture_holds_the_cases_and_the_margin(oracle_eval):
    g, frames, overlaps, _ = oracle_eval
    counts = [(len(gt['type']), len(dt['type'])) for gt, dt in frames]
    assert any(n == 0 and k > 0 for n, k in counts) and any(n > 0 and k == 0 for n, k in counts)
    assert {0, 1, 3, 8} <= set(g['gt_types'].tolist())                                   # Car, Van, Pedestrian, DontCare
    for d in range(3):
        assert {-1, 0, 1} <= set(g[f'ignored_gt_{d}'].tolist())
    assert len(np.unique(g['dt_scores'])) < len(g['dt_scores'])                          # tied scores
    assert any(((ov > 0.25).sum(axis=1) >= 2).any() for ov in overlaps if ov.size)       # one detection over two ground truths
    allov = np.concatenate([ov.reshape(-1) for ov in overlaps])
    assert np.abs(allov - 0.5).min() > 1e-3 and np.abs(allov - 0.7).min() > 1e-3
    assert np.array_equal(g['dt_scores'], g['dt_scores'].astype(np.float32).astype(np.float64))


def test_oracle_protocol_equals_the_reference(oracle_eval):
    g, frames, overlaps, res = oracle_eval
    for d in range(3):
        codes = [R.clean_data(gt, dt, 0, d) for gt, dt in frames]
        assert np.array_equal(np.concatenate([c[1] for c in codes]), g[f'ignored_gt_{d}'])
        assert np.array_equal(np.concatenate([c[2] for c in codes]), g[f'ignored_dt_{d}'])
        assert sum(c[0] for c in codes) == g['num_valid_gt'][d]
    assert np.array_equal(res['num_thresholds'], g['num_thresholds'])
    assert np.abs(res['thresholds'] - g['thresholds']).max() <= 1e-12
    assert np.abs(res['precision'] - g['precision']).max() <= 1e-12
    assert np.abs(R.get_map(res['precision']) - g['ap']).max() <= 1e-12
    for (d, k), pr in res['stats'].items():
        assert np.array_equal(pr, g['stats'][d, k, :len(pr)])


def test_product_host_functions_equal_the_reference(oracle_eval):
    from mask_bev_amd import kitti_eval as KE
    g, frames, _, res = oracle_eval
    for d in range(3):
        codes = [KE.clean_data(gt, dt, 0, d) for gt, dt in frames]
        assert np.array_equal(np.concatenate([c[1] for c in codes]), g[f'ignored_gt_{d}'])
        assert np.array_equal(np.concatenate([c[2] for c in codes]), g[f'ignored_dt_{d}'])
        assert sum(c[0] for c in codes) == g['num_valid_gt'][d] and codes[0][1].dtype == np.int32
        assert KE.clean_data(frames[0][0], frames[0][1], 'Car', d)[0] == codes[0][0]
    assert np.abs(KE.get_mAP(g['precision']) - g['ap']).max() <= 1e-12
    rng = np.random.default_rng(0)
    for n, num_gt in ((0, 5), (1, 1), (7, 9), (60, 60), (200, 231)):
        s = (rng.integers(0, 50, n) / 50).astype(np.float64)
        assert np.array_equal(KE.get_thresholds(s.copy(), num_gt), R.get_thresholds(s.copy(), num_gt))
    assert len(KE.get_thresholds(np.linspace(0, 1, 500), 500)) == 41
    # a pedestrian evaluation: Person_sitting is the neighbouring class
    gt = dict(type=np.array([3, 4, 0]), bbox=np.array([[0, 0, 1, 90.]] * 3), occluded=np.zeros(3, dtype=int), truncated=np.zeros(3))
    n, ig, idt = KE.clean_data(gt, dict(type=np.array([3, 0]), bbox=np.array([[0, 0, 1, 90.], [0, 0, 1, 10.]])), 1, 0)
    assert (n, ig.tolist(), idt.tolist()) == (1, [0, 1, -1], [0, 1])


def _iou(a, b, criterion=-1):
    return float(R.rotate_iou(np.array([a], dtype=np.float64), np.array([b], dtype=np.float64), criterion)[0, 0])


def test_oracle_overlap_closed_forms():
    # axis-aligned pairs against the analytic IoU
    rng = np.random.default_rng(1)
    for _ in range(20):
        a = [rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(1, 6), rng.uniform(1, 6), 0.0]
        b = [a[0] + rng.uniform(-3, 3), a[1] + rng.uniform(-3, 3), rng.uniform(1, 6), rng.uniform(1, 6), 0.0]
        iw = min(a[0] + a[2] / 2, b[0] + b[2] / 2) - max(a[0] - a[2] / 2, b[0] - b[2] / 2)
        ih = min(a[1] + a[3] / 2, b[1] + b[3] / 2) - max(a[1] - a[3] / 2, b[1] - b[3] / 2)
        inter = max(iw, 0) * max(ih, 0)
        assert _iou(a, b) == pytest.approx(inter / (a[2] * a[3] + b[2] * b[3] - inter), abs=1e-12)
        assert _iou(a, b, 2) == pytest.approx(inter, abs=1e-12)
    # the axes swap at pi / 2: a 4 x 2 box turned by pi / 2 is a 2 x 4 box
    assert _iou([1, 2, 4, 2, np.pi / 2], [1, 2, 2, 4, 0.0]) == pytest.approx(1.0, abs=1e-12)
    for ang in (0.0, 0.3, -1.2, 2.9):
        box = [3.0, -2.0, 4.5, 1.7, ang]
        assert _iou(box, box) == pytest.approx(1.0, abs=1e-12)                                       # identical
        far = [box[0] + 20, box[1], 4.5, 1.7, ang + 0.4]
        assert _iou(box, far) == 0.0 and _iou(box, far, 2) == 0.0                                   # disjoint: exactly 0
        inner = [3.1, -2.05, 1.0, 0.5, ang]
        assert _iou(inner, box) == pytest.approx(0.5 / (4.5 * 1.7), abs=1e-12)                      # inside: the area ratio
        assert _iou(inner, box, 0) == pytest.approx(1.0, abs=1e-12)
        assert _iou(inner, box, 1) == pytest.approx(0.5 / (4.5 * 1.7), abs=1e-12)
        turned = [box[0], box[1], box[2], box[3], ang + np.pi / 2]                                  # a cross: a w x w square
        assert _iou(box, turned, 0) == pytest.approx(1.7 / 4.5, abs=1e-12)
        assert _iou(box, turned, 1) == pytest.approx(1.7 / 4.5, abs=1e-12)
    # the corners are those of box_vertices: a box at +30 degrees meets a probe that the box at -30 degrees misses
    from mask_bev_amd.rasterize import box_vertices
    probe = [1.5, 1.0, 0.4, 0.4, 0.0]
    assert _iou([0, 0, 4, 1, np.deg2rad(30)], probe, 2) > 0.1 and _iou([0, 0, 4, 1, np.deg2rad(-30)], probe, 2) == 0.0
    verts = box_vertices([[50.0, 50.0, 0, 4, 1, 0, np.deg2rad(30)]], (0, 100), (0, 100), 1000, 1000)[0]
    want = np.array(R.corners([50.0, 50.0, 4, 1, np.deg2rad(30)])) * 10
    assert np.array_equal(verts, np.trunc(want).astype(np.int32))


def test_oracle_box_fit_closed_forms():
    m = np.zeros((20, 30), dtype=bool)
    assert R.fit_box(m)[0] == 0 and not R.fit_box(m)[2].any()
    m[4:7, 10:18] = True                                               # 3 rows (y) x 8 columns (x)
    n, mom, box = R.fit_box(m)
    assert n == 24 and mom[0] == 3 * sum(range(10, 18)) and mom[1] == 8 * sum(range(4, 7))
    assert box.tolist() == [13.5, 5.0, 8.0, 3.0, 0.0]
    n, _, box = R.fit_box(m.T)                                          # 8 rows x 3 columns: the axis is y
    assert box[:2].tolist() == [5.0, 13.5] and box[4] == pytest.approx(np.pi / 2) and np.allclose(box[2:4], [8.0, 3.0], atol=1e-12)
    sq = np.zeros((16, 16), dtype=bool)
    sq[3:9, 5:11] = True
    assert R.fit_box(sq)[2].tolist() == [7.5, 5.5, 6.0, 6.0, 0.0] and R.fit_box(np.ones((9, 9), dtype=bool))[2][4] == 0.0
    one = np.zeros((5, 5), dtype=bool)
    one[2, 3] = True
    assert R.fit_box(one)[2].tolist() == [3.0, 2.0, 1.0, 1.0, 0.0]


def test_cells_to_metres_inverts_box_vertices():
    from mask_bev_amd.rasterize import boxes_from_cells, box_vertices
    x_range, y_range, nx, ny = (0.0, 80.0), (-40.0, 40.0), 800, 800
    # the cell box of an axis-aligned block of cells 100 .. 139 (x) by 200 .. 219 (y)
    cells = torch.tensor([[119.5, 209.5, 40.0, 20.0, 0.0], [119.5, 209.5, 20.0, 40.0, np.pi / 2], [10.0, 20.0, 3.0, 8.0, 0.25]])
    got = boxes_from_cells(cells, x_range, y_range, nx, ny).double().numpy()
    assert got.dtype == np.float64 and np.allclose(got[0], [12.0, -19.0, 4.0, 2.0, 0.0], atol=1e-6)
    assert np.allclose(got[1, :4], [12.0, -19.0, 4.0, 2.0], atol=1e-6) and abs(abs(got[1, 4]) - np.pi) < 1e-6    # l >= w
    assert np.allclose(got[2], [1.05, -37.95, 0.8, 0.3, 0.25 + np.pi / 2], atol=1e-6) and np.all(got[:, 2] >= got[:, 3])
    # back through box_vertices: the painted corners are the block's
    v = box_vertices([[got[0, 0], got[0, 1], 0, got[0, 2], got[0, 3], 0, got[0, 4]]], x_range, y_range, nx, ny)[0]
    assert sorted(set(v[:, 0].tolist())) in ([99, 140], [100, 140], [99, 139], [100, 139])
    assert sorted(set(v[:, 1].tolist())) in ([199, 220], [200, 220], [199, 219], [200, 219])


def test_alias_modules_expose_the_reference_names():
    import importlib
    from mask_bev_amd import kitti_eval as KE
    ke = importlib.import_module('mask_bev.evaluation.kitti_eval')
    for name in ('eval_kitti', 'get_mAP', 'get_mAP_v2', 'get_thresholds', 'clean_data', 'bev_box_overlap', 'eval_class',
                 'get_official_eval_result', 'mask_to_pred'):
        assert getattr(ke, name) is getattr(KE, name), name
    ri = importlib.import_module('mask_bev.evaluation.rotate_iou')
    assert callable(ri.rotate_iou_gpu_eval)
    importlib.import_module('mask_bev.evaluation')


def test_cpu_tensors_are_refused():
    from mask_bev_amd import _lib, kitti_eval as KE, ops
    from mask_bev_amd._lib import MaskBevHipError
    for name in ('mbv_fit_boxes', 'mbv_rotate_iou', 'mbv_kitti_statistics', 'mbv_kitti_statistics_workspace_bytes'):
        assert name in _lib.SIGNATURES
    words = torch.zeros((2, ((8 * 8 + 63) // 64) * 2), dtype=torch.int32)
    with pytest.raises(MaskBevHipError):
        ops.fit_boxes(ops.PackedMasks(words, 8, 8), torch.tensor([0, 1]))
    with pytest.raises(MaskBevHipError):
        ops.rotate_iou(torch.zeros(2, 5), torch.zeros(3, 5))
    g = golden()
    frames = golden_frames(g)
    labels = [gt for gt, _ in frames]
    preds = [dict(boxes=torch.from_numpy(dt['boxes']).float(), score=torch.from_numpy(dt['score']).float(), type=dt['type'])
             for _, dt in frames]
    with pytest.raises(MaskBevHipError):
        KE.eval_kitti(labels, preds, device='cpu')
