"""CPU tests of the panoptic protocol (K32): the numpy restatement (tests/panoptic_ref.py) against an independently written
plain-loop version and against hand-computed answers, ``semantic_kitti_class_lut`` on the committed sample, the formulas of
``DevicePanopticQuality.compute`` and the launcher's label path and configuration keys."""
import os

import numpy as np
import pytest

from tests import panoptic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, 'tests', 'golden', 'semantic_kitti_sample', '000000.label')
LUT = np.array([-1, 0, 1], dtype=np.int32)           # semantic 0 ignored, 1 everything else, 2 the thing


def _same(a, b):
    for k in ('stats', 'confusion', 'n_gt', 'gt_key', 'gt_area', 'pred_area'):
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])
    assert np.allclose(a['iou'], b['iou'], rtol=1e-12, atol=0) and a['ignored'] == b['ignored'] and a['in_pair'] == b['in_pair']


@pytest.mark.parametrize('seed,P,C,max_gt,min_points', [(0, 5, 2, 16, 3), (1, 9, 3, 16, 0), (2, 1, 4, 4, 8), (3, 0, 2, 16, 1)])
def test_restatement_equals_the_plain_loops(seed, P, C, max_gt, min_points):
    rng = np.random.default_rng(seed)
    lengths = [0, 37, 300, 1]
    pq, gw, qc, lut = R.random_case(rng, lengths, P, C)
    a = R.frames(pq, gw, lengths, qc, lut, C, max_gt, min_points)
    b = R.frames(pq, gw, lengths, qc, lut, C, max_gt, min_points, one=R.plain_frame)
    _same(a, b)
    if P >= 5:
        assert a['stats'][..., 0].sum() > 0 and a['in_pair'] > 50 and a['ignored'] > 5


def test_planted_frames_agree_too():
    for P, C in ((1, 2), (7, 3), (1024, 2)):
        pq, gw, lengths, qc, lut = R.planted_case(P, C)
        for max_gt in (8, 64):
            _same(R.frames(pq, gw, lengths, qc, lut, C, max_gt, R.MIN_POINTS),
                  R.frames(pq, gw, lengths, qc, lut, C, max_gt, R.MIN_POINTS, one=R.plain_frame))


def _one(pred, sem, inst, query_class=(1, 1), min_points=2, max_gt=8, lut=LUT, C=2):
    return R.frame(np.array(pred), R.as_i32(R.word(sem, inst)), np.array(query_class), lut, C, max_gt, min_points)


def test_known_answers():
    # one perfect match: four points of instance 3 under query 0, two background points
    r = _one([0, 0, 0, 0, -1, -1], [2, 2, 2, 2, 1, 1], [3, 3, 3, 3, 0, 0])
    assert r['stats'][1].tolist() == [1, 0, 0] and r['iou'][1] == 1.0 and r['confusion'].tolist() == [[2, 0], [0, 4]]
    assert r['n_gt'] == 1 and r['gt_key'][0] == (1 << 16) | 3 and r['gt_area'][0] == 4 and r['pred_area'].tolist() == [4, 0]
    # inter = 2, union = 4: iou = 0.5 is no match; both sides have 3 >= min_points points: one fp, one fn
    r = _one([-1, 0, 0, 0], [2, 2, 2, 1], [1, 1, 1, 0])
    assert r['stats'][1].tolist() == [0, 1, 1] and r['iou'][1] == 0.0
    # unmatched segments of exactly min_points and of min_points - 1 elements, on both sides
    r = _one([-1] * 5 + [0] * 3 + [1] * 2, [2] * 5 + [1] * 5, [1, 1, 1, 2, 2] + [0] * 5, min_points=3)
    assert r['stats'][1].tolist() == [0, 1, 1] and r['gt_area'][:2].tolist() == [3, 2] and r['pred_area'].tolist() == [3, 2]
    # instance id 0 is a thing like any other
    r = _one([1, 1, 1], [2, 2, 2], [0, 0, 0])
    assert r['stats'][1].tolist() == [1, 0, 0] and r['gt_key'][0] == 1 << 16 and r['n_gt'] == 1
    # an ignored element under the prediction is not its area: 3 / (3 + 3 - 3) with it ignored ...
    r = _one([0, 0, 0, 0, 0, 0], [2, 2, 2, 0, 0, 0], [4, 4, 4, 0, 0, 0])
    assert r['stats'][1].tolist() == [1, 0, 0] and r['iou'][1] == 1.0 and r['pred_area'][0] == 3 and r['ignored'] == 3
    # ... and 3 / (3 + 6 - 3) = 0.5, no match, with the same three points in class 0 instead
    r = _one([0, 0, 0, 0, 0, 0], [2, 2, 2, 1, 1, 1], [4, 4, 4, 0, 0, 0])
    assert r['stats'][1].tolist() == [0, 1, 1] and r['pred_area'][0] == 6
    # a query of no thing class is class 0 with no instance; values outside the sizes are never indices
    r = _one([0, 0, 7, -5, 2 ** 30], [2, 2, 2, 9, 65535], [1, 1, 1, 0, 0], query_class=(0, 1))
    assert r['stats'][1].tolist() == [0, 0, 1] and r['confusion'].tolist() == [[0, 0], [3, 0]] and r['ignored'] == 2
    # more segments than max_gt: zeros, n_gt reports it, the confusion and the prediction's area stay
    r = _one([0] * 4, [2] * 4, [1, 2, 3, 4], max_gt=3, min_points=1)
    assert r['n_gt'] == 4 and not r['stats'].any() and r['pred_area'][0] == 4 and r['confusion'][1, 1] == 4
    assert r['gt_key'].tolist() == [(1 << 16) | k for k in (1, 2, 3)]


def test_semantic_kitti_class_lut_on_the_sample():
    from mask_bev_amd.metrics import semantic_kitti_class_lut
    lut = semantic_kitti_class_lut()
    assert lut.dtype == np.int32 and lut.shape == (260,)
    assert [int(lut[i]) for i in (0, 1, 10, 40, 252, 259)] == [-1, -1, 1, 0, -1, 0] and (lut == 1).sum() == 1 and (lut == -1).sum() == 3
    raw = np.fromfile(SAMPLE, dtype='<u4')
    sem, inst = raw & 0xffff, raw >> 16
    assert raw.shape == (257,) and sorted(set(sem.tolist())) == [0, 1, 10, 40, 252] and sorted(set(inst.tolist())) == [0, 1, 2, 3, 4, 5]
    cls = lut[sem]
    assert (cls == 1).sum() == (sem == 10).sum() > 0 and (cls == -1).sum() == np.isin(sem, (0, 1, 252)).sum() > 0
    # the file against itself through the restatement: every static car is a true positive
    query = np.where(sem == 10, inst.astype(np.int64), -1).astype(np.int32)
    r = R.frame(query, raw.view(np.int32), np.ones(6, dtype=np.int32), lut, 2, 16, 1)
    cars = len(set(inst[sem == 10].tolist()))
    assert r['stats'][1].tolist() == [cars, 0, 0] and r['iou'][1] == cars and r['ignored'] == (cls == -1).sum()
    two = semantic_kitti_class_lut(things=((10, 252), (40,)), ignore=(0,), length=300)
    assert two.shape == (300,) and [int(two[i]) for i in (0, 1, 10, 252, 40)] == [-1, 0, 1, 1, 2]
    with pytest.raises(ValueError):
        semantic_kitti_class_lut(things=((300,),))


def test_panoptic_quality_formulas():
    from mask_bev_amd.metrics import panoptic_quality
    conf = np.array([[50, 4, 0], [6, 30, 2], [0, 0, 0]])
    r = panoptic_quality([0, 3, 0], [0, 1, 2], [0, 2, 0], [0.0, 2.4, 0.0], conf)
    assert r['per_class']['pq'][1] == pytest.approx(2.4 / 4.5) and r['per_class']['sq'][1] == pytest.approx(0.8)
    assert r['per_class']['rq'][1] == pytest.approx(3 / 4.5) and r['per_class']['iou'][1] == pytest.approx(30 / 42)
    assert r['per_class']['pq'][2] == 0.0 and r['per_class']['sq'][2] == 0.0 and r['per_class']['rq'][2] == 0.0
    assert r['per_class']['iou'][2] == 0.0 and r['per_class']['iou'][0] == pytest.approx(50 / 60)
    assert r['pq'] == pytest.approx(2.4 / 4.5 / 2) and r['sq'] == pytest.approx(0.4) and r['iou'] == pytest.approx(30 / 42 / 2)
    assert r['per_class']['tp'] == [0, 3, 0] and r['per_class']['fp'] == [0, 1, 2] and r['per_class']['fn'] == [0, 2, 0]
    z = panoptic_quality(np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2), np.zeros((2, 2)))
    assert z['pq'] == 0.0 and z['sq'] == 0.0 and z['rq'] == 0.0 and z['iou'] == 0.0 and z['per_class']['tp'] == [0, 0]


def test_device_metric_state_on_cpu_tensors():
    """``append_state`` / ``compute`` are plain torch: K32's records of two batches as CPU tensors."""
    import torch
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.metrics import DevicePanopticQuality, panoptic_quality
    pq, gw, lengths, qc, lut = R.planted_case(7, 3)
    ref = R.frames(pq, gw, lengths, qc, lut, 3, 64, R.MIN_POINTS)
    m = DevicePanopticQuality(3, lut, min_points=R.MIN_POINTS, max_gt=64)
    assert m.compute()['frames'] == 0
    for part in (slice(0, 2), slice(2, 4)):
        m.append_state(*(torch.from_numpy(ref[k][part]) for k in ('stats', 'iou', 'confusion', 'n_gt')))
    got = m.compute()
    want = panoptic_quality(ref['stats'][..., 0].sum(0), ref['stats'][..., 1].sum(0), ref['stats'][..., 2].sum(0), ref['iou'].sum(0),
                            ref['confusion'].sum(0))
    assert got['frames'] == 4 and got['per_class'] == want['per_class'] and got['pq'] == want['pq'] > 0
    small = DevicePanopticQuality(3, lut, max_gt=8)
    small.append_state(*(torch.from_numpy(ref[k]) for k in ('stats', 'iou', 'confusion', 'n_gt')))
    with pytest.raises(MaskBevHipError, match='1 of 4 frames'):
        small.compute()
    with pytest.raises(ValueError):
        DevicePanopticQuality(17, lut)


def _three_frames(n_gt=(1, 2, 0)):
    """Hand-made K32 records of 3 frames and 2 classes as CPU tensors: (F, C, 3) tp / fp / fn, (F, C) IoU sums, (F, C, C)
    confusion, (F) ground-truth segments."""
    import torch
    stats = torch.tensor([[[0, 0, 0], [2, 1, 0]], [[0, 0, 0], [1, 0, 2]], [[0, 0, 0], [0, 1, 0]]], dtype=torch.int32)
    iou = torch.tensor([[0.0, 1.5], [0.0, 0.625], [0.0, 0.0]], dtype=torch.float64)
    conf = torch.tensor([[[40, 3], [2, 30]], [[10, 0], [7, 12]], [[5, 4], [0, 0]]], dtype=torch.int32)
    return stats, iou, conf, torch.tensor(n_gt, dtype=torch.int32)


def test_compute_without_reduce_equals_compute():
    """No process group: ``compute(reduce=False)`` is ``compute()`` key for key, on fed and on fresh metrics, and both raise
    on a frame above ``max_gt``."""
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.metrics import DevicePanopticQuality
    m = DevicePanopticQuality(2, LUT, min_points=1, max_gt=4)
    fresh = m.compute(reduce=False)
    assert fresh == m.compute() and fresh['frames'] == 0
    assert fresh['per_class']['tp'] == fresh['per_class']['fp'] == fresh['per_class']['fn'] == [0, 0]
    m.append_state(*_three_frames())
    alone, summed = m.compute(reduce=False), m.compute()
    assert set(alone) == set(summed) == {'pq', 'sq', 'rq', 'iou', 'per_class', 'frames'}
    for key in summed:
        assert alone[key] == summed[key], key
    assert alone['frames'] == 3 and alone['per_class']['tp'] == [0, 3] and alone['per_class']['fp'] == [0, 2]
    assert alone['sq'] == pytest.approx(2.125 / 3) and alone['iou'] == pytest.approx(42 / (42 + 9 + 7))
    over = DevicePanopticQuality(2, LUT, min_points=1, max_gt=4)
    over.append_state(*_three_frames(n_gt=(1, 5, 0)))
    for kw in ({}, dict(reduce=False)):
        with pytest.raises(MaskBevHipError, match='1 of 3 frames'):
            over.compute(**kw)


def test_prediction_label_path(tmp_path):
    import pathlib
    from mask_bev_amd.evaluate import prediction_label_path
    p = prediction_label_path(tmp_path / 'out', '/d/sequences/08/velodyne/000123.bin')
    assert p == tmp_path / 'out' / 'sequences' / '08' / 'predictions' / '000123.label'
    assert p.parent.is_dir() and not p.exists()
    assert prediction_label_path(tmp_path / 'out', pathlib.Path('/d/sequences/08/velodyne/000124.bin')).parent == p.parent


def test_launcher_label_path_and_config_keys():
    import pathlib
    from mask_bev_amd.evaluate import format_point_panoptic, panoptic_settings, point_panoptic_evaluation, semantic_kitti_label_path
    p = semantic_kitti_label_path('/data/sequences/08/velodyne/000123.bin')
    assert p == pathlib.Path('/data/sequences/08/labels/000123.label')
    assert panoptic_settings({}) == (50, ((10,),), (0, 1, 252))
    got = panoptic_settings(dict(panoptic_min_points=30, panoptic_things=[[10, 252], 18], panoptic_ignore=[0]))
    assert got == (30, ((10, 252), (18,)), (0,))
    assert point_panoptic_evaluation(None, {}, None, [(pathlib.Path('/nowhere/sequences/08/velodyne/000000.bin'), None)]) is None
    res = dict(pq=0.5, sq=0.75, rq=2 / 3, iou=0.25, per_class=dict(tp=[0, 4], fp=[0, 1], fn=[0, 3]))
    assert format_point_panoptic(res) == 'point PQ 0.5000 SQ 0.7500 RQ 0.6667 IoU 0.2500 (car; tp 4 fp 1 fn 3)'


def test_binding_declares_k32():
    from mask_bev_amd import _lib
    for name in ('mbv_panoptic_frames', 'mbv_panoptic_frames_workspace_bytes'):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['mbv_panoptic_frames'][1]) == 22 and len(_lib.SIGNATURES['mbv_panoptic_frames_workspace_bytes'][1]) == 4
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    assert 'mbv_panoptic_frames(' in header and 'mbv_panoptic_frames_workspace_bytes(' in header
