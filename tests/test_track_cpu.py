"""CPU checks of K33's yardstick and host side: the two restatements of tests/track_ref.py against each other, the scripted
scene's event log, the pose helpers, DeviceTubeAssociation's arithmetic, the label writer and the binding table."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(frames, h, w, x_lo, y_lo, voxel, q_num, p, min_iou, max_age, min_cells, log=None):
    a, b = R.fresh_state(h, w, p), R.fresh_state(h, w, p)
    for im, m in frames:
        qa, ta = R.step(a, im, m, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells, log)
        qb, tb = R.plain_step(b, im, m, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells)
        assert np.array_equal(qa, qb) and np.array_equal(ta, tb)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    return a


@pytest.mark.parametrize('seed', range(6))
def test_restatements_agree_on_random_scenes(seed):
    h, w = ((40, 48), (33, 65))[seed % 2]
    q, p = ((8, 8), (4, 4), (4, 6))[seed % 3]
    frames, x_lo, y_lo = R.random_scene(seed, h, w, q, frames=5)
    end = _both(frames, h, w, x_lo, y_lo, 0.5, q, p, 0.3, 1, 4)
    assert end['counters'][2] == 5 and end['counters'][1] >= 2


def test_restatements_agree_on_scattered_cells():
    rng = np.random.default_rng(3)
    frames = [(rng.integers(-2, 13, (20, 24)).astype(np.int32), np.array([[1.0, 0.0, 0.5 * k], [0.0, 1.0, 0.0]])) for k in range(3)]
    end = _both(frames, 20, 24, -6.0, -5.0, 0.5, 12, 40, 0.02, 2, 2)
    assert end['counters'][0] > 12


def test_scripted_scene_event_log():
    pr = R.SCRIPT_PARAMS
    log = []
    end = _both(R.scripted_scene(), R.H0, R.W0, R.X_LO0, R.Y_LO0, R.VOXEL0, pr['q_num'], pr['p'], pr['min_iou'], pr['max_age'],
                pr['min_cells'], log)
    kinds = lambda k: [e for e in log if e[0] == k]
    # a match under ego rotation plus translation: object A keeps id 0 in every frame although its query index changes
    a_matches = [e for e in kinds('match') if e[4] == 0]
    assert [e[1] for e in a_matches] == [1, 2, 3, 4, 5] and len({e[2] for e in a_matches}) > 1
    assert any(e[5] < e[6] for e in a_matches)                         # and not by a perfect overlap
    assert [e[3] for e in kinds('birth')] == list(range(7))
    # B (id 1) coasts in frame 2 and is re-identified in frame 3 with its old id: last seen in frame 1
    assert ('coast', 2, 1, 1) in log
    assert any(e[1] == 3 and e[4] == 1 and e[7] == 1 for e in kinds('match'))
    assert ('coast', 1, 2, 2) in log and ('death', 2, 2, 2) in log     # C: coasts one frame, then dies by age
    assert [e[3] for e in kinds('drop')] == [3, 4] and end['counters'].tolist() == [4, 7, 6, 2]


def test_constructed_frames():
    cases = R.constructed_cases()
    logs = {}
    for name, (frames, pr) in cases.items():
        logs[name] = []
        _both(frames, 6, 8, 0.0, 0.0, 1.0, pr['q_num'], pr['p'], pr['min_iou'], pr['max_age'], pr['min_cells'], logs[name])
    # a query below min_cells is left out; its two cells fall through to the warped track, which coasts
    log = logs['fall_through']
    assert ('small', 1, 1, 2) in log and ('fall_through', 1, 2) in log and ('coast', 1, 0, 0) in log
    assert not [e for e in log if e[0] == 'birth' and e[1] == 1]
    # ties: query 0 takes track 0 (not 1) at IoU 1/4; query 1 (not 2) takes track 2 at IoU 2/4, query 2 is born
    log = logs['tie']
    m = {e[2]: e for e in log if e[0] == 'match' and e[1] == 1}
    assert m[0][3] == 0 and (m[0][5], m[0][6]) == (1, 4) and m[0][8] >= 1
    assert m[1][3] == 2 and (m[1][5], m[1][6]) == (2, 4) and m[1][8] >= 1 and 2 not in m
    assert ('birth', 1, 2, 3) in log and ('coast', 1, 1, 1) in log
    # inter = 1, union = 2 at min_iou = 0.5 is accepted
    m = [e for e in logs['half'] if e[0] == 'match']
    assert len(m) == 1 and (m[0][5], m[0][6]) == (1, 2) and m[0][2] == 3


def test_pose_helpers():
    from mask_bev_amd.tracking import prev_from_cur_2d, velodyne_poses
    rng = np.random.default_rng(0)

    def pose():
        a, b, c = rng.uniform(-0.2, 0.2, 3)
        rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        t = np.eye(4)
        t[:3, :3], t[:3, 3] = rz @ ry @ rx, rng.uniform(-5, 5, 3)
        return t

    p0, p1 = pose(), pose()
    m = prev_from_cur_2d(p0, p1)
    rel = np.linalg.inv(p0) @ p1
    assert m.shape == (2, 3) and m.dtype == np.float64 and m.flags['C_CONTIGUOUS']
    assert np.array_equal(m, np.array([[rel[0, 0], rel[0, 1], rel[0, 3]], [rel[1, 0], rel[1, 1], rel[1, 3]]]))
    assert 'roll' in prev_from_cur_2d.__doc__.lower() and 'pitch' in prev_from_cur_2d.__doc__.lower()
    # a planar motion: a point of the current frame lands where the full transform puts it
    a, b = R.pose_2d(1.0, 2.0, 0.3), R.pose_2d(1.5, 2.2, 0.35)
    m = prev_from_cur_2d(a, b)
    pt = np.array([3.0, -1.0, 0.0, 1.0])
    assert np.allclose(m @ np.array([3.0, -1.0, 1.0]), (np.linalg.inv(a) @ b @ pt)[:2], rtol=0, atol=1e-12)
    tr = pose()
    poses = np.stack([pose() for _ in range(3)])
    got = velodyne_poses(poses, dict(velo_to_cam=tr))
    assert got.shape == (3, 4, 4)
    for k in range(3):
        assert np.allclose(got[k], np.linalg.inv(tr) @ poses[k] @ tr, rtol=0, atol=1e-12)
    assert np.array_equal(velodyne_poses(poses, tr), got)


@pytest.mark.parametrize('cit', [(3, 8, 6), (2, 16, 9)])
def test_tube_restatements_and_metric_on_cpu_tensors(cit):
    from mask_bev_amd import ops
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.metrics import DeviceTubeAssociation, lstq
    c, i, t = cit
    pred, words, lut = R.random_elements(7, 20000, c, i, t)
    tables = R.fresh_tables(c, i, t)
    for part in np.array_split(np.arange(20000), 3):
        R.tube_accumulate(tables, pred[part], words[part], lut, c, i, t)
    exact, over = R.plain_tube(pred, words, lut, c, i, t)
    assert over == tables['overflow'].tolist() and min(over) > 0
    assoc, class_assoc, class_tubes = R.tube_scores(tables, c, i)
    assert set(exact) == set(np.nonzero(tables['gt_size'])[0].tolist()) and len(exact) >= 4
    for r in range(assoc.shape[0]):
        want = float(exact.get(r, 0))
        assert abs(assoc[r] - want) <= 1e-12 * want
    assert 0 not in [r % i for r in exact]                             # instance id 0 is no tube
    rec = ops.TubeTables(torch.from_numpy(tables['gt_size']), torch.from_numpy(tables['pred_size']), torch.from_numpy(tables['pair']),
                         torch.from_numpy(tables['overflow'].copy()), c, i, t)
    metric = DeviceTubeAssociation(c, lut, id_limit=i, max_tracks=t, tables=rec)
    with pytest.raises(MaskBevHipError):
        metric.compute()
    rec.overflow.zero_()
    res = metric.compute()
    want = Fraction(sum(exact.values(), Fraction(0)), len(exact))
    assert res['tubes'] == len(exact) and abs(res['s_assoc'] - float(want)) <= 1e-12 * float(want)
    assert res['per_class']['tubes'] == class_tubes.tolist() and res['overflow'] == [0, 0]
    for k in range(1, c):
        rows = [v for r, v in exact.items() if r // i == k - 1]
        if rows:
            assert abs(res['per_class']['s_assoc'][k] - float(sum(rows, Fraction(0)) / len(rows))) <= 1e-12
    assert lstq(0.25, 0.64) == pytest.approx(0.4, abs=1e-15) and 'thing classes' in DeviceTubeAssociation.__doc__.lower()
    empty = DeviceTubeAssociation(c, lut).compute()
    assert empty['s_assoc'] == 0.0 and empty['tubes'] == 0
    with pytest.raises(MaskBevHipError):                               # no CPU fallback of the kernels
        metric.update(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(MaskBevHipError):
        ops.tube_scores(rec)


def test_label_writer_with_instance_ids(tmp_path):
    from mask_bev_amd.predict import write_semantic_kitti_labels
    pq = np.array([-1, 0, 3, 3, 7, -1], np.int32)
    write_semantic_kitti_labels(tmp_path / 'a.label', pq)
    default = (tmp_path / 'a.label').read_bytes()
    assert default == np.array([0, 1 << 16 | 10, 4 << 16 | 10, 4 << 16 | 10, 8 << 16 | 10, 0], '<u4').tobytes()
    write_semantic_kitti_labels(tmp_path / 'b.label', torch.from_numpy(pq), semantic_id=10, instance_ids=None)
    assert (tmp_path / 'b.label').read_bytes() == default
    ids = np.array([-1, 40, 65534, 65534, 0, -1], np.int32)
    write_semantic_kitti_labels(tmp_path / 'c.label', pq, instance_ids=torch.from_numpy(ids))
    got = np.fromfile(str(tmp_path / 'c.label'), '<u4')
    assert got.tolist() == [0, 41 << 16 | 10, 65535 << 16 | 10, 65535 << 16 | 10, 1 << 16 | 10, 0]
    with pytest.raises(ValueError):
        write_semantic_kitti_labels(tmp_path / 'd.label', pq, instance_ids=np.array([0, 0, 0, 0, 65535, 0]))
    with pytest.raises(ValueError):
        write_semantic_kitti_labels(tmp_path / 'd.label', pq, instance_ids=ids[:3])
    assert not (tmp_path / 'd.label').exists()


def test_binding_table_and_header():
    from mask_bev_amd import _lib, build, ops
    names = ('mbv_track_frames', 'mbv_track_frames_workspace_bytes', 'mbv_tube_accumulate', 'mbv_tube_scores')
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    for name in names:
        assert name in _lib.SIGNATURES and name + '(' in header
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [22, 4, 13, 10]
    assert _lib.ABI_VERSION == 59 and build.FILE_FLAGS['track.hip'] == ['-ffp-contract=off']
    for name in ('track_frames', 'tube_accumulate', 'tube_scores', 'TrackState', 'TrackFrames', 'TubeTables', 'TubeScores'):
        assert hasattr(ops, name)
    with pytest.raises(_lib.MaskBevHipError):
        ops.track_frames(torch.zeros((1, 4, 4), dtype=torch.int32), torch.zeros((1, 2, 3), dtype=torch.float64),
                         ops.TrackState.fresh(4, 4, 4, 'cpu'), 0.0, 0.0, 1.0, 4)
