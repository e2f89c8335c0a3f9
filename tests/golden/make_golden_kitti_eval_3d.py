#!/usr/bin/env python3
"""Golden vectors for the KITTI 3D evaluation (K26b, K27 and mask_bev_amd/kitti_eval.py, ``metric='3d'``): the PROTOCOL, as
the reference runs it.

    python tests/golden/make_golden_kitti_eval_3d.py /path/to/the/reference/checkout

The stand-in scheme of make_golden_kitti_eval.py: the reference's own mask_bev/evaluation/kitti_eval.py is imported UNMODIFIED
from the checkout given on the command line; ``numba.jit`` is the identity, ``cv2`` and (where missing) ``matplotlib`` are
empty modules, and ``mask_bev.evaluation.rotate_iou.rotate_iou_gpu_eval`` is the float64 oracle of tests/kitti_eval_ref.py
(the reference's kernel needs numba-CUDA) — so the fixture pins ``d3_box_overlap_kernel`` (the z part and the criteria) and the
protocol's own lines, NOT the reference's BEV intersection.  Its ``d3_box_overlap``, ``clean_data``, ``eval_class``
(``metric=2``, ``num_parts=1``, the camera defaults ``z_axis=1``, ``z_center=1.0``), ``compute_statistics_jit`` and
``get_mAP_v2`` are run on 12 synthetic frames.

The frames are made in the velodyne frame, boxes (x, y, z, l, w, h, yaw) with z the bottom face — what the product takes — and
handed to the reference in a camera frame that is a fixed signed permutation of it: camera (x, y, z) = velodyne (x, -z, y),
``dimensions`` = (l, h, w), ``rotation_y`` = yaw.  The camera's y points down and ``location`` is the bottom face, so the
reference's interval [y - h, y] is the velodyne interval [z, z + h] mirrored: the same overlap.

Only inputs and recorded outputs are committed (tests/golden/kitti_eval_3d.npz).  The script ASSERTS that no 3-D overlap lies
within 1e-3 of 0.5 or 0.7, so a float32 overlap cannot move a match, that all scores are float32 values, and that the frames
hold pairs that overlap in BEV but not in z.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import kitti_eval_ref as R  # noqa: E402
from tests import point_lift_ref as L  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)


def _identity_jit(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda fn: fn


numba = types.ModuleType('numba')
numba.jit = _identity_jit
sys.modules['numba'] = numba
sys.modules['cv2'] = types.ModuleType('cv2')
for _name in ('matplotlib', 'matplotlib.pyplot'):
    try:
        __import__(_name)
    except ImportError:
        sys.modules[_name] = types.ModuleType(_name)
_riou = types.ModuleType('mask_bev.evaluation.rotate_iou')
_riou.rotate_iou_gpu_eval = lambda boxes, qboxes, criterion=-1, device_id=0: R.rotate_iou(boxes, qboxes, criterion)
sys.modules['mask_bev.evaluation.rotate_iou'] = _riou
sys.path.insert(0, sys.argv[1])
from mask_bev.evaluation import kitti_eval as K  # noqa: E402

assert os.path.abspath(K.__file__).startswith(os.path.abspath(sys.argv[1])), K.__file__

CAR, VAN, PEDESTRIAN, DONTCARE = 0, 1, 3, 8


def make_frames(rng):
    """Per frame (gt boxes (n, 7), gt types, occluded, truncated, image heights, dt boxes (k, 7), dt types, scores)."""
    frames = []
    for f in range(12):
        n = 0 if f == 3 else int(rng.integers(4, 10))
        gt = np.zeros((n, 7))
        cols = max(1, int(np.ceil(np.sqrt(max(n, 1)))))
        for i in range(n):                                              # a jittered lattice: ground truths do not overlap
            gt[i] = [8 + 12 * (i % cols) + rng.uniform(-1, 1), -20 + 12 * (i // cols) + rng.uniform(-1, 1),
                     rng.uniform(-1.9, -1.4), rng.uniform(3.2, 5.0), rng.uniform(1.5, 2.1), rng.uniform(1.4, 1.9),
                     rng.uniform(-np.pi, np.pi)]
        types_ = rng.choice([CAR, CAR, CAR, CAR, CAR, CAR, VAN, PEDESTRIAN, DONTCARE], n)
        occluded = rng.choice([0, 0, 0, 0, 1, 2, 3], n)
        truncated = rng.choice([0.0, 0.0, 0.0, 0.1, 0.2, 0.4, 0.6], n)
        heights = rng.choice([20.0, 30.0, 45.0, 80.0, 80.0, 120.0], n)
        dts, dtt = [], []
        if f != 5:
            for i in range(n):
                if rng.random() < 0.8:                                  # a detection near the ground truth: any IoU from 0.1 up
                    scale = rng.choice([0.05, 0.15, 0.3, 0.6])
                    d = gt[i] + np.array([rng.normal() * scale, rng.normal() * scale * 0.5, rng.normal() * 0.15 * scale,
                                          rng.normal() * 0.2 * scale, rng.normal() * 0.1 * scale, rng.normal() * 0.15 * scale,
                                          rng.normal() * 0.1 * scale])
                    dts.append(d)
                    dtt.append(CAR if rng.random() < 0.9 else PEDESTRIAN)
                if rng.random() < 0.25:                                 # a second detection on the same ground truth
                    dts.append(gt[i] + np.array([rng.normal() * 0.3, rng.normal() * 0.2, 0.1, 0.1, 0.05, -0.1, 0.05]))
                    dtt.append(CAR)
                if rng.random() < 0.15:                                 # right in BEV, but floating above the ground truth
                    dts.append(gt[i] + np.array([0.05, 0.02, gt[i, 5] + 0.3, 0.0, 0.0, 0.0, 0.01]))
                    dtt.append(CAR)
            for _ in range(int(rng.integers(0, 4))):                    # false positives away from the lattice
                dts.append([rng.uniform(5, 60), rng.uniform(25, 38), rng.uniform(-1.9, -1.4), rng.uniform(3, 5),
                            rng.uniform(1.5, 2.1), rng.uniform(1.4, 1.9), rng.uniform(-np.pi, np.pi)])
                dtt.append(CAR)
        if f == 7 and n >= 2:
            # two ground truths side by side and one detection over both
            gt[0] = [30.0, 30.0, -1.7, 4.0, 1.8, 1.6, 0.0]
            gt[1] = [30.0, 32.0, -1.7, 4.0, 1.8, 1.6, 0.0]
            types_[:2], occluded[:2], truncated[:2], heights[:2] = CAR, 0, 0.0, 80.0
            dts.append([30.0, 31.0, -1.7, 4.0, 3.3, 1.6, 0.0])
            dtt.append(CAR)
        dt = np.array(dts, dtype=np.float64).reshape(-1, 7)
        scores = (rng.integers(8, 64, dt.shape[0]) / 64.0).astype(np.float32).astype(np.float64)     # ties, f32 values
        frames.append((gt, types_.astype(np.int64), occluded.astype(np.int64), truncated, heights, dt,
                       np.array(dtt, dtype=np.int64), scores))
    return frames


def camera(b):
    """velodyne (n, 7) [x, y, z, l, w, h, yaw] → the reference's location (n, 3), dimensions (n, 3), rotation_y (n)."""
    n = b.shape[0]
    return (np.stack([b[:, 0], -b[:, 2], b[:, 1]], axis=1).reshape(n, 3), np.stack([b[:, 3], b[:, 5], b[:, 4]], axis=1).reshape(n, 3),
            b[:, 6].copy())


def camera7(b):
    loc, dims, rot = camera(b)
    return np.concatenate([loc, dims, rot[:, None]], axis=1)


def margins_ok(frames):
    for gt, _, _, _, _, dt, _, _ in frames:
        ov = L.rotate_iou_3d(dt, gt)
        if np.any(np.abs(ov - 0.5) < 1e-3) or np.any(np.abs(ov - 0.7) < 1e-3):
            return False
    return True


def annos(frames):
    gt_annos, dt_annos = [], []
    for gt, tp, occ, trunc, h, dt, dtt, sc in frames:
        n, k = gt.shape[0], dt.shape[0]
        bbox = np.stack([np.zeros(n), np.zeros(n), np.full(n, 50.0), h], axis=1).reshape(n, 4)
        loc, dims, rot = camera(gt)
        gt_annos.append(dict(name=np.array([R.KITTI_TYPES[t] for t in tp], dtype='<U16'), bbox=bbox, location=loc,
                             dimensions=dims, rotation_y=rot, score=np.zeros(n), alpha=np.zeros(n), occluded=occ,
                             truncated=trunc))
        loc, dims, rot = camera(dt)
        dt_annos.append(dict(name=np.array([R.KITTI_TYPES[t] for t in dtt], dtype='<U16'),
                             bbox=np.tile(np.array([[0.0, 0.0, 0.0, 100.0]]), (k, 1)).reshape(k, 4), location=loc,
                             dimensions=dims, rotation_y=rot, score=sc.copy(), alpha=np.zeros(k)))
    return gt_annos, dt_annos


def main():
    seed = 31
    while True:
        frames = make_frames(np.random.default_rng(seed))
        if margins_ok(frames):
            break
        seed += 1
    gt_annos, dt_annos = annos(frames)
    all_scores = np.concatenate([f[7] for f in frames])
    assert np.array_equal(all_scores, all_scores.astype(np.float32).astype(np.float64))
    assert len(np.unique(all_scores)) < len(all_scores)                                    # tied scores
    out = {'seed': np.array(seed)}
    cat = lambda k, dtype: np.concatenate([np.asarray(f[k]).reshape((-1,) + np.asarray(f[k]).shape[1:]) for f in frames]).astype(dtype)   # noqa: E731
    out['gt_boxes'], out['gt_types'], out['gt_occluded'] = cat(0, np.float64), cat(1, np.int64), cat(2, np.int64)
    out['gt_truncated'], out['gt_heights'] = cat(3, np.float64), cat(4, np.float64)
    out['dt_boxes'], out['dt_types'], out['dt_scores'] = cat(5, np.float64), cat(6, np.int64), cat(7, np.float64)
    out['gt_offsets'] = np.concatenate([[0], np.cumsum([f[0].shape[0] for f in frames])]).astype(np.int64)
    out['dt_offsets'] = np.concatenate([[0], np.cumsum([f[5].shape[0] for f in frames])]).astype(np.int64)
    assert set(out['gt_types'].tolist()) >= {CAR, VAN, PEDESTRIAN, DONTCARE}

    # the reference's d3_box_overlap per frame, detections first (as its eval_class calls calculate_iou_partly), in the camera
    # frame; the oracle in the velodyne frame must agree, and some pairs must meet in BEV but not in z
    overlaps = [K.d3_box_overlap(camera7(f[5]), camera7(f[0]), z_axis=1, z_center=1.0).astype(np.float64) for f in frames]
    bev_only = 0
    for f, ov in zip(frames, overlaps):
        assert np.abs(ov - L.rotate_iou_3d(f[5], f[0])).max(initial=0.0) <= 1e-12
        bev_only += int(((R.rotate_iou(f[5][:, L.BEV], f[0][:, L.BEV]) > 0.3) & (ov == 0)).sum())
    assert bev_only >= 3, bev_only
    out['overlaps'] = np.concatenate([ov.reshape(-1) for ov in overlaps])
    for crit in (0, 1, 2):                                               # the other criteria, on the densest frame
        big = int(np.argmax([ov.size for ov in overlaps]))
        ref = K.d3_box_overlap(camera7(frames[big][5]), camera7(frames[big][0]), criterion=crit, z_axis=1, z_center=1.0)
        assert np.abs(ref - L.rotate_iou_3d(frames[big][5], frames[big][0], crit)).max() <= 1e-12

    valid = []
    for d in range(3):
        codes = [K.clean_data(g, t, 0, d) for g, t in zip(gt_annos, dt_annos)]
        valid.append(sum(c[0] for c in codes))
        out[f'ignored_gt_{d}'] = np.concatenate([np.array(c[1], dtype=np.int64) for c in codes])
        out[f'ignored_dt_{d}'] = np.concatenate([np.array(c[2], dtype=np.int64) for c in codes])
    out['num_valid_gt'] = np.array(valid, dtype=np.int64)
    assert valid[0] < valid[2]

    # eval_class, 3D (metric 2).  min_overlaps is indexed [level, metric, class]: the Car column of get_official_eval_result
    min_overlaps = np.array([[[0.7], [0.7], [0.7]], [[0.7], [0.5], [0.5]]])
    copies = ([{k: v.copy() for k, v in a.items()} for a in gt_annos], [{k: v.copy() for k, v in a.items()} for a in dt_annos])
    ret = K.eval_class(copies[0], copies[1], [0], [0, 1, 2], 2, min_overlaps, num_parts=1)
    out['precision'], out['thresholds'] = ret['precision'][0], ret['thresholds'][0]                   # (3, 2, 41)
    out['ap'] = K.get_mAP_v2(ret['precision'])[0]                                                      # (3, 2)
    assert np.all(np.isfinite(out['precision'])) and out['ap'].max() > 10

    stats = np.zeros((3, 2, 41, 3), dtype=np.int64)
    counts = np.zeros((3, 2), dtype=np.int64)
    for d in range(3):
        for k, mo in enumerate((0.7, 0.5)):
            matched = []
            args = []
            for i, (g, t) in enumerate(zip(gt_annos, dt_annos)):
                gd = np.concatenate([g['bbox'], g['alpha'][:, None]], 1)
                dd = np.concatenate([t['bbox'], t['alpha'][:, None], t['score'][:, None]], 1)
                ig = out[f'ignored_gt_{d}'][out['gt_offsets'][i]:out['gt_offsets'][i + 1]]
                idt = out[f'ignored_dt_{d}'][out['dt_offsets'][i]:out['dt_offsets'][i + 1]]
                args.append((overlaps[i], gd, dd, ig, idt, np.zeros((0, 4)), 2))
                matched += K.compute_statistics_jit(*args[-1], min_overlap=mo, thresh=0.0, compute_fp=False)[4].tolist()
            th = np.array(K.get_thresholds(np.array(matched), valid[d]))
            assert np.array_equal(th, out['thresholds'][d, k, :len(th)]) and not out['thresholds'][d, k, len(th):].any()
            counts[d, k] = len(th)
            for ti, thresh in enumerate(th):
                for a in args:
                    stats[d, k, ti] += K.compute_statistics_jit(*a, min_overlap=mo, thresh=thresh, compute_fp=True)[:3]
    out['stats'], out['num_thresholds'] = stats, counts
    path = os.path.join(HERE, 'kitti_eval_3d.npz')
    np.savez_compressed(path, **out)
    print('seed', seed, 'frames', len(frames), 'gt', len(out['gt_boxes']), 'dt', len(out['dt_boxes']), 'valid', valid)
    print('thresholds per (difficulty, overlap)', counts.tolist(), 'pairs that meet in BEV only', bev_only)
    print('AP', np.round(out['ap'], 3).tolist())
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
