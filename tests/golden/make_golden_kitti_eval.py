#!/usr/bin/env python3
"""Golden vectors for the KITTI BEV evaluation (K27 and mask_bev_amd/kitti_eval.py): the PROTOCOL, as the reference runs it.

    python tests/golden/make_golden_kitti_eval.py /path/to/the/reference/checkout

The reference's own mask_bev/evaluation/kitti_eval.py is imported UNMODIFIED from the checkout given on the command line and
its ``clean_data``, ``compute_statistics_jit``, ``get_thresholds``, ``eval_class`` (``metric=1``, ``num_parts=1``) and
``get_mAP_v2`` are run on 12 synthetic frames.  Packages that are not installed are served by stand-ins: ``numba.jit`` is the
identity, ``cv2`` an empty module, ``matplotlib`` an empty module, and ``mask_bev.evaluation.rotate_iou`` a module whose
``rotate_iou_gpu_eval`` is the float64 oracle of tests/kitti_eval_ref.py (the reference's kernel needs numba-CUDA) — so the
fixture pins the protocol's own lines and NOT the reference's IoU kernel.

Only inputs and recorded outputs are committed (tests/golden/kitti_eval.npz).  The frames hold a frame without ground truth,
one without detections, Van, Pedestrian and DontCare labels, labels ignored at every difficulty, tied scores and a detection
that overlaps two ground truths.  The script ASSERTS that no overlap lies within 1e-3 of 0.5 or 0.7, so a float32 overlap
cannot move a match, and that all scores are float32 values.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import kitti_eval_ref as R  # noqa: E402

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
    """Per frame (gt boxes (n, 5), gt types, occluded, truncated, image heights, dt boxes (k, 5), dt types, scores)."""
    frames = []
    for f in range(12):
        n = 0 if f == 3 else int(rng.integers(4, 10))
        gt = np.zeros((n, 5))
        cols = max(1, int(np.ceil(np.sqrt(max(n, 1)))))
        for i in range(n):                                              # a jittered lattice: ground truths do not overlap
            gt[i] = [8 + 12 * (i % cols) + rng.uniform(-1, 1), -20 + 12 * (i // cols) + rng.uniform(-1, 1),
                     rng.uniform(3.2, 5.0), rng.uniform(1.5, 2.1), rng.uniform(-np.pi, np.pi)]
        types_ = rng.choice([CAR, CAR, CAR, CAR, CAR, CAR, VAN, PEDESTRIAN, DONTCARE], n)
        occluded = rng.choice([0, 0, 0, 0, 1, 2, 3], n)
        truncated = rng.choice([0.0, 0.0, 0.0, 0.1, 0.2, 0.4, 0.6], n)
        heights = rng.choice([20.0, 30.0, 45.0, 80.0, 80.0, 120.0], n)
        dts, dtt = [], []
        if f != 5:
            for i in range(n):
                if rng.random() < 0.8:                                  # a detection near the ground truth: any IoU from 0.2 up
                    scale = rng.choice([0.05, 0.15, 0.3, 0.6])
                    d = gt[i] + np.array([rng.normal() * scale, rng.normal() * scale * 0.5, rng.normal() * 0.2 * scale,
                                          rng.normal() * 0.1 * scale, rng.normal() * 0.1 * scale])
                    dts.append(d)
                    dtt.append(CAR if rng.random() < 0.9 else PEDESTRIAN)
                if rng.random() < 0.25:                                 # a second detection on the same ground truth
                    dts.append(gt[i] + np.array([rng.normal() * 0.3, rng.normal() * 0.2, 0.1, 0.05, 0.05]))
                    dtt.append(CAR)
            for _ in range(int(rng.integers(0, 4))):                    # false positives away from the lattice
                dts.append([rng.uniform(5, 60), rng.uniform(25, 38), rng.uniform(3, 5), rng.uniform(1.5, 2.1),
                            rng.uniform(-np.pi, np.pi)])
                dtt.append(CAR)
        if f == 7 and n >= 2:
            # two ground truths side by side and one detection over both: IoU with each about 0.4 .. 0.6
            gt[0] = [30.0, 30.0, 4.0, 1.8, 0.0]
            gt[1] = [30.0, 32.0, 4.0, 1.8, 0.0]
            types_[:2], occluded[:2], truncated[:2], heights[:2] = CAR, 0, 0.0, 80.0
            dts.append([30.0, 31.0, 4.0, 3.3, 0.0])
            dtt.append(CAR)
        dt = np.array(dts, dtype=np.float64).reshape(-1, 5)
        scores = (rng.integers(8, 64, dt.shape[0]) / 64.0).astype(np.float32).astype(np.float64)     # ties, f32 values
        frames.append((gt, types_.astype(np.int64), occluded.astype(np.int64), truncated, heights, dt,
                       np.array(dtt, dtype=np.int64), scores))
    return frames


def margins_ok(frames):
    for gt, _, _, _, _, dt, _, _ in frames:
        ov = R.rotate_iou(dt, gt)
        if np.any(np.abs(ov - 0.5) < 1e-3) or np.any(np.abs(ov - 0.7) < 1e-3):
            return False
    return True


def annos(frames):
    gt_annos, dt_annos = [], []
    for gt, tp, occ, trunc, h, dt, dtt, sc in frames:
        n, k = gt.shape[0], dt.shape[0]
        bbox = np.stack([np.zeros(n), np.zeros(n), np.full(n, 50.0), h], axis=1).reshape(n, 4)
        gt_annos.append(dict(name=np.array([R.KITTI_TYPES[t] for t in tp], dtype='<U16'), bbox=bbox,
                             location=np.stack([gt[:, 0], np.zeros(n), gt[:, 1]], axis=1).reshape(n, 3),
                             dimensions=np.stack([gt[:, 2], np.zeros(n), gt[:, 3]], axis=1).reshape(n, 3),
                             rotation_y=gt[:, 4].copy(), score=np.zeros(n), alpha=np.zeros(n), occluded=occ, truncated=trunc))
        dt_annos.append(dict(name=np.array([R.KITTI_TYPES[t] for t in dtt], dtype='<U16'),
                             bbox=np.tile(np.array([[0.0, 0.0, 0.0, 100.0]]), (k, 1)).reshape(k, 4),
                             location=np.stack([dt[:, 0], np.zeros(k), dt[:, 1]], axis=1).reshape(k, 3),
                             dimensions=np.stack([dt[:, 2], np.zeros(k), dt[:, 3]], axis=1).reshape(k, 3),
                             rotation_y=dt[:, 4].copy(), score=sc.copy(), alpha=np.zeros(k)))
    return gt_annos, dt_annos


def main():
    seed = 27
    while True:
        frames = make_frames(np.random.default_rng(seed))
        if margins_ok(frames):
            break
        seed += 1
    gt_annos, dt_annos = annos(frames)
    # the frame of the planted detection: it overlaps both ground truths above 0.25
    ov7 = R.rotate_iou(frames[7][5][-1:], frames[7][0][:2])
    assert np.all(ov7 > 0.25), ov7
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

    # clean_data, per difficulty and frame
    valid = []
    for d in range(3):
        codes = [K.clean_data(g, t, 0, d) for g, t in zip(gt_annos, dt_annos)]
        valid.append(sum(c[0] for c in codes))
        out[f'ignored_gt_{d}'] = np.concatenate([np.array(c[1], dtype=np.int64) for c in codes])
        out[f'ignored_dt_{d}'] = np.concatenate([np.array(c[2], dtype=np.int64) for c in codes])
        assert {0, 1, -1} <= set(out[f'ignored_gt_{d}'].tolist())
    out['num_valid_gt'] = np.array(valid, dtype=np.int64)
    assert valid[0] < valid[2]

    # eval_class, BEV.  min_overlaps is indexed [level, metric, class]
    min_overlaps = np.array([[[0.7], [0.7], [0.7]], [[0.7], [0.5], [0.5]]])
    copies = ([{k: v.copy() for k, v in a.items()} for a in gt_annos], [{k: v.copy() for k, v in a.items()} for a in dt_annos])
    ret = K.eval_class(copies[0], copies[1], [0], [0, 1, 2], 1, min_overlaps, num_parts=1)
    out['precision'], out['thresholds'] = ret['precision'][0], ret['thresholds'][0]                   # (3, 2, 41)
    out['ap'] = K.get_mAP_v2(ret['precision'])[0]                                                      # (3, 2)
    assert np.all(np.isfinite(out['precision'])) and out['ap'].max() > 10

    # tp / fp / fn per threshold, from compute_statistics_jit called as fused_compute_statistics calls it
    overlaps = [R.rotate_iou(f[5], f[0]) for f in frames]
    stats = np.zeros((3, 2, 41, 3), dtype=np.int64)
    counts = np.zeros((3, 2), dtype=np.int64)
    for d in range(3):
        for k, mo in enumerate((0.7, 0.5)):
            matched = []
            for i, (g, t) in enumerate(zip(gt_annos, dt_annos)):
                gd = np.concatenate([g['bbox'], g['alpha'][:, None]], 1)
                dd = np.concatenate([t['bbox'], t['alpha'][:, None], t['score'][:, None]], 1)
                ig = out[f'ignored_gt_{d}'][out['gt_offsets'][i]:out['gt_offsets'][i + 1]]
                idt = out[f'ignored_dt_{d}'][out['dt_offsets'][i]:out['dt_offsets'][i + 1]]
                matched += K.compute_statistics_jit(overlaps[i], gd, dd, ig, idt, np.zeros((0, 4)), 1, min_overlap=mo,
                                                    thresh=0.0, compute_fp=False)[4].tolist()
            th = np.array(K.get_thresholds(np.array(matched), valid[d]))
            assert np.array_equal(th, out['thresholds'][d, k, :len(th)]) and not out['thresholds'][d, k, len(th):].any()
            counts[d, k] = len(th)
            for ti, thresh in enumerate(th):
                for i, (g, t) in enumerate(zip(gt_annos, dt_annos)):
                    gd = np.concatenate([g['bbox'], g['alpha'][:, None]], 1)
                    dd = np.concatenate([t['bbox'], t['alpha'][:, None], t['score'][:, None]], 1)
                    ig = out[f'ignored_gt_{d}'][out['gt_offsets'][i]:out['gt_offsets'][i + 1]]
                    idt = out[f'ignored_dt_{d}'][out['dt_offsets'][i]:out['dt_offsets'][i + 1]]
                    stats[d, k, ti] += K.compute_statistics_jit(overlaps[i], gd, dd, ig, idt, np.zeros((0, 4)), 1,
                                                                min_overlap=mo, thresh=thresh, compute_fp=True)[:3]
    out['stats'], out['num_thresholds'] = stats, counts
    path = os.path.join(HERE, 'kitti_eval.npz')
    np.savez_compressed(path, **out)
    print('seed', seed, 'frames', len(frames), 'gt', len(out['gt_boxes']), 'dt', len(out['dt_boxes']), 'valid', valid)
    print('thresholds per (difficulty, overlap)', counts.tolist())
    print('AP', np.round(out['ap'], 3).tolist())
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
