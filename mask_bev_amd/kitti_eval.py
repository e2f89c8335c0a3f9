"""KITTI BEV and 3D evaluation on the device: "Car BEV AP, easy / moderate / hard" for boxes fitted to predicted instance
masks and, when the predictions carry a height lifted from the points (``Predictions.boxes3d``, K31), "Car 3D AP".

What the reference does in mask_bev/evaluation/kitti_eval.py (the official KITTI protocol in numba on the host) and
mask_bev/evaluation/rotate_iou.py (a numba-CUDA rotated-box IoU, launched per part of the set), here on three kernels:
K25 fits an oriented box to every kept mask (``Predictions.boxes``), K26 computes the rotated-box overlaps of all frames in
one launch, K27 runs the protocol's greedy assignment for all frames and score thresholds at once.  The host keeps what is
per box or per evaluation: the class / difficulty codes (``clean_data``), the 41 recall sample points (``get_thresholds``)
and the 11-point AP (``get_mAP``).

Departures from the reference, all deliberate:
* No image-box line (the model predicts no image box), and with it no DontCare regions and no orientation score (AOS),
  which only the image-box metric uses.  The ``3d`` line is printed when every prediction carries ``boxes3d``: the model
  predicts no height either, but the scan has a z for every point, and K31 lifts the z-extent of the returns inside a mask
  (``Predictions.boxes3d``); K26b then multiplies K26's BEV intersection by the common z-interval — the reference's
  ``d3_box_overlap`` with ``z_center = 1``, in a z-up frame — and K27 runs unchanged.  The reference's own ``mask_to_pred``
  writes a height of 0, so its ``3d`` line is meaningless.  NOT pinned: that height is the extent of the returns — ground to
  roof only if the ground is in range, stretched by overhanging structure unless a quantile extent is used — and no accuracy
  number on real KITTI has been measured.
* Boxes are (x, y, l, w, yaw) in the VELODYNE frame with the corner convention of ``rasterize.box_vertices`` and
  ``batch.kitti_labels_to_velodyne`` (yaw turns counter-clockwise), not camera-frame (x, z) boxes with a clockwise angle:
  an overlap does not depend on the frame it is computed in.
* ``mask_to_pred`` there takes ``cv2.minAreaRect`` of the largest contour (and, thresholding a sigmoid at 127, can never
  produce a box).  By default ALL set cells of a mask are used and the box is the moment-axis box of K25.
  ``method='min_area_rect'`` (``Predictions.boxes``, ``mask_to_pred``; the launcher's ``kitti_box_method``) follows the
  reference's recipe on the device: the largest 8-connected component (K30a), then its minimum-area rectangle (K30b), both
  pinned against an exact oracle.  Still not pinned: the reference selects the contour by ``cv2.contourArea`` (K30a counts
  cells), and OpenCV's own floating-point rectangle arithmetic (K30b chooses in exact integers).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops_eval
from ._lib import MaskBevHipError
from .rasterize import KITTI_TYPES

CLASS_NAMES = ('car', 'pedestrian', 'cyclist', 'van', 'person_sitting')      # the protocol's class indices 0 .. 4
MIN_HEIGHT = (40, 25, 25)                 # pixels of the image box, per difficulty (easy, moderate, hard)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
N_SAMPLE_PTS = 41
DIFFICULTIES = ('easy', 'moderate', 'hard')
BEV_MIN_OVERLAPS = {0: (0.7, 0.5), 1: (0.5, 0.25), 2: (0.5, 0.25), 3: (0.7, 0.5), 4: (0.5, 0.25)}   # official, relaxed
# the `3d` rows of the reference's get_official_eval_result (overlap_mod / overlap_easy): the same numbers as its `bev` rows
D3_MIN_OVERLAPS = {0: (0.7, 0.5), 1: (0.5, 0.25), 2: (0.5, 0.25), 3: (0.7, 0.5), 4: (0.5, 0.25)}
METRICS = ('bev', '3d')
_DT_HEIGHT = 100.0                        # the reference's dummy image box [0, 0, 0, 100] of a prediction


def _class_index(current_class) -> int:
    if isinstance(current_class, str):
        return CLASS_NAMES.index(current_class.lower())
    return int(current_class)


def clean_data(gt: dict, dt: dict, current_class=0, difficulty: int = 0) -> Tuple[int, np.ndarray, np.ndarray]:
    """Per-box codes of one frame for a class and a difficulty.  ``gt``: a label dictionary as ``batch.read_kitti_label``
    returns it (``type`` codes into ``rasterize.KITTI_TYPES``, ``bbox``, ``occluded``, ``truncated``); ``dt``: ``type``
    (k) codes and optionally ``bbox`` (k, 4) (absent: 100 pixels high, the reference's dummy box) →
    ``(num_valid_gt, ignored_gt (n) int32, ignored_dt (k) int32)``: 0 counted; 1 of the class but harder than the
    difficulty, or the neighbouring class (Van for Car, Person_sitting for Pedestrian); -1 another class."""
    want = CLASS_NAMES[_class_index(current_class)]
    neighbour = {'car': 'van', 'pedestrian': 'person_sitting'}.get(want, '')
    names = np.array([KITTI_TYPES[int(t)].lower() for t in np.asarray(gt['type']).reshape(-1)], dtype=object)
    n = names.shape[0]
    bbox = np.asarray(gt['bbox'], dtype=np.float64).reshape(n, 4)
    hard = ((np.asarray(gt['occluded']).reshape(n) > MAX_OCCLUSION[difficulty])
            | (np.asarray(gt['truncated'], dtype=np.float64).reshape(n) > MAX_TRUNCATION[difficulty])
            | (bbox[:, 3] - bbox[:, 1] <= MIN_HEIGHT[difficulty]))
    same = names == want
    ignored_gt = np.full((n,), -1, dtype=np.int32)
    ignored_gt[(names == neighbour) | (same & hard)] = 1
    ignored_gt[same & ~hard] = 0
    dt_names = np.array([KITTI_TYPES[int(t)].lower() for t in np.asarray(dt['type']).reshape(-1)], dtype=object)
    k = dt_names.shape[0]
    if dt.get('bbox') is not None:
        b = np.asarray(dt['bbox'], dtype=np.float64).reshape(k, 4)
        height = np.abs(b[:, 3] - b[:, 1])
    else:
        height = np.full((k,), _DT_HEIGHT)
    ignored_dt = np.where(height < MIN_HEIGHT[difficulty], 1, np.where(dt_names == want, 0, -1)).astype(np.int32)
    return int((ignored_gt == 0).sum()), ignored_gt, ignored_dt


def get_thresholds(scores, num_gt: int, num_sample_pts: int = N_SAMPLE_PTS) -> np.ndarray:
    """The score thresholds at the recall sample points 0, 1 / 40, ..., 1: ``scores`` are those of the detections matched
    as true positives; walking them in descending order, a score is taken when its recall (i + 1) / num_gt is the closest
    to the current sample point, which then advances.  At most ``num_sample_pts`` values, float64."""
    scores = np.sort(np.asarray(scores, dtype=np.float64).reshape(-1))[::-1]
    step, current, out = 1.0 / (num_sample_pts - 1.0), 0.0, []
    last = scores.shape[0] - 1
    for i, score in enumerate(scores):
        left = (i + 1) / num_gt
        right = (i + 2) / num_gt if i < last else left
        if i < last and (right - current) < (current - left):
            continue
        out.append(score)
        current += step
    return np.array(out, dtype=np.float64)


def get_mAP(prec) -> np.ndarray:
    """11-point interpolated AP in percent over the last axis: every 4th of the 41 sample points, divided by 11."""
    prec = np.asarray(prec, dtype=np.float64)
    return prec[..., ::4].sum(-1) / 11 * 100


get_mAP_v2 = get_mAP


def _as_device_f32(x, device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=torch.float32)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).to(device, non_blocking=True)


def _gt_bev(label: dict) -> np.ndarray:
    if 'boxes' not in label:
        raise ValueError('eval_kitti: labels must be in the velodyne frame (batch.kitti_labels_to_velodyne adds `boxes`)')
    return np.asarray(label['boxes'], dtype=np.float64).reshape(-1, 7)[:, [0, 1, 3, 4, 6]]


def _gt_3d(label: dict) -> np.ndarray:
    if 'boxes' not in label:
        raise ValueError('eval_kitti: labels must be in the velodyne frame (batch.kitti_labels_to_velodyne adds `boxes`)')
    return np.asarray(label['boxes'], dtype=np.float64).reshape(-1, 7)


def d3_box_overlap(boxes, qboxes, criterion: int = -1, device=None) -> np.ndarray:
    """(N, 7), (K, 7) arrays [x, y, z, dx, dy, dz, angle], z the bottom face → (N, K) float32 overlaps through K26b (one
    frame, synchronises)."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    a, b = _as_device_f32(np.asarray(boxes).reshape(-1, 7), dev), _as_device_f32(np.asarray(qboxes).reshape(-1, 7), dev)
    out, _ = ops_eval.rotate_iou_3d(a, b, criterion=criterion)
    return out.view(a.shape[0], b.shape[0]).cpu().numpy()


def bev_box_overlap(boxes, qboxes, criterion: int = -1, device=None) -> np.ndarray:
    """(N, 5), (K, 5) arrays [x, y, dx, dy, angle] → (N, K) float32 overlaps through K26 (one frame, synchronises)."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    a, b = _as_device_f32(np.asarray(boxes).reshape(-1, 5), dev), _as_device_f32(np.asarray(qboxes).reshape(-1, 5), dev)
    out, _ = ops_eval.rotate_iou(a, b, criterion=criterion)
    return out.view(a.shape[0], b.shape[0]).cpu().numpy()


@torch.no_grad()
def eval_class(labels: Sequence[dict], predictions: Sequence[dict], current_classes=(0,), difficultys=(0, 1, 2),
               min_overlaps=None, device=None, metric: str = 'bev') -> dict:
    """The BEV metric (``metric='bev'``, the reference's ``metric == 1``) or the 3D metric (``metric='3d'``, its
    ``metric == 2``: ``boxes3d`` (k, 7) [x, y, z_bottom, l, w, h, yaw] of the predictions against all seven columns of the
    labels' ``boxes``, through K26b) for F frames.

    ``labels``: per frame a velodyne-frame label dictionary (``batch.kitti_labels_to_velodyne``: ``boxes`` (n, 7), ``type``,
    ``bbox``, ``occluded``, ``truncated``).  ``predictions``: per frame ``{'boxes': (k, 5) [x, y, l, w, yaw], 'score': (k),
    'type': (k) codes}`` as ``Predictions.kitti_predictions`` returns them (device tensors or arrays).  ``min_overlaps``:
    (K, C) — per overlap level and class; default the official and the relaxed BEV thresholds.

    Returns ``precision`` and ``thresholds`` (C, D, K, 41) float64, ``num_thresholds`` (C, D, K), ``stats`` (C, D, K, 41, 3)
    int64 (tp, fp, fn per threshold), ``num_valid_gt`` (C, D) and ``min_overlaps``.

    All per-pair and per-frame work runs on the device: one K26 launch, then per (class, difficulty, overlap) one K27 launch
    that collects the matched scores and one that counts tp / fp / fn at all thresholds.  Host synchronisations per call: TWO,
    whatever the number of frames — the copy of the matched scores of all combinations, and the copy of their (T, 3) sums."""
    if metric not in METRICS:
        raise ValueError(f'eval_class: metric must be one of {METRICS}, got {metric!r}')
    if len(labels) != len(predictions):
        raise ValueError('eval_class: one prediction entry per label frame expected')
    if len(labels) == 0:
        raise ValueError('eval_class: no frame')
    classes = [_class_index(c) for c in current_classes]
    if min_overlaps is None:
        table = BEV_MIN_OVERLAPS if metric == 'bev' else D3_MIN_OVERLAPS
        min_overlaps = np.array([[table[c][k] for c in classes] for k in range(2)], dtype=np.float64)
    min_overlaps = np.asarray(min_overlaps, dtype=np.float64).reshape(-1, len(classes))
    if device is None:
        devs = [p['boxes'].device for p in predictions if isinstance(p['boxes'], torch.Tensor) and p['boxes'].is_cuda]
        device = devs[0] if devs else torch.device('cuda', torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise MaskBevHipError(f'eval_class needs a ROCm device (no CPU fallback), got {dev}')
    box_key, width = ('boxes', 5) if metric == 'bev' else ('boxes3d', 7)
    if any(box_key not in p for p in predictions):
        raise ValueError(f"eval_class: metric {metric!r} needs `{box_key}` in every prediction")
    for p in predictions:
        for key in (box_key, 'score'):
            if isinstance(p[key], torch.Tensor) and not p[key].is_cuda and p[key].numel() > 0:
                raise MaskBevHipError('eval_class: prediction tensors must live on the ROCm device (or be numpy arrays)')

    dt_counts = [int(p[box_key].shape[0]) for p in predictions]
    gt_boxes = [_gt_bev(lab) if metric == 'bev' else _gt_3d(lab) for lab in labels]
    dt_tab = torch.cat([_as_device_f32(p[box_key], dev).reshape(-1, width) for p in predictions])
    dt_scores = torch.cat([_as_device_f32(p['score'], dev).reshape(-1) for p in predictions])
    gt_tab = _as_device_f32(np.concatenate(gt_boxes), dev)
    dt_off = np.concatenate([[0], np.cumsum(dt_counts)])
    gt_off = np.concatenate([[0], np.cumsum([b.shape[0] for b in gt_boxes])])
    overlap_fn = ops_eval.rotate_iou if metric == 'bev' else ops_eval.rotate_iou_3d
    overlaps, offs = overlap_fn(dt_tab, gt_tab, dt_off, gt_off, criterion=-1)               # detections first, as the protocol
    dt_types = [np.asarray(p['type'].cpu() if isinstance(p['type'], torch.Tensor) else p['type']).reshape(-1)
                for p in predictions]
    dt_host = [{'type': t, 'bbox': p.get('bbox')} for t, p in zip(dt_types, predictions)]

    nc, nd, nk = len(classes), len(difficultys), min_overlaps.shape[0]
    combos, valid = [], np.zeros((nc, nd), dtype=np.int64)
    for m, cls in enumerate(classes):
        for l, difficulty in enumerate(difficultys):
            codes = [clean_data(g, d, cls, difficulty) for g, d in zip(labels, dt_host)]
            valid[m, l] = sum(c[0] for c in codes)
            ign_gt = torch.from_numpy(np.concatenate([c[1] for c in codes]).astype(np.int32)).to(dev, non_blocking=True)
            ign_dt = torch.from_numpy(np.concatenate([c[2] for c in codes]).astype(np.int32)).to(dev, non_blocking=True)
            for k in range(nk):
                combos.append((m, l, k, ign_gt, ign_dt, float(min_overlaps[k, m])))
    # pass 1: the scores of the true positives with no threshold, for every combination; ONE copy to the host
    first = [ops_eval.kitti_statistics(overlaps, offs, ig, idt, dt_scores, mo, None, compute_fp=False, collect_scores=True)
             for _, _, _, ig, idt, mo in combos]
    tp_scores = torch.stack([f[1] for f in first]).cpu().numpy()                                  # synchronisation 1
    tp_flags = torch.stack([f[2] for f in first]).cpu().numpy()
    thresholds = np.zeros((nc, nd, nk, N_SAMPLE_PTS))
    counts = np.zeros((nc, nd, nk), dtype=np.int64)
    table = np.zeros((len(combos), N_SAMPLE_PTS), dtype=np.float32)
    for i, (m, l, k, _, _, _) in enumerate(combos):
        th = get_thresholds(tp_scores[i][tp_flags[i] != 0], valid[m, l]) if valid[m, l] > 0 else np.zeros((0,))
        counts[m, l, k] = th.shape[0]
        thresholds[m, l, k, :th.shape[0]] = th
        table[i, :th.shape[0]] = th                                     # the scores are f32 values: the round trip is exact
    table_dev = torch.from_numpy(table).to(dev, non_blocking=True)
    # pass 2: tp / fp / fn at every threshold; the padding thresholds are computed and dropped; ONE copy to the host
    second = [ops_eval.kitti_statistics(overlaps, offs, ig, idt, dt_scores, mo, table_dev[i], compute_fp=True)
              for i, (_, _, _, ig, idt, mo) in enumerate(combos)]
    sums = torch.stack(second).cpu().numpy()                                                      # synchronisation 2
    precision = np.zeros((nc, nd, nk, N_SAMPLE_PTS))
    stats = np.zeros((nc, nd, nk, N_SAMPLE_PTS, 3), dtype=np.int64)
    for i, (m, l, k, _, _, _) in enumerate(combos):
        t = counts[m, l, k]
        pr = sums[i, :t]
        stats[m, l, k, :t] = pr
        p = pr[:, 0] / np.maximum(pr[:, 0] + pr[:, 1], 1)
        precision[m, l, k, :t] = np.maximum.accumulate(p[::-1])[::-1]                           # max over the later points
    return dict(precision=precision, thresholds=thresholds, num_thresholds=counts, stats=stats, num_valid_gt=valid,
                min_overlaps=min_overlaps)


class EvalResult(str):
    """The result text of the reference's ``get_official_eval_result`` (the ``bev`` lines, and the ``3d`` lines when the
    predictions carry ``boxes3d``); the numbers are in ``metrics``:
    ``{'Car': {'bev_ap@0.70': {'easy': .., 'moderate': .., 'hard': ..}, 'bev_ap@0.50': {...}}}`` (with ``boxes3d`` also
    ``'3d_ap@0.70'``, ``'3d_ap@0.50'``) and in ``raw`` (what ``eval_class`` returned for the BEV metric; with ``boxes3d`` it
    gains the entry ``'3d'``: what ``eval_class(metric='3d')`` returned)."""
    metrics: Dict[str, dict]
    raw: dict


def get_official_eval_result(labels: Sequence[dict], predictions: Sequence[dict], current_classes=(0,),
                             difficultys=(0, 1, 2), device=None) -> EvalResult:
    """``eval_class`` formatted as the reference formats it: per class and overlap level a header line and the ``bev  AP:``
    line with the APs of the difficulties; when EVERY prediction dictionary has ``boxes3d`` (``Predictions.kitti_predictions``
    with ``scans``), a ``3d   AP:`` line follows each of them.  The ``bbox`` and ``aos`` lines are omitted: nothing here
    predicts an image box.  The header shows the BEV overlap; the 3D table holds the same numbers."""
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    classes = [_class_index(c) for c in current_classes]
    raw = eval_class(labels, predictions, classes, difficultys, device=device)
    ap = get_mAP(raw['precision'])                                              # (C, D, K)
    with_3d = len(predictions) > 0 and all('boxes3d' in p for p in predictions)
    if with_3d:
        raw = dict(raw)
        raw['3d'] = eval_class(labels, predictions, classes, difficultys, device=device, metric='3d')
        ap3d = get_mAP(raw['3d']['precision'])
    text, metrics = '', {}
    for m, cls in enumerate(classes):
        name = KITTI_TYPES[[t.lower() for t in KITTI_TYPES].index(CLASS_NAMES[cls])]
        metrics[name] = {}
        for k in range(raw['min_overlaps'].shape[0]):
            mo = raw['min_overlaps'][k, m]
            text += f'{name} AP(Average Precision)@{mo:.2f}:\n'
            text += 'bev  AP:' + ', '.join(f'{v:.2f}' for v in ap[m, :, k]) + '\n'
            metrics[name][f'bev_ap@{mo:.2f}'] = {DIFFICULTIES[d]: float(ap[m, l, k]) for l, d in enumerate(difficultys)}
            if with_3d:
                mo3 = raw['3d']['min_overlaps'][k, m]
                text += '3d   AP:' + ', '.join(f'{v:.2f}' for v in ap3d[m, :, k]) + '\n'
                metrics[name][f'3d_ap@{mo3:.2f}'] = {DIFFICULTIES[d]: float(ap3d[m, l, k]) for l, d in enumerate(difficultys)}
    out = EvalResult(text)
    out.metrics, out.raw = metrics, raw
    return out


def eval_kitti(labels: Sequence[dict], predictions: Sequence[dict], device=None) -> EvalResult:
    """Car BEV AP at overlaps 0.7 and 0.5, easy / moderate / hard, for F frames: ``labels`` the velodyne-frame label
    dictionaries (``batch.kitti_labels_to_velodyne(batch.read_kitti_label(..), calib)``), ``predictions`` what
    ``Predictions.kitti_predictions`` returns per scan.  The returned string prints as the reference's block (the image-box
    lines are omitted; the ``3d   AP:`` lines appear when every prediction carries ``boxes3d``) and carries the numbers in
    ``.metrics``.  Two host synchronisations per call and metric, independent of the number of frames (see ``eval_class``)."""
    return get_official_eval_result(labels, predictions, [0], (0, 1, 2), device=device)


def mask_to_pred(predictions, x_range, y_range=None, voxel_size=None, method: str = 'moment') -> List[dict]:
    """The reference's name for masks → boxes: ``Predictions.kitti_predictions`` (``method='moment'``: K25;
    ``'min_area_rect'``: K30a + K30b, the reference's own recipe)."""
    return predictions.kitti_predictions(x_range, y_range, voxel_size, method=method)


__all__ = ['clean_data', 'get_thresholds', 'get_mAP', 'get_mAP_v2', 'bev_box_overlap', 'd3_box_overlap', 'eval_class', 'eval_kitti',
           'get_official_eval_result', 'mask_to_pred', 'EvalResult', 'CLASS_NAMES', 'N_SAMPLE_PTS']
