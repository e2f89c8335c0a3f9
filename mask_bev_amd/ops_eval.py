"""K25 — oriented box of a bit-packed mask (csrc/box_fit.hip); K26 — rotated-box overlap over ragged frames
(csrc/rotate_iou.hip), K26b — the same with heights (``rotate_iou_3d``); K27 — KITTI tp / fp / fn of all frames and score thresholds (csrc/kitti_stats.hip).  The three
kernels behind ``kitti_eval`` (KITTI BEV AP) and ``Predictions.boxes``.  K30a — largest 8-connected component of a packed
mask (csrc/mask_components.hip) and K30b — minimum-area rectangle of a packed mask (csrc/min_area_rect.hip), behind
``Predictions.boxes(method='min_area_rect')``.  K29 — pairwise overlap of bit-packed masks and the COCO per-image matching on its integer tables (csrc/mask_map.hip), behind ``metrics.DeviceMaskMeanAveragePrecision``.  K32 — per-frame panoptic tp / fp / fn, IoU sums and confusion of point or BEV
instances (csrc/panoptic.hip), behind ``metrics.DevicePanopticQuality``.
The definitions are in include/maskbev_hip.h."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import MaskBevHipError, check
from .ops_core import _need_gpu, _ptr, _stream, _workspace
from .ops_loss import PackedMasks

Offsets = Union[torch.Tensor, Sequence[int], np.ndarray]


@torch.no_grad()
def fit_boxes(masks: PackedMasks, rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """masks: the R maps at (H, W) of a :class:`PackedMasks`; rows (r) integer device tensor, the maps to fit →
    ``(n (r) int32, moments (r, 5) int64 = Σx Σy Σx² Σy² Σxy, boxes (r, 5) f32 = cx cy dx dy theta)`` in cell units: the
    moment-axis box of ALL set cells (K25); a row with ``n == 0`` gets a box of zeros.  No host synchronisation."""
    lib = _lib.load()
    words = masks.words
    _need_gpu(words, rows)
    h, w = int(masks.h), int(masks.w)
    if h < 1 or w < 1 or h * w > 1024 * 1024:
        raise MaskBevHipError(f'fit_boxes: grid {h}x{w} outside 1 <= H*W <= 1024*1024')
    if words.dim() != 2 or words.dtype != torch.int32 or words.shape[1] != lib.mbv_packed_mask_words(h, w):
        raise MaskBevHipError(f'fit_boxes: words must be (R, {lib.mbv_packed_mask_words(h, w)}) int32 for a {h}x{w} grid')
    if rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64) or rows.device != words.device:
        raise MaskBevHipError('fit_boxes: rows must be a 1-d int32 / int64 tensor on the masks\' device')
    words, rows = words.contiguous(), rows.to(torch.int32).contiguous()
    r, dev = rows.numel(), words.device
    n = torch.empty((r,), dtype=torch.int32, device=dev)
    moments = torch.empty((r, 5), dtype=torch.int64, device=dev)
    boxes = torch.empty((r, 5), dtype=torch.float32, device=dev)
    if r > 0:
        if words.shape[0] == 0:
            raise MaskBevHipError('fit_boxes: rows to fit but no map')
        check(lib.mbv_fit_boxes(_ptr(words), words.shape[0], h, w, _ptr(rows), r, _ptr(n), _ptr(moments), _ptr(boxes),
                                _stream()), 'mbv_fit_boxes')
    return n, moments, boxes


def _packed_and_rows(masks: PackedMasks, rows: torch.Tensor, what: str):
    """The argument checks K30a and K30b share: (lib, contiguous words, int32 rows, h, w)."""
    words = masks.words
    _need_gpu(words, rows)
    lib = _lib.load()
    h, w = int(masks.h), int(masks.w)
    if not (1 <= h <= 1024 and 1 <= w <= 1024):
        raise MaskBevHipError(f'{what}: grid {h}x{w} outside 1 <= H, W <= 1024')
    if words.dim() != 2 or words.dtype != torch.int32 or words.shape[1] != lib.mbv_packed_mask_words(h, w):
        raise MaskBevHipError(f'{what}: words must be (R, {lib.mbv_packed_mask_words(h, w)}) int32 for a {h}x{w} grid')
    if rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64) or rows.device != words.device:
        raise MaskBevHipError(f'{what}: rows must be a 1-d int32 / int64 tensor on the masks\' device')
    if rows.numel() > 0 and words.shape[0] == 0:
        raise MaskBevHipError(f'{what}: rows to do but no map')
    return lib, words.contiguous(), rows.to(torch.int32).contiguous(), h, w


@torch.no_grad()
def largest_component(masks: PackedMasks, rows: torch.Tensor) -> Tuple[PackedMasks, torch.Tensor, torch.Tensor]:
    """masks: the R maps at (H, W) of a :class:`PackedMasks`, H, W <= 1024; rows (r) integer device tensor (any order, repeats;
    a row outside the table counts as an empty map) → ``(kept, n (r) int32, components (r) int32)``: ``kept`` the
    :class:`PackedMasks` of the r listed maps reduced to their largest 8-connected component (K30a: most cells, ties to the
    component holding the lowest raster index), ``n`` its cells, ``components`` how many the map had.  No host
    synchronisation."""
    lib, words, rows, h, w = _packed_and_rows(masks, rows, 'largest_component')
    r, dev = rows.numel(), words.device
    out = torch.empty((r, words.shape[1]), dtype=torch.int32, device=dev)
    n = torch.empty((r,), dtype=torch.int32, device=dev)
    components = torch.empty((r,), dtype=torch.int32, device=dev)
    if r > 0:
        ws = _workspace(lib.mbv_largest_component_workspace_bytes(h, w, r), dev)
        check(lib.mbv_largest_component(_ptr(words), words.shape[0], h, w, _ptr(rows), r, _ptr(out), _ptr(n),
                                        _ptr(components), _ptr(ws), ws.numel(), _stream()), 'mbv_largest_component')
    return PackedMasks(out, h, w), n, components


@torch.no_grad()
def min_area_boxes(masks: PackedMasks, rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """masks, rows as :func:`largest_component` → ``(n (r) int32, hull (r) int32, boxes (r, 5) f32 = cx cy dx dy theta)`` in
    cell units: the minimum-area rectangle of ALL set cells of each listed map (K30b), chosen in exact integer arithmetic
    among the directions of the strictly convex hull's edges; ``hull`` is the hull's vertex count; theta in (-pi/4, pi/4];
    the extents carry K25's unit-cell support, so ``rasterize.boxes_from_cells`` applies.  A row with ``n == 0`` gets a box
    of zeros.  No host synchronisation."""
    lib, words, rows, h, w = _packed_and_rows(masks, rows, 'min_area_boxes')
    r, dev = rows.numel(), words.device
    n = torch.empty((r,), dtype=torch.int32, device=dev)
    hull = torch.empty((r,), dtype=torch.int32, device=dev)
    boxes = torch.empty((r, 5), dtype=torch.float32, device=dev)
    if r > 0:
        check(lib.mbv_min_area_boxes(_ptr(words), words.shape[0], h, w, _ptr(rows), r, _ptr(n), _ptr(hull), _ptr(boxes),
                                     _stream()), 'mbv_min_area_boxes')
    return n, hull, boxes


def _host_offsets(offsets: Offsets, total: int, what: str) -> np.ndarray:
    """Per-frame offsets as a checked host array.  A device tensor is copied back (one synchronisation): pass host
    sequences where the frame sizes are known on the host, as ``kitti_eval`` does."""
    if isinstance(offsets, torch.Tensor):
        offsets = offsets.detach().cpu().numpy()
    host = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if host.size < 2 or host[0] != 0 or host[-1] != total or np.any(np.diff(host) < 0):
        raise ValueError(f'{what}: offsets must ascend from 0 to {total}, got {host.tolist()[:8]} ...')
    if total >= 2 ** 31:
        raise ValueError(f'{what}: more than 2^31 - 1 rows')
    return host


class FrameOffsets:
    """The per-frame offsets of two ragged tables and of their per-frame (n_f, k_f) pair matrices, on the host (``a``, ``b``,
    ``pairs``: int64 arrays of frames + 1 entries) and on the device (``a_dev``, ``b_dev`` int32, ``pairs_dev`` int64)."""

    def __init__(self, a: Offsets, n_a: int, b: Offsets, n_b: int, device):
        self.a, self.b = _host_offsets(a, n_a, 'first table'), _host_offsets(b, n_b, 'second table')
        if self.a.size != self.b.size:
            raise ValueError('the two tables have different numbers of frames')
        self.frames = self.a.size - 1
        self.pairs = np.concatenate([[0], np.cumsum(np.diff(self.a) * np.diff(self.b))]).astype(np.int64)
        self.total = int(self.pairs[-1])
        dev = torch.device(device)
        self.a_dev = torch.from_numpy(self.a.astype(np.int32)).to(dev, non_blocking=True)
        self.b_dev = torch.from_numpy(self.b.astype(np.int32)).to(dev, non_blocking=True)
        self.pairs_dev = torch.from_numpy(self.pairs).to(dev, non_blocking=True)


def _box_table(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 5:
        raise MaskBevHipError(f'{what} must be (N, 5) f32 [x, y, dx, dy, angle], got {tuple(t.shape)} {t.dtype}')
    return t.contiguous()


@torch.no_grad()
def rotate_iou(boxes: torch.Tensor, qboxes: torch.Tensor, box_offsets: Offsets = None, qbox_offsets: Offsets = None,
               criterion: int = -1, offsets: Optional[FrameOffsets] = None) -> Tuple[torch.Tensor, FrameOffsets]:
    """boxes (N, 5), qboxes (K, 5) f32 device tables [x, y, dx, dy, angle] (corners as ``rasterize.box_vertices`` makes
    them: the angle turns counter-clockwise) with per-frame offsets (F + 1; ``None``: one frame) → ``(overlaps, offsets)``:
    the F per-frame (n_f, k_f) matrices concatenated in one f32 device tensor, frame f at ``offsets.pairs[f]``.
    ``criterion``: -1 IoU, 0 intersection over the first box's area, 1 over the second's, 2 the intersection.  One K26 launch;
    no host synchronisation when the offsets are host sequences (or a :class:`FrameOffsets` from an earlier call)."""
    lib = _lib.load()
    _need_gpu(boxes, qboxes)
    boxes, qboxes = _box_table(boxes, 'rotate_iou: boxes'), _box_table(qboxes, 'rotate_iou: qboxes')
    if boxes.device != qboxes.device:
        raise MaskBevHipError('rotate_iou: tables on different devices')
    if criterion not in (-1, 0, 1, 2):
        raise ValueError(f'rotate_iou: criterion must be -1, 0, 1 or 2, got {criterion}')
    n, k, dev = boxes.shape[0], qboxes.shape[0], boxes.device
    if offsets is None:
        offsets = FrameOffsets([0, n] if box_offsets is None else box_offsets, n,
                               [0, k] if qbox_offsets is None else qbox_offsets, k, dev)
    elif offsets.a[-1] != n or offsets.b[-1] != k:
        raise ValueError('rotate_iou: offsets of other tables')
    out = torch.empty((offsets.total,), dtype=torch.float32, device=dev)
    if offsets.total > 0:
        check(lib.mbv_rotate_iou(_ptr(boxes), n, _ptr(qboxes), k, _ptr(offsets.a_dev), _ptr(offsets.b_dev),
                                 _ptr(offsets.pairs_dev), offsets.frames, offsets.total, int(criterion), _ptr(out),
                                 _stream()), 'mbv_rotate_iou')
    return out, offsets


@torch.no_grad()
def rotate_iou_3d(boxes: torch.Tensor, qboxes: torch.Tensor, box_offsets: Offsets = None, qbox_offsets: Offsets = None,
                  criterion: int = -1, offsets: Optional[FrameOffsets] = None) -> Tuple[torch.Tensor, FrameOffsets]:
    """:func:`rotate_iou` for boxes with a height (K26b): boxes (N, 7), qboxes (K, 7) f32 device tables
    [x, y, z, dx, dy, dz, angle] with z the BOTTOM face (``batch.kitti_labels_to_velodyne``'s ``boxes``).  The overlap is the
    BEV intersection times the common z-interval, by ``criterion`` over -1 the union of the volumes, 0 the first box's
    volume, 1 the second's, 2 nothing; exactly 0 where the polygons do not meet or the z-intervals do not overlap.  Offsets,
    output layout and synchronisation as :func:`rotate_iou`."""
    lib = _lib.load()
    _need_gpu(boxes, qboxes)
    for t, what in ((boxes, 'boxes'), (qboxes, 'qboxes')):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 7:
            raise MaskBevHipError(f'rotate_iou_3d: {what} must be (N, 7) f32 [x, y, z, dx, dy, dz, angle], got '
                                  f'{tuple(t.shape)} {t.dtype}')
    boxes, qboxes = boxes.contiguous(), qboxes.contiguous()
    if boxes.device != qboxes.device:
        raise MaskBevHipError('rotate_iou_3d: tables on different devices')
    if criterion not in (-1, 0, 1, 2):
        raise ValueError(f'rotate_iou_3d: criterion must be -1, 0, 1 or 2, got {criterion}')
    n, k, dev = boxes.shape[0], qboxes.shape[0], boxes.device
    if offsets is None:
        offsets = FrameOffsets([0, n] if box_offsets is None else box_offsets, n,
                               [0, k] if qbox_offsets is None else qbox_offsets, k, dev)
    elif offsets.a[-1] != n or offsets.b[-1] != k:
        raise ValueError('rotate_iou_3d: offsets of other tables')
    out = torch.empty((offsets.total,), dtype=torch.float32, device=dev)
    if offsets.total > 0:
        check(lib.mbv_rotate_iou_3d(_ptr(boxes), n, _ptr(qboxes), k, _ptr(offsets.a_dev), _ptr(offsets.b_dev),
                                    _ptr(offsets.pairs_dev), offsets.frames, offsets.total, int(criterion), _ptr(out),
                                    _stream()), 'mbv_rotate_iou_3d')
    return out, offsets


@torch.no_grad()
def kitti_statistics(overlaps: torch.Tensor, offsets: FrameOffsets, ignored_gt: torch.Tensor, ignored_dt: torch.Tensor,
                     dt_scores: torch.Tensor, min_overlap: float, thresholds: Optional[torch.Tensor] = None,
                     compute_fp: bool = True, collect_scores: bool = False):
    """K27 on K26's overlaps with the detections as the FIRST table (``offsets.a``: detections, ``offsets.b``: ground truth):
    ``ignored_gt`` (n_gt) / ``ignored_dt`` (n_dt) int32 codes -1, 0, 1, ``dt_scores`` (n_dt) f32, ``thresholds`` (T) f32
    (``None``: the single threshold 0) → ``stats`` (T, 3) int64 = tp, fp, fn over all frames.  ``collect_scores`` (T = 1,
    the pass in front of ``get_thresholds``) also returns ``(tp_scores (n_gt) f32, tp_flags (n_gt) int32)``: per ground
    truth whether it was matched as a true positive, and by which score.  Device tensors in, device tensors out, no host
    synchronisation."""
    lib = _lib.load()
    _need_gpu(overlaps, ignored_gt, ignored_dt, dt_scores, thresholds)
    dev = overlaps.device
    n_dt, n_gt = int(offsets.a[-1]), int(offsets.b[-1])
    if overlaps.dtype != torch.float32 or overlaps.numel() != offsets.total:
        raise MaskBevHipError(f'kitti_statistics: overlaps must hold {offsets.total} f32 values')
    if (ignored_gt.dtype != torch.int32 or ignored_gt.numel() != n_gt or ignored_dt.dtype != torch.int32
            or ignored_dt.numel() != n_dt or dt_scores.dtype != torch.float32 or dt_scores.numel() != n_dt):
        raise MaskBevHipError(f'kitti_statistics: ignored_gt ({n_gt}) i32, ignored_dt ({n_dt}) i32 and dt_scores ({n_dt}) f32 '
                              'expected')
    if thresholds is None:
        thresholds = torch.zeros((1,), dtype=torch.float32, device=dev)
    if thresholds.dtype != torch.float32 or thresholds.dim() != 1 or not 1 <= thresholds.numel() <= 65535:
        raise MaskBevHipError('kitti_statistics: thresholds must be (T) f32 with 1 <= T <= 65535')
    t = thresholds.numel()
    if collect_scores and t != 1:
        raise ValueError('kitti_statistics: collect_scores needs a single threshold')
    for x in (ignored_gt, ignored_dt, dt_scores, thresholds):
        if x.device != dev:
            raise MaskBevHipError('kitti_statistics: tensors on different devices')
    overlaps, ignored_gt, ignored_dt = overlaps.contiguous(), ignored_gt.contiguous(), ignored_dt.contiguous()
    dt_scores, thresholds = dt_scores.contiguous(), thresholds.contiguous()
    stats = torch.empty((t, 3), dtype=torch.int64, device=dev)
    tp_scores = torch.empty((n_gt,), dtype=torch.float32, device=dev) if collect_scores else None
    tp_flags = torch.empty((n_gt,), dtype=torch.int32, device=dev) if collect_scores else None
    nbytes = lib.mbv_kitti_statistics_workspace_bytes(n_dt, t)
    ws = _workspace(nbytes, dev)
    check(lib.mbv_kitti_statistics(_ptr(overlaps), _ptr(offsets.pairs_dev), _ptr(offsets.a_dev), _ptr(offsets.b_dev),
                                   offsets.frames, n_dt, n_gt, offsets.total, _ptr(ignored_gt), _ptr(ignored_dt),
                                   _ptr(dt_scores), float(min_overlap), _ptr(thresholds), t, int(bool(compute_fp)),
                                   _ptr(stats), _ptr(tp_scores), _ptr(tp_flags), _ptr(ws), ws.numel(), _stream()),
          'mbv_kitti_statistics')
    return (stats, tp_scores, tp_flags) if collect_scores else stats


def _packed_rows(masks: PackedMasks, n: int, what: str) -> int:
    words = masks.words
    if words.dim() != 2 or words.dtype != torch.int32 or not words.is_contiguous():
        raise MaskBevHipError(f'{what}: words must be a contiguous (rows, words) int32 tensor')
    if n < 0 or (n == 0 and words.shape[0] != 0) or (n > 0 and words.shape[0] % n != 0):
        raise MaskBevHipError(f'{what}: {words.shape[0]} maps do not divide into {n} images')
    return words.shape[0] // n if n > 0 else 0


@torch.no_grad()
def pairwise_mask_overlap(pred: PackedMasks, gt: PackedMasks, n: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """pred: the n * Q predicted maps, gt: the n * G ground-truth maps of n images, bit-packed on one grid →
    ``(inter (n, Q, G), pred_area (n, Q), gt_area (n, G))`` int32 popcounts (K29a): exact.  Q, G <= 1024.  No host
    synchronisation."""
    lib = _lib.load()
    _need_gpu(pred.words, gt.words)
    if (int(pred.h), int(pred.w)) != (int(gt.h), int(gt.w)) or pred.words.device != gt.words.device:
        raise MaskBevHipError('pairwise_mask_overlap: the two sets of maps must share grid and device')
    q, g = _packed_rows(pred, n, 'pairwise_mask_overlap: pred'), _packed_rows(gt, n, 'pairwise_mask_overlap: gt')
    nwords = lib.mbv_packed_mask_words(int(pred.h), int(pred.w))
    if pred.words.shape[1] != nwords or gt.words.shape[1] != nwords:
        raise MaskBevHipError(f'pairwise_mask_overlap: {nwords} words per map expected for a {pred.h}x{pred.w} grid')
    dev = pred.words.device
    inter = torch.empty((n, q, g), dtype=torch.int32, device=dev)
    pred_area = torch.empty((n, q), dtype=torch.int32, device=dev)
    gt_area = torch.empty((n, g), dtype=torch.int32, device=dev)
    check(lib.mbv_pairwise_mask_overlap(_ptr(pred.words), _ptr(gt.words), n, q, g, nwords, _ptr(inter), _ptr(pred_area),
                                        _ptr(gt_area), _stream()), 'mbv_pairwise_mask_overlap')
    return inter, pred_area, gt_area


@torch.no_grad()
def coco_match(inter: torch.Tensor, pred_area: torch.Tensor, gt_area: torch.Tensor, scores: torch.Tensor,
               pred_labels: torch.Tensor, gt_labels: torch.Tensor, num_labels: int, iou_thrs: torch.Tensor,
               area_ranges: torch.Tensor, max_det: int):
    """K29b on K29a's tables: ``inter`` (n, Q, G), ``pred_area`` (n, Q), ``gt_area`` (n, G) int32, ``scores`` (n, Q) f32,
    ``pred_labels`` (n, Q) / ``gt_labels`` (n, G) int32, ``iou_thrs`` (T) f64, ``area_ranges`` (A, 2) f64 with T * A <= 64 →
    ``(rank (n, Q) int32, matched (n, Q) int64, ignored (n, Q) int64, npig (n, num_labels, A) int32)``: COCOeval.evaluateImg
    of every (image, class, area range, threshold); bit a * T + t of the two masks.  Device tensors in and out, no host
    synchronisation."""
    lib = _lib.load()
    _need_gpu(inter, pred_area, gt_area, scores, pred_labels, gt_labels, iou_thrs, area_ranges)
    if inter.dim() != 3:
        raise MaskBevHipError(f'coco_match: inter must be (n, Q, G), got {tuple(inter.shape)}')
    n, q, g = inter.shape
    dev = inter.device
    for x, shape, dtype, what in ((inter, (n, q, g), torch.int32, 'inter'), (pred_area, (n, q), torch.int32, 'pred_area'),
                                  (gt_area, (n, g), torch.int32, 'gt_area'), (scores, (n, q), torch.float32, 'scores'),
                                  (pred_labels, (n, q), torch.int32, 'pred_labels'),
                                  (gt_labels, (n, g), torch.int32, 'gt_labels')):
        if tuple(x.shape) != shape or x.dtype != dtype or x.device != dev:
            raise MaskBevHipError(f'coco_match: {what} must be {shape} {dtype} on {dev}, got {tuple(x.shape)} {x.dtype}')
    if iou_thrs.dtype != torch.float64 or iou_thrs.dim() != 1 or area_ranges.dtype != torch.float64 \
            or area_ranges.dim() != 2 or area_ranges.shape[1] != 2 or iou_thrs.device != dev or area_ranges.device != dev:
        raise MaskBevHipError('coco_match: iou_thrs must be (T) f64 and area_ranges (A, 2) f64 on the tables\' device')
    t, a = iou_thrs.numel(), area_ranges.shape[0]
    if t < 1 or a < 1 or t * a > 64 or num_labels < 1 or max_det < 1:
        raise MaskBevHipError(f'coco_match: T = {t}, A = {a} (T * A <= 64), num_labels = {num_labels}, max_det = {max_det}')
    inter, pred_area, gt_area = inter.contiguous(), pred_area.contiguous(), gt_area.contiguous()
    scores, pred_labels, gt_labels = scores.contiguous(), pred_labels.contiguous(), gt_labels.contiguous()
    iou_thrs, area_ranges = iou_thrs.contiguous(), area_ranges.contiguous()
    rank = torch.empty((n, q), dtype=torch.int32, device=dev)
    matched = torch.empty((n, q), dtype=torch.int64, device=dev)
    ignored = torch.empty((n, q), dtype=torch.int64, device=dev)
    npig = torch.empty((n, int(num_labels), a), dtype=torch.int32, device=dev)
    check(lib.mbv_coco_match(_ptr(inter), _ptr(pred_area), _ptr(gt_area), _ptr(scores), _ptr(pred_labels), _ptr(gt_labels),
                             n, q, g, int(num_labels), _ptr(iou_thrs), t, _ptr(area_ranges), a, int(max_det), _ptr(rank),
                             _ptr(matched), _ptr(ignored), _ptr(npig), _stream()), 'mbv_coco_match')
    return rank, matched, ignored, npig


@dataclass
class PanopticFrames:
    """K32's outputs for F frames, P queries and C classes, on the device (include/maskbev_hip.h, K32): ``frame_stats``
    (F, C, 3) int32 = tp, fp, fn; ``frame_iou`` (F, C) f64 — the IoU sums of the true positives; ``confusion`` (F, C, C) int64
    [gt class][prediction class]; ``n_gt`` (F) int32 — the true number of ground-truth segments (a frame with more than
    ``max_gt`` has zeros in ``frame_stats`` and ``frame_iou``); ``gt_key`` (F, max_gt) int32 = class << 16 | instance,
    ascending, -1 past the end; ``gt_area`` (F, max_gt) int32; ``pred_area`` (F, P) int32."""
    frame_stats: torch.Tensor
    frame_iou: torch.Tensor
    confusion: torch.Tensor
    n_gt: torch.Tensor
    gt_key: torch.Tensor
    gt_area: torch.Tensor
    pred_area: torch.Tensor
    max_gt: int


@torch.no_grad()
def panoptic_frames(pred_query: torch.Tensor, gt_words: torch.Tensor, lengths_or_offsets, query_class: torch.Tensor,
                    class_lut: torch.Tensor, num_classes: int, max_gt: int = 256, min_points: int = 50) -> PanopticFrames:
    """K32: ``pred_query`` (N) int32 — per element (point or BEV cell) of the F concatenated frames the query that owns it, -1
    for none; ``gt_words`` (N) int32 / uint32 — the ground truth in the ``.label`` layout (semantic id low, instance id high
    16 bits); ``lengths_or_offsets`` — the frames' element counts (a host sequence of F integers) or their (F + 1) int32
    offsets on the device; ``query_class`` (F, P) int32 — the class of every query (outside 1 .. num_classes - 1: no thing);
    ``class_lut`` (L) int32 device table semantic id → class, -1 = ignored → :class:`PanopticFrames`.  Device tensors only;
    no host synchronisation."""
    lib = _lib.load()
    _need_gpu(pred_query, gt_words, query_class, class_lut)
    dev = pred_query.device
    if pred_query.dim() != 1 or pred_query.dtype != torch.int32:
        raise MaskBevHipError(f'panoptic_frames: pred_query must be (N) int32, got {tuple(pred_query.shape)} {pred_query.dtype}')
    if gt_words.dtype == getattr(torch, 'uint32', None):
        gt_words = gt_words.view(torch.int32)
    if gt_words.dtype != torch.int32 or tuple(gt_words.shape) != tuple(pred_query.shape):
        raise MaskBevHipError(f'panoptic_frames: gt_words must be ({pred_query.numel()}) int32 / uint32, got '
                              f'{tuple(gt_words.shape)} {gt_words.dtype}')
    if query_class.dim() != 2 or query_class.dtype != torch.int32:
        raise MaskBevHipError(f'panoptic_frames: query_class must be (frames, P) int32, got {tuple(query_class.shape)} '
                              f'{query_class.dtype}')
    if class_lut.dim() != 1 or class_lut.dtype != torch.int32:
        raise MaskBevHipError('panoptic_frames: class_lut must be a 1-d int32 table')
    frames, p = int(query_class.shape[0]), int(query_class.shape[1])
    n, c, max_gt, min_points = pred_query.numel(), int(num_classes), int(max_gt), int(min_points)
    if not (1 <= c <= 16 and p <= 1024 and 1 <= max_gt <= 1024 and min_points >= 0 and frames <= 65535 and n < 2 ** 31 - 1):
        raise MaskBevHipError(f'panoptic_frames: num_classes {c} (1 .. 16), P {p} (<= 1024), max_gt {max_gt} (1 .. 1024), '
                              f'min_points {min_points} (>= 0), frames {frames} (<= 65535) or {n} elements out of range')
    if torch.is_tensor(lengths_or_offsets):
        offsets = lengths_or_offsets
        if offsets.dtype != torch.int32 or tuple(offsets.shape) != (frames + 1,) or offsets.device != dev:
            raise MaskBevHipError(f'panoptic_frames: offsets must be ({frames + 1}) int32 on the elements\' device')
    else:
        lens = [int(v) for v in lengths_or_offsets]
        if len(lens) != frames or any(v < 0 for v in lens) or sum(lens) != n:
            raise MaskBevHipError(f'panoptic_frames: {len(lens)} lengths summing to {sum(lens)} for {frames} frames of {n} elements')
        offs = [0]
        for v in lens:
            offs.append(offs[-1] + v)
        offsets = torch.tensor(offs, dtype=torch.int32).to(dev, non_blocking=True)
    for x in (gt_words, query_class, class_lut):
        if x.device != dev:
            raise MaskBevHipError('panoptic_frames: tensors on different devices')
    pred_query, gt_words, offsets = pred_query.contiguous(), gt_words.contiguous(), offsets.contiguous()
    query_class, class_lut = query_class.contiguous(), class_lut.contiguous()
    out = PanopticFrames(torch.empty((frames, c, 3), dtype=torch.int32, device=dev),
                         torch.empty((frames, c), dtype=torch.float64, device=dev),
                         torch.empty((frames, c, c), dtype=torch.int64, device=dev),
                         torch.empty((frames,), dtype=torch.int32, device=dev),
                         torch.empty((frames, max_gt), dtype=torch.int32, device=dev),
                         torch.empty((frames, max_gt), dtype=torch.int32, device=dev),
                         torch.empty((frames, p), dtype=torch.int32, device=dev), max_gt)
    if frames == 0:
        return out
    nbytes = lib.mbv_panoptic_frames_workspace_bytes(frames, p, max_gt, c)
    ws = _workspace(nbytes, dev)
    check(lib.mbv_panoptic_frames(_ptr(pred_query), _ptr(gt_words), n, _ptr(offsets), frames, _ptr(query_class), p,
                                  _ptr(class_lut), class_lut.numel(), c, max_gt, min_points, _ptr(out.frame_stats),
                                  _ptr(out.frame_iou), _ptr(out.confusion), _ptr(out.n_gt), _ptr(out.gt_key),
                                  _ptr(out.gt_area), _ptr(out.pred_area), _ptr(ws), ws.numel(), _stream()),
          'mbv_panoptic_frames')
    return out


__all__ = ['fit_boxes', 'largest_component', 'min_area_boxes', 'rotate_iou', 'rotate_iou_3d', 'kitti_statistics', 'FrameOffsets', 'pairwise_mask_overlap', 'coco_match', 'panoptic_frames', 'PanopticFrames']
