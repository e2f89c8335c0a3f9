"""Inference: scans → instances, eager or replayed from a HIP graph.

The head's last decoder output — class logits (B, Q, K+1) and mask logits (B, Q, ny/4, nx/4) — is turned into instances
on the device by K21 (csrc/instances.hip, ops_instances.py): query selection (first argmax, softmax score, keep =
label > 0 and score >= threshold; SURVEY.md §8a: class 0 = empty) and the BEV masks at the encoder's (ny, nx) grid,
interpolated on the fly with upsample_bilinear2d's align_corners=False arithmetic (set where the logit is > 0, i.e.
sigmoid > 0.5), bit-packed, with areas, mask scores and a per-pixel instance map.  No (B, Q, ny, nx) tensor is made.

:class:`GraphedPredictStep` runs the encoder eagerly (pillar counts are dynamic) into a static input buffer — the same
hand-off as :class:`~mask_bev_amd.graph.GraphedTrainStep` — and replays backbone + head + K21 as one captured graph.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import List, Optional, Tuple

import math

import numpy as np
import torch

from . import ops
from ._lib import MaskBevHipError


BOX_METHODS = ('moment', 'min_area_rect')     # Predictions.boxes: K25 | K30a + K30b


@dataclass
class GroundSettings:
    """What :meth:`Predictions.lift` needs to estimate the ground itself (K35): ``radius_m`` — the half-width of the window a
    cell's ground height is the lowest return of, in metres; ``clearance`` — a point is labelled only above ground +
    clearance; ``max_height`` — and at most that far above it (None: no limit); ``z_floor`` — returns below it are not ground
    candidates (None: no floor).  The defaults rest on geometry, not on measurement: 1.6 m is half a car's width plus slack, so
    the window of a cell under a car reaches the visible road beside it; 0.3 m is above road noise and the 8 cm a window
    minimum loses on a 5 % slope, below a sill."""
    radius_m: float = 1.6
    clearance: float = 0.3
    max_height: Optional[float] = None
    z_floor: Optional[float] = None

    def radius_cells(self, voxel_size_x: float) -> int:
        """``ceil(radius_m / voxel_size_x)``; ``ValueError`` above ``ops.MAX_GROUND_RADIUS`` cells."""
        cells = int(math.ceil(float(self.radius_m) / float(voxel_size_x)))
        if not 0 <= cells <= ops.MAX_GROUND_RADIUS:
            raise ValueError(f'ground radius {self.radius_m} m is {cells} cells of {voxel_size_x} m; the limit is '
                             f'{ops.MAX_GROUND_RADIUS} cells')
        return cells


@dataclass
class ResolveSettings:
    """K42: how the kept queries of one decoder output are reconciled with each other (``extract_instances(...,
    resolve=)``).  Thresholds are integer ratios (num, den) with 1 <= num <= den <= 65535; everything is exact integer
    arithmetic on the device.  ``nms_iou`` — greedy mask NMS: in descending score a surviving query suppresses every later one
    (of its label, with ``same_label``) whose mask IoU with it is >= num / den (None: no NMS);  ``min_overlap`` — Mask2Former's
    overlap filter: after the instance map is rebuilt from the survivors, a query that owns less than num / den of its own mask
    in it is dropped (None: only ``min_cells``);  ``min_cells`` — and one that owns fewer cells than this;  ``exclusive`` —
    ``masks`` and ``areas`` become the cells every query won (disjoint), not its thresholded mask.  1/2 and 4/5 are the
    conventional mask-NMS IoU and Mask2Former's OVERLAP_THRESHOLD; neither is tuned or measured on real data here."""
    nms_iou: Optional[Tuple[int, int]] = (1, 2)
    min_overlap: Optional[Tuple[int, int]] = (4, 5)
    min_cells: int = 1
    same_label: bool = True
    exclusive: bool = False

    def __post_init__(self):
        for name in ('nms_iou', 'min_overlap'):
            r = getattr(self, name)
            if r is None:
                continue
            try:
                num, den = r
                ok = (not isinstance(num, bool) and not isinstance(den, bool) and int(num) == num and int(den) == den
                      and 1 <= int(num) <= int(den) <= 65535)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f'ResolveSettings: {name} must be None or an integer ratio (num, den) with '
                                 f'1 <= num <= den <= 65535, got {r!r}')
            setattr(self, name, (int(num), int(den)))
        mc = self.min_cells
        if isinstance(mc, bool) or not isinstance(mc, (int, np.integer)) or not 0 <= int(mc) < 2 ** 31:
            raise ValueError(f'ResolveSettings: min_cells must be an integer >= 0, got {mc!r}')
        self.min_cells = int(mc)
        self.same_label, self.exclusive = bool(self.same_label), bool(self.exclusive)


def unpack_bits(words: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """Bit-packed maps (N, words) int32 in the mbv_pack_binary_masks layout (pixel y*w + x at bit (y*w + x) % 32 of word
    (y*w + x) // 32) → (N, h, w) bool, on the words' device."""
    n = words.shape[0]
    shifts = torch.arange(32, dtype=torch.int32, device=words.device)
    bits = (words.to(torch.int32).unsqueeze(-1) >> shifts) & 1
    return bits.reshape(n, -1)[:, :h * w].reshape(n, h, w).bool()


@dataclass
class Predictions:
    """K21's outputs for a batch of B scans and Q queries, on the device (or on the host after :meth:`cpu`).

    labels (B, Q) int32 — first argmax of the class logits (0 = empty);  scores (B, Q) f32 — softmax probability of that
    label;  keep (B, Q) bool — label > 0 and score >= the threshold;  masks — :class:`ops.PackedMasks` of the B*Q maps at
    (H, W) (row b*Q + q), or None;  areas (B, Q) int32 — set pixels;  mask_scores (B, Q) f32 — mean sigmoid over the set
    pixels (0 for an empty mask);  instance_map (B, H, W) int32 — per pixel the kept query with a set bit maximising
    score * sigmoid, -1 for none (or None).

    With ``resolve=`` (K42, :class:`ResolveSettings`) ``keep`` is what survived mask NMS and the overlap filter and
    ``instance_map`` the map of those queries alone;  suppressed_by (B, Q) int32 — the surviving query that suppressed this one
    in the NMS, -1 for nobody;  owned (B, Q) int32 — the cells a query won in the map rebuilt after the NMS (0 outside it), also
    for a query the filter then dropped.  Both are None without ``resolve``.  ``masks`` and ``areas`` stay the thresholded
    masks unless ``exclusive``; then they are the cells won (``areas == owned`` on kept queries), while ``mask_scores`` still
    describes the UNRESOLVED masks."""
    labels: torch.Tensor
    scores: torch.Tensor
    keep: torch.Tensor
    masks: Optional[ops.PackedMasks]
    areas: Optional[torch.Tensor]
    mask_scores: Optional[torch.Tensor]
    instance_map: Optional[torch.Tensor]
    grid_hw: Tuple[int, int]
    suppressed_by: Optional[torch.Tensor] = None
    owned: Optional[torch.Tensor] = None

    def _map(self, fn) -> 'Predictions':
        vals = {}
        for f in fields(self):
            v = getattr(self, f.name)
            if isinstance(v, ops.PackedMasks):
                v = ops.PackedMasks(fn(v.words), v.h, v.w)
            elif torch.is_tensor(v):
                v = fn(v)
            vals[f.name] = v
        return Predictions(**vals)

    def clone(self) -> 'Predictions':
        """A copy that the next replay of a :class:`GraphedPredictStep` does not overwrite."""
        return self._map(lambda t: t.clone())

    def cpu(self) -> 'Predictions':
        return self._map(lambda t: t.cpu())

    def instances(self, b: int) -> List[dict]:
        """The kept queries of scan ``b`` in query order: ``{'query', 'label', 'score', 'mask_score', 'area', 'mask'}``,
        ``mask`` the dense (H, W) bool map unpacked on demand (None without masks).  Synchronises with the device."""
        q = self.labels.shape[1]
        idx = torch.nonzero(self.keep[b]).flatten().tolist()
        rows = torch.tensor([b * q + i for i in idx], dtype=torch.long, device=self.labels.device)
        dense = (unpack_bits(self.masks.words.index_select(0, rows.to(self.masks.words.device)), self.masks.h, self.masks.w)
                 if self.masks is not None and idx else None)
        labels, scores = self.labels[b].tolist(), self.scores[b].tolist()
        areas = self.areas[b].tolist() if self.areas is not None else None
        ms = self.mask_scores[b].tolist() if self.mask_scores is not None else None
        out = []
        for j, i in enumerate(idx):
            out.append(dict(query=i, label=labels[i], score=scores[i], mask_score=None if ms is None else ms[i],
                            area=None if areas is None else areas[i], mask=None if dense is None else dense[j]))
        return out

    def _grid_ranges(self, x_range, y_range, voxel_size):
        if y_range is None and hasattr(x_range, 'x_range'):              # a rasteriser (or anything with its attributes)
            r = x_range
            x_range, y_range, voxel_size = r.x_range, r.y_range, r.voxel_size
        if y_range is None or voxel_size is None:
            raise ValueError('boxes: pass x_range, y_range and voxel_size, or a rasteriser')
        h, w = self.masks.h, self.masks.w
        nx, ny = int((x_range[1] - x_range[0]) / voxel_size), int((y_range[1] - y_range[0]) / voxel_size)
        if (ny, nx) != (h, w):
            raise ValueError(f'boxes: the ranges make a {ny}x{nx} (ny, nx) grid, the masks are {h}x{w}')
        return x_range, y_range, nx, ny

    def lift(self, scans, module_or_geometry, z_bins: int = 64, quantiles=(0., 1.), ground=None) -> 'ops.PointInstances':
        """K31, ``ops.lift_instances``: the instance map lifted to the points of ``scans`` — the list of (N_i, 3 | 4) device
        tensors these predictions were made from — with the encoder's voxel geometry (a module, or its ``VoxelGeometry``):
        per point the query that owns its BEV cell (-1: none, and every point the voxeliser drops), and per query the points
        and their z-extent.  No host synchronisation.  On the static outputs of a :class:`GraphedPredictStep` it must run
        before the next replay overwrites ``instance_map``.  ``ground`` (K35): None — every return in an owned cell is labelled,
        road under the car too; an ``ops.GroundMap`` of the same scans — only the returns more than 0.3 m above it are; a
        :class:`GroundSettings` — the map is computed from ``scans`` first (``ops.ground_map``), clearance and height
        limit are the record's.  ``z_ground`` of the result is then set."""
        if self.instance_map is None:
            raise MaskBevHipError('lift: these predictions were made without an instance map')
        geom = voxel_geometry(module_or_geometry)
        extra = {}
        if isinstance(ground, GroundSettings):
            extra = dict(ground=ops.ground_map(scans, geom, ground.radius_cells(geom.voxel_size[0]), z_floor=ground.z_floor),
                         clearance=ground.clearance, max_height=ground.max_height)
        elif ground is not None:
            extra = dict(ground=ground)
        return ops.lift_instances(scans, self.instance_map, geom, self.labels.shape[1], z_bins=z_bins, quantiles=quantiles,
                                  **extra)

    def query_classes(self) -> torch.Tensor:
        """(B, Q) int32, the panoptic class of every query: its label (1 .. K; index 0 of the class logits is "empty", so a
        kept query's label is already a thing class) where ``keep``, else 0.  No host synchronisation."""
        return torch.where(self.keep, self.labels.to(torch.int32), torch.zeros_like(self.labels, dtype=torch.int32))

    def panoptic_points(self, lifted: 'ops.PointInstances', gt_words, metric) -> 'ops.PanopticFrames':
        """Feeds a :class:`~mask_bev_amd.metrics.DevicePanopticQuality` with the lifted point labels of these predictions
        (``lifted``: :meth:`lift` of the scans) against ``gt_words``, the list of the scans' ``.label`` words as (N_i) uint32 /
        int32 device tensors (semantic id low, instance id high 16 bits) in the scans' point order.  K32; returns the
        frames' record.  No host synchronisation."""
        gt_words = list(gt_words)
        if len(gt_words) != len(lifted.lengths) or any(w.dim() != 1 or int(w.shape[0]) != n
                                                       for w, n in zip(gt_words, lifted.lengths)):
            raise MaskBevHipError(f'panoptic_points: one (N_i) tensor of label words per scan expected, of {list(lifted.lengths)} '
                                  f'points, got {[tuple(w.shape) for w in gt_words]}')
        u32 = getattr(torch, 'uint32', None)
        gt_words = [w.view(torch.int32) if w.dtype == u32 else w for w in gt_words]
        words = gt_words[0] if len(gt_words) == 1 else torch.cat(gt_words)
        return metric.update(lifted.point_query, self.query_classes(), words, lifted.scan_offsets)

    def panoptic_bev(self, gt_instance_maps: torch.Tensor, metric, gt_class: int = 1) -> 'ops.PanopticFrames':
        """Feeds a :class:`~mask_bev_amd.metrics.DevicePanopticQuality` with the BEV instance map of these predictions, one
        cell an element: ``gt_instance_maps`` (B, ny, nx) integer device map in the cell layout of ``instance_map``, with the
        ids as ``batch.instance_targets`` reads them — 0 = background, > 0 = an instance (a rasteriser's (B, nx, ny) map:
        ``.permute(0, 2, 1)``); ids keep their low 16 bits.  The words are synthesised on the device: an instance cell
        carries semantic id ``gt_class``, a background cell 0, so the metric's ``class_lut`` must map those two (e.g.
        ``numpy.arange(num_classes)``).  K32; returns the frames' record.  No host synchronisation."""
        if self.instance_map is None:
            raise MaskBevHipError('panoptic_bev: these predictions were made without an instance map')
        m = self.instance_map
        if tuple(gt_instance_maps.shape) != tuple(m.shape) or gt_instance_maps.device != m.device \
                or gt_instance_maps.dtype.is_floating_point:
            raise MaskBevHipError(f'panoptic_bev: an integer ground-truth map {tuple(m.shape)} (B, ny, nx) on the predictions\' '
                                  f'device expected, got {tuple(gt_instance_maps.shape)} {gt_instance_maps.dtype}')
        if not 0 <= int(gt_class) <= 0xffff:
            raise ValueError(f'panoptic_bev: gt_class {gt_class} outside 16 bits')
        ids = gt_instance_maps.to(torch.int64).reshape(-1)
        words = torch.where(ids > 0, ((ids & 0xffff) << 16) | int(gt_class), torch.zeros_like(ids))
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)      # the u32 bits in an int32 tensor
        b, cells = m.shape[0], m.shape[1] * m.shape[2]
        return metric.update(m.reshape(-1).contiguous(), self.query_classes(), words, [cells] * b)

    def visibility(self, scans, module_or_geometry, settings=None) -> torch.Tensor:
        """K38a, ``ops.visibility_map``: the (B, ny, nx) uint8 visibility map of ``scans`` — the scans these predictions were
        made from — in the cell layout of ``instance_map`` (bit 0 PASSED, bit 1 HIT, 0 unknown), with the encoder's voxel
        geometry (a module, or its ``VoxelGeometry``).  ``settings``: a ``tracking.OcclusionSettings`` — its ``origin`` and
        ``z_top``; None takes that record's defaults.  No host synchronisation."""
        from .ops_track import OcclusionSettings
        settings = OcclusionSettings() if settings is None else settings
        return ops.visibility_map(scans, voxel_geometry(module_or_geometry), origin=settings.origin, z_top=settings.z_top)

    def track(self, tracker, poses=None, prev_from_cur=None, visibility=None) -> torch.Tensor:
        """Steps a :class:`~mask_bev_amd.tracking.InstanceTracker` through the B frames of these predictions — CONSECUTIVE
        scans of one sequence, in order — and returns ``query_track`` (B, Q) int32: the global track id of every query, -1
        where the query owns too few cells.  ``poses`` (B, 4, 4) f64 sensor poses, or ``prev_from_cur`` (B, 2, 3) f64.  K33a;
        no host synchronisation.  ``visibility``: :meth:`visibility` of the same scans, for a tracker made with ``occlusion=``
        (K38b)."""
        if self.instance_map is None:
            raise MaskBevHipError('track: these predictions were made without an instance map')
        if visibility is None:
            return tracker.update(self.instance_map, poses=poses, prev_from_cur=prev_from_cur)
        return tracker.update(self.instance_map, poses=poses, prev_from_cur=prev_from_cur, visibility=visibility)

    def fused(self, fusion, query_track: torch.Tensor, poses=None, visibility=None, query_velocity=None):
        """Steps a :class:`~mask_bev_amd.tracking.FootprintFusion` through the B frames of these predictions — CONSECUTIVE
        scans of one sequence, in order — with ``query_track`` (B, Q) of :meth:`track` for the same frames (K39a), and turns
        the fused query map back into masks (K39b).  Returns ``(Predictions, fused_ids)``: the predictions carry
        ``instance_map`` = the fused query per cell and the ``masks`` / ``areas`` of that map, so :meth:`lift`,
        :meth:`boxes`, :meth:`boxes3d`, :meth:`kitti_predictions`, ``panoptic_*``, :meth:`point_tracks` and :meth:`render`
        work on them unchanged; ``labels``, ``scores`` and ``keep`` are these predictions' own, and ``mask_scores`` still
        describes the UNFUSED masks (a remembered cell has no logit).  ``fused_ids`` (B, ny, nx) int32 is the global track id
        per cell; a footprint that is only remembered — its track has no query in the frame — is in ``fused_ids`` alone.
        ``poses`` (B, 4, 4) f64 sensor poses (None: a standing sensor); ``visibility``: :meth:`visibility` of the
        same scans; ``query_velocity`` (B, Q, 2) f64 of a tracker with a motion model.  No host synchronisation."""
        if self.instance_map is None:
            raise MaskBevHipError('fused: these predictions were made without an instance map')
        out = fusion.update(self.instance_map, query_track, poses=poses, visibility=visibility,
                            query_velocity=query_velocity)
        masks, areas = ops.masks_from_map(out.queries, self.labels.shape[1])
        return Predictions(self.labels, self.scores, self.keep, masks, areas, self.mask_scores, out.queries, self.grid_hw), out.ids

    def point_tracks(self, lifted: 'ops.PointInstances', query_track: torch.Tensor) -> torch.Tensor:
        """The global track id of every point: ``query_track`` (B, Q) from :meth:`track`, gathered by K31's ``point_query``
        (``lifted``: :meth:`lift` of the same scans); -1 stays -1.  (N) int32 in the scans' concatenated point order.  No host
        synchronisation."""
        b, q = query_track.shape
        pq = lifted.point_query.long()
        if b != len(lifted.lengths):
            raise MaskBevHipError(f'point_tracks: query_track of {b} frames for {len(lifted.lengths)} lifted scans')
        if q == 0 or pq.numel() == 0:
            return torch.full_like(lifted.point_query, -1)
        # the scan of a point: how many scans end at or before it
        scan = torch.bucketize(torch.arange(pq.numel(), device=pq.device), lifted.scan_offsets[1:].long(), right=True)
        ids = query_track.reshape(-1)[scan.clamp_(max=b - 1) * q + pq.clamp(0, q - 1)]
        return torch.where((pq >= 0) & (pq < q), ids, torch.full_like(ids, -1)).to(torch.int32)

    def render(self, settings=None, scans=None, module=None, query_track=None, gt_maps=None, boxes=None, gt_boxes=None,
               ranges=None) -> torch.Tensor:
        """K36: one BEV frame per scan, ``(B, ny * scale, nx * scale, 3)`` uint8 on the device, composed there by
        ``ops.render_bev`` in one launch; ``settings``: a :class:`~mask_bev_amd.render.RenderSettings` (None: its defaults).
        Always: the instance map, every owned cell blended with its query's palette colour.  ``scans`` (with ``module``, or its
        ``VoxelGeometry``): underneath, the returns per cell on a logarithmic grey scale (K36a, ``ops.cell_counts``).
        ``query_track`` (B, Q) int32 of :meth:`track`: colours by global track id, so an object keeps its colour over a
        sequence; a query without a track is grey.  ``gt_maps`` (B, ny, nx) integer map in the layout of ``instance_map`` (a
        rasteriser's (B, nx, ny) map: ``.permute(0, 2, 1)``): a one-pixel contour around every ground-truth instance.
        ``gt_boxes``: per scan an (n, 7) array of label boxes [x, y, z, l, w, h, yaw] in the velodyne frame, outlined in a
        second colour; ``boxes='pred'``: the outlines of :meth:`boxes` on top — both need ``ranges`` = (x_range, y_range
        [, voxel_size]) or a rasteriser.  No host synchronisation, except with ``boxes='pred'``, which costs the two of
        :meth:`boxes` and is off by default.  ``mask_bev_amd.render.write_png`` writes a frame (``image[b]``) without PIL.
        Raises ``MaskBevHipError`` for predictions made without an instance map."""
        from .render import render_predictions
        return render_predictions(self, settings, scans=scans, module=module, query_track=query_track, gt_maps=gt_maps,
                                  boxes=boxes, gt_boxes=gt_boxes, ranges=ranges)

    def boxes(self, x_range, y_range=None, voxel_size=None, method: str = 'moment') -> dict:
        """Oriented BEV boxes of the kept queries, in metres: ``x_range``, ``y_range``, ``voxel_size`` of the grid, or a
        rasteriser (``KittiRasterizer``) in place of ``x_range``.  ``method='moment'``: K25, ``ops.fit_boxes``, the
        moment-axis box of all set cells of a mask.  ``method='min_area_rect'``: K30a then K30b, ``ops.largest_component`` and
        ``ops.min_area_boxes``, the minimum-area rectangle of the mask's largest 8-connected component (what the reference's
        ``mask_to_pred`` asks of OpenCV; stray cells do not stretch the box).  A kept query whose mask is empty yields no box.
        Returns, for the R remaining rows in (scan, query) order, ``boxes`` (R, 5) f32 [x, y, l, w, yaw] (velodyne frame, the
        yaw of ``rasterize.box_vertices``, l >= w), ``scores`` (R) f32, ``scan`` (R) and ``query`` (R) int64, ``cells`` (R)
        int32 (``min_area_rect``: the cells of the kept component) — tensors where the predictions live.
        Synchronises with the device (twice, whatever the method: the kept rows, then the non-empty ones)."""
        return self._boxes(x_range, y_range, voxel_size, method)[0]

    def _boxes(self, x_range, y_range, voxel_size, method, also=None):
        """:meth:`boxes`; ``also`` (B * Q) bool on the device: a second condition on the rows that remain, folded into the
        second synchronisation.  Returns (the dictionary, the remaining rows b * Q + q)."""
        from .rasterize import boxes_from_cells
        if method not in BOX_METHODS:
            raise ValueError(f'boxes: method must be one of {BOX_METHODS}, got {method!r}')
        if self.masks is None:
            raise MaskBevHipError('boxes: these predictions were made without masks')
        x_range, y_range, nx, ny = self._grid_ranges(x_range, y_range, voxel_size)
        q = self.labels.shape[1]
        rows = torch.nonzero(self.keep.reshape(-1)).flatten()
        if method == 'moment':
            n, _, cell_boxes = ops.fit_boxes(self.masks, rows.to(self.masks.words.device))
        else:
            kept, _, _ = ops.largest_component(self.masks, rows.to(self.masks.words.device))
            n, _, cell_boxes = ops.min_area_boxes(kept, torch.arange(rows.numel(), dtype=torch.int32, device=kept.words.device))
        full = torch.nonzero(n > 0 if also is None else (n > 0) & also[rows].to(n.device)).flatten()
        rows, n, cell_boxes = rows[full.to(rows.device)], n[full], cell_boxes[full]
        return dict(boxes=boxes_from_cells(cell_boxes, x_range, y_range, nx, ny), scores=self.scores.reshape(-1)[rows],
                    scan=torch.div(rows, q, rounding_mode='floor'), query=rows % q, cells=n), rows

    def boxes3d(self, scans, module_or_geometry, x_range, y_range=None, voxel_size=None, method: str = 'moment',
                extent='minmax', min_points: int = 1, ground=None, bottom: str = 'points') -> dict:
        """:meth:`boxes` with a height from the points (K31, :meth:`lift` of ``scans`` with the encoder's geometry): what
        :meth:`boxes` returns plus ``boxes3d`` (R, 7) f32 [x, y, z_bottom, l, w, h, yaw] — the columns of
        ``batch.kitti_labels_to_velodyne``'s ``boxes`` — and ``points`` (R) int32, the lifted points of the row's query.
        ``extent='minmax'``: z_bottom and h from the lowest and the highest point whose BEV cell the query owns;
        ``extent=(q_lo, q_hi)``: from the edges of the bins, among 64 over the geometry's z range, that hold the points
        of those two quantiles (an outlier above a car no longer stretches it).  Rows with fewer than ``min_points`` (>= 1)
        lifted points are dropped: a mask with no return has no height.  The height is the z-extent of the returns inside the
        mask — ground to roof only if the ground is in range.  ``ground`` (K35, as in :meth:`lift`): only the returns above the
        estimated ground count, so z_bottom is the lowest kept return; with ``bottom='ground'`` (needs ``ground``) z_bottom is
        ``z_ground``, the estimated ground under the object, and h reaches from there to the top: the box stands on the
        ground as a KITTI label does.  No synchronisation beyond the two of :meth:`boxes`."""
        if bottom not in ('points', 'ground'):
            raise ValueError(f"boxes3d: bottom must be 'points' or 'ground', got {bottom!r}")
        if bottom == 'ground' and ground is None:
            raise ValueError("boxes3d: bottom='ground' needs ground= (a GroundMap or GroundSettings)")
        if int(min_points) < 1:
            raise ValueError('boxes3d: min_points must be at least 1 (a mask with no return has no height)')
        if isinstance(extent, str):
            if extent != 'minmax':
                raise ValueError(f"boxes3d: extent must be 'minmax' or (q_lo, q_hi), got {extent!r}")
            quantiles = (0., 1.)
        else:
            quantiles = (float(extent[0]), float(extent[1]))
        if self.masks is None:
            raise MaskBevHipError('boxes: these predictions were made without masks')
        lifted = self.lift(scans, module_or_geometry, quantiles=quantiles, **({} if ground is None else dict(ground=ground)))
        counts = lifted.counts.reshape(-1)
        out, rows = self._boxes(x_range, y_range, voxel_size, method, also=counts >= int(min_points))
        rows = rows.to(counts.device)
        lo, hi = (lifted.z_min, lifted.z_max) if isinstance(extent, str) else (lifted.z_lo, lifted.z_hi)
        if bottom == 'ground':
            lo = lifted.z_ground
        z, top = lo.reshape(-1)[rows], hi.reshape(-1)[rows]
        b = out['boxes']
        z, top = z.to(b.device), top.to(b.device)
        out['boxes3d'] = torch.stack([b[:, 0], b[:, 1], z, b[:, 2], b[:, 3], top - z, b[:, 4]], dim=1)
        out['points'] = counts[rows]
        return out

    def kitti_predictions(self, x_range, y_range=None, voxel_size=None, method: str = 'moment', scans=None, module=None,
                          extent='minmax', min_points: int = 1, ground=None, bottom: str = 'points') -> List[dict]:
        """Per scan what ``kitti_eval.eval_kitti`` takes: ``{'boxes': (k, 5) [x, y, l, w, yaw], 'score': (k), 'type': (k)
        int64}`` of the scan's kept, non-empty queries; every box has the type Car (index 0 of ``rasterize.KITTI_TYPES``).
        With ``scans`` (and ``module``, or its ``VoxelGeometry``) every dictionary also carries ``boxes3d`` (k, 7) of
        :meth:`boxes3d` (``extent``, ``min_points``, ``ground``, ``bottom`` as there) and ``boxes`` are its BEV columns: the 3D lines of the
        evaluation.  Arguments and synchronisation as :meth:`boxes`, plus one copy of the per-scan counts."""
        if scans is None:
            if ground is not None or bottom != 'points':
                raise ValueError('kitti_predictions: ground and bottom apply to the 3D boxes, which need scans')
            out = self.boxes(x_range, y_range, voxel_size, method=method)
        else:
            if module is None:
                raise ValueError('kitti_predictions: scans need the module (or its VoxelGeometry) they were voxelised with')
            out = self.boxes3d(scans, module, x_range, y_range, voxel_size, method=method, extent=extent,
                               min_points=min_points, ground=ground, bottom=bottom)
        counts = torch.bincount(out['scan'], minlength=self.labels.shape[0]).tolist()
        boxes, scores = torch.split(out['boxes'], counts), torch.split(out['scores'], counts)
        dicts = [dict(boxes=b, score=s, type=torch.zeros((b.shape[0],), dtype=torch.int64)) for b, s in zip(boxes, scores)]
        if scans is not None:
            for d, b3 in zip(dicts, torch.split(out['boxes3d'], counts)):
                d['boxes3d'] = b3
        return dicts


def voxel_geometry(module_or_geometry):
    """The encoder's ``VoxelGeometry`` of a module (or of its encoder), or the geometry itself."""
    g = module_or_geometry
    for name in ('_encoder', '_voxel_layer', 'geometry'):
        g = getattr(g, name, g)
    if not (hasattr(g, 'pc_range') and hasattr(g, 'voxel_size') and hasattr(g, 'grid')):
        raise MaskBevHipError('a MaskBevModule, its encoder or a VoxelGeometry is expected')
    return g


def write_semantic_kitti_labels(path, point_query, semantic_id: int = 10, instance_ids=None) -> None:
    """A SemanticKITTI ``.label`` file of one scan from its per-point queries (``PointInstances.per_scan()``; a tensor
    anywhere, or an array): ``uint32`` per point, the instance id ``query + 1`` in the upper 16 bits and ``semantic_id``
    (default 10, car) in the lower 16; 0 for an unlabelled point (query -1).  With ``instance_ids`` — per point the global
    track id of ``Predictions.point_tracks``, -1 = unlabelled — the instance id is ``id + 1`` instead, the same for an object
    in every scan of a sequence; an id above 65534 raises ``ValueError``.  ``batch.read_semantic_kitti_label`` reads the file
    back as (semantic, instance).  Copies a device tensor to the host."""
    q = point_query.detach().cpu().numpy() if torch.is_tensor(point_query) else np.asarray(point_query)
    q = q.astype(np.int64).reshape(-1)
    if not 0 <= int(semantic_id) <= 0xffff:
        raise ValueError(f'write_semantic_kitti_labels: semantic_id {semantic_id} outside 16 bits')
    if instance_ids is not None:
        ids = instance_ids.detach().cpu().numpy() if torch.is_tensor(instance_ids) else np.asarray(instance_ids)
        ids = ids.astype(np.int64).reshape(-1)
        if ids.shape != q.shape:
            raise ValueError(f'write_semantic_kitti_labels: {ids.size} instance ids for {q.size} points')
        if ids.size and (ids.min() < -1 or ids.max() > 0xfffe):
            raise ValueError('write_semantic_kitti_labels: instance ids must lie in -1 .. 65534 (the instance id has 16 bits)')
        q = ids
    if q.size and (q.min() < -1 or q.max() > 0xfffe):
        raise ValueError('write_semantic_kitti_labels: queries must lie in -1 .. 65534 (the instance id has 16 bits)')
    out = np.where(q >= 0, ((q + 1) << 16) | int(semantic_id), 0).astype('<u4')
    out.tofile(str(path))


def _resolve_settings(resolve, masks: bool, instance_map: bool) -> Optional[ResolveSettings]:
    if resolve is None:
        return None
    if not isinstance(resolve, ResolveSettings):
        raise TypeError(f'resolve must be a ResolveSettings or None, got {type(resolve).__name__}')
    if not (masks and instance_map):
        raise ValueError('resolve needs masks=True and instance_map=True: the rule reads the masks and rebuilds the map')
    return resolve


def extract_instances(cls: torch.Tensor, mask_logits: torch.Tensor, grid_hw, score_threshold: float = 0.0,
                      masks: bool = True, instance_map: bool = True, resolve: Optional[ResolveSettings] = None) -> Predictions:
    """K21a + K21b on one decoder output: cls (B, Q, K+1) f32 / bf16 / fp16 and mask_logits (B, Q, h, w) f32 on the device,
    grid_hw = (H, W) the BEV grid.  ``masks=False`` skips the packed masks, areas and mask scores; ``instance_map=False``
    the map.  Device tensors only (a CPU tensor raises MaskBevHipError).

    ``resolve`` (K42, a :class:`ResolveSettings`; needs both flags): K21b's first pass makes masks, areas and mask scores only;
    K42a + K42b suppress duplicates among the kept queries; a second K21b pass over the survivors makes the instance map; K42c
    drops the queries that own too little of their mask in it and clears their cells; with ``exclusive`` K39b turns the map
    back into masks.  No host synchronisation; all of it can be captured in a graph."""
    ops._need_gpu(cls, mask_logits)
    if cls.dim() != 3 or mask_logits.dim() != 4 or tuple(cls.shape[:2]) != tuple(mask_logits.shape[:2]):
        raise MaskBevHipError(f'extract_instances: cls (B, Q, K+1) and mask logits (B, Q, h, w) expected, got '
                              f'{tuple(cls.shape)} and {tuple(mask_logits.shape)}')
    resolve = _resolve_settings(resolve, masks, instance_map)
    grid = (int(grid_hw[0]), int(grid_hw[1]))
    labels, scores, keep = ops.select_queries(cls, score_threshold)
    if resolve is None:
        out = ops.extract_masks(mask_logits, scores, keep, grid_hw, masks=masks, instance_map=instance_map)
        return Predictions(labels, scores, keep, out['masks'], out['areas'], out['mask_scores'], out['instance_map'], grid)
    out = ops.extract_masks(mask_logits, scores, keep, grid_hw, masks=True, instance_map=False)
    pm, areas = out['masks'], out['areas']
    if resolve.nms_iou is not None:
        inter = ops.mask_self_overlap(pm, keep)
        keep, suppressed_by = ops.mask_nms(inter, scores, labels, keep, resolve.nms_iou, resolve.same_label)
    else:
        suppressed_by = torch.full_like(labels, -1, dtype=torch.int32)
    imap = ops.extract_masks(mask_logits, scores, keep, grid_hw, masks=False, instance_map=True)['instance_map']
    keep, owned = ops.overlap_filter(imap, areas, keep, resolve.min_overlap, resolve.min_cells)
    if resolve.exclusive:
        pm, areas = ops.masks_from_map(imap, int(labels.shape[1]))
    return Predictions(labels, scores, keep, pm, areas, out['mask_scores'], imap, grid, suppressed_by, owned)


def grid_hw(module) -> Tuple[int, int]:
    """The module's BEV grid (ny, nx): the size of the encoder's pseudo-image and of the ground-truth masks."""
    enc = module._encoder
    return enc._num_voxel_y, enc._num_voxel_x


class _EvalMode:
    """Eval mode (the voxeliser's test-time max_voxels, the PFN's running statistics) for the duration, then the previous
    mode back."""

    def __init__(self, module):
        self.m = module

    def __enter__(self):
        self.was = self.m.training
        self.m.train(False)

    def __exit__(self, *exc):
        self.m.train(self.was)
        return False


def predict(module, scans, score_threshold: float = 0.0, masks: bool = True, instance_map: bool = True,
            resolve: Optional[ResolveSettings] = None) -> Predictions:
    """Eager inference on a list of (N_i, pc_dim) device scans: forward in eval mode under no_grad, K21 on the last
    decoder output (MaskBevModule.predict); ``resolve``: K42, as in :func:`extract_instances`."""
    resolve = _resolve_settings(resolve, masks, instance_map)
    with _EvalMode(module), torch.no_grad():
        cls, mk, _ = module(scans)
        return extract_instances(cls[-1], mk[-1], grid_hw(module), score_threshold, masks, instance_map, resolve)


class GraphedPredictStep:
    """``step(scans) -> Predictions`` with backbone + head + K21 (and, with ``resolve=``, K42: every stage of
    :func:`extract_instances` inside the graph) replayed from one HIP graph.

    The encoder runs eagerly in eval mode and writes into the graph's static input (the 16-bit patch rows of
    ``module._patch_handoff()``, or the f32 map with its registered absmax record in fp32 compute).  The returned
    :class:`Predictions` are the graph's static outputs: the NEXT replay overwrites them (``.clone()`` to keep them).
    The lift to the points (``Predictions.lift``, ``boxes3d``) is not part of the graph: it runs eagerly on the step's
    ``Predictions`` and the same ``scans``, and must run before the next replay overwrites ``instance_map``.
    The batch size is fixed at construction.  Weights are read at replay time, so in-place parameter updates (optimizer
    steps on the parameters or on a parameter arena and its 16-bit shadow) are followed; the decoder's weight copies are
    refreshed by a launch inside the graph.  May live beside a :class:`~mask_bev_amd.graph.GraphedTrainStep` (validation
    during training).  Construct it before any eager backward on the default stream, like the training graph."""

    def __init__(self, module, example_scans, score_threshold: float = 0.0, masks: bool = True,
                 instance_map: bool = True, warmup_iters: int = 2, resolve: Optional[ResolveSettings] = None):
        m = self.m = module
        self.batch = len(example_scans)
        self.score_threshold = float(score_threshold)
        self._flags = (masks, instance_map, _resolve_settings(resolve, masks, instance_map))
        self._grid = grid_hw(m)
        dev = example_scans[0].device
        with _EvalMode(m), torch.no_grad():
            self._patch = m._patch_handoff()
            with m._autocast():
                x = m._encoder(example_scans, patch=self._patch)
            rows = x.rows if isinstance(x, ops.PatchTokens) else x
            self.x_static = torch.zeros_like(rows)
            self._x_in = (ops.PatchTokens(self.x_static, x.channels, x.patch) if isinstance(x, ops.PatchTokens)
                          else self.x_static)
            static_rec = None
            if not isinstance(x, ops.PatchTokens) and self.x_static.dtype == torch.float32 and ops.static_amax_wanted():
                # fp32 compute: K3 leaves the map's absmax record at a fixed address for the captured patch projection
                static_rec = ops.static_amax_register(self.x_static)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.x_static.copy_(rows)
                if static_rec is not None:
                    static_rec.copy_(ops.f32_absmax([self.x_static.view(-1, self.x_static.shape[-1])]))
                for _ in range(warmup_iters):
                    self._forward()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            ops.amax_new_capture()        # records made inside an earlier capture (a training graph) are not this graph's
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = self._forward()
            torch.cuda.synchronize()

    def _forward(self) -> Predictions:
        m = self.m
        dt = m._compute_dtype
        with torch.autocast('cuda', dtype=dt or torch.bfloat16, enabled=dt is not None, cache_enabled=False):
            feats = m._backbone(self._x_in)
            cls, mk, _ = m._panoptic_head(feats)
        return extract_instances(cls[-1], mk[-1], self._grid, self.score_threshold, *self._flags)

    def step(self, scans) -> Predictions:
        if self.graph is None:
            raise MaskBevHipError('GraphedPredictStep: closed')
        if len(scans) != self.batch:
            raise MaskBevHipError(f'GraphedPredictStep: captured for {self.batch} scans, got {len(scans)}')
        m = self.m
        with _EvalMode(m), torch.no_grad():
            with m._autocast():                        # eager: K1 → K2 → K3 into the static buffer
                m._encoder(scans, patch=self._patch, out=self.x_static)
            self.graph.replay()
        return self.out

    __call__ = step

    def close(self):
        """Release the graph and its memory pool (the returned Predictions die with it)."""
        self.graph = None
        self.out = None
        self._x_in = None
        self.x_static = None
