"""K21 — instance extraction at inference (csrc/instances.hip): query selection from the class logits and the BEV masks,
areas, mask scores and instance map of one decoder output, straight from the (h, w) logits with no (B, Q, H, W)
intermediate.  K31 — the lift of that instance map to the points of the scans (csrc/point_lift.hip): per-point query labels,
points per query and their z-extent.  K35 — a ground height per BEV cell from the scans themselves and the lift restricted to the
returns above it (same file).  K42 — the kept queries reconciled with each other (csrc/resolve.hip): the pairwise overlap of the
kept masks, greedy mask NMS and Mask2Former's overlap filter on the instance map.  Class convention: index 0 = empty, > 0 = object; a pixel is set when its interpolated
logit is > 0 (sigmoid > 0.5)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import MaskBevHipError, check
from .ops_core import _dt_flag, _need_gpu, _ptr, _stream, _workspace
from .ops_loss import PackedMasks


@torch.no_grad()
def select_queries(cls: torch.Tensor, score_threshold: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """cls (B, Q, K+1) f32 / bf16 / fp16, K+1 <= 256 → labels (B, Q) int32 (first argmax), scores (B, Q) f32
    (softmax[label]), keep (B, Q) bool (label > 0 and score >= score_threshold).  One K21a launch."""
    lib = _lib.load()
    _need_gpu(cls)
    if cls.dim() != 3:
        raise MaskBevHipError(f'select_queries: cls must be (B, Q, K+1), got {tuple(cls.shape)}')
    b, q, k = cls.shape
    if not 0 < k <= 256:
        raise MaskBevHipError(f'select_queries: 1 <= K+1 <= 256 classes, got {k}')
    cls = cls.contiguous()
    dev = cls.device
    labels = torch.empty((b, q), dtype=torch.int32, device=dev)
    scores = torch.empty((b, q), dtype=torch.float32, device=dev)
    keep = torch.empty((b, q), dtype=torch.bool, device=dev)
    check(lib.mbv_select_queries(_ptr(cls), _dt_flag(cls.dtype), b * q, k, float(score_threshold), _ptr(labels),
                                 _ptr(scores), _ptr(keep), _stream()), 'mbv_select_queries')
    return labels, scores, keep


@torch.no_grad()
def extract_masks(logits: torch.Tensor, scores: torch.Tensor, keep: torch.Tensor, grid_hw, masks: bool = True,
                  instance_map: bool = True) -> Dict[str, Optional[object]]:
    """logits (B, Q, h, w) f32, scores (B, Q) f32 and keep (B, Q) bool of :func:`select_queries` → a dict with
    ``masks`` (:class:`PackedMasks` of the B*Q maps at grid_hw = (H, W)), ``areas`` (B, Q) int32, ``mask_scores`` (B, Q)
    f32 (mean sigmoid over the set pixels, 0 when empty) — all three None when ``masks`` is False — and ``instance_map``
    (B, H, W) int32 (best kept query by score * sigmoid, -1 for none; None when ``instance_map`` is False).  K21b + its
    fixed-order reduction; deterministic."""
    lib = _lib.load()
    _need_gpu(logits, scores, keep)
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise MaskBevHipError(f'extract_masks: logits must be (B, Q, h, w) f32, got {tuple(logits.shape)} {logits.dtype}')
    b, q, h, w = logits.shape
    H, W = int(grid_hw[0]), int(grid_hw[1])
    if H <= 0 or W <= 0 or H * W > 1024 * 1024:
        raise MaskBevHipError(f'extract_masks: BEV grid {H}x{W} outside 1 <= H*W <= 1024*1024')
    if (tuple(scores.shape) != (b, q) or scores.dtype != torch.float32 or tuple(keep.shape) != (b, q)
            or keep.dtype != torch.bool):
        raise MaskBevHipError('extract_masks: scores must be (B, Q) f32 and keep (B, Q) bool')
    if not (scores.device == keep.device == logits.device):
        raise MaskBevHipError('extract_masks: tensors on different devices')
    dev = logits.device
    logits, scores, keep = logits.contiguous(), scores.contiguous(), keep.contiguous()
    words = torch.empty((b * q, lib.mbv_packed_mask_words(H, W)), dtype=torch.int32, device=dev) if masks else None
    areas = torch.empty((b, q), dtype=torch.int32, device=dev) if masks else None
    mscores = torch.empty((b, q), dtype=torch.float32, device=dev) if masks else None
    imap = torch.empty((b, H, W), dtype=torch.int32, device=dev) if instance_map else None
    ws = None
    nbytes = 0
    if masks and b * q > 0:
        nbytes = lib.mbv_extract_masks_workspace_bytes(b, q, h, w, H, W)
        if nbytes == 0:
            raise MaskBevHipError(f'extract_masks: {h}x{w} logits on a {H}x{W} grid are not supported')
        ws = _workspace(nbytes, dev)
    check(lib.mbv_extract_masks(_ptr(logits), _ptr(scores), _ptr(keep), b, q, h, w, H, W, _ptr(words), _ptr(areas),
                                _ptr(mscores), _ptr(imap), _ptr(ws), nbytes if ws is not None else 0, _stream()),
          'mbv_extract_masks')
    return dict(masks=PackedMasks(words, H, W) if masks else None, areas=areas, mask_scores=mscores, instance_map=imap)


def _ratio(what: str, ratio, num_min: int = 1) -> Tuple[int, int]:
    """An integer ratio (num, den) with num_min <= num <= den <= 65535, or MaskBevHipError."""
    try:
        num, den = ratio
        ok = int(num) == num and int(den) == den and num_min <= int(num) <= int(den) <= 65535 and int(den) >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise MaskBevHipError(f'{what}: an integer ratio (num, den) with {num_min} <= num <= den <= 65535 expected, got {ratio!r}')
    return int(num), int(den)


def _frame_table(what: str, name: str, t: torch.Tensor, shape, dtype, dev) -> torch.Tensor:
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev:
        raise MaskBevHipError(f'{what}: {name} must be {tuple(shape)} {dtype} on {dev}, got '
                              f'{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} {getattr(t, "dtype", "")}')
    return t.contiguous()


@torch.no_grad()
def mask_self_overlap(masks: PackedMasks, keep: torch.Tensor) -> torch.Tensor:
    """K42a: ``masks`` — the B * Q packed maps of :func:`extract_masks` (row b * Q + q), ``keep`` (B, Q) bool → ``inter``
    (B, Q, Q) int32: the popcount of row i AND row j where both are kept (the diagonal: a kept mask's area), 0 wherever either is
    not.  Only kept rows are read, every unordered pair once.  Q <= 1024.  Exact; no host synchronisation."""
    lib = _lib.load()
    _need_gpu(masks.words, keep)
    words = masks.words
    if keep.dim() != 2 or keep.dtype != torch.bool or keep.device != words.device:
        raise MaskBevHipError(f'mask_self_overlap: keep must be (B, Q) bool on the masks\' device, got {tuple(keep.shape)} '
                              f'{keep.dtype}')
    b, q = (int(v) for v in keep.shape)
    nwords = lib.mbv_packed_mask_words(int(masks.h), int(masks.w))
    if words.dim() != 2 or words.dtype != torch.int32 or not words.is_contiguous() or tuple(words.shape) != (b * q, nwords):
        raise MaskBevHipError(f'mask_self_overlap: words must be a contiguous ({b * q}, {nwords}) int32 tensor for {b} x {q} '
                              f'maps on a {masks.h}x{masks.w} grid, got {tuple(words.shape)} {words.dtype}')
    if q > 1024 or b > 65535 or nwords > 32768:
        raise MaskBevHipError(f'mask_self_overlap: Q {q} <= 1024, B {b} <= 65535 or H * W <= 2^20 violated')
    keep = keep.contiguous()
    inter = torch.empty((b, q, q), dtype=torch.int32, device=words.device)
    check(lib.mbv_mask_self_overlap(_ptr(words), _ptr(keep), b, q, nwords, _ptr(inter), _stream()), 'mbv_mask_self_overlap')
    return inter


@torch.no_grad()
def mask_nms(inter: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, keep: torch.Tensor, iou=(1, 2),
             same_label: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """K42b, greedy mask NMS: ``inter`` (B, Q, Q) int32 of :func:`mask_self_overlap`, ``scores`` (B, Q) f32, ``labels`` (B, Q)
    int32 and ``keep`` (B, Q) bool of :func:`select_queries`; ``iou`` = (num, den).  The kept queries in descending score (ties:
    the smaller q first); a survivor i suppresses every later, not yet suppressed j (of its label, with ``same_label``) with
    ``inter * den >= num * union`` and ``union > 0`` — equality suppresses, a suppressed query suppresses nobody.  Returns
    ``(keep (B, Q) bool, suppressed_by (B, Q) int32)``, -1 where nobody did.  Exact integers; no host synchronisation."""
    lib = _lib.load()
    _need_gpu(inter, scores, labels, keep)
    if keep.dim() != 2:
        raise MaskBevHipError(f'mask_nms: keep must be (B, Q) bool, got {tuple(keep.shape)}')
    b, q = (int(v) for v in keep.shape)
    dev = keep.device
    num, den = _ratio('mask_nms: iou', iou)
    keep = _frame_table('mask_nms', 'keep', keep, (b, q), torch.bool, dev)
    inter = _frame_table('mask_nms', 'inter', inter, (b, q, q), torch.int32, dev)
    scores = _frame_table('mask_nms', 'scores', scores, (b, q), torch.float32, dev)
    labels = _frame_table('mask_nms', 'labels', labels, (b, q), torch.int32, dev)
    if q > 1024 or b > 65535:
        raise MaskBevHipError(f'mask_nms: Q {q} <= 1024 or B {b} <= 65535 violated')
    keep_out = torch.empty((b, q), dtype=torch.bool, device=dev)
    suppressed_by = torch.empty((b, q), dtype=torch.int32, device=dev)
    check(lib.mbv_mask_nms(_ptr(inter), _ptr(scores), _ptr(labels), _ptr(keep), b, q, num, den, 1 if same_label else 0,
                           _ptr(keep_out), _ptr(suppressed_by), _stream()), 'mbv_mask_nms')
    return keep_out, suppressed_by


@torch.no_grad()
def overlap_filter(instance_map: torch.Tensor, areas: torch.Tensor, keep: torch.Tensor, min_overlap=(4, 5),
                   min_cells: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """K42c, Mask2Former's overlap filter: ``instance_map`` (B, H, W) int32 contiguous — CHANGED IN PLACE —, ``areas`` (B, Q)
    int32 and ``keep`` (B, Q) bool.  ``owned[q]`` = cells of the map equal to q (0 for q outside ``keep``); a kept q is dropped
    iff ``owned < min_cells`` or ``owned * den < num * area`` (``min_overlap`` = (num, den); None: the first test only).  One
    pass; the cells of every query that is not kept afterwards become -1.  Returns ``(keep (B, Q) bool, owned (B, Q) int32)``.
    Exact integers; no host synchronisation."""
    lib = _lib.load()
    _need_gpu(instance_map, areas, keep)
    if keep.dim() != 2:
        raise MaskBevHipError(f'overlap_filter: keep must be (B, Q) bool, got {tuple(keep.shape)}')
    b, q = (int(v) for v in keep.shape)
    dev = keep.device
    num, den = (0, 1) if min_overlap is None else _ratio('overlap_filter: min_overlap', min_overlap)
    if int(min_cells) != min_cells or not 0 <= int(min_cells) < 2 ** 31:
        raise MaskBevHipError(f'overlap_filter: min_cells must be an integer >= 0, got {min_cells!r}')
    if (instance_map.dim() != 3 or instance_map.dtype != torch.int32 or instance_map.shape[0] != b
            or instance_map.device != dev or not instance_map.is_contiguous()):
        raise MaskBevHipError(f'overlap_filter: instance_map must be a contiguous ({b}, H, W) int32 tensor on keep\'s device '
                              f'(it is changed in place), got {tuple(instance_map.shape)} {instance_map.dtype}')
    h, w = int(instance_map.shape[1]), int(instance_map.shape[2])
    keep = _frame_table('overlap_filter', 'keep', keep, (b, q), torch.bool, dev)
    areas = _frame_table('overlap_filter', 'areas', areas, (b, q), torch.int32, dev)
    if q > 1024 or b > 65535 or not 1 <= h * w <= 1024 * 1024:
        raise MaskBevHipError(f'overlap_filter: Q {q} <= 1024, B {b} <= 65535 or 1 <= H * W {h * w} <= 2^20 violated')
    keep_out = torch.empty((b, q), dtype=torch.bool, device=dev)
    owned = torch.empty((b, q), dtype=torch.int32, device=dev)
    check(lib.mbv_overlap_filter(_ptr(instance_map), _ptr(areas), _ptr(keep), b, h, w, q, num, den, int(min_cells), _ptr(owned),
                                 _ptr(keep_out), _stream()), 'mbv_overlap_filter')
    return keep_out, owned


@dataclass
class PointInstances:
    """K31's outputs for a batch of B scans and Q queries, on the device: ``point_query`` (total_points) int32 — per point of
    the concatenated scans the query that owns its BEV cell, -1 for none (and for every point K1 drops); ``scan_offsets``
    (B + 1) int32 on the device; ``counts`` (B, Q) int32 — lifted points per query; ``z_min``, ``z_max``, ``z_lo``, ``z_hi``
    (B, Q) f32 — the extremes of a query's points and the histogram edges of the two quantiles (include/maskbev_hip.h, K31),
    zeros for a query without a point.  ``lengths``: the scans' point counts, known on the host.  ``z_ground`` (B, Q) f32, only
    from a lift with a ground map (K35b): the lowest ground height under the query's kept points, 0 without one."""
    point_query: torch.Tensor
    scan_offsets: torch.Tensor
    counts: torch.Tensor
    z_min: torch.Tensor
    z_max: torch.Tensor
    z_lo: torch.Tensor
    z_hi: torch.Tensor
    lengths: Tuple[int, ...]
    z_ground: Optional[torch.Tensor] = None

    def per_scan(self) -> List[torch.Tensor]:
        """The labels of every scan: a list of (N_i,) views of ``point_query``.  No host synchronisation."""
        return list(torch.split(self.point_query, list(self.lengths)))


@dataclass
class GroundMap:
    """K35a's outputs for a batch of B scans, on the device: ``ground`` (B, gy, gx) f32 — per BEV cell (row = y-cell, column =
    x-cell, the layout of ``instance_map``) the lowest return within ``radius`` cells, +inf where that window holds none;
    ``cell_min`` (B, gy, gx) f32 — the lowest return of the cell itself, +inf for an empty cell."""
    ground: torch.Tensor
    cell_min: torch.Tensor
    radius: int


MAX_GROUND_RADIUS = 32        # cells: the halo K35a's window passes stage in LDS


def _concat_scans(what: str, scans: Sequence[torch.Tensor], dev):
    """The scans as K1 takes them: (points (sum N_i, dim) f32 contiguous, dim, lengths, scan_offsets (B + 1) i32 on ``dev``)."""
    dim = int(scans[0].shape[1]) if scans[0].dim() == 2 else -1
    if dim not in (3, 4) or any(p.dim() != 2 or p.shape[1] != dim or p.device != dev for p in scans):
        raise MaskBevHipError(f'{what}: scans must be (N_i, 3) or (N_i, 4) tensors of one width on the map\'s device')
    lens = [int(p.shape[0]) for p in scans]
    points = scans[0] if len(scans) == 1 else torch.cat(list(scans), 0)
    points = points.to(torch.float32).contiguous()
    offs = [0]
    for l in lens:
        offs.append(offs[-1] + l)
    return points, dim, lens, torch.tensor(offs, dtype=torch.int32).to(dev, non_blocking=True)


@torch.no_grad()
def ground_map(scans: Sequence[torch.Tensor], geom, radius: int, z_floor: Optional[float] = None,
               prefilter: bool = True) -> GroundMap:
    """K35a: a ground height for every BEV cell of every scan — the lowest z among the points K1's cell rule accepts (``geom``,
    ``prefilter`` as in :func:`lift_instances`) and that are not below ``z_floor`` (None: no floor), per cell and then over
    the window of ``radius`` cells (0 .. 32) around it.  One return below the road pulls the ground down over its whole
    window; ``z_floor`` is the only defence.  Device tensors only; no host synchronisation."""
    lib = _lib.load()
    if len(scans) == 0:
        raise ValueError('ground_map: empty batch')
    _need_gpu(*scans)
    radius = int(radius)
    if not 0 <= radius <= MAX_GROUND_RADIUS:
        raise ValueError(f'ground_map: radius {radius} outside 0 .. {MAX_GROUND_RADIUS} cells')
    batch, dev = len(scans), scans[0].device
    points, dim, lens, scan_offsets = _concat_scans('ground_map', scans, dev)
    gx, gy, gz = (int(v) for v in geom.grid)
    cell_min = torch.empty((batch, gy, gx), dtype=torch.float32, device=dev)
    ground = torch.empty((batch, gy, gx), dtype=torch.float32, device=dev)
    nbytes = lib.mbv_ground_map_workspace_bytes(batch, gx, gy)
    if nbytes == 0:
        raise MaskBevHipError(f'ground_map: a batch of {batch} on a {gy}x{gx} grid is not supported')
    ws = _workspace(nbytes, dev)
    r, v = geom.pc_range, geom.voxel_size
    check(lib.mbv_ground_map(_ptr(points), dim, sum(lens), _ptr(scan_offsets), batch, r[0], r[1], r[2], r[3], r[4], r[5],
                             v[0], v[1], v[2], gx, gy, gz, 1 if prefilter else 0, radius,
                             float('-inf') if z_floor is None else float(z_floor), _ptr(cell_min), _ptr(ground), _ptr(ws),
                             ws.numel(), _stream()), 'mbv_ground_map')
    return GroundMap(ground, cell_min, radius)


def origin_cell(geom, origin) -> Tuple[int, int]:
    """The BEV cell (cx, cy) of a sensor at ``origin`` = (x, y, z): K1's arithmetic in numpy f32 — ``floor((p - min) / vs)`` as
    a separate subtraction and division — without the range rejection: the cell may lie outside the grid (KITTI's
    ``x_range = (0, 80)`` puts a sensor at x = 0 on the edge)."""
    import numpy as np
    f = np.float32
    r, v = geom.pc_range, geom.voxel_size
    cx = np.floor((f(origin[0]) - f(r[0])) / f(v[0]))
    cy = np.floor((f(origin[1]) - f(r[1])) / f(v[1]))
    if not (abs(cx) <= 2 ** 20 and abs(cy) <= 2 ** 20):        # NaN and inf land here
        raise ValueError(f'origin_cell: the origin {tuple(origin)} lies more than 2^20 cells from the grid\'s corner')
    return int(cx), int(cy)


@torch.no_grad()
def visibility_map(scans: Sequence[torch.Tensor], geom, origin=(0., 0., 0.), z_top: float = -0.2,
                   prefilter: bool = True) -> torch.Tensor:
    """K38a: which BEV cells every scan could observe → (B, gy, gx) uint8, the layout of ``instance_map``: bit 0 PASSED — a
    beam crossed the cell at or below ``z_top`` on its way to the lowest return of some other cell; bit 1 HIT — the cell holds a
    return K1's cell rule accepts (``geom``, ``prefilter`` as in :func:`lift_instances`); 0 — unknown: no beam says anything
    about the cell at that height.  ``origin`` = (x, y, z) of the sensor in the scan's frame; ``z_top`` is absolute in that
    frame, not relative to the ground: the default -0.2 m is a 1.5 m roof under a sensor 1.73 m above the road — geometry,
    not measurement.  One ray per cell; returns outside the grid cast none; the ring next to a roof-mounted sensor stays
    unknown.  Device tensors only; no host synchronisation."""
    lib = _lib.load()
    if len(scans) == 0:
        raise ValueError('visibility_map: empty batch')
    _need_gpu(*scans)
    batch, dev = len(scans), scans[0].device
    points, dim, lens, scan_offsets = _concat_scans('visibility_map', scans, dev)
    gx, gy, gz = (int(v) for v in geom.grid)
    ocx, ocy = origin_cell(geom, origin)
    vis = torch.empty((batch, gy, gx), dtype=torch.uint8, device=dev)
    nbytes = lib.mbv_visibility_map_workspace_bytes(batch, gx, gy)
    if nbytes == 0:
        raise MaskBevHipError(f'visibility_map: a batch of {batch} on a {gy}x{gx} grid is not supported')
    ws = _workspace(nbytes, dev)
    r, v = geom.pc_range, geom.voxel_size
    check(lib.mbv_visibility_map(_ptr(points), dim, sum(lens), _ptr(scan_offsets), batch, r[0], r[1], r[2], r[3], r[4], r[5],
                                 v[0], v[1], v[2], gx, gy, gz, 1 if prefilter else 0, ocx, ocy, float(origin[2]), float(z_top),
                                 _ptr(vis), _ptr(ws), ws.numel(), _stream()), 'mbv_visibility_map')
    return vis


VIS_PASSED, VIS_HIT = 1, 2


@torch.no_grad()
def lift_instances(scans: Sequence[torch.Tensor], instance_map: torch.Tensor, geom, num_queries: int, z_bins: int = 64,
                   quantiles: Tuple[float, float] = (0., 1.), prefilter: bool = True, ground=None, clearance: float = 0.3,
                   max_height: Optional[float] = None) -> PointInstances:
    """K31: ``scans`` — the list of (N_i, 3 | 4) f32 device tensors the module takes; ``instance_map`` (B, gy, gx) int32 of
    :func:`extract_masks`; ``geom`` — the encoder's ``VoxelGeometry`` (``prefilter``: the encoder's strict range filter in
    front of K1, on by default as there) → :class:`PointInstances`.  ``quantiles`` = (q_lo, q_hi) pick ``z_lo`` / ``z_hi``
    among ``z_bins`` equal bins over the geometry's z range.  With ``ground`` — a :class:`GroundMap` or a (B, gy, gx) f32
    tensor — K35b: a point keeps its query only when ``z > g + clearance`` and ``z <= g + max_height`` (None: no limit) with
    ``g`` the ground height of its cell; counts and z columns are then those of the kept points and ``z_ground`` is set.
    Device tensors only; no host synchronisation."""
    lib = _lib.load()
    if len(scans) == 0:
        raise ValueError('lift_instances: empty batch')
    _need_gpu(instance_map, *scans)
    batch, dev = len(scans), instance_map.device
    points, dim, lens, scan_offsets = _concat_scans('lift_instances', scans, dev)
    gx, gy, gz = (int(v) for v in geom.grid)
    if instance_map.dtype != torch.int32 or tuple(instance_map.shape) != (batch, gy, gx):
        raise MaskBevHipError(f'lift_instances: instance_map must be ({batch}, {gy}, {gx}) int32, got '
                              f'{tuple(instance_map.shape)} {instance_map.dtype}')
    q_lo, q_hi = float(quantiles[0]), float(quantiles[1])
    if not 0 <= int(num_queries) <= 1024 or not 1 <= int(z_bins) <= 256 or not 0.0 <= q_lo <= q_hi <= 1.0:
        raise MaskBevHipError(f'lift_instances: num_queries {num_queries} (<= 1024), z_bins {z_bins} (1 .. 256) or quantiles '
                              f'{(q_lo, q_hi)} (0 <= q_lo <= q_hi <= 1) out of range')
    num_queries, z_bins = int(num_queries), int(z_bins)
    n = sum(lens)
    instance_map = instance_map.contiguous()
    point_query = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.empty((batch, num_queries), dtype=torch.int32, device=dev)
    z_extent = torch.empty((batch, num_queries, 4), dtype=torch.float32, device=dev)
    r, v = geom.pc_range, geom.voxel_size
    z_ground = None
    if ground is None:
        nbytes = lib.mbv_lift_instances_workspace_bytes(batch, num_queries, z_bins)
        ws = _workspace(nbytes, dev) if nbytes > 0 else None
        check(lib.mbv_lift_instances(_ptr(points), dim, n, _ptr(scan_offsets), batch, r[0], r[1], r[2], r[3], r[4], r[5],
                                     v[0], v[1], v[2], gx, gy, gz, 1 if prefilter else 0, _ptr(instance_map), num_queries,
                                     z_bins, q_lo, q_hi, _ptr(point_query), _ptr(counts), _ptr(z_extent), _ptr(ws),
                                     ws.numel() if ws is not None else 0, _stream()), 'mbv_lift_instances')
    else:
        gmap = ground.ground if isinstance(ground, GroundMap) else ground
        if (not torch.is_tensor(gmap) or gmap.dtype != torch.float32 or tuple(gmap.shape) != (batch, gy, gx)
                or gmap.device != dev):
            raise MaskBevHipError(f'lift_instances: ground must be a GroundMap or a ({batch}, {gy}, {gx}) f32 tensor on the '
                                  f'map\'s device')
        gmap = gmap.contiguous()
        z_ground = torch.empty((batch, num_queries), dtype=torch.float32, device=dev)
        nbytes = lib.mbv_lift_instances_ground_workspace_bytes(batch, num_queries, z_bins)
        ws = _workspace(nbytes, dev) if nbytes > 0 else None
        check(lib.mbv_lift_instances_ground(_ptr(points), dim, n, _ptr(scan_offsets), batch, r[0], r[1], r[2], r[3], r[4],
                                            r[5], v[0], v[1], v[2], gx, gy, gz, 1 if prefilter else 0, _ptr(instance_map),
                                            num_queries, z_bins, q_lo, q_hi, _ptr(gmap), float(clearance),
                                            float('inf') if max_height is None else float(max_height), _ptr(point_query),
                                            _ptr(counts), _ptr(z_extent), _ptr(z_ground), _ptr(ws),
                                            ws.numel() if ws is not None else 0, _stream()), 'mbv_lift_instances_ground')
    return PointInstances(point_query, scan_offsets, counts, z_extent[..., 0], z_extent[..., 1], z_extent[..., 2],
                          z_extent[..., 3], tuple(lens), z_ground)


__all__ = ['select_queries', 'extract_masks', 'mask_self_overlap', 'mask_nms', 'overlap_filter','lift_instances', 'PointInstances', 'ground_map', 'GroundMap',
           'MAX_GROUND_RADIUS', 'visibility_map', 'origin_cell', 'VIS_PASSED', 'VIS_HIT']
