"""The tracker step over consecutive BEV instance maps of one sequence (csrc/track.hip) — K33a, with two optional parts, both
off by default: K37's constant-velocity motion model and gated re-association, and K38b's occlusion-aware ageing from K38a's
visibility maps (which runs on K37's step) — and K33b, tube association, the S_assoc term of LSTQ.  Behind
``tracking.InstanceTracker`` and ``metrics.DeviceTubeAssociation``.  K39 (csrc/fuse.hip), behind
``tracking.FootprintFusion`` and ``Predictions.fused``: the tracked footprints fused over time in a rolling world grid, and a
query map turned back into packed masks.  The definitions are in include/maskbev_hip.h."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import MaskBevHipError, check
from .ops_core import _need_gpu, _ptr, _stream, _workspace


@dataclass
class TrackMotion:
    """K37's motion record of a tracker, on the device (include/maskbev_hip.h): ``pos`` (P, 2) f64 — the centroid of every live
    track in metres, x then y, in the coordinates of the frame last processed; ``vel`` (P, 2) f64 — metres per frame in the
    same coordinates (motion over ground in sensor axes); ``motion_counters`` (2) int32 = gated, reserved 0."""
    pos: torch.Tensor
    vel: torch.Tensor
    motion_counters: torch.Tensor

    @staticmethod
    def fresh(max_tracks: int, device) -> 'TrackMotion':
        return TrackMotion(torch.zeros((int(max_tracks), 2), dtype=torch.float64, device=device),
                           torch.zeros((int(max_tracks), 2), dtype=torch.float64, device=device),
                           torch.zeros((2,), dtype=torch.int32, device=device))


@dataclass
class MotionSettings:
    """K37's settings (``tracking.MotionSettings`` is this class): ``gain`` in [0, 1] — the share of a frame's innovation
    (measured centroid minus predicted) that goes into the velocity; ``gate_m`` >= 0 in metres — the centroid-distance gate of
    the second stage, 0 switches it off; ``max_speed`` >= 0 in metres per frame — a track predicted to move further is not
    advected: the kernel's ``max_shift`` is ``floor(max_speed / voxel)`` cells.  The defaults are geometry, not measurement:
    3.0 m is just over the 2.8 m an oncoming car moves per frame at 100 km/h relative and 10 Hz; 6.0 m per frame is 216 km/h
    at 10 Hz."""
    gain: float = 0.5
    gate_m: float = 3.0
    max_speed: float = 6.0

    def __post_init__(self):
        self.gain, self.gate_m, self.max_speed = float(self.gain), float(self.gate_m), float(self.max_speed)
        if not (0.0 <= self.gain <= 1.0 and 0.0 <= self.gate_m < math.inf and 0.0 <= self.max_speed < math.inf):
            raise ValueError(f'MotionSettings: gain {self.gain} in [0, 1], gate_m {self.gate_m} >= 0 and max_speed '
                             f'{self.max_speed} >= 0, all finite, expected')

    def max_shift(self, voxel: float) -> int:
        """``floor(max_speed / voxel)`` cells, at most 2^31 - 1."""
        return int(min(math.floor(self.max_speed / float(voxel)), 2 ** 31 - 1))


@dataclass
class TrackOcclusion:
    """K38b's record of a tracker, on the device (include/maskbev_hip.h): ``live_held`` (P) int32 — the frames every live track
    has been held since its last match; ``occlusion_counters`` (2) int32 = held, reserved 0."""
    live_held: torch.Tensor
    occlusion_counters: torch.Tensor

    @staticmethod
    def fresh(max_tracks: int, device) -> 'TrackOcclusion':
        return TrackOcclusion(torch.zeros((int(max_tracks),), dtype=torch.int32, device=device),
                              torch.zeros((2,), dtype=torch.int32, device=device))


@dataclass
class OcclusionSettings:
    """K38's settings (``tracking.OcclusionSettings`` is this class): ``z_top`` in metres, absolute in the sensor frame — the
    roof height of the objects one asks about, K38a's; ``hidden_fraction`` = (num, den) with 0 < num <= den — a track that goes
    unmatched is held when at least num / den of its warped footprint lies on cells of visibility 0; ``max_hold`` >= 0 — the
    most frames in a row a track is held, 0 holds none; ``origin`` = (x, y, z) of the sensor in the scan's frame.  The defaults
    are geometry, not measurement: -0.2 m is a 1.5 m roof under a sensor 1.73 m above the road; half of the footprint must be
    hidden; 10 frames is one second at 10 Hz."""
    z_top: float = -0.2
    hidden_fraction: Tuple[int, int] = (1, 2)
    max_hold: int = 10
    origin: Tuple[float, float, float] = (0., 0., 0.)

    def __post_init__(self):
        self.z_top, self.max_hold = float(self.z_top), int(self.max_hold)
        self.hidden_fraction = (int(self.hidden_fraction[0]), int(self.hidden_fraction[1]))
        self.origin = tuple(float(v) for v in self.origin)
        num, den = self.hidden_fraction
        if not (0 < num <= den < 2 ** 31 and 0 <= self.max_hold < 2 ** 31 and math.isfinite(self.z_top) and len(self.origin) == 3
                and all(math.isfinite(v) for v in self.origin)):
            raise ValueError(f'OcclusionSettings: hidden_fraction {self.hidden_fraction} with 0 < num <= den, max_hold '
                             f'{self.max_hold} >= 0, a finite z_top {self.z_top} and a finite origin {self.origin} (x, y, z) expected')


@dataclass
class TrackState:
    """The tracker's persistent state on the device (include/maskbev_hip.h, K33a): ``state_map`` (H, W) int32 — a local
    track index or -1; ``live_id`` / ``live_seen`` (P) int32 — the global id and the frame of the last match of every live
    track; ``counters`` (4) int32 = n_live, next_id, frame, dropped.  ``motion``: K37's record, None without the motion
    model.  ``occlusion``: K38b's record, None without occlusion-aware ageing (which needs ``motion`` too)."""
    state_map: torch.Tensor
    live_id: torch.Tensor
    live_seen: torch.Tensor
    counters: torch.Tensor
    motion: Optional[TrackMotion] = None
    occlusion: Optional[TrackOcclusion] = None

    @staticmethod
    def fresh(h: int, w: int, max_tracks: int, device, motion: bool = False, occlusion: bool = False) -> 'TrackState':
        """``motion`` / ``occlusion``: with the fresh sub-records; ``occlusion`` implies the motion record."""
        return TrackState(torch.full((int(h), int(w)), -1, dtype=torch.int32, device=device),
                          torch.full((int(max_tracks),), -1, dtype=torch.int32, device=device),
                          torch.full((int(max_tracks),), -1, dtype=torch.int32, device=device),
                          torch.zeros((4,), dtype=torch.int32, device=device),
                          TrackMotion.fresh(max_tracks, device) if motion or occlusion else None,
                          TrackOcclusion.fresh(max_tracks, device) if occlusion else None)


@dataclass
class TrackFrames:
    """K33a's outputs for F frames: ``query_track`` (F, Q) int32 — the global id of every query, -1 when it is not present;
    ``track_map`` (F, H, W) int32 — the global id on the cells of present queries, else -1 (None when not asked for);
    ``query_velocity`` (F, Q, 2) f64 — K37: the velocity of a present query's track in metres per frame, 0 for a query that is
    not present (None without the motion model)."""
    query_track: torch.Tensor
    track_map: Optional[torch.Tensor]
    query_velocity: Optional[torch.Tensor] = None


@dataclass
class TubeTables:
    """K33b's running tables for C classes, ``id_limit`` I and ``max_tracks`` T, on the device: ``gt_size`` ((C - 1) * I)
    int64, ``pred_size`` (T) int64, ``pair`` ((C - 1) * I, T) int32, ``overflow`` (2) int64 — elements of an instance id >= I,
    of a track id >= T."""
    gt_size: torch.Tensor
    pred_size: torch.Tensor
    pair: torch.Tensor
    overflow: torch.Tensor
    num_classes: int
    id_limit: int
    max_tracks: int

    @staticmethod
    def zeros(num_classes: int, id_limit: int, max_tracks: int, device) -> 'TubeTables':
        c, i, t = int(num_classes), int(id_limit), int(max_tracks)
        if not (1 <= c <= 16 and 1 <= i <= 65536 and 1 <= t <= 2 ** 20 and (c - 1) * i * t < 2 ** 31 - 1):
            raise MaskBevHipError(f'TubeTables: num_classes {c} (1 .. 16), id_limit {i} (1 .. 65536), max_tracks {t} (1 .. 2^20) '
                                  'or their product (< 2^31 - 1) out of range')
        rows = (c - 1) * i
        return TubeTables(torch.zeros((rows,), dtype=torch.int64, device=device), torch.zeros((t,), dtype=torch.int64, device=device),
                          torch.zeros((rows, t), dtype=torch.int32, device=device), torch.zeros((2,), dtype=torch.int64, device=device),
                          c, i, t)


@dataclass
class TubeScores:
    """``assoc`` ((C - 1) * I) f64 — the association score of every ground-truth tube (0 for an empty row); ``class_assoc`` (C)
    f64 — the sums over a class's tubes; ``class_tubes`` (C) int32 — their number."""
    assoc: torch.Tensor
    class_assoc: torch.Tensor
    class_tubes: torch.Tensor


@torch.no_grad()
def track_frames(instance_maps: torch.Tensor, prev_from_cur: torch.Tensor, state: TrackState, x_lo: float, y_lo: float,
                 voxel: float, num_queries: int, min_iou: float = 0.3, max_age: int = 2, min_cells: int = 4,
                 track_map: bool = False, motion: Optional[MotionSettings] = None,
                 cur_from_prev: Optional[torch.Tensor] = None, occlusion: Optional[OcclusionSettings] = None,
                 visibility: Optional[torch.Tensor] = None) -> TrackFrames:
    """K33a: ``instance_maps`` (F, H, W) int32 — F consecutive frames of ONE sequence, a query in [0, num_queries) or -1 per
    cell; ``prev_from_cur`` (F, 2, 3) f64 — per frame the map of its BEV coordinates into the previous frame's; ``state`` is
    stepped in place.  Device tensors only; no host synchronisation.
    ``motion``: K37 — the step with the motion model; ``state.motion`` must hold the record.  ``cur_from_prev`` (F, 2, 3) f64
    is the inverse of ``prev_from_cur``; when it is absent it is computed on the device (:func:`invert_transforms`).
    ``occlusion``: K38b — the step through ``mbv_track_frames_occluded``; ``state.motion`` and ``state.occlusion`` must hold
    the records.  Without ``motion`` it runs with gain = gate = 0, K33a's matching.  ``visibility`` (F, H, W) uint8, K38a's
    maps of the same frames (``ops.visibility_map``); None holds no track: the step is then K37's."""
    lib = _lib.load()
    _need_gpu(instance_maps, prev_from_cur, state.state_map, state.live_id, state.live_seen, state.counters)
    dev = instance_maps.device
    if instance_maps.dim() != 3 or instance_maps.dtype != torch.int32:
        raise MaskBevHipError(f'track_frames: instance_maps must be (F, H, W) int32, got {tuple(instance_maps.shape)} '
                              f'{instance_maps.dtype}')
    f, h, w = (int(v) for v in instance_maps.shape)
    if tuple(prev_from_cur.shape) != (f, 2, 3) or prev_from_cur.dtype != torch.float64:
        raise MaskBevHipError(f'track_frames: prev_from_cur must be ({f}, 2, 3) float64, got {tuple(prev_from_cur.shape)} '
                              f'{prev_from_cur.dtype}')
    q, p = int(num_queries), int(state.live_id.numel())
    _check_fields('track_frames: state', dev, (('state_map', state.state_map, (h, w), torch.int32),
                                               ('live_id', state.live_id, (p,), torch.int32),
                                               ('live_seen', state.live_seen, (p,), torch.int32),
                                               ('counters', state.counters, (4,), torch.int32)))
    if prev_from_cur.device != dev:
        raise MaskBevHipError('track_frames: tensors on different devices')
    if not (0 <= q <= p <= 1024 and h * w <= 1024 * 1024 and int(min_cells) >= 1 and int(max_age) >= 0):
        raise MaskBevHipError(f'track_frames: Q {q} <= P {p} <= 1024, H * W {h * w} <= 2^20, min_cells {min_cells} >= 1 or '
                              f'max_age {max_age} >= 0 violated')
    instance_maps, prev_from_cur = instance_maps.contiguous(), prev_from_cur.contiguous()
    out = TrackFrames(torch.empty((f, q), dtype=torch.int32, device=dev),
                      torch.empty((f, h, w), dtype=torch.int32, device=dev) if track_map else None)
    if visibility is not None and occlusion is None:
        raise MaskBevHipError('track_frames: a visibility map given without occlusion settings')
    step = (f, h, w, float(x_lo), float(y_lo), float(voxel), q, p, float(min_iou), int(max_age), int(min_cells))
    rec, occ = state.motion, state.occlusion
    if motion is not None or occlusion is not None:                     # K38b's entry is K37's: it needs the motion record too
        if rec is None:
            raise MaskBevHipError('track_frames: motion or occlusion settings given, but state.motion is None (TrackMotion.fresh)')
        _need_gpu(rec.pos, rec.vel, rec.motion_counters)
        _check_fields('track_frames: state.motion', dev, (('pos', rec.pos, (p, 2), torch.float64),
                                                          ('vel', rec.vel, (p, 2), torch.float64),
                                                          ('motion_counters', rec.motion_counters, (2,), torch.int32)))
        if not float(voxel) > 0.0:
            raise MaskBevHipError(f'track_frames: voxel {float(voxel)} > 0 expected')
        model = (motion.gain, motion.gate_m, motion.max_shift(float(voxel))) if motion is not None else (0.0, 0.0, 0)
        if occlusion is not None:
            if occ is None:
                raise MaskBevHipError('track_frames: occlusion settings given, but state.occlusion is None (TrackOcclusion.fresh)')
            _need_gpu(occ.live_held, occ.occlusion_counters)
            _check_fields('track_frames: state.occlusion', dev, (('live_held', occ.live_held, (p,), torch.int32),
                                                                 ('occlusion_counters', occ.occlusion_counters, (2,), torch.int32)))
            if visibility is not None:
                _need_gpu(visibility)
                if tuple(visibility.shape) != (f, h, w) or visibility.dtype != torch.uint8 or visibility.device != dev:
                    raise MaskBevHipError(f'track_frames: visibility must be ({f}, {h}, {w}) uint8 on {dev}, got '
                                          f'{tuple(visibility.shape)} {visibility.dtype}')
                visibility = visibility.contiguous()
        if cur_from_prev is None:
            cur_from_prev = invert_transforms(prev_from_cur)
        _need_gpu(cur_from_prev)
        if tuple(cur_from_prev.shape) != (f, 2, 3) or cur_from_prev.dtype != torch.float64 or cur_from_prev.device != dev:
            raise MaskBevHipError(f'track_frames: cur_from_prev must be ({f}, 2, 3) float64 on {dev}, got '
                                  f'{tuple(cur_from_prev.shape)} {cur_from_prev.dtype}')
        cur_from_prev = cur_from_prev.contiguous()
        out.query_velocity = torch.empty((f, q, 2), dtype=torch.float64, device=dev)
    if f == 0:
        return out
    frames = (_ptr(instance_maps), _ptr(prev_from_cur))
    lists = (_ptr(state.state_map), _ptr(state.live_id), _ptr(state.live_seen))
    if occlusion is not None:
        name = 'mbv_track_frames_occluded'
        args = frames + (_ptr(cur_from_prev), _ptr(visibility)) + step + model + occlusion.hidden_fraction + \
            (occlusion.max_hold,) + lists + (_ptr(occ.live_held), _ptr(state.counters), _ptr(rec.pos), _ptr(rec.vel), _ptr(rec.motion_counters),
                  _ptr(occ.occlusion_counters), _ptr(out.query_track), _ptr(out.track_map), _ptr(out.query_velocity))
    elif motion is not None:
        name = 'mbv_track_frames_motion'
        args = frames + (_ptr(cur_from_prev),) + step + model + lists + (
            _ptr(state.counters), _ptr(rec.pos), _ptr(rec.vel), _ptr(rec.motion_counters), _ptr(out.query_track),
            _ptr(out.track_map), _ptr(out.query_velocity))
    else:
        name = 'mbv_track_frames'
        args = frames + step + lists + (_ptr(state.counters), _ptr(out.query_track), _ptr(out.track_map))
    ws = _workspace(getattr(lib, name + '_workspace_bytes')(h, w, q, p), dev)
    check(getattr(lib, name)(*args, _ptr(ws), ws.numel(), _stream()), name)
    return out


def _check_fields(what: str, dev, fields) -> None:
    """Every (name, tensor, shape, dtype) of ``fields`` is a contiguous tensor of that shape and dtype on ``dev``."""
    for name, x, shape, dt in fields:
        if tuple(x.shape) != shape or x.dtype != dt or x.device != dev or not x.is_contiguous():
            raise MaskBevHipError(f'{what}.{name} must be a contiguous {shape} {dt} tensor on {dev}')


def invert_transforms(prev_from_cur: torch.Tensor) -> torch.Tensor:
    """``cur_from_prev`` (F, 2, 3) f64: the first two rows of the inverse of every ``prev_from_cur`` completed to 3 x 3 with the
    row 0 0 1 — by the adjugate of the 2 x 2 part, elementwise on the input's device, no host synchronisation."""
    m = prev_from_cur.to(torch.float64)
    a, b, tx, c, d, ty = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2], m[:, 1, 0], m[:, 1, 1], m[:, 1, 2]
    det = a * d - b * c
    n00, n01, n10, n11 = d / det, -b / det, -c / det, a / det
    return torch.stack([torch.stack([n00, n01, -(n00 * tx + n01 * ty)], dim=1),
                        torch.stack([n10, n11, -(n10 * tx + n11 * ty)], dim=1)], dim=1).contiguous()


@torch.no_grad()
def tube_accumulate(pred_track: torch.Tensor, gt_words: torch.Tensor, class_lut: torch.Tensor, tables: TubeTables) -> TubeTables:
    """K33b: adds the elements ``pred_track`` (N) int32 (the global track id, -1 = none) / ``gt_words`` (N) int32 / uint32
    (``.label`` layout) to ``tables``; ``class_lut`` (L) int32 as in ``panoptic_frames``.  No host synchronisation."""
    lib = _lib.load()
    _need_gpu(pred_track, gt_words, class_lut, tables.gt_size, tables.pred_size, tables.pair, tables.overflow)
    dev = pred_track.device
    if pred_track.dim() != 1 or pred_track.dtype != torch.int32:
        raise MaskBevHipError(f'tube_accumulate: pred_track must be (N) int32, got {tuple(pred_track.shape)} {pred_track.dtype}')
    if gt_words.dtype == getattr(torch, 'uint32', None):
        gt_words = gt_words.view(torch.int32)
    if gt_words.dtype != torch.int32 or tuple(gt_words.shape) != tuple(pred_track.shape):
        raise MaskBevHipError(f'tube_accumulate: gt_words must be ({pred_track.numel()}) int32 / uint32, got '
                              f'{tuple(gt_words.shape)} {gt_words.dtype}')
    if class_lut.dim() != 1 or class_lut.dtype != torch.int32:
        raise MaskBevHipError('tube_accumulate: class_lut must be a 1-d int32 table')
    _check_fields('tube_accumulate: tables', dev, _tube_fields(tables))
    if gt_words.device != dev or class_lut.device != dev:
        raise MaskBevHipError('tube_accumulate: tensors on different devices')
    n = pred_track.numel()
    if n >= 2 ** 31 - 1:
        raise MaskBevHipError(f'tube_accumulate: {n} elements out of range')
    pred_track, gt_words, class_lut = pred_track.contiguous(), gt_words.contiguous(), class_lut.contiguous()
    check(lib.mbv_tube_accumulate(_ptr(pred_track), _ptr(gt_words), n, _ptr(class_lut), class_lut.numel(), tables.num_classes,
                                  tables.id_limit, tables.max_tracks, _ptr(tables.gt_size), _ptr(tables.pred_size),
                                  _ptr(tables.pair), _ptr(tables.overflow), _stream()), 'mbv_tube_accumulate')
    return tables


def _tube_fields(tables: TubeTables):
    rows, t = (tables.num_classes - 1) * tables.id_limit, tables.max_tracks
    return (('gt_size', tables.gt_size, (rows,), torch.int64), ('pred_size', tables.pred_size, (t,), torch.int64),
            ('pair', tables.pair, (rows, t), torch.int32), ('overflow', tables.overflow, (2,), torch.int64))


@torch.no_grad()
def tube_scores(tables: TubeTables) -> TubeScores:
    """K33b: the association score of every ground-truth tube of ``tables`` and the class sums.  No host synchronisation."""
    lib = _lib.load()
    _need_gpu(tables.gt_size, tables.pred_size, tables.pair, tables.overflow)
    dev = tables.pred_size.device
    _check_fields('tube_scores: tables', dev, _tube_fields(tables))
    c, rows = tables.num_classes, (tables.num_classes - 1) * tables.id_limit
    out = TubeScores(torch.empty((rows,), dtype=torch.float64, device=dev), torch.empty((c,), dtype=torch.float64, device=dev),
                     torch.empty((c,), dtype=torch.int32, device=dev))
    check(lib.mbv_tube_scores(_ptr(tables.gt_size), _ptr(tables.pred_size), _ptr(tables.pair), c, tables.id_limit,
                              tables.max_tracks, _ptr(out.assoc), _ptr(out.class_assoc), _ptr(out.class_tubes), _stream()),
          'mbv_tube_scores')
    return out


@dataclass
class FusionSettings:
    """K39a's settings (``tracking.FusionSettings`` is this class): a store cell's evidence ``count`` lives in [0, ``cap``]; a
    detection of the owner adds ``hit``, a detection of another id takes ``hit`` away (and takes the cell over at 0), a seen
    cell without a detection loses ``miss``; a cell is read out with ``count >= min_count``.  ``static_speed`` >= 0 in metres
    per frame: with a ``query_velocity``, a query faster than this is moving — passed through, never accumulated; None, the
    default, treats every query as static.  The defaults are geometry, not measurement: two frames of agreement show a
    cell, eight frames of memory bridge 0.8 s at 10 Hz."""
    cap: int = 8
    hit: int = 1
    miss: int = 1
    min_count: int = 2
    static_speed: Optional[float] = None

    def __post_init__(self):
        self.cap, self.hit, self.miss, self.min_count = int(self.cap), int(self.hit), int(self.miss), int(self.min_count)
        if self.static_speed is not None:
            self.static_speed = float(self.static_speed)
        if not (1 <= self.cap < 2 ** 31 and 1 <= self.hit < 2 ** 31 and 0 <= self.miss < 2 ** 31 and 1 <= self.min_count < 2 ** 31
                and (self.static_speed is None or 0.0 <= self.static_speed < math.inf)):
            raise ValueError(f'FusionSettings: cap {self.cap} >= 1, hit {self.hit} >= 1, miss {self.miss} >= 0, min_count '
                             f'{self.min_count} >= 1 and static_speed {self.static_speed} None or finite and >= 0 expected')


def fusion_store_size(h: int, w: int) -> int:
    """The smallest store side K39a accepts for an (h, w) grid: even, with (S - 4)^2 >= h^2 + w^2."""
    s = math.isqrt(int(h) ** 2 + int(w) ** 2)
    s += 4 + (s * s < int(h) ** 2 + int(w) ** 2)
    return s + (s & 1)


@dataclass
class FusionState:
    """K39a's state of one sequence, on the device (include/maskbev_hip.h): ``owner`` (S, S) int32 — the global track id that
    owns a store cell, -1 for none; ``count`` (S, S) int32 — its evidence; ``window`` (4) int64 = wx0, wy0, frames, 0."""
    owner: torch.Tensor
    count: torch.Tensor
    window: torch.Tensor

    @staticmethod
    def fresh(h: int, w: int, device) -> 'FusionState':
        s = fusion_store_size(h, w)
        return FusionState(torch.full((s, s), -1, dtype=torch.int32, device=device),
                           torch.zeros((s, s), dtype=torch.int32, device=device),
                           torch.zeros((4,), dtype=torch.int64, device=device))


@dataclass
class FusedFrames:
    """K39a's outputs for F frames: ``ids`` (F, H, W) int32 — the global track id that owns every sensor cell after fusion, -1
    for none; ``queries`` (F, H, W) int32 — the frame's query of that id (the smallest static one), -1 where the id has no
    query in this frame: a footprint that is only remembered."""
    ids: torch.Tensor
    queries: Optional[torch.Tensor]


@torch.no_grad()
def fuse_frames(instance_maps: torch.Tensor, query_track: torch.Tensor, world_from_cur: torch.Tensor,
                cur_from_world: torch.Tensor, state: FusionState, x_lo: float, y_lo: float, voxel: float,
                settings: Optional[FusionSettings] = None, visibility: Optional[torch.Tensor] = None,
                query_velocity: Optional[torch.Tensor] = None, queries: bool = True) -> FusedFrames:
    """K39a: ``instance_maps`` (F, H, W) int32 — F consecutive frames of ONE sequence; ``query_track`` (F, Q) int32 — the
    tracker's ids of the same frames; ``world_from_cur`` / ``cur_from_world`` (F, 2, 3) f64 — every frame's BEV coordinates
    into the frame of the sequence's first scan, and back; ``state`` is stepped in place.  ``visibility`` (F, H, W) uint8,
    K38a's maps: without it every cell counts as seen.  ``query_velocity`` (F, Q, 2) f64, K37's: used only with
    ``settings.static_speed``.  Device tensors only; no host synchronisation."""
    lib = _lib.load()
    settings = settings if settings is not None else FusionSettings()
    _need_gpu(instance_maps, query_track, world_from_cur, cur_from_world, state.owner, state.count, state.window)
    dev = instance_maps.device
    if instance_maps.dim() != 3 or instance_maps.dtype != torch.int32:
        raise MaskBevHipError(f'fuse_frames: instance_maps must be (F, H, W) int32, got {tuple(instance_maps.shape)} '
                              f'{instance_maps.dtype}')
    f, h, w = (int(v) for v in instance_maps.shape)
    if query_track.dim() != 2 or int(query_track.shape[0]) != f or query_track.dtype != torch.int32:
        raise MaskBevHipError(f'fuse_frames: query_track must be ({f}, Q) int32, got {tuple(query_track.shape)} {query_track.dtype}')
    q, s = int(query_track.shape[1]), int(state.owner.shape[0])
    fields = [('instance_maps', instance_maps, (f, h, w), torch.int32), ('query_track', query_track, (f, q), torch.int32),
              ('world_from_cur', world_from_cur, (f, 2, 3), torch.float64),
              ('cur_from_world', cur_from_world, (f, 2, 3), torch.float64)]
    if visibility is not None:
        fields.append(('visibility', visibility, (f, h, w), torch.uint8))
    if settings.static_speed is None:
        query_velocity = None
    if query_velocity is not None:
        fields.append(('query_velocity', query_velocity, (f, q, 2), torch.float64))
    _need_gpu(*(x for _, x, _, _ in fields))
    for name, x, shape, dt in fields:
        if tuple(x.shape) != shape or x.dtype != dt or x.device != dev:
            raise MaskBevHipError(f'fuse_frames: {name} must be a {shape} {dt} tensor on {dev}, got {tuple(x.shape)} {x.dtype}')
    instance_maps, query_track, world_from_cur, cur_from_world = (x.contiguous() for _, x, _, _ in fields[:4])
    visibility = visibility.contiguous() if visibility is not None else None
    query_velocity = query_velocity.contiguous() if query_velocity is not None else None
    _check_fields('fuse_frames: state', dev, (('owner', state.owner, (s, s), torch.int32), ('count', state.count, (s, s), torch.int32),
                                              ('window', state.window, (4,), torch.int64)))
    if not (q <= 1024 and h * w <= 1024 * 1024 and s % 2 == 0 and fusion_store_size(h, w) <= s <= 8192 and float(voxel) > 0.0):
        raise MaskBevHipError(f'fuse_frames: Q {q} <= 1024, H * W {h * w} <= 2^20, an even store side {s} in '
                              f'[{fusion_store_size(h, w)}, 8192] or voxel {float(voxel)} > 0 violated')
    out = FusedFrames(torch.empty((f, h, w), dtype=torch.int32, device=dev),
                      torch.empty((f, h, w), dtype=torch.int32, device=dev) if queries else None)
    if f == 0 or h * w == 0:
        return out
    speed = settings.static_speed if settings.static_speed is not None else 0.0
    check(lib.mbv_fuse_frames(_ptr(instance_maps), _ptr(query_track), _ptr(world_from_cur), _ptr(cur_from_world), _ptr(visibility),
                              _ptr(query_velocity), f, h, w, s, float(x_lo), float(y_lo), float(voxel), q, settings.cap,
                              settings.hit, settings.miss, settings.min_count, speed, _ptr(state.owner), _ptr(state.count),
                              _ptr(state.window), _ptr(out.ids), _ptr(out.queries), _stream()), 'mbv_fuse_frames')
    return out


@torch.no_grad()
def masks_from_map(maps: torch.Tensor, num_queries: int):
    """K39b: ``maps`` (F, H, W) int32, a query in [0, ``num_queries``) per cell (anything else: none) → (``PackedMasks`` of the
    F * Q rows f * Q + q in the layout of ``pack_binary_masks``, ``areas`` (F, Q) int32).  No host synchronisation."""
    from .ops_loss import PackedMasks
    lib = _lib.load()
    _need_gpu(maps)
    if maps.dim() != 3 or maps.dtype != torch.int32:
        raise MaskBevHipError(f'masks_from_map: maps must be (F, H, W) int32, got {tuple(maps.shape)} {maps.dtype}')
    f, h, w = (int(v) for v in maps.shape)
    q = int(num_queries)
    if not (0 <= q <= 1024 and f <= 65535 and h >= 1 and w >= 1 and h * w <= 1024 * 1024):
        raise MaskBevHipError(f'masks_from_map: Q {q} <= 1024, F {f} <= 65535 or 1 <= H * W {h * w} <= 2^20 violated')
    maps = maps.contiguous()
    words = torch.empty((f * q, lib.mbv_packed_mask_words(h, w)), dtype=torch.int32, device=maps.device)
    areas = torch.empty((f, q), dtype=torch.int32, device=maps.device)
    check(lib.mbv_masks_from_map(_ptr(maps), f, h, w, q, _ptr(words), _ptr(areas), _stream()), 'mbv_masks_from_map')
    return PackedMasks(words, h, w), areas


__all__ = ['track_frames', 'invert_transforms', 'tube_accumulate', 'tube_scores', 'TrackState', 'TrackMotion', 'MotionSettings',
           'TrackOcclusion', 'OcclusionSettings',
           'TrackFrames', 'TubeTables', 'TubeScores',
           'FusionSettings', 'FusionState', 'FusedFrames', 'fusion_store_size', 'fuse_frames', 'masks_from_map']
