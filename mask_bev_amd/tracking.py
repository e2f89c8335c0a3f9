"""Instance tracking over a sequence (K33a, csrc/track.hip): one stable global id per object from the per-frame BEV
instance maps of ``MaskBevModule.predict``, after ego-motion compensation with the sequence's poses.

There are no appearance features: an object is matched to the track whose footprint, warped into the current frame by the
ego motion, it overlaps best (greedy, exact IoU order).  The motion model is off by default: a parked car keeps its id; a
moving car keeps it only while its footprints of consecutive frames overlap.

``InstanceTracker(..., motion=MotionSettings())`` turns on K37: every track carries a centroid and a ground-relative
velocity (constant velocity, a fixed gain), its footprint is shifted by the predicted whole cells before the overlap is
taken, and what the overlap leaves open is matched by centroid distance within a gate — so a fast car that never overlapped
itself is picked up in its second frame and keeps its id.  Its limits: shifts are whole cells, so a coasting track's
footprint drifts by up to half a cell per frame; the gate can hand a lost track to another detection within ``gate_m`` of
its prediction.  The defaults of ``MotionSettings`` are geometry, not measurement; no LSTQ on real SemanticKITTI is pinned.

``InstanceTracker(..., occlusion=OcclusionSettings())`` turns on K38b: ``update(..., visibility=)`` takes K38a's visibility
maps of the same frames (``ops.visibility_map`` / ``Predictions.visibility``), and a track that goes unmatched while at least
``hidden_fraction`` of its warped footprint lies on cells no beam certified does not age, for at most ``max_hold`` frames in
a row — a car behind a truck keeps its id, a false positive that vanishes in the open still dies after ``max_age``.  Its
limits: ``z_top`` is absolute in the sensor frame, not relative to K35's ground; returns outside the grid cast no rays; the
blind ring next to a roof-mounted sensor is "unknown", so tracks there are held up to ``max_hold``; one ray per cell, to its
lowest return.  The defaults are geometry, not measurement, and nothing is claimed about LSTQ on real data.

:class:`FootprintFusion` (K39a) is the tracker's per-cell memory: which id owned which place, in a world-anchored grid that
scrolls with the ego.  It runs behind the tracker on its ``query_track`` and is off unless used; see the class.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from ._lib import MaskBevHipError
from .ops_track import FusionSettings, MotionSettings, OcclusionSettings

_IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=np.float64)


def prev_from_cur_2d(pose_prev, pose_cur) -> np.ndarray:
    """The (2, 3) f64 map of the current frame's BEV coordinates into the previous frame's, from the two 4 x 4 f64 sensor
    poses (sensor → world): rows 0 and 1, columns 0, 1 and 3 of ``inv(pose_prev) @ pose_cur``.  Roll, pitch and z are
    dropped: the map is the planar part of the relative motion, exact for a vehicle that only yaws and moves in its plane."""
    rel = np.linalg.inv(np.asarray(pose_prev, dtype=np.float64)) @ np.asarray(pose_cur, dtype=np.float64)
    return np.ascontiguousarray(rel[:2][:, [0, 1, 3]])


def cur_from_prev_2d(prev_from_cur) -> np.ndarray:
    """The (2, 3) f64 inverse of a ``prev_from_cur``: the first two rows of the inverse of the map completed to 3 x 3."""
    full = np.vstack([np.asarray(prev_from_cur, dtype=np.float64).reshape(2, 3), [0.0, 0.0, 1.0]])
    return np.ascontiguousarray(np.linalg.inv(full)[:2])


def velodyne_poses(poses, calib) -> np.ndarray:
    """SemanticKITTI's ``poses.txt`` is in the left camera's frame: ``inv(Tr) @ pose @ Tr`` per scan gives the (N, 4, 4) f64
    poses of the LiDAR.  ``poses`` from ``batch.read_poses``; ``calib`` from ``batch.read_calib`` (its ``velo_to_cam``) or the
    4 x 4 ``Tr`` itself."""
    tr = np.asarray(calib['velo_to_cam'] if isinstance(calib, dict) else calib, dtype=np.float64)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    inv = np.linalg.inv(tr)
    return np.stack([inv @ p @ tr for p in poses]) if len(poses) else np.zeros((0, 4, 4))


class InstanceTracker:
    """The tracker of one sequence.  ``x_range``, ``y_range``, ``voxel_size`` describe the BEV grid of the instance maps
    ((ny, nx) cells, cell (iy, ix) centred at ``x_range[0] + (ix + 0.5) * voxel_size``, ``y_range[0] + (iy + 0.5) *
    voxel_size``); ``num_queries`` Q <= ``max_tracks`` P <= 1024.  A query with fewer than ``min_cells`` cells is left out; a
    pair needs an IoU of at least ``min_iou``; a track unmatched for more than ``max_age`` frames is forgotten.  The state
    lives on the device; :meth:`update` synchronises nothing and :meth:`counters` is the one host copy.  ``motion``: a
    :class:`MotionSettings` turns on the constant-velocity motion model and the gated second stage (K37); None, the default,
    is K33a's step.  ``occlusion``: an :class:`OcclusionSettings` turns on occlusion-aware ageing (K38b) for the frames whose
    visibility map is passed to :meth:`update`; with ``motion`` None it runs on K33a's matching (gain = gate = 0)."""

    def __init__(self, x_range, y_range, voxel_size: float, num_queries: int, max_tracks: int = 256, min_iou: float = 0.3,
                 max_age: int = 2, min_cells: int = 4, device='cuda', motion: Optional[MotionSettings] = None,
                 occlusion: Optional[OcclusionSettings] = None):
        self.x_lo, self.y_lo, self.voxel = float(x_range[0]), float(y_range[0]), float(voxel_size)
        self.w = int((x_range[1] - x_range[0]) / voxel_size)
        self.h = int((y_range[1] - y_range[0]) / voxel_size)
        self.num_queries, self.max_tracks = int(num_queries), int(max_tracks)
        self.min_iou, self.max_age, self.min_cells = float(min_iou), int(max_age), int(min_cells)
        if not 0 <= self.num_queries <= self.max_tracks <= 1024:
            raise ValueError(f'InstanceTracker: num_queries {num_queries} <= max_tracks {max_tracks} <= 1024 expected')
        if self.min_cells < 1 or self.max_age < 0 or self.h * self.w > 1024 * 1024:
            raise ValueError('InstanceTracker: min_cells >= 1, max_age >= 0 and at most 2^20 cells expected')
        if motion is not None and not isinstance(motion, MotionSettings):
            raise ValueError(f'InstanceTracker: motion must be a MotionSettings or None, got {type(motion).__name__}')
        if motion is not None and not self.voxel > 0.0:
            raise ValueError(f'InstanceTracker: voxel_size {voxel_size} > 0 expected with a motion model')
        if occlusion is not None and not isinstance(occlusion, OcclusionSettings):
            raise ValueError(f'InstanceTracker: occlusion must be an OcclusionSettings or None, got {type(occlusion).__name__}')
        if occlusion is not None and not self.voxel > 0.0:
            raise ValueError(f'InstanceTracker: voxel_size {voxel_size} > 0 expected with occlusion-aware ageing')
        self.motion, self.occlusion = motion, occlusion
        self.device = torch.device(device)
        self.reset()

    def reset(self) -> None:
        """A fresh sequence: no live track, ids from 0, and the next frame takes the identity transform."""
        self.state = ops.TrackState.fresh(self.h, self.w, self.max_tracks, self.device, motion=self.motion is not None,
                                          occlusion=self.occlusion is not None)
        self._last_pose: Optional[np.ndarray] = None
        self._started = False

    def _transforms(self, b: int, poses, prev_from_cur):
        """→ (prev_from_cur on the device, the same on the host or None when it was given as a device tensor)"""
        if prev_from_cur is not None and torch.is_tensor(prev_from_cur):
            m = prev_from_cur.to(self.device, torch.float64).reshape(b, 2, 3)
            if not self._started:                          # the first frame after reset(): nothing to warp
                m = m.clone()
                m[0] = torch.from_numpy(_IDENTITY).to(self.device)
            return m, None
        if prev_from_cur is not None:
            out = np.array(np.asarray(prev_from_cur, dtype=np.float64).reshape(b, 2, 3))
            if not self._started:
                out[0] = _IDENTITY
        else:
            out = np.empty((b, 2, 3), dtype=np.float64)
            if poses is None:
                out[:] = _IDENTITY                         # a standing sensor
            else:
                poses = np.asarray(poses, dtype=np.float64).reshape(b, 4, 4)
                last = self._last_pose
                for k in range(b):
                    out[k] = _IDENTITY if last is None else prev_from_cur_2d(last, poses[k])
                    last = poses[k]
                self._last_pose = last
        return torch.from_numpy(out).to(self.device, non_blocking=True), out

    @torch.no_grad()
    def update(self, pred_or_instance_maps, poses=None, prev_from_cur=None, track_map: bool = False, record: bool = False,
               visibility=None):
        """``pred_or_instance_maps``: a ``Predictions`` or its (B, ny, nx) int32 ``instance_map`` — B CONSECUTIVE frames of
        the sequence.  ``poses`` (B, 4, 4) f64 sensor poses on the host (the last pose is remembered between calls), or
        ``prev_from_cur`` (B, 2, 3) f64 on the host or the device; with neither, the sensor stands still.  Returns
        ``query_track`` (B, Q) int32 on the device — the global id of every query, -1 where it is not present — or, with
        ``track_map=True``, the ``ops.TrackFrames`` record that also holds the (B, ny, nx) map of global ids; ``record=True``
        returns that record without the map — with a motion model it holds ``query_velocity`` (B, Q, 2) f64, metres per
        frame over ground in the axes of each frame's sensor.  With a motion model the inverse transforms are computed on
        the host with the transforms themselves, and on the device where ``prev_from_cur`` is a device tensor.
        ``visibility`` (B, ny, nx) uint8 — K38a's maps of the same frames, for a tracker made with ``occlusion=``; without it
        no track is held in these frames."""
        maps = getattr(pred_or_instance_maps, 'instance_map', pred_or_instance_maps)
        if maps is None:
            raise MaskBevHipError('InstanceTracker.update: these predictions were made without an instance map')
        if maps.dim() != 3 or tuple(maps.shape[1:]) != (self.h, self.w):
            raise MaskBevHipError(f'InstanceTracker.update: (B, {self.h}, {self.w}) instance maps expected, got {tuple(maps.shape)}')
        m, host = self._transforms(int(maps.shape[0]), poses, prev_from_cur)
        n = None
        if visibility is not None and self.occlusion is None:
            raise MaskBevHipError('InstanceTracker.update: a visibility map for a tracker made without occlusion=')
        if (self.motion is not None or self.occlusion is not None) and host is not None:
            inv = np.stack([cur_from_prev_2d(x) for x in host]) if len(host) else np.zeros((0, 2, 3), dtype=np.float64)
            n = torch.from_numpy(inv).to(self.device, non_blocking=True)
        out = ops.track_frames(maps, m, self.state, self.x_lo, self.y_lo, self.voxel, self.num_queries, self.min_iou,
                               self.max_age, self.min_cells, track_map=track_map, motion=self.motion, cur_from_prev=n,
                               occlusion=self.occlusion, visibility=visibility)
        self._started = self._started or maps.shape[0] > 0
        return out if track_map or record else out.query_track

    def counters(self) -> dict:
        """The one host copy: ``{'live', 'tracks', 'frames', 'dropped'}`` — the live tracks, the ids given out so far, the
        frames seen since :meth:`reset` and the tracks dropped because ``max_tracks`` were live; with a motion model also
        ``'gated'`` — the pairs the second stage took; with occlusion-aware ageing also ``'held'`` — the times a track was
        held for a frame."""
        n_live, next_id, frame, dropped = (int(v) for v in self.state.counters.cpu())
        out = dict(live=n_live, tracks=next_id, frames=frame, dropped=dropped)
        if self.motion is not None:
            out['gated'] = int(self.state.motion.motion_counters.cpu()[0])
        if self.occlusion is not None:
            out['held'] = int(self.state.occlusion.occlusion_counters.cpu()[0])
        return out


class FootprintFusion:
    """Tracked footprints fused over time (K39a, csrc/fuse.hip): per-cell memory of which track owned a place, in a
    world-anchored store that scrolls by whole cells with the ego, so nothing is re-sampled from frame to frame.  The world is
    the sensor frame of the first pose after :meth:`reset`.  ``x_range``, ``y_range``, ``voxel_size``, ``num_queries``: the
    tracker's; ``settings``: a :class:`FusionSettings` (None: its defaults).  A detection adds evidence to its cell, a seen
    empty cell loses it, an unseen cell (``visibility`` 0) holds it: a parked car the detector misses for a frame, or the half
    of one that went out of sight, stays in the fused map under its id.
    Limits: moving objects (``settings.static_speed`` with a ``query_velocity``) are passed through, not accumulated; both
    gathers are nearest-cell, so a footprint seen under a turning ego loses and gains border cells; the id of a track that
    died persists under cells nobody sees until the window leaves them; z is ignored; the defaults are geometry, not
    measurement, and no PQ, LSTQ or AP on real data is claimed."""

    def __init__(self, x_range, y_range, voxel_size: float, num_queries: int, settings: Optional[FusionSettings] = None,
                 device='cuda'):
        self.x_lo, self.y_lo, self.voxel = float(x_range[0]), float(y_range[0]), float(voxel_size)
        self.w = int((x_range[1] - x_range[0]) / voxel_size)
        self.h = int((y_range[1] - y_range[0]) / voxel_size)
        self.num_queries = int(num_queries)
        if settings is not None and not isinstance(settings, FusionSettings):
            raise ValueError(f'FootprintFusion: settings must be a FusionSettings or None, got {type(settings).__name__}')
        self.settings = settings if settings is not None else FusionSettings()
        if not (0 <= self.num_queries <= 1024 and self.h * self.w <= 1024 * 1024 and self.voxel > 0.0):
            raise ValueError('FootprintFusion: num_queries <= 1024, at most 2^20 cells and voxel_size > 0 expected')
        if ops.fusion_store_size(self.h, self.w) > 8192:
            raise ValueError(f'FootprintFusion: a {self.h} x {self.w} grid needs a store wider than 8192 cells')
        self.device = torch.device(device)
        self.reset()

    def reset(self) -> None:
        """A fresh sequence: an empty store, and the next pose becomes the world frame."""
        self.state = ops.FusionState.fresh(self.h, self.w, self.device)
        self._origin: Optional[np.ndarray] = None

    def transforms(self, b: int, poses=None, world_from_cur=None):
        """→ (world_from_cur, cur_from_world), both (b, 2, 3) f64 on the host: from ``poses`` (b, 4, 4) f64 sensor poses —
        ``prev_from_cur_2d(origin, pose)`` with the first pose after :meth:`reset` as the origin, which is remembered — or
        from ``world_from_cur`` itself; with neither the sensor stands still.  The inverses are taken on the host in f64."""
        if world_from_cur is not None:
            if torch.is_tensor(world_from_cur):
                world_from_cur = world_from_cur.detach().cpu().numpy()
            m = np.array(np.asarray(world_from_cur, dtype=np.float64).reshape(b, 2, 3))
        elif poses is None:
            m = np.tile(_IDENTITY, (b, 1, 1))
        else:
            poses = np.asarray(poses, dtype=np.float64).reshape(b, 4, 4)
            if self._origin is None and b > 0:
                self._origin = poses[0].copy()
            m = np.stack([prev_from_cur_2d(self._origin, p) for p in poses]) if b else np.zeros((0, 2, 3))
        with np.errstate(all='ignore'):
            n = np.stack([_inverse_or_nan(x) for x in m]) if b else np.zeros((0, 2, 3))
        return m, n

    @torch.no_grad()
    def update(self, pred_or_instance_maps, query_track, poses=None, world_from_cur=None, visibility=None, query_velocity=None):
        """``pred_or_instance_maps``: a ``Predictions`` or its (B, ny, nx) int32 ``instance_map`` — B CONSECUTIVE frames;
        ``query_track`` (B, Q) int32 of the tracker for the same frames.  ``poses`` (B, 4, 4) f64 sensor poses on the host, or
        ``world_from_cur`` (B, 2, 3) f64; with neither, the sensor stands still.  ``visibility`` (B, ny, nx) uint8, K38a's;
        ``query_velocity`` (B, Q, 2) f64, K37's (used with ``settings.static_speed`` only).  Returns ``ops.FusedFrames``:
        ``ids`` and ``queries`` (B, ny, nx) int32 on the device.  No host synchronisation (a ``world_from_cur`` given as a
        device tensor is copied to the host for its inverse)."""
        maps = getattr(pred_or_instance_maps, 'instance_map', pred_or_instance_maps)
        if maps is None:
            raise MaskBevHipError('FootprintFusion.update: these predictions were made without an instance map')
        if maps.dim() != 3 or tuple(maps.shape[1:]) != (self.h, self.w):
            raise MaskBevHipError(f'FootprintFusion.update: (B, {self.h}, {self.w}) instance maps expected, got {tuple(maps.shape)}')
        if query_track.dim() != 2 or tuple(query_track.shape) != (int(maps.shape[0]), self.num_queries):
            raise MaskBevHipError(f'FootprintFusion.update: query_track ({int(maps.shape[0])}, {self.num_queries}) expected, got '
                                  f'{tuple(query_track.shape)}')
        m, n = self.transforms(int(maps.shape[0]), poses, world_from_cur)
        m, n = (torch.from_numpy(np.ascontiguousarray(x)).to(self.device, non_blocking=True) for x in (m, n))
        return ops.fuse_frames(maps, query_track, m, n, self.state, self.x_lo, self.y_lo, self.voxel, self.settings,
                               visibility=visibility, query_velocity=query_velocity)


def _inverse_or_nan(m) -> np.ndarray:
    """``cur_from_prev_2d``, with NaN for a map that has no inverse (K39a then takes the frame as invalid)."""
    if not np.all(np.isfinite(m)):
        return np.full((2, 3), np.nan)
    try:
        return cur_from_prev_2d(m)
    except np.linalg.LinAlgError:
        return np.full((2, 3), np.nan)


__all__ = ['InstanceTracker', 'MotionSettings', 'OcclusionSettings', 'FusionSettings', 'FootprintFusion', 'prev_from_cur_2d',
           'cur_from_prev_2d', 'velodyne_poses']
