"""K22 — SemanticKITTI scene → instance-id map (csrc/rasterize.hip): binning of the labelled points of a scene into
per-instance bit images (K22a), close + open with a k x k square in LDS and painting (K22b).  Where two closed-and-opened
instances claim one cell the highest id wins (the reference paints in the hash order of a Python set).

K24 — KITTI / Waymo box tables → instance-id maps (csrc/box_rasterize.hip): integer box corners in, one launch for a batch,
the fill rule of include/maskbev_hip.h; the last box in table order wins a cell, as in the reference's paint loop."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import MaskBevHipError, check
from .ops_core import _need_gpu, _ptr, _stream, _workspace


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


@torch.no_grad()
def rasterize_scene(points: torch.Tensor, inst: torch.Tensor, scan_offsets: torch.Tensor, transforms: torch.Tensor,
                    centre_inst: Optional[torch.Tensor], x_range: Sequence[float], y_range: Sequence[float],
                    z_range: Sequence[float], voxel_size: float, nx: int, ny: int, morph_kernel_size: int = 9,
                    min_points: int = 1, max_instances: int = 1024, phases: int = 3,
                    out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """points (N, 3 | 4) f32 / f64, inst (N) i32, scan_offsets (S + 1) i32, transforms (S, 4, 4) f64, centre_inst (n) i32 or
    None (None = every instance with a kept point is present) → (instance_map (nx, ny) i32, status (1) i32, workspace).
    ``phases`` 1 / 2 run K22a / K22b alone on ``workspace`` (measurements)."""
    lib = _lib.load()
    _need_gpu(points, inst, scan_offsets, transforms, centre_inst)
    if points.dim() != 2 or points.shape[1] not in (3, 4) or points.dtype not in (torch.float32, torch.float64):
        raise MaskBevHipError(f'rasterize_scene: points must be (N, 3 | 4) f32 / f64, got {tuple(points.shape)} {points.dtype}')
    n, stride = points.shape
    s = scan_offsets.numel() - 1
    if (inst.dtype != torch.int32 or inst.numel() != n or scan_offsets.dtype != torch.int32 or s < 0
            or transforms.dtype != torch.float64 or tuple(transforms.shape) != (s, 4, 4)
            or (centre_inst is not None and centre_inst.dtype != torch.int32)):
        raise MaskBevHipError('rasterize_scene: inst (N) i32, scan_offsets (S + 1) i32, transforms (S, 4, 4) f64, '
                              'centre_inst i32 expected')
    dev = points.device
    points, inst = _aligned(points), _aligned(inst)
    scan_offsets, transforms = scan_offsets.contiguous(), transforms.contiguous()
    centre_inst = None if centre_inst is None else centre_inst.contiguous()
    nbytes = lib.mbv_rasterize_workspace_bytes(nx, ny, max_instances)
    if nbytes == 0:
        raise MaskBevHipError(f'rasterize_scene: grid {nx} x {ny} with {max_instances} instances is not supported')
    if workspace is None:
        workspace = _workspace(nbytes, dev)
    if out is None:
        out = torch.empty((nx, ny), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib.mbv_rasterize(_ptr(points), int(points.dtype == torch.float64), stride, _ptr(inst), n, _ptr(scan_offsets), s,
                            _ptr(transforms), _ptr(centre_inst), -1 if centre_inst is None else centre_inst.numel(),
                            float(x_range[0]), float(x_range[1]), float(y_range[0]), float(y_range[1]),
                            float(z_range[0]), float(z_range[1]), float(voxel_size), nx, ny, morph_kernel_size,
                            int(min_points), max_instances, phases, _ptr(out), _ptr(status), _ptr(workspace),
                            workspace.numel(), _stream()), 'mbv_rasterize')
    return out, status, workspace


@torch.no_grad()
def rasterize_paint(occupancy: torch.Tensor, bbox: torch.Tensor, slot_ids: torch.Tensor, n_slots: torch.Tensor, ny: int,
                    morph_kernel_size: int = 9, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K22b alone: occupancy (S, nx, ceil(ny / 32)) i32 bit images (bit b of word w of row ix = cell (ix, 32 w + b)), bbox
    (S, 4) i32 inclusive xmin, ymin, xmax, ymax of the set cells (xmax < 0: empty), slot_ids (S) i32, n_slots (1) i32 →
    instance_map (nx, ny) i32 of the closed-and-opened instances, highest id on top."""
    lib = _lib.load()
    _need_gpu(occupancy, bbox, slot_ids, n_slots)
    s, nx, wpr = occupancy.shape
    if (occupancy.dtype != torch.int32 or wpr != (ny + 31) // 32 or bbox.dtype != torch.int32
            or tuple(bbox.shape) != (s, 4) or slot_ids.dtype != torch.int32 or slot_ids.numel() != s
            or n_slots.dtype != torch.int32 or n_slots.numel() != 1):
        raise MaskBevHipError('rasterize_paint: occupancy (S, nx, ceil(ny / 32)) i32, bbox (S, 4) i32, slot_ids (S) i32, '
                              'n_slots (1) i32 expected')
    occupancy, bbox, slot_ids = occupancy.contiguous(), bbox.contiguous(), slot_ids.contiguous()
    if out is None:
        out = torch.empty((nx, ny), dtype=torch.int32, device=occupancy.device)
    check(lib.mbv_rasterize_paint(_ptr(occupancy), _ptr(bbox), _ptr(slot_ids), _ptr(n_slots), s, nx, ny,
                                  morph_kernel_size, _ptr(out), _stream()), 'mbv_rasterize_paint')
    return out


@torch.no_grad()
def rasterize_boxes(vertices: torch.Tensor, ids: torch.Tensor, frame_offsets: Union[torch.Tensor, Sequence[int]], nx: int,
                    ny: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K24: vertices (N, 4, 2) i32 cell coordinates (|c| <= 2^20), ids (N) i32, frame_offsets (B + 1) → maps (B, nx, ny) i32,
    every cell written (``out`` needs no zeroing).  ``frame_offsets`` as a host sequence is checked here (ascending from 0 to
    N) and uploaded; as a device i32 tensor it is taken as it is, and the kernel reads no row beyond its last entry."""
    lib = _lib.load()
    _need_gpu(vertices, ids)
    n = ids.numel()
    if (vertices.dtype != torch.int32 or ids.dtype != torch.int32 or vertices.numel() != n * 8
            or (n > 0 and tuple(vertices.shape[-2:]) != (4, 2))):
        raise MaskBevHipError('rasterize_boxes: vertices (N, 4, 2) i32 and ids (N) i32 expected')
    dev = vertices.device
    if isinstance(frame_offsets, torch.Tensor):
        _need_gpu(frame_offsets)
        if frame_offsets.dtype != torch.int32:
            raise MaskBevHipError('rasterize_boxes: frame_offsets must be i32')
        offs = frame_offsets.contiguous()
    else:
        host = np.asarray(frame_offsets, dtype=np.int64).reshape(-1)
        if host.size < 2 or host[0] != 0 or host[-1] != n or np.any(np.diff(host) < 0):
            raise ValueError(f'rasterize_boxes: frame_offsets must ascend from 0 to {n}, got {host.tolist()}')
        offs = torch.from_numpy(host.astype(np.int32)).to(dev, non_blocking=True)
    b = offs.numel() - 1
    if b < 1:
        raise ValueError('rasterize_boxes: empty batch')
    if n == 0:                                    # no box at all: the entry point still wants non-null tables
        vertices = torch.zeros((1, 4, 2), dtype=torch.int32, device=dev)
        ids = torch.zeros((1,), dtype=torch.int32, device=dev)
    vertices, ids = _aligned(vertices), ids.contiguous()
    if out is None:
        out = torch.empty((b, nx, ny), dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or tuple(out.shape) != (b, nx, ny) or not out.is_contiguous() or not out.is_cuda:
        raise MaskBevHipError(f'rasterize_boxes: out must be a contiguous ({b}, {nx}, {ny}) i32 device tensor')
    check(lib.mbv_rasterize_boxes(_ptr(vertices), _ptr(ids), _ptr(offs), b, int(nx), int(ny), _ptr(out), _stream()),
          'mbv_rasterize_boxes')
    return out


__all__ = ['rasterize_scene', 'rasterize_paint', 'rasterize_boxes']
