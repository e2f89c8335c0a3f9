"""K22 — SemanticKITTI scene → instance-id map (csrc/rasterize.hip): binning of the labelled points of a scene into
per-instance bit images (K22a), close + open with a k x k square in LDS and painting (K22b).  Where two closed-and-opened
instances claim one cell the highest id wins (the reference paints in the hash order of a Python set).

K34 — the same for a whole batch on a scene bank that stays on the device (``mbv_rasterize_bank``): segments of the bank and their
transforms in, the bank read in place, maps bit-equal to K22's.

K24 — KITTI / Waymo box tables → instance-id maps (csrc/box_rasterize.hip): integer box corners in, one launch for a batch,
the fill rule of include/maskbev_hip.h; the last box in table order wins a cell, as in the reference's paint loop."""
from __future__ import annotations

import ctypes
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


BANK_CHUNK_POINTS = 2048      # bank points one workgroup of K34 bins: 256 lanes x 2 quads


def bank_chunks(seg_count, sample_seg_offsets, chunk_points: int = BANK_CHUNK_POINTS) -> np.ndarray:
    """The work list of ``mbv_rasterize_bank``: every segment cut into pieces of ``chunk_points`` points → (n_chunks, 4) i32
    rows (segment, first point inside the segment, sample, 0), in table order.  An empty segment gives no row."""
    cnt = np.asarray(seg_count, dtype=np.int64).reshape(-1)
    offs = np.asarray(sample_seg_offsets, dtype=np.int64).reshape(-1)
    per = (cnt + chunk_points - 1) // chunk_points
    seg = np.repeat(np.arange(cnt.size, dtype=np.int64), per)
    first = (np.arange(seg.size, dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)) * chunk_points
    sample = np.repeat(np.arange(offs.size - 1, dtype=np.int64), np.diff(offs))[seg]
    return np.stack([seg, first, sample, np.zeros_like(seg)], axis=1).astype(np.int32)


@torch.no_grad()
def rasterize_bank(points: torch.Tensor, inst: torch.Tensor, seg_start, seg_count, sample_seg_offsets, transforms,
                   centre_start, centre_count, x_range: Sequence[float], y_range: Sequence[float],
                   z_range: Sequence[float], voxel_size: float, nx: int, ny: int, morph_kernel_size: int = 9,
                   min_points: int = 1, max_instances: int = 1024, phases: int = 3, out: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None, chunk_points: int = BANK_CHUNK_POINTS
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """K34: ``points`` (n_bank, 3) f32 and ``inst`` (n_bank) i32, the bank on the device, read in place.  Host arrays:
    ``seg_start`` (n_seg) / ``seg_count`` (n_seg) bank ranges of the (sample, scan) pairs in table order,
    ``sample_seg_offsets`` (B + 1), ``transforms`` (n_seg, 4, 4) f64, ``centre_start`` / ``centre_count`` (B) (count < 0:
    ``remove_unseen`` off for that sample).  The tables are checked here (MBV_ERR_BAD_ARG for a range outside the bank), cut
    into chunks and uploaded in one asynchronous copy; nothing synchronises.
    → (instance_maps (B, nx, ny) i32, status (B) i32, workspace)."""
    lib = _lib.load()
    _need_gpu(points, inst)
    if (points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32 or inst.dtype != torch.int32
            or inst.dim() != 1 or inst.numel() != points.shape[0] or not points.is_contiguous() or not inst.is_contiguous()
            or points.data_ptr() % 16 or inst.data_ptr() % 16):
        raise MaskBevHipError('rasterize_bank: the bank must be contiguous, 16-byte aligned (n, 3) f32 points and (n) i32 inst')
    n_bank, dev = points.shape[0], points.device
    start = np.ascontiguousarray(seg_start, dtype=np.int64).reshape(-1)
    count = np.ascontiguousarray(seg_count, dtype=np.int32).reshape(-1)
    offs = np.asarray(sample_seg_offsets, dtype=np.int64).reshape(-1)
    tf = np.ascontiguousarray(transforms, dtype=np.float64).reshape(-1, 4, 4)
    c_start = np.ascontiguousarray(centre_start, dtype=np.int64).reshape(-1)
    c_count = np.ascontiguousarray(centre_count, dtype=np.int32).reshape(-1)
    n_seg, b = start.size, offs.size - 1
    if out is not None and (out.dtype != torch.int32 or tuple(out.shape) != (max(b, 0), nx, ny) or not out.is_contiguous()
                            or not out.is_cuda):
        raise MaskBevHipError(f'rasterize_bank: out must be a contiguous ({b}, {nx}, {ny}) i32 device tensor')
    if b == 0:
        empty = torch.empty((0,), dtype=torch.int32, device=dev)
        return (torch.empty((0, nx, ny), dtype=torch.int32, device=dev) if out is None else out), empty, empty
    seen = c_count >= 0
    if (b < 0 or count.size != n_seg or tf.shape[0] != n_seg or c_start.size != b or c_count.size != b
            or offs[0] != 0 or offs[-1] != n_seg or np.any(np.diff(offs) < 0)
            or np.any(start < 0) or np.any(count < 0) or np.any(start + count > n_bank)
            or np.any(c_start[seen] < 0) or np.any(c_start[seen] + c_count[seen] > n_bank)
            or chunk_points < 4 or chunk_points % 4):
        check(-1, 'mbv_rasterize_bank (tables: segments and centre scans must lie inside the bank, sample_seg_offsets must '
                  'ascend from 0 to the number of segments)')
    chunks = bank_chunks(count, offs, chunk_points)
    nbytes = lib.mbv_rasterize_bank_workspace_bytes(b, nx, ny, max_instances)
    if nbytes == 0:
        raise MaskBevHipError(f'rasterize_bank: {b} grids of {nx} x {ny} with {max_instances} instances are not supported')
    # one host buffer, one copy: every table at a 256-byte boundary
    parts = [start, count, tf, chunks, c_start, c_count]
    at = np.cumsum([0] + [(p.nbytes + 255) // 256 * 256 for p in parts])
    host = np.zeros(max(int(at[-1]), 256), dtype=np.uint8)
    for p, o in zip(parts, at):
        host[o:o + p.nbytes] = p.reshape(-1).view(np.uint8)
    tables = torch.from_numpy(host).to(dev, non_blocking=True)
    ptr = [ctypes.c_void_p(tables.data_ptr() + int(o)) for o in at[:-1]]
    if workspace is None:
        workspace = _workspace(nbytes, dev)
    if out is None:
        out = torch.empty((b, nx, ny), dtype=torch.int32, device=dev)
    status = torch.empty((b,), dtype=torch.int32, device=dev)
    check(lib.mbv_rasterize_bank(_ptr(points), _ptr(inst), n_bank, ptr[0], ptr[1], n_seg, ptr[2], ptr[3], len(chunks),
                                 int(chunk_points), ptr[4], ptr[5], b, float(x_range[0]), float(x_range[1]),
                                 float(y_range[0]), float(y_range[1]), float(z_range[0]), float(z_range[1]),
                                 float(voxel_size), nx, ny, morph_kernel_size, int(min_points), max_instances, phases,
                                 _ptr(out), _ptr(status), _ptr(workspace), workspace.numel(), _stream()),
          'mbv_rasterize_bank')
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


__all__ = ['rasterize_scene', 'rasterize_bank', 'bank_chunks', 'BANK_CHUNK_POINTS', 'rasterize_paint', 'rasterize_boxes']
