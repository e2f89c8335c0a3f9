"""K23 — training augmentations on the device (csrc/augment.hip): the per-point op program (K23a), order and selection by
compaction or one stable sort (K23b), the nearest-neighbour warp of cached instance maps (K23c).  The op records and their
random decisions are made by ``augment.DeviceAugmentation``; this module only hands buffers to the library."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import MaskBevHipError, check
from .ops_core import _need_gpu, _ptr, _stream, _workspace

AUGMENT_RECORD_BYTES = 656             # one scan's op record (include/maskbev_hip.h, K23)


@torch.no_grad()
def augment_points(points: torch.Tensor, scan_offsets: torch.Tensor, records: torch.Tensor, mode: int,
                   workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """points (N, 3 | 4) f32, scan_offsets (B + 1) i32, records (B * 656) u8 → (out (N, dim) f32 of which the first
    out_offsets[B] rows are written, out_offsets (B + 1) i32, out_counts (B) i32), all on the device, no sync.  ``mode`` 0: no
    point removed or moved, 1: drops only (stable compaction), 2: shuffle / decimate somewhere in the batch (stable sort)."""
    lib = _lib.load()
    _need_gpu(points, scan_offsets, records)
    if points.dim() != 2 or points.shape[1] not in (3, 4):
        raise ValueError(f'augment_points: points must be (N, 3 | 4), got {tuple(points.shape)}')
    if points.dtype != torch.float32:
        raise MaskBevHipError(f'augment_points: points must be f32, got {points.dtype}')
    n, dim = points.shape
    b = scan_offsets.numel() - 1
    if scan_offsets.dtype != torch.int32 or b < 1 or records.dtype != torch.uint8 or records.numel() != b * AUGMENT_RECORD_BYTES:
        raise MaskBevHipError('augment_points: scan_offsets (B + 1) i32 with B >= 1 and records (B * 656) u8 expected')
    points, scan_offsets, records = points.contiguous(), scan_offsets.contiguous(), records.contiguous()
    dev = points.device
    nbytes = lib.mbv_augment_workspace_bytes(n, b, mode)
    if nbytes == 0:
        raise MaskBevHipError(f'augment_points: {n} points in {b} scans, mode {mode}: not supported')
    if workspace is None:
        workspace = _workspace(nbytes, dev)
    out = torch.empty_like(points)
    out_offsets = torch.empty((b + 1,), dtype=torch.int32, device=dev)
    out_counts = torch.empty((b,), dtype=torch.int32, device=dev)
    check(lib.mbv_augment_points(_ptr(points), dim, n, _ptr(scan_offsets), b, _ptr(records), mode, _ptr(out),
                                 _ptr(out_offsets), _ptr(out_counts), _ptr(workspace), workspace.numel(), _stream()),
          'mbv_augment_points')
    return out, out_offsets, out_counts


@torch.no_grad()
def warp_instance_maps(maps: torch.Tensor, mats: torch.Tensor, cx: float, cy: float) -> torch.Tensor:
    """maps (B, nx, ny) i32, mats (B, 2, 2) f64 = every sample's composed matrix (original → augmented), (cx, cy) = the cell
    coordinate of the origin → the warped maps (B, nx, ny) i32: nearest source cell, 0 from outside the grid."""
    lib = _lib.load()
    _need_gpu(maps, mats)
    if maps.dim() != 3 or maps.dtype != torch.int32:
        raise MaskBevHipError(f'warp_instance_maps: maps must be (B, nx, ny) i32, got {tuple(maps.shape)} {maps.dtype}')
    b, nx, ny = maps.shape
    if mats.dtype != torch.float64 or mats.numel() != b * 4:
        raise MaskBevHipError('warp_instance_maps: mats (B, 2, 2) f64 expected')
    maps, mats = maps.contiguous(), mats.contiguous()
    out = torch.empty_like(maps)
    check(lib.mbv_warp_instance_maps(_ptr(maps), _ptr(mats), b, nx, ny, float(cx), float(cy), _ptr(out), _stream()),
          'mbv_warp_instance_maps')
    return out


__all__ = ['augment_points', 'warp_instance_maps', 'AUGMENT_RECORD_BYTES']
