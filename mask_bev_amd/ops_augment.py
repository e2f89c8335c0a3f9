"""K23 — training augmentations on the device (csrc/augment.hip): the per-point op program (K23a), order and selection by
compaction or one stable sort (K23b), the nearest-neighbour warp of cached instance maps (K23c).  The op records and their
random decisions are made by ``augment.DeviceAugmentation``; this module only hands buffers to the library.
K28 — KITTI object augmentations (csrc/object_augment.hip): points against a host-made box table (moved, removed, joined by
pasted bank points) and the membership index ``ObjectBank.build`` cuts its samples with."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import MaskBevHipError, check
from .ops_core import _need_gpu, _ptr, _stream, _workspace

AUGMENT_RECORD_BYTES = 656             # one scan's op record (include/maskbev_hip.h, K23)
BOX_ROW = 14                           # f64 per row of K28's box table (include/maskbev_hip.h, K28)
MAX_BOXES_PER_SCAN = 128


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


def _host_offsets(offsets, what: str, total: int) -> np.ndarray:
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 2 or offsets[0] != 0 or offsets[-1] != total or (np.diff(offsets) < 0).any():
        raise ValueError(f'object_augment: {what} must ascend from 0 to {total}')
    return offsets


@torch.no_grad()
def object_augment(points: torch.Tensor, scan_offsets, box_table: torch.Tensor, box_offsets,
                   bank_points: Optional[torch.Tensor] = None, paste_segments=None, paste_offsets=None,
                   workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """points (N, 3 | 4) f32 and box_table (n_boxes, 14) f64 on the device; scan_offsets, box_offsets, paste_offsets (B + 1)
    and paste_segments (S, 2) = (first bank row, rows) on the HOST (the caller made them there); bank_points (P, 4) f32 on the
    device → (out (N + pasted rows, dim) f32 of which the first out_offsets[B] rows are written, out_offsets (B + 1) i32,
    out_counts (B) i32), all on the device, no sync.  A scan with more than 128 boxes is refused."""
    lib = _lib.load()
    _need_gpu(points, box_table, bank_points)
    if points.dim() != 2 or points.shape[1] not in (3, 4):
        raise ValueError(f'object_augment: points must be (N, 3 | 4), got {tuple(points.shape)}')
    if points.dtype != torch.float32:
        raise MaskBevHipError(f'object_augment: points must be f32, got {points.dtype}')
    if box_table.dtype != torch.float64 or box_table.dim() != 2 or box_table.shape[1] != BOX_ROW:
        raise MaskBevHipError(f'object_augment: box_table must be (n, {BOX_ROW}) f64')
    n, dim = points.shape
    scan_offsets = _host_offsets(scan_offsets, 'scan_offsets', n)
    b = scan_offsets.size - 1
    box_offsets = _host_offsets(box_offsets, 'box_offsets', box_table.shape[0])
    segments = np.zeros((0, 2), dtype=np.int32) if paste_segments is None else \
        np.ascontiguousarray(paste_segments, dtype=np.int32).reshape(-1, 2)
    paste_offsets = _host_offsets(np.zeros(b + 1) if paste_offsets is None else paste_offsets, 'paste_offsets', len(segments))
    if box_offsets.size != b + 1 or paste_offsets.size != b + 1:
        raise ValueError('object_augment: scan_offsets, box_offsets and paste_offsets must have the same length')
    n_bank = 0 if bank_points is None else int(bank_points.shape[0])
    if len(segments):
        if bank_points is None or bank_points.dim() != 2 or bank_points.shape[1] != 4 or bank_points.dtype != torch.float32:
            raise MaskBevHipError('object_augment: bank_points must be (P, 4) f32')
        if (segments < 0).any() or (segments.sum(1) > n_bank).any():
            raise ValueError('object_augment: a pasted segment leaves the bank')
        bank_points = bank_points.contiguous()
    n_paste = int(segments[:, 1].sum())
    points, box_table = points.contiguous(), box_table.contiguous()
    dev = points.device
    nbytes = lib.mbv_object_augment_workspace_bytes(n, b, len(segments))
    if nbytes == 0:
        raise MaskBevHipError(f'object_augment: {n} points in {b} scans, {len(segments)} pasted segments: not supported')
    if workspace is None:
        workspace = _workspace(nbytes, dev)
    host = np.concatenate([scan_offsets, box_offsets, paste_offsets, segments.reshape(-1)]).astype(np.int32)
    tables = torch.from_numpy(host).to(dev, non_blocking=True)                  # one upload for the four index tables
    d_scan, d_box, d_paste, d_seg = tables[:b + 1], tables[b + 1:2 * b + 2], tables[2 * b + 2:3 * b + 3], tables[3 * b + 3:]
    out = torch.empty((n + n_paste, dim), dtype=torch.float32, device=dev)
    out_offsets = torch.empty((b + 1,), dtype=torch.int32, device=dev)
    out_counts = torch.empty((b,), dtype=torch.int32, device=dev)
    check(lib.mbv_object_augment(_ptr(points), dim, n, _ptr(d_scan), b, _ptr(box_table), _ptr(d_box), box_table.shape[0],
                                 int(np.diff(box_offsets).max()), _ptr(bank_points), n_bank, _ptr(d_seg), _ptr(d_paste),
                                 len(segments), n_paste, _ptr(out), _ptr(out_offsets), _ptr(out_counts), _ptr(workspace),
                                 workspace.numel(), _stream()), 'mbv_object_augment')
    return out, out_offsets, out_counts


@torch.no_grad()
def points_in_boxes(points: torch.Tensor, box_table: torch.Tensor) -> torch.Tensor:
    """points (N, 3 | 4) f32, box_table (n, 14) f64 → (N) i32: the first row that holds the point (K28's membership rule:
    strict on every face), or -1."""
    lib = _lib.load()
    _need_gpu(points, box_table)
    if points.dim() != 2 or points.shape[1] not in (3, 4) or points.dtype != torch.float32:
        raise MaskBevHipError(f'points_in_boxes: points must be (N, 3 | 4) f32, got {tuple(points.shape)} {points.dtype}')
    if box_table.dtype != torch.float64 or box_table.dim() != 2 or box_table.shape[1] != BOX_ROW:
        raise MaskBevHipError(f'points_in_boxes: box_table must be (n, {BOX_ROW}) f64')
    points, box_table = points.contiguous(), box_table.contiguous()
    index = torch.empty((points.shape[0],), dtype=torch.int32, device=points.device)
    check(lib.mbv_points_in_boxes(_ptr(points), points.shape[1], points.shape[0], _ptr(box_table), box_table.shape[0],
                                  _ptr(index), _stream()), 'mbv_points_in_boxes')
    return index


__all__ = ['augment_points', 'warp_instance_maps', 'object_augment', 'points_in_boxes', 'AUGMENT_RECORD_BYTES', 'BOX_ROW',
           'MAX_BOXES_PER_SCAN']
