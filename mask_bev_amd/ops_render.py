"""K36 — BEV frames composed on the device (csrc/render.hip): K36a the returns per BEV cell of a batch of scans, with K1's cell
rule; K36b the (B, H, W, 3) uint8 picture of those counts, a predicted instance map (coloured by query or by track id), the
contour of a ground-truth map and box outlines — integer arithmetic throughout, stated in include/maskbev_hip.h (K36) and
restated as plain loops in tests/render_ref.py."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import MaskBevHipError, check
from .ops_core import _need_gpu, _ptr, _stream
from .ops_instances import _concat_scans

RENDER_BOX_CHUNK = 64          # kBoxChunk of render.hip (mbv_render_box_chunk()): the boxes K36b stages in LDS at a time
MAX_RENDER_SIDE = 4096         # pixels
MAX_RENDER_SCALE = 8
MAX_RENDER_LINE = 32           # half-pixel units
RENDER_CORNER_BOUND = 16384    # half-pixel units: a box with a corner coordinate beyond it is skipped and counted


@torch.no_grad()
def cell_counts(scans: Sequence[torch.Tensor], geom, prefilter: bool = True) -> torch.Tensor:
    """K36a: ``scans`` — the list of (N_i, 3 | 4) f32 device tensors the module takes; ``geom`` — the encoder's
    ``VoxelGeometry`` (``prefilter``: the encoder's strict range filter in front of K1, on by default as there) → ``counts``
    (B, gy, gx) int32, the points of every scan that K1's cell rule puts into each BEV cell (row = y-cell, column = x-cell: the
    layout of ``instance_map``).  Device tensors only; no host synchronisation."""
    lib = _lib.load()
    if len(scans) == 0:
        raise ValueError('cell_counts: empty batch')
    _need_gpu(*scans)
    batch, dev = len(scans), scans[0].device
    points, dim, lens, scan_offsets = _concat_scans('cell_counts', scans, dev)
    gx, gy, gz = (int(v) for v in geom.grid)
    counts = torch.empty((batch, gy, gx), dtype=torch.int32, device=dev)
    r, v = geom.pc_range, geom.voxel_size
    check(lib.mbv_cell_counts(_ptr(points), dim, sum(lens), _ptr(scan_offsets), batch, r[0], r[1], r[2], r[3], r[4], r[5],
                              v[0], v[1], v[2], gx, gy, gz, 1 if prefilter else 0, _ptr(counts), _stream()), 'mbv_cell_counts')
    return counts


def _rgb(what: str, value) -> int:
    """(r, g, b) in 0 .. 255 → r | g << 8 | b << 16."""
    c = tuple(int(v) for v in value)
    if len(c) != 3 or any(not 0 <= v <= 255 for v in c):
        raise ValueError(f'render_bev: {what} must be three integers in 0 .. 255, got {value!r}')
    return c[0] | (c[1] << 8) | (c[2] << 16)


def _table(what: str, t: Optional[torch.Tensor], dtype, shape, dev) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dtype != dtype or t.device != dev or any(
            s is not None and int(s) != int(n) for s, n in zip(shape, t.shape)) or t.dim() != len(shape):
        want = tuple('*' if s is None else s for s in shape)
        raise MaskBevHipError(f'render_bev: {what} must be a {want} {dtype} tensor on the image\'s device, got '
                              f'{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} '
                              f'{t.dtype if torch.is_tensor(t) else ""}')
    return t.contiguous()


@torch.no_grad()
def render_bev(batch: int, grid_hw: Tuple[int, int], device, scale: int = 1, flip_rows: bool = False,
               counts: Optional[torch.Tensor] = None, density_lut: Optional[torch.Tensor] = None,
               instance_map: Optional[torch.Tensor] = None, num_queries: int = 0, id_table: Optional[torch.Tensor] = None,
               palette: Optional[torch.Tensor] = None, alpha: int = 128, untracked_rgb=(128, 128, 128),
               gt_map: Optional[torch.Tensor] = None, gt_background: int = 0, gt_rgb=(255, 255, 255),
               box_corners: Optional[torch.Tensor] = None, box_rgb: Optional[torch.Tensor] = None,
               box_offsets: Optional[torch.Tensor] = None, line: int = 2) -> Tuple[torch.Tensor, torch.Tensor]:
    """K36b: the picture of ``batch`` scans on a BEV grid ``grid_hw`` = (gy, gx) at an integer ``scale`` (1 .. 8; at most 4096
    pixels a side) → ``(image (B, gy * scale, gx * scale, 3) uint8, skipped (B) int32)`` on ``device``.  Every layer is
    optional (None): ``counts`` (B, gy, gx) int32 of :func:`cell_counts` through ``density_lut`` (16, 3) uint8 (level =
    min(bit_length(count), 15); without counts the whole picture starts as ``density_lut[0]``, without the table as black);
    ``instance_map`` (B, gy, gx) int32 blended in with ``alpha`` (0 .. 256) in the colour ``palette[id % P]`` (``palette``
    (P, 3) uint8), id = the query, or ``id_table[b, q]`` ((B, num_queries) int32; a negative id gives ``untracked_rgb``);
    ``gt_map`` (B, gy, gx) int32 as a one-pixel inner contour in ``gt_rgb`` around every cell value other than
    ``gt_background``; ``box_corners`` (R, 4, 2) int32 in half-pixel units (:func:`mask_bev_amd.render.box_corners`) with
    ``box_rgb`` (R, 3) uint8 and ``box_offsets`` (B + 1) int32, outlines ``line`` half-pixels thick (1 .. 32), later rows on
    top; ``skipped[b]`` counts the scan's boxes with a corner coordinate outside ±16384, which are not drawn.  ``flip_rows``
    writes pixel row py to image row H - 1 - py.  The exact rule: include/maskbev_hip.h, K36.  Device tensors only; one launch,
    no host synchronisation."""
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise MaskBevHipError('render_bev: a ROCm device is expected (mask_bev_amd has no CPU fallback)')
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    batch, gy, gx, scale, line, alpha = int(batch), int(grid_hw[0]), int(grid_hw[1]), int(scale), int(line), int(alpha)
    num_queries = int(num_queries)
    if batch < 1 or gx < 1 or gy < 1:
        raise ValueError(f'render_bev: batch {batch} and grid {gy}x{gx} must be at least 1')
    if not 1 <= scale <= MAX_RENDER_SCALE:
        raise ValueError(f'render_bev: scale {scale} outside 1 .. {MAX_RENDER_SCALE}')
    if gx * scale > MAX_RENDER_SIDE or gy * scale > MAX_RENDER_SIDE:
        raise MaskBevHipError(f'render_bev: a {gy * scale}x{gx * scale} image is larger than {MAX_RENDER_SIDE} pixels a side')
    if not 0 <= alpha <= 256:
        raise ValueError(f'render_bev: alpha {alpha} outside 0 .. 256')
    if not 1 <= line <= MAX_RENDER_LINE:
        raise ValueError(f'render_bev: line {line} outside 1 .. {MAX_RENDER_LINE} half-pixels')
    cells = (batch, gy, gx)
    counts = _table('counts', counts, torch.int32, cells, dev)
    density_lut = _table('density_lut', density_lut, torch.uint8, (16, 3), dev)
    instance_map = _table('instance_map', instance_map, torch.int32, cells, dev)
    id_table = _table('id_table', id_table, torch.int32, (batch, num_queries), dev)
    palette = _table('palette', palette, torch.uint8, (None, 3), dev)
    gt_map = _table('gt_map', gt_map, torch.int32, cells, dev)
    box_corners = _table('box_corners', box_corners, torch.int32, (None, 4, 2), dev)
    if counts is not None and density_lut is None:
        raise ValueError('render_bev: counts need a density_lut')
    if instance_map is not None and (palette is None or palette.shape[0] < 1 or num_queries < 0):
        raise ValueError('render_bev: an instance_map needs a palette of at least one colour and num_queries >= 0')
    n_boxes = 0 if box_corners is None else int(box_corners.shape[0])
    if box_corners is not None:
        box_rgb = _table('box_rgb', box_rgb, torch.uint8, (n_boxes, 3), dev)
        box_offsets = _table('box_offsets', box_offsets, torch.int32, (batch + 1,), dev)
        if box_rgb is None or box_offsets is None:
            raise ValueError('render_bev: box_corners need box_rgb and box_offsets')
    image = torch.empty((batch, gy * scale, gx * scale, 3), dtype=torch.uint8, device=dev)
    skipped = torch.empty((batch,), dtype=torch.int32, device=dev)
    check(lib.mbv_render_bev(batch, gx, gy, scale, 1 if flip_rows else 0, _ptr(counts), _ptr(density_lut), _ptr(instance_map),
                             num_queries, _ptr(id_table), _ptr(palette), 0 if palette is None else int(palette.shape[0]), alpha,
                             _rgb('untracked_rgb', untracked_rgb), _ptr(gt_map), int(gt_background), _rgb('gt_rgb', gt_rgb),
                             _ptr(box_corners) if n_boxes else None, _ptr(box_rgb) if n_boxes else None,
                             _ptr(box_offsets) if n_boxes else None, n_boxes, line, _ptr(image), _ptr(skipped), _stream()),
          'mbv_render_bev')
    return image, skipped


__all__ = ['cell_counts', 'render_bev', 'RENDER_BOX_CHUNK', 'MAX_RENDER_SIDE', 'MAX_RENDER_SCALE', 'MAX_RENDER_LINE',
           'RENDER_CORNER_BOUND']
