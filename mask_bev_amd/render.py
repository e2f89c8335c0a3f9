"""BEV frames of scans, predicted instances, tracks and boxes (K36): the settings, the colour tables, the way from metre boxes
to the half-pixel corners ``ops.render_bev`` draws, and a PNG writer that needs nothing beyond the standard library.

The picture itself is composed on the device (csrc/render.hip); what leaves it is one (H, W, 3) uint8 array per frame.  Not
covered: the reference's OpenGL 3-D viewer and its per-query logit heat maps (``normalize_img``, ``sigmoid_img``).
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import MaskBevHipError

_MASK32 = 0xffffffff


def _mix32(x: int) -> int:
    """An integer finaliser (xor-shift-multiply): every input bit reaches every output bit."""
    x &= _MASK32
    x ^= x >> 16
    x = (x * 0x7feb352d) & _MASK32
    x ^= x >> 15
    x = (x * 0x846ca68b) & _MASK32
    x ^= x >> 16
    return x


def _hue_rgb(hue: int, hi: int, lo: int) -> Tuple[int, int, int]:
    """The colour wheel in 6 x 256 integer steps between the channel values ``lo`` and ``hi``."""
    sector, f = divmod(hue % 1536, 256)
    up = lo + (hi - lo) * f // 255
    down = hi - (hi - lo) * f // 255
    return ((hi, up, lo), (down, hi, lo), (lo, hi, up), (lo, down, hi), (up, lo, hi), (hi, lo, down))[sector]


def instance_palette(n: int, seed: int = 0) -> np.ndarray:
    """``n`` distinct mid-bright colours, (n, 3) uint8, from integer arithmetic alone: entry i takes the hue ``start + 949 i``
    of a 1536-step wheel (949 / 1536 is close to the golden ratio and coprime to it, so neighbours in i are far apart in
    hue), its brightest channel in 176 .. 239 and its darkest in 48 .. 79 from a hash of (i, seed).  A colour that an earlier
    entry already has moves on along the wheel, so no two entries are equal (n <= 4096).  The same (n, seed) gives the same
    table on every machine; the first entries do not depend on n."""
    n = int(n)
    if not 1 <= n <= 4096:
        raise ValueError(f'instance_palette: n {n} outside 1 .. 4096')
    start = _mix32(2 * int(seed) + 1) % 1536
    out, seen = np.zeros((n, 3), dtype=np.uint8), set()
    for i in range(n):
        h = _mix32(i ^ _mix32(int(seed) + 0x9e3779b9))
        hi, lo = 176 + (h & 63), 48 + ((h >> 8) & 31)
        hue = start + 949 * i
        rgb = _hue_rgb(hue, hi, lo)
        while rgb in seen:
            hue += 1
            rgb = _hue_rgb(hue, hi, lo)
        seen.add(rgb)
        out[i] = rgb
    return out


def default_density_lut() -> Tuple[Tuple[int, int, int], ...]:
    """Level 0 (an empty cell) black, level k grey 17 k: 1 return 17, 2 - 3 returns 34, .. 16384 and more returns 255."""
    return tuple((17 * k, 17 * k, 17 * k) for k in range(16))


@dataclass
class RenderSettings:
    """How :meth:`~mask_bev_amd.predict.Predictions.render` draws.  ``scale``: pixels per BEV cell along each axis (1 .. 8);
    ``alpha``: weight of an instance colour over the density, 0 .. 256; ``line``: thickness of the box outlines in half-pixels
    (1 .. 32); ``density_lut``: 16 colours for min(bit_length(returns in the cell), 15); ``palette_size`` and ``palette_seed``:
    :func:`instance_palette`; ``untracked_rgb``: a query the tracker gave no id; ``gt_rgb``: the ground-truth contour;
    ``box_rgb`` / ``gt_box_rgb``: predicted and label boxes; ``gt_background``: the value of ``gt_maps`` that has no contour;
    ``flip_rows``: y up (image row 0 is the grid's last y-cell) instead of the array order."""
    scale: int = 2
    alpha: int = 128
    line: int = 2
    density_lut: Sequence[Tuple[int, int, int]] = field(default_factory=default_density_lut)
    palette_size: int = 256
    palette_seed: int = 0
    untracked_rgb: Tuple[int, int, int] = (128, 128, 128)
    gt_rgb: Tuple[int, int, int] = (255, 255, 255)
    box_rgb: Tuple[int, int, int] = (255, 64, 64)
    gt_box_rgb: Tuple[int, int, int] = (64, 255, 64)
    gt_background: int = 0
    flip_rows: bool = False

    def __post_init__(self):
        self._tables = {}
        lut = np.asarray(self.density_lut)
        if lut.shape != (16, 3) or lut.min() < 0 or lut.max() > 255:
            raise ValueError('RenderSettings: density_lut must be 16 colours of three integers in 0 .. 255')
        if not 1 <= int(self.scale) <= ops.MAX_RENDER_SCALE or not 0 <= int(self.alpha) <= 256 \
                or not 1 <= int(self.line) <= ops.MAX_RENDER_LINE:
            raise ValueError(f'RenderSettings: scale {self.scale} (1 .. {ops.MAX_RENDER_SCALE}), alpha {self.alpha} (0 .. 256) or '
                             f'line {self.line} (1 .. {ops.MAX_RENDER_LINE}) out of range')

    def tables(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(density_lut (16, 3), palette (palette_size, 3))`` uint8 on ``device``, uploaded once per device."""
        device = torch.device(device)
        if device not in self._tables:
            lut = torch.from_numpy(np.asarray(self.density_lut, dtype=np.uint8).reshape(16, 3).copy())
            pal = torch.from_numpy(instance_palette(self.palette_size, self.palette_seed))
            self._tables[device] = (lut.to(device), pal.to(device))
        return self._tables[device]


def box_corners(boxes, x_range, y_range, nx: int, ny: int, scale: int) -> np.ndarray:
    """``boxes`` (n, 5) [x, y, l, w, yaw] or (n, 7) [x, y, z, l, w, h, yaw] in metres (an array, or a tensor anywhere) → (n, 4, 2)
    int32 corners (x, y) in HALF-PIXEL units of an image with ``scale`` pixels per cell, in f64: the corners are
    ``rasterize.box_vertices``' — centre ± l / 2 along (cos yaw, sin yaw) ± w / 2 along the normal, in that order around the box —
    mapped to cell coordinates ``c = (p - lo) / (hi - lo) * n`` (cell i covers [i, i + 1), so does pixel i of i * scale), then
    ``floor(2 * scale * c + 0.5)``: the centre of pixel px is 2 px + 1.  A non-finite entry raises ``ValueError``; a corner far
    outside is clipped to ±2^30 (``ops.render_bev`` skips and counts a box beyond ±16384)."""
    if torch.is_tensor(boxes):
        boxes = boxes.detach().cpu().numpy()
    b = np.asarray(boxes, dtype=np.float64)
    b = b.reshape(-1, b.shape[-1] if b.ndim == 2 else 5)
    if b.shape[1] not in (5, 7):
        raise ValueError(f'box_corners: (n, 5) or (n, 7) boxes expected, got {b.shape}')
    if not np.all(np.isfinite(b)):
        raise ValueError('box_corners: a box has a non-finite entry')
    x, y, yaw = b[:, 0], b[:, 1], b[:, -1]
    l, w = (b[:, 2], b[:, 3]) if b.shape[1] == 5 else (b[:, 3], b[:, 4])
    c, s = np.cos(yaw), np.sin(yaw)
    sl = np.array([1.0, -1.0, -1.0, 1.0])[None, :] * (l / 2)[:, None]
    sw = np.array([1.0, 1.0, -1.0, -1.0])[None, :] * (w / 2)[:, None]
    px = x[:, None] + sl * c[:, None] - sw * s[:, None]
    py = y[:, None] + sl * s[:, None] + sw * c[:, None]
    cx = (px - float(x_range[0])) / (float(x_range[1]) - float(x_range[0])) * int(nx)
    cy = (py - float(y_range[0])) / (float(y_range[1]) - float(y_range[0])) * int(ny)
    half = np.floor(2.0 * int(scale) * np.stack([cx, cy], axis=-1) + 0.5)
    if not np.all(np.isfinite(half)):
        raise ValueError('box_corners: an empty range')
    return np.clip(half, -2.0 ** 30, 2.0 ** 30).astype(np.int32)


# ---- PNG ---------------------------------------------------------------------------------------------------------------------

_PNG_MAGIC = b'\x89PNG\r\n\x1a\n'


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & _MASK32)


def png_bytes(image) -> bytes:
    """An (H, W, 3) uint8 image (an array, or a tensor anywhere) as an 8-bit RGB PNG: filter type 0 on every row, one IDAT
    chunk, zlib level 6.  The same image gives the same bytes."""
    if torch.is_tensor(image):
        image = image.detach().cpu().numpy()
    a = np.ascontiguousarray(image)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'write_png: an (H, W, 3) uint8 image expected, got {a.shape} {a.dtype}')
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)                # a filter byte (0: none) in front of every row
    rows[:, 1:] = a.reshape(h, 3 * w)
    return (_PNG_MAGIC + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
            + _chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + _chunk(b'IEND', b''))


def write_png(path, image) -> None:
    """:func:`png_bytes` of ``image`` written to ``path``.  Copies a device tensor to the host."""
    with open(str(path), 'wb') as f:
        f.write(png_bytes(image))


def read_png(path) -> np.ndarray:
    """The (H, W, 3) uint8 image of a file :func:`write_png` made (8-bit RGB, no interlace, filter type 0 on every row);
    anything else raises ``ValueError``.  Checks every chunk's CRC."""
    with open(str(path), 'rb') as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f'read_png: {path} is not a PNG file')
    pos, header, idat, ended = 8, None, [], False
    while pos + 12 <= len(data) and not ended:
        n, = struct.unpack('>I', data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n]) if pos + 12 + n <= len(data) else (None,)
        if len(body) != n or crc != (zlib.crc32(kind + body) & _MASK32):
            raise ValueError(f'read_png: {path} has a damaged {kind!r} chunk')
        if kind == b'IHDR':
            header = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            ended = True
        pos += 12 + n
    if header is None or not ended or header[2:] != (8, 2, 0, 0, 0):
        raise ValueError(f'read_png: {path} is not an 8-bit RGB PNG without interlace')
    w, h = header[:2]
    raw = np.frombuffer(zlib.decompress(b''.join(idat)), dtype=np.uint8)
    if raw.size != h * (1 + 3 * w):
        raise ValueError(f'read_png: {path} holds {raw.size} bytes for a {h}x{w} image')
    rows = raw.reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError(f'read_png: {path} uses row filters; only files of write_png are read')
    return rows[:, 1:].reshape(h, w, 3).copy()


# ---- Predictions.render ------------------------------------------------------------------------------------------------------

def _ranges(ranges):
    """``ranges``: (x_range, y_range) [, voxel_size], or anything with ``x_range`` and ``y_range`` (a rasteriser)."""
    if ranges is None:
        raise ValueError('render: boxes need ranges=(x_range, y_range) or a rasteriser')
    if hasattr(ranges, 'x_range'):
        return tuple(ranges.x_range), tuple(ranges.y_range)
    return tuple(ranges[0]), tuple(ranges[1])


def render_predictions(pred, settings: Optional[RenderSettings] = None, scans=None, module=None, query_track=None,
                       gt_maps=None, boxes=None, gt_boxes=None, ranges=None, return_skipped: bool = False):
    """:meth:`mask_bev_amd.predict.Predictions.render` (documented there)."""
    if pred.instance_map is None:
        raise MaskBevHipError('render: these predictions were made without an instance map')
    s = settings if settings is not None else RenderSettings()
    imap = pred.instance_map
    dev = imap.device
    batch, ny, nx = (int(v) for v in imap.shape)
    num_queries = int(pred.labels.shape[1])
    lut, palette = s.tables(dev)
    counts = None
    if scans is not None:
        if module is None:
            raise ValueError('render: scans need the module (or its VoxelGeometry) they were voxelised with')
        from .predict import voxel_geometry
        if len(scans) != batch:
            raise MaskBevHipError(f'render: {len(scans)} scans for predictions of {batch}')
        counts = ops.cell_counts(scans, voxel_geometry(module))
        if tuple(counts.shape) != (batch, ny, nx):
            raise MaskBevHipError(f'render: the geometry makes a {tuple(counts.shape[1:])} grid, the instance map is {ny}x{nx}')
    if query_track is not None:
        if tuple(query_track.shape) != (batch, num_queries):
            raise MaskBevHipError(f'render: query_track must be ({batch}, {num_queries}), got {tuple(query_track.shape)}')
        query_track = query_track.to(device=dev, dtype=torch.int32)
    if gt_maps is not None:
        if not torch.is_tensor(gt_maps) or tuple(gt_maps.shape) != (batch, ny, nx) or gt_maps.dtype.is_floating_point:
            raise MaskBevHipError(f'render: gt_maps must be an integer ({batch}, {ny}, {nx}) map (B, ny, nx) — a rasteriser\'s '
                                  f'(B, nx, ny) map: .permute(0, 2, 1)')
        gt_maps = gt_maps.to(device=dev, dtype=torch.int32)
    per_scan = [[] for _ in range(batch)]                         # (corners (k, 4, 2), rgb) in drawing order
    if gt_boxes is not None:
        if len(gt_boxes) != batch:
            raise ValueError(f'render: one array of label boxes per scan expected, got {len(gt_boxes)} for {batch}')
        xr, yr = _ranges(ranges)
        for b, rows in enumerate(gt_boxes):
            c = box_corners(np.asarray(rows.detach().cpu() if torch.is_tensor(rows) else rows, dtype=np.float64).reshape(-1, 7),
                            xr, yr, nx, ny, s.scale)
            per_scan[b].append((c, s.gt_box_rgb))
    if boxes is not None:
        if boxes != 'pred':
            raise ValueError(f"render: boxes must be None or 'pred', got {boxes!r}")
        xr, yr = _ranges(ranges)
        vs = ranges.voxel_size if hasattr(ranges, 'voxel_size') else (ranges[2] if len(ranges) > 2 else
                                                                      (float(xr[1]) - float(xr[0])) / nx)
        out = pred.boxes(xr, yr, vs)
        rows, scan = out['boxes'].cpu().numpy(), out['scan'].cpu().numpy()
        for b in range(batch):
            per_scan[b].append((box_corners(rows[scan == b], xr, yr, nx, ny, s.scale), s.box_rgb))
    extra = {}
    if any(len(c) for parts in per_scan for c, _ in parts):
        corners = np.concatenate([c for parts in per_scan for c, _ in parts])
        rgb = np.concatenate([np.tile(np.asarray(col, dtype=np.uint8), (len(c), 1)) for parts in per_scan for c, col in parts])
        offsets = np.concatenate([[0], np.cumsum([sum(len(c) for c, _ in parts) for parts in per_scan])]).astype(np.int32)
        extra = dict(box_corners=torch.from_numpy(corners).to(dev, non_blocking=True),
                     box_rgb=torch.from_numpy(rgb).to(dev, non_blocking=True),
                     box_offsets=torch.from_numpy(offsets).to(dev, non_blocking=True))
    image, skipped = ops.render_bev(batch, (ny, nx), dev, scale=s.scale, flip_rows=s.flip_rows, counts=counts, density_lut=lut,
                                    instance_map=imap, num_queries=num_queries, id_table=query_track, palette=palette,
                                    alpha=s.alpha, untracked_rgb=s.untracked_rgb, gt_map=gt_maps,
                                    gt_background=s.gt_background, gt_rgb=s.gt_rgb, line=s.line, **extra)
    return (image, skipped) if return_skipped else image


__all__ = ['RenderSettings', 'instance_palette', 'default_density_lut', 'box_corners', 'png_bytes', 'write_png', 'read_png',
           'render_predictions']
