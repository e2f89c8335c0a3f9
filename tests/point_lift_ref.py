"""Plain numpy restatement of K31 (csrc/point_lift.hip) and of K26b's 3-D overlap, the yardsticks of
tests/test_k31_point_lift_gpu.py.

K31, operation by operation in float32 and integers (every intermediate is rounded to float32, as the kernel compiled
without contraction rounds it):
  cell     c = floor((p - min) / vs) per axis; rejected when c < 0 or c >= grid on any of the three axes (NaN fails every
           compare); under ``prefilter`` the strict min < p < max on all three axes first
  query    instance_map[b, cy, cx] (row = y-cell, column = x-cell); a value outside [0, num_queries) counts as -1
  extent   z_min / z_max of a query's points; with bw = (z_max - z_min) / float(z_bins) of the GEOMETRY,
           bin(z) = clamp(int(floor((z - z_min) / bw)), 0, z_bins - 1), rank(q) = clamp(int(floor(q * float(n - 1))), 0, n - 1),
           k(r) = the first bin whose cumulative count exceeds r:
           z_lo = z_min + float(k(rank(q_lo))) * bw,  z_hi = z_min + float(k(rank(q_hi)) + 1) * bw,
           each clamped into [z_min, z_max] of the query's own points; four zeros for a query without a point.

K26b in float64: ``kitti_eval_ref.rotate_iou(..., criterion=2)`` times the common z-interval, divided by the criterion's
denominator; 0 where either is empty.  Boxes are (x, y, z, dx, dy, dz, angle) with z the bottom face.
"""
import numpy as np

from tests import kitti_eval_ref as R

F = np.float32


def point_cells(points, pc_range, voxel_size, grid, prefilter):
    """points (N, >= 3) → (ok (N) bool, cx, cy (N) int64; 0 where not ok): K1's cell rule in float32."""
    p = np.asarray(points, dtype=F).reshape(-1, np.asarray(points).shape[-1])
    lo, hi, vs = np.asarray(pc_range[:3], dtype=F), np.asarray(pc_range[3:], dtype=F), np.asarray(voxel_size, dtype=F)
    ok = np.ones((p.shape[0],), dtype=bool)
    cells = []
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for a in range(3):
            x = p[:, a]
            if prefilter:
                ok &= (lo[a] < x) & (x < hi[a])
            c = np.floor(((x - lo[a]).astype(F) / vs[a]).astype(F)).astype(F)
            ok &= (c >= F(0)) & (c < F(grid[a]))
            cells.append(c)
    cx = np.where(ok, cells[0], 0).astype(np.int64)
    cy = np.where(ok, cells[1], 0).astype(np.int64)
    return ok, cx, cy


def _rank(q, n):
    r = int(np.floor(F(F(q) * F(n - 1))))
    return min(max(r, 0), n - 1)


def lift(scans, instance_map, pc_range, voxel_size, grid, num_queries, z_bins=64, quantiles=(0., 1.), prefilter=True):
    """scans: list of (N_i, 3 | 4) float32 arrays; instance_map (B, gy, gx) int → dict(point_query (sum N_i) int32, counts
    (B, Q) int32, z_extent (B, Q, 4) float32 = z_min, z_max, z_lo, z_hi)."""
    imap = np.asarray(instance_map)
    batch = len(scans)
    z0, z1 = F(pc_range[2]), F(pc_range[5])
    bw = F(F(z1 - z0) / F(z_bins))
    labels = []
    counts = np.zeros((batch, num_queries), dtype=np.int32)
    ext = np.zeros((batch, num_queries, 4), dtype=F)
    for b, pts in enumerate(scans):
        pts = np.asarray(pts, dtype=F)
        ok, cx, cy = point_cells(pts, pc_range, voxel_size, grid, prefilter)
        v = imap[b, cy, cx].astype(np.int64)
        q = np.where(ok & (v >= 0) & (v < num_queries), v, -1).astype(np.int32)
        labels.append(q)
        for k in np.unique(q[q >= 0]):
            z = pts[q == k, 2]
            n = z.shape[0]
            with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
                fb = np.floor(((z - z0).astype(F) / bw).astype(F))
            bins = np.where(fb >= F(z_bins), z_bins - 1, np.where(fb >= F(0), fb, 0)).astype(np.int64)
            cum = np.cumsum(np.bincount(bins, minlength=z_bins))
            k_lo = int(np.argmax(cum > _rank(quantiles[0], n)))
            k_hi = int(np.argmax(cum > _rank(quantiles[1], n)))
            zmin, zmax = z.min(), z.max()
            lo_edge = F(z0 + F(F(k_lo) * bw))
            hi_edge = F(z0 + F(F(k_hi + 1) * bw))
            counts[b, k] = n
            ext[b, k] = [zmin, zmax, min(max(lo_edge, zmin), zmax), min(max(hi_edge, zmin), zmax)]
    return dict(point_query=np.concatenate(labels) if labels else np.zeros((0,), dtype=np.int32), counts=counts, z_extent=ext)


def z_overlap(boxes, qboxes, dtype=np.float64):
    """(N, 7), (K, 7) → (N, K): max(0, min(z + dz) - max(z))."""
    a, b = np.asarray(boxes, dtype=dtype).reshape(-1, 7), np.asarray(qboxes, dtype=dtype).reshape(-1, 7)
    top = np.minimum((a[:, 2] + a[:, 5])[:, None], (b[:, 2] + b[:, 5])[None, :])
    bottom = np.maximum(a[:, 2][:, None], b[:, 2][None, :])
    return np.maximum(top - bottom, dtype(0))


BEV = [0, 1, 3, 4, 6]


def intersection_3d(boxes, qboxes, dtype=np.float64):
    """The intersection volumes (criterion 2) in ``dtype``."""
    a, b = np.asarray(boxes, dtype=dtype).reshape(-1, 7), np.asarray(qboxes, dtype=dtype).reshape(-1, 7)
    return (R.rotate_iou(a[:, BEV], b[:, BEV], 2, dtype) * z_overlap(a, b, dtype)).astype(dtype)


def overlap_from_intersection_3d(inter, boxes, qboxes, criterion):
    dtype = inter.dtype.type
    a, b = np.asarray(boxes, dtype=dtype).reshape(-1, 7), np.asarray(qboxes, dtype=dtype).reshape(-1, 7)
    vol_a, vol_b = np.abs(a[:, 3] * a[:, 4] * a[:, 5])[:, None], np.abs(b[:, 3] * b[:, 4] * b[:, 5])[None, :]
    den = {-1: vol_a + vol_b - inter, 0: vol_a + 0 * inter, 1: vol_b + 0 * inter, 2: np.ones_like(inter)}[criterion]
    out = np.zeros_like(inter)
    np.divide(inter, den, out=out, where=inter > 0)
    return out


def rotate_iou_3d(boxes, qboxes, criterion=-1, dtype=np.float64):
    """(N, 7), (K, 7) → (N, K) in ``dtype``."""
    return overlap_from_intersection_3d(intersection_3d(boxes, qboxes, dtype), boxes, qboxes, criterion)
