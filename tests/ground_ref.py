"""Plain numpy restatement of K35 (csrc/point_lift.hip), written from the words of include/maskbev_hip.h, the yardstick of
tests/test_k35_ground_lift_gpu.py.  float32 and integers only.

K35a  a point takes part iff K1's cell rule accepts it (``point_lift_ref.point_cells``) and z >= z_floor;
      cell_min[b, cy, cx] = the minimum z of the cell's points, +inf without one;
      ground[b, cy, cx]   = the minimum of cell_min over cy' in [max(0, cy - r), min(gy - 1, cy + r)], cx' likewise.
      Every minimum is an unsigned-integer minimum on the order-preserving encoding (negative floats: all bits flipped;
      others: the sign bit set), so -0.0 < +0.0.
K35b  q as in K31; with g = ground[b, cy, cx] the point keeps q iff z > g + clearance and z <= g + max_height (one rounded f32
      add each); counts and the four z columns are K31's over the kept points; z_ground[b, q] = the minimum of g over them,
      0 without one.
"""
import numpy as np

from tests import point_lift_ref as L

F = np.float32
ENC_INF = np.uint32(0xff800000)              # encode(+inf)


def encode(z):
    u = np.ascontiguousarray(z, dtype=F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def decode(e):
    e = np.ascontiguousarray(e, dtype=np.uint32)
    return np.where(e & np.uint32(0x80000000), e & np.uint32(0x7fffffff), ~e).astype(np.uint32).view(F)


def participating(points, pc_range, voxel_size, grid, prefilter, z_floor):
    """(N, >= 3) → (ok (N) bool, cx, cy (N) int64): the cell rule and the floor."""
    pts = np.asarray(points, dtype=F)
    ok, cx, cy = L.point_cells(pts, pc_range, voxel_size, grid, prefilter)
    with np.errstate(invalid='ignore'):
        ok = ok & (pts[:, 2] >= F(z_floor))
    return ok, cx, cy


def cell_minima(scans, pc_range, voxel_size, grid, prefilter=True, z_floor=-np.inf):
    """list of (N_i, 3 | 4) → (B, gy, gx) uint32, the encoded cell minima."""
    enc = np.full((len(scans), grid[1], grid[0]), ENC_INF, dtype=np.uint32)
    for b, pts in enumerate(scans):
        pts = np.asarray(pts, dtype=F)
        ok, cx, cy = participating(pts, pc_range, voxel_size, grid, prefilter, z_floor)
        np.minimum.at(enc[b], (cy[ok], cx[ok]), encode(pts[ok, 2]))
    return enc


def window_min(enc, radius):
    """(..., gy, gx) uint32 → the minimum over the clipped (2 radius + 1)^2 window, by shifted views along x, then y."""
    out = np.array(enc, dtype=np.uint32, copy=True)
    for axis in (-1, -2):
        src = np.moveaxis(out.copy(), axis, -1)
        dst = src.copy()
        n = src.shape[-1]
        for d in range(1, min(int(radius), n - 1) + 1):
            dst[..., d:] = np.minimum(dst[..., d:], src[..., :n - d])
            dst[..., :n - d] = np.minimum(dst[..., :n - d], src[..., d:])
        out = np.moveaxis(dst, -1, axis)
    return np.ascontiguousarray(out)


def window_min_brute(enc, radius):
    """The same cell by cell, as the header words it; (gy, gx) uint32."""
    gy, gx = enc.shape
    out = np.empty_like(enc)
    for cy in range(gy):
        for cx in range(gx):
            m = int(ENC_INF)
            for y in range(max(0, cy - radius), min(gy - 1, cy + radius) + 1):
                for x in range(max(0, cx - radius), min(gx - 1, cx + radius) + 1):
                    m = min(m, int(enc[y, x]))
            out[cy, cx] = m
    return out


def ground_map(scans, pc_range, voxel_size, grid, radius, z_floor=-np.inf, prefilter=True):
    """→ dict(cell_min, ground), both (B, gy, gx) float32."""
    enc = cell_minima(scans, pc_range, voxel_size, grid, prefilter, z_floor)
    return dict(cell_min=decode(enc), ground=decode(window_min(enc, radius)))


def lift_ground(scans, instance_map, ground, pc_range, voxel_size, grid, num_queries, clearance=0.3, max_height=np.inf,
                z_bins=64, quantiles=(0., 1.), prefilter=True):
    """→ dict(point_query (sum N_i) int32, counts (B, Q) int32, z_extent (B, Q, 4) f32, z_ground (B, Q) f32)."""
    imap, gmap = np.asarray(instance_map), np.asarray(ground, dtype=F)
    batch = len(scans)
    labels, kept_scans = [], []
    z_ground = np.zeros((batch, num_queries), dtype=F)
    for b, pts in enumerate(scans):
        pts = np.asarray(pts, dtype=F)
        ok, cx, cy = L.point_cells(pts, pc_range, voxel_size, grid, prefilter)
        v = imap[b, cy, cx].astype(np.int64)
        q = np.where(ok & (v >= 0) & (v < num_queries), v, -1).astype(np.int32)
        g, z = gmap[b, cy, cx], pts[:, 2]
        with np.errstate(invalid='ignore', over='ignore'):
            keep = (z > (g + F(clearance)).astype(F)) & (z <= (g + F(max_height)).astype(F))
        q = np.where(keep, q, -1).astype(np.int32)
        labels.append(q)
        kept_scans.append(pts[q >= 0])
        for k in np.unique(q[q >= 0]):
            z_ground[b, k] = decode(encode(g[q == k]).min(keepdims=True))[0]
    # K31's counts and z columns over the kept points alone: their cells, hence their queries, are unchanged
    ref = L.lift(kept_scans, imap, pc_range, voxel_size, grid, num_queries, z_bins, quantiles, prefilter)
    for b in range(batch):
        assert np.array_equal(ref['point_query'][sum(s.shape[0] for s in kept_scans[:b]):][:kept_scans[b].shape[0]],
                              labels[b][labels[b] >= 0])
    return dict(point_query=np.concatenate(labels) if labels else np.zeros((0,), dtype=np.int32), counts=ref['counts'],
                z_extent=ref['z_extent'], z_ground=z_ground)
