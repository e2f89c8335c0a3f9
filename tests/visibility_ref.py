"""K38a restated: the BEV visibility map of a scan, from the words of include/maskbev_hip.h — the yardstick of
tests/test_k38_visibility_gpu.py.  `visibility_map` is the numpy version (the targets are K35a's encoded cell minima of
tests/ground_ref.py, every ray a vector over k in int64 and float32); `plain_visibility` restates the rule independently in
plain loops: Python ints for the line, `np.float32` scalars for the height test, the lowest return of a cell by comparing
the encoded integers one point at a time.  tests/test_visibility_cpu.py holds them against each other.  Nothing here imports
the package."""
import numpy as np

from tests import ground_ref as G
from tests import point_lift_ref as L

F = np.float32
PASSED, HIT = 1, 2


def origin_cell(pc_range, voxel_size, origin):
    """(cx, cy) of the sensor: K1's arithmetic in f32, a separate subtraction and division, without the range rejection."""
    cx = np.floor((F(origin[0]) - F(pc_range[0])) / F(voxel_size[0]))
    cy = np.floor((F(origin[1]) - F(pc_range[1])) / F(voxel_size[1]))
    return int(cx), int(cy)


def visibility_map(scans, pc_range, voxel_size, grid, origin_cx, origin_cy, origin_z, z_top, prefilter=True):
    """list of (N_i, 3 | 4) → (B, gy, gx) uint8."""
    gx, gy = int(grid[0]), int(grid[1])
    enc = G.cell_minima(scans, pc_range, voxel_size, grid, prefilter)
    z_end = G.decode(enc)
    vis = np.zeros((len(scans), gy, gx), np.uint8)
    oz, zt = F(origin_z), F(z_top)
    for b in range(len(scans)):
        tys, txs = np.nonzero(enc[b] != G.ENC_INF)
        passed = np.zeros((gy, gx), bool)
        for ty, tx in zip(tys.tolist(), txs.tolist()):
            dx, dy = tx - origin_cx, ty - origin_cy
            n = max(abs(dx), abs(dy))
            if n == 0:
                continue
            k = np.arange(n, dtype=np.int64)
            cy = origin_cy + (2 * k * dy + n) // (2 * n)
            cx = origin_cx + (2 * k * dx + n) // (2 * n)
            with np.errstate(all='ignore'):
                lhs = ((z_end[b, ty, tx] - oz).astype(F) * k.astype(F)).astype(F)
                rhs = F(F(zt - oz) * F(n))
                ok = (lhs <= rhs) & (cx >= 0) & (cx < gx) & (cy >= 0) & (cy < gy)
            passed[cy[ok], cx[ok]] = True
        vis[b] = passed.astype(np.uint8) * PASSED | (enc[b] != G.ENC_INF).astype(np.uint8) * HIT
    return vis


def _enc_int(z):
    u = int(np.array(z, dtype=F).view(np.uint32))
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


def plain_visibility(points, pc_range, voxel_size, grid, origin_cx, origin_cy, origin_z, z_top, prefilter=True):
    """One scan in plain loops → (gy, gx) uint8."""
    gx, gy = int(grid[0]), int(grid[1])
    pts = np.asarray(points, dtype=F)
    ok, cxs, cys = L.point_cells(pts, pc_range, voxel_size, grid, prefilter) if len(pts) else ((), (), ())
    lowest = {}                                                    # (ty, tx) → (encoded z, z)
    for i in range(len(pts)):
        if not ok[i]:
            continue
        key, e = (int(cys[i]), int(cxs[i])), _enc_int(pts[i, 2])
        if key not in lowest or e < lowest[key][0]:
            lowest[key] = (e, F(pts[i, 2]))
    vis = [[0] * gx for _ in range(gy)]
    oz, zt = F(origin_z), F(z_top)
    with np.errstate(all='ignore'):
        for (ty, tx), (_, z_end) in lowest.items():
            vis[ty][tx] |= HIT
            dx, dy = tx - origin_cx, ty - origin_cy
            n = max(abs(dx), abs(dy))
            rise, rhs = F(z_end - oz), F(F(zt - oz) * F(n))
            for k in range(n):
                cy = origin_cy + (2 * k * dy + n) // (2 * n)       # Python's // rounds towards minus infinity
                cx = origin_cx + (2 * k * dx + n) // (2 * n)
                if not (0 <= cx < gx and 0 <= cy < gy):
                    continue
                if F(rise * F(k)) <= rhs:
                    vis[cy][cx] |= PASSED
    return np.array(vis, np.uint8).reshape(gy, gx)


# ---- scenes -------------------------------------------------------------------------------------------------------------------

# 53 (x) by 37 (y) cells of 0.5 m, one z cell of 4 m: a 37 x 53 map
RANGE, VOXEL, GRID = [-10.0, -8.0, -3.0, 16.5, 10.5, 1.0], [0.5, 0.5, 4.0], [53, 37, 1]
ORIGINS = dict(inside=(0.2, 0.3, 0.0), edge=(-9.9, 3.3, 0.0), outside=(-14.0, -11.0, 0.0))


def cell_centre(cx, cy, z, pc_range=RANGE, voxel=VOXEL):
    return [pc_range[0] + (cx + 0.5) * voxel[0], pc_range[1] + (cy + 0.5) * voxel[1], z, 0.5]


def scripted_scans(origin, dim=4, seed=38):
    """Three scans on the 37 x 53 grid, the second empty.  Scan 0: targets in all eight octants of the origin's cell, on both
    axes and on the four exact diagonals, one in the origin's own cell (when that lies in the grid), two returns in one cell
    with different z, a -0.0 / +0.0 pair, NaN coordinates, points outside the range and on its border.  Scan 2: random."""
    ocx, ocy = origin_cell(RANGE, VOXEL, origin)
    rng = np.random.default_rng(seed)
    pts = []
    for dx, dy in ((9, 0), (-9, 0), (0, 7), (0, -7), (6, 6), (-6, 6), (6, -6), (-6, -6),          # axes and diagonals
                   (11, 4), (4, 11), (-4, 11), (-11, 4), (-11, -4), (-4, -11), (4, -11), (11, -4),  # the eight octants
                   (17, 5), (3, 2), (-2, 1), (25, -13), (40, 20), (50, 30), (30, 36), (1, 0), (0, 0)):
        cx, cy = ocx + dx, ocy + dy
        if 0 <= cx < GRID[0] and 0 <= cy < GRID[1]:
            pts.append(cell_centre(cx, cy, float(rng.uniform(-2.0, -0.5))))
    a, b = (20, 9), (33, 30)
    pts += [cell_centre(*a, -1.0), cell_centre(*a, -1.75), cell_centre(*a, -0.25)]                  # the lowest of three
    pts += [cell_centre(*b, 0.0), cell_centre(*b, -0.0), cell_centre(*b, 0.0)]                      # -0.0 is the minimum
    pts += [[np.nan, 1.0, -1.0, 0.1], [1.0, np.nan, -1.0, 0.1], [1.0, 1.0, np.nan, 0.1], [np.inf, 1.0, -1.0, 0.1]]
    pts += [[-10.0, 0.0, -1.0, 0.1], [16.5, 0.0, -1.0, 0.1], [0.0, 10.5, -1.0, 0.1], [0.0, 0.0, 1.0, 0.1], [0.0, 0.0, -3.0, 0.1],
            [40.0, 0.0, -1.0, 0.1], [0.0, -30.0, -1.0, 0.1], [0.0, 0.0, 5.0, 0.1]]                  # the prefilter / K1 reject
    s0 = np.array(pts, dtype=F)
    n2 = 700
    s2 = np.stack([rng.uniform(-11.0, 17.5, n2), rng.uniform(-9.0, 11.5, n2), rng.uniform(-3.5, 1.5, n2),
                   rng.uniform(0, 1, n2)], axis=1).astype(F)
    return [s[:, :dim].copy() for s in (s0, np.zeros((0, 4), F), s2)]


def height_scans():
    """One scan for the height test with the origin in cell (10, 10) of the 37 x 53 grid and origin_z = 0: a target 8 cells
    out whose z makes the two sides equal at k = 4 with z_top = -0.5 (z_end = -1.0: -1.0 * 4 == -0.5 * 8), one with z_end
    above z_top, and one far target."""
    return [np.array([cell_centre(18, 10, -1.0), cell_centre(10, 18, 0.25), cell_centre(2, 14, -2.0), cell_centre(40, 30, -1.5)],
                     dtype=F)]


def large_scans(seed=39):
    """256 x 256 cells of 0.25 m around the origin; targets in the four corners and random ones: rays of more than 128 cells
    from an origin in one corner."""
    rng = np.random.default_rng(seed)
    pc_range, voxel, grid = [-32.0, -32.0, -3.0, 32.0, 32.0, 1.0], [0.25, 0.25, 4.0], [256, 256, 1]
    pts = [cell_centre(cx, cy, -1.7, pc_range, voxel) for cx, cy in ((0, 0), (255, 255), (0, 255), (255, 0), (255, 128), (130, 255))]
    n = 300
    rnd = np.stack([rng.uniform(-32, 32, n), rng.uniform(-32, 32, n), rng.uniform(-2.5, 0.5, n), rng.uniform(0, 1, n)], axis=1)
    return [np.concatenate([np.array(pts), rnd]).astype(F)], pc_range, voxel, grid
