#!/usr/bin/env python3
"""Golden vectors for the rasteriser row: SemanticKITTI scene -> instance-id map.

Runs only in the build container.  The reference's own
    mask_bev/datasets/semantic_kitti/semantic_kitti_rasterizer.py   (SemanticKittiRasterizer, :12-94)
is imported UNMODIFIED from /root/reference.  Its ``import cv2`` (OpenCV is not installed) is served by a stand-in
module that provides only MORPH_RECT / MORPH_CLOSE / MORPH_OPEN, getStructuringElement and morphologyEx, written from
OpenCV's documented behaviour on scipy.ndimage.grey_dilation / grey_erosion (mode='constant', cval 0 for the dilation
and 255 for the erosion: BORDER_CONSTANT with morphologyDefaultBorderValue never wins).  The fixture therefore pins the
reference's own lines — transform, strict range test, floor division, instance selection, composition — and NOT
OpenCV's morphology, which stays "restated from the published behaviour".

Only inputs and recorded outputs are committed (tests/golden/rasterizer.npz): per-scan f32 points, labels, poses, maps.
Every labelled point is drawn as cell + in-cell offset in [0.05, 0.95] in the centre frame and transformed back, and the
script ASSERTS that every transformed coordinate — through the world frame in two products as the reference goes, and
through one combined matrix as K22 goes — is at least 1e-6 m from a cell edge and from a range bound, so f64 rounding
cannot move a point and comparisons are exact.

    python tests/golden/make_golden_rasterizer.py
"""
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import rasterize_ref as RR  # noqa: E402


def _cv2_stand_in():
    cv2 = types.ModuleType('cv2')
    cv2.MORPH_RECT, cv2.MORPH_OPEN, cv2.MORPH_CLOSE = 0, 2, 3

    def getStructuringElement(shape, ksize):
        assert shape == cv2.MORPH_RECT
        return np.ones((ksize[1], ksize[0]), dtype=np.uint8)

    def _dilate(img, kernel):
        return ndimage.grey_dilation(img, footprint=kernel.astype(bool), mode='constant', cval=0)

    def _erode(img, kernel):
        return ndimage.grey_erosion(img, footprint=kernel.astype(bool), mode='constant', cval=255)

    def morphologyEx(img, op, kernel):
        assert img.dtype == np.uint8 and kernel.shape[0] % 2 == 1 and kernel.shape[1] % 2 == 1
        if op == cv2.MORPH_CLOSE:
            return _erode(_dilate(img, kernel), kernel)
        if op == cv2.MORPH_OPEN:
            return _dilate(_erode(img, kernel), kernel)
        raise NotImplementedError(op)

    cv2.getStructuringElement, cv2.morphologyEx = getStructuringElement, morphologyEx
    return cv2


sys.modules['cv2'] = _cv2_stand_in()
for _name in ('tqdm', 'matplotlib', 'matplotlib.pyplot'):
    try:
        __import__(_name)
    except ImportError:
        sys.modules[_name] = types.ModuleType(_name)
sys.path.insert(0, '/root/reference')
from mask_bev.datasets.semantic_kitti.semantic_kitti_rasterizer import SemanticKittiRasterizer  # noqa: E402

MARGIN = 1e-6


def pose(yaw, pitch, roll, t):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    m = np.eye(4)
    m[:3, :3] = rz @ ry @ rx
    m[:3, 3] = t
    return m


POSES = np.stack([pose(0.31, 0.010, -0.020, [812.4, -1341.7, 3.1]),
                  pose(0.43, -0.015, 0.012, [818.9, -1338.2, 3.3]),          # the centre scan
                  pose(0.58, 0.020, 0.005, [826.0, -1333.5, 3.2])])
CENTRE = 1


def blob_cells(rng, x0, y0, sx, sy, n):
    """n cells of an sx x sy rectangle: its outline (what a lidar sees of a car) plus a few inside."""
    cells = set()
    while len(cells) < n:
        if rng.random() < 0.7:
            if rng.random() < 0.5:
                c = (rng.integers(0, sx), rng.choice([0, sy - 1]))
            else:
                c = (rng.choice([0, sx - 1]), rng.integers(0, sy))
        else:
            c = (rng.integers(0, sx), rng.integers(0, sy))
        cells.add((int(x0 + c[0]), int(y0 + c[1])))
    return sorted(cells)


def make_case(rng, ranges, vs, nx_ny, boxes, clutter, z_out_fraction=0.0, centre_counts=None):
    """boxes: list of (id, x0, y0, sx, sy, n_cells) in cell units (may reach outside the grid).  Returns the per-scan
    f32 points, labels and the checks of the margins."""
    (xr, yr, zr) = ranges
    nx, ny = RR.grid_size(xr, vs), RR.grid_size(yr, vs)
    assert (nx, ny) == nx_ny, (nx, ny)
    pts_c, ids = [], []
    for inst, x0, y0, sx, sy, n in boxes:
        for (cx, cy) in blob_cells(rng, x0, y0, sx, sy, n):
            for _ in range(int(rng.integers(1, 3))):
                z = rng.uniform(zr[0] + 0.5, zr[1] - 0.5)
                if rng.random() < z_out_fraction:
                    z = zr[1] + rng.uniform(0.5, 2.0) if rng.random() < 0.5 else zr[0] - rng.uniform(0.5, 2.0)
                pts_c.append([xr[0] + (cx + rng.uniform(0.05, 0.95)) * vs, yr[0] + (cy + rng.uniform(0.05, 0.95)) * vs, z])
                ids.append(inst)
    for _ in range(clutter):                                         # unlabelled points, anywhere (also out of range)
        pts_c.append([rng.uniform(xr[0] * 1.3, xr[1] * 1.3), rng.uniform(yr[0] * 1.3, yr[1] * 1.3),
                      rng.uniform(zr[0] * 1.3, zr[1] * 1.3)])
        ids.append(0)
    pts_c = np.array(pts_c, dtype=np.float64).reshape(-1, 3)
    ids = np.array(ids, dtype=np.uint32)
    perm = rng.permutation(len(ids))
    pts_c, ids = pts_c[perm], ids[perm]
    scan_of = rng.integers(0, len(POSES), len(ids))
    if centre_counts is not None:                                    # id -> exact number of its points in the centre scan
        for inst, cnt in centre_counts.items():
            where = np.flatnonzero(ids == inst)
            scan_of[where] = np.where(scan_of[where] == CENTRE, 0, scan_of[where])
            scan_of[where[:cnt]] = CENTRE
    homo = np.hstack([pts_c, np.ones((len(ids), 1))])
    world = (POSES[CENTRE] @ homo.T).T
    points, inst = [], []
    for s in range(len(POSES)):
        sel = scan_of == s
        local = (np.linalg.inv(POSES[s]) @ world[sel].T).T
        pc = np.zeros((int(sel.sum()), 4), dtype=np.float32)
        pc[:, :3] = local[:, :3].astype(np.float32)
        pc[:, 3] = rng.random(int(sel.sum())).astype(np.float32)     # remission
        points.append(pc)
        inst.append(ids[sel])
    return points, inst


def check_margins(points, inst, ranges, vs):
    """Both routes to the centre frame keep every labelled point >= MARGIN from every cell edge and range bound."""
    inv_c = np.linalg.inv(POSES[CENTRE])
    scene = RR.aggregate_scene(points, POSES)
    two = (inv_c @ np.hstack([scene[:, :3], np.ones((scene.shape[0], 1))]).T).T
    one = np.concatenate([((inv_c @ POSES[s]) @ np.hstack([p[:, :3].astype(np.float64), np.ones((p.shape[0], 1))]).T).T
                          for s, p in enumerate(points)])
    lab = np.concatenate(inst) != 0
    for route in (two, one):
        for axis, (lo, hi) in enumerate(ranges):
            c = route[lab, axis]
            assert np.all(np.abs(c - lo) >= MARGIN) and np.all(np.abs(c - hi) >= MARGIN)
            if axis < 2:
                f = (c - lo) / vs
                assert np.all(np.abs(f - np.round(f)) * vs >= MARGIN)
    assert np.array_equal(np.floor((two[lab, :2] - [ranges[0][0], ranges[1][0]]) / vs),
                          np.floor((one[lab, :2] - [ranges[0][0], ranges[1][0]]) / vs))


class _Stub:
    pass


def run_reference(points, inst, ranges, vs, remove_unseen, min_points, k=9):
    scan, scene = _Stub(), _Stub()
    scan.velo_to_inv_pose = np.linalg.inv(POSES[CENTRE])
    scan.inst_label = inst[CENTRE]
    scene.point_cloud = RR.aggregate_scene(points, POSES)
    scene.inst_label = np.concatenate(inst)
    r = SemanticKittiRasterizer(ranges[0], ranges[1], ranges[2], vs, remove_unseen=remove_unseen, min_points=min_points,
                                morph_kernel_size=k)
    m = r.get_mask_around(scan, scene)
    # the restatement given the reference's paint order reproduces its map bit for bit
    in_range_inst, _ = RR.cells_of(scene.point_cloud, scene.inst_label, scan.velo_to_inv_pose, *ranges, vs)
    if remove_unseen:
        order = set()                                                  # built as :74-78 build it: same hash order
        for i in set(scan.inst_label) - {0}:
            if np.count_nonzero(scan.inst_label == i) >= min_points:
                order.add(i)
        order = list(order)
    else:
        order = list(set(in_range_inst) - {0})
    again, masks = RR.get_mask_around(scene.point_cloud, scene.inst_label, scan.velo_to_inv_pose, *ranges, vs,
                                      centre_inst=scan.inst_label, remove_unseen=remove_unseen, min_points=min_points,
                                      morph_kernel_size=k, order=order, return_masks=True)
    assert np.array_equal(again, m)
    return m, np.array([int(i) for i in order], dtype=np.int64), masks


def lattice_boxes(rng, nx, ny, count, ids):
    """`count` boxes on a coarse lattice: at least 9 empty cells between any two."""
    pitch_x, pitch_y = 62, 72
    spots = [(4 + i * pitch_x, 4 + j * pitch_y) for i in range((nx - 8) // pitch_x + 1) for j in range((ny - 8) // pitch_y + 1)
             if 4 + i * pitch_x + 34 < nx and 4 + j * pitch_y + 34 < ny]
    rng.shuffle(spots)
    boxes = []
    for inst, (x0, y0) in zip(ids[:count], spots):
        sx, sy = (int(rng.integers(20, 32)), int(rng.integers(9, 15)))
        if rng.random() < 0.5:
            sx, sy = sy, sx
        boxes.append((int(inst), x0 + int(rng.integers(0, 3)), y0 + int(rng.integers(0, 3)), sx, sy, int(rng.integers(30, 60))))
    assert len(boxes) == count
    for a in range(count):
        for b in range(a + 1, count):
            _, ax, ay, asx, asy, _ = boxes[a]
            _, bx, by, bsx, bsy, _ = boxes[b]
            gap = max(bx - (ax + asx), ax - (bx + bsx), by - (ay + asy), ay - (by + bsy))
            assert gap >= 9, (boxes[a], boxes[b])
    return boxes


def main():
    rng = np.random.default_rng(22)
    out = {'poses': POSES, 'centre': np.array(CENTRE)}
    big = ((-40, 40), (-40, 40), (-10, 10))
    cases = {}
    # (a) 500 x 500, ~40 well separated instances + clutter; remove_unseen False, and True with min_points = 3
    ids_a = rng.choice(np.arange(1, 3000), 40, replace=False)
    boxes_a = lattice_boxes(rng, 500, 500, 40, ids_a)
    centre_counts = {int(i): int(c) for i, c in zip(ids_a, rng.choice([0, 1, 2, 3, 4, 7], 40))}
    cases['a'] = (big, 0.16, (500, 500), boxes_a, 1500, 0.0, centre_counts)
    # (b) a non-square grid
    cases['b'] = (((-8, 8), (-9.6, 9.6), (-3, 3)), 0.16, (100, 120),
                  [(7, 10, 12, 24, 11, 40), (300, 60, 20, 12, 26, 45), (65535, 50, 80, 30, 14, 50)], 300, 0.0, None)
    # (c) instances cut by the range bounds on every side and on the z bounds; one touches a grid corner
    cases['c'] = (big, 0.16, (500, 500),
                  [(11, -12, 200, 26, 12, 50), (12, 486, 100, 26, 12, 50), (13, 150, -6, 12, 26, 50),
                   (14, 300, 488, 12, 26, 50), (15, 0, 0, 7, 7, 30), (16, 240, 240, 28, 13, 60), (17, 493, 493, 7, 7, 35)],
                  400, 0.0, None)
    cases['c_z'] = (big, 0.16, (500, 500), [(21, 100, 100, 28, 13, 60), (22, 300, 320, 13, 28, 60)], 100, 0.4, None)
    # (d) three deliberately touching pairs
    cases['d'] = (big, 0.16, (500, 500),
                  [(260, 50, 50, 26, 12, 70), (519, 74, 52, 26, 12, 70), (2184, 200, 300, 12, 26, 70),
                   (1037, 204, 324, 12, 26, 70), (5, 400, 100, 24, 12, 70), (40000, 403, 110, 24, 12, 70),
                   (77, 300, 80, 20, 10, 40)], 300, 0.0, None)
    # (e) an empty scene: clutter only
    cases['e'] = (big, 0.16, (500, 500), [], 500, 0.0, None)

    for name, (ranges, vs, nx_ny, boxes, clutter, z_out, cc) in cases.items():
        points, inst = make_case(rng, ranges, vs, nx_ny, boxes, clutter, z_out, cc)
        check_margins(points, inst, ranges, vs)
        out[f'{name}_ranges'] = np.array(ranges, dtype=np.float64)
        out[f'{name}_vs'] = np.array(vs)
        out[f'{name}_points'] = np.concatenate(points)
        out[f'{name}_inst'] = np.concatenate(inst)
        out[f'{name}_offsets'] = np.concatenate([[0], np.cumsum([len(i) for i in inst])]).astype(np.int32)
        m, order, masks = run_reference(points, inst, ranges, vs, False, 1)
        assert m.shape == nx_ny
        out[f'{name}_map'] = m.astype(np.int32)
        out[f'{name}_order'] = order
        if name == 'a':
            mu, order_u, _ = run_reference(points, inst, ranges, vs, True, 3)
            assert 0 < len(order_u) < 40 and not np.array_equal(mu, m)
            out['a_map_unseen'] = mu.astype(np.int32)
            out['a_order_unseen'] = order_u
            out['a_min_points'] = np.array(3)
        if name == 'd':
            claims = sum(v.astype(np.int64) for v in masks.values())
            multi, fg = int((claims > 1).sum()), int((claims > 0).sum())
            assert 0 < multi <= 0.10 * fg, (multi, fg)
        else:
            claims = sum(v.astype(np.int64) for v in masks.values()) if masks else np.zeros(nx_ny, dtype=np.int64)
            assert int((claims > 1).sum()) == 0, name
        print(name, nx_ny, 'points', len(out[f'{name}_inst']), 'labelled', int((out[f'{name}_inst'] != 0).sum()),
              'instances in map', len(np.unique(m)) - 1)
    path = os.path.join(HERE, 'rasterizer.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
