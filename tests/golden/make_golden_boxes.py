#!/usr/bin/env python3
"""Golden vectors for the box rasterisers (K24): KITTI / Waymo box tables -> instance-id maps.

    python tests/golden/make_golden_boxes.py /path/to/the/reference/checkout

The reference's own
    mask_bev/datasets/kitti/kitti_rasterizer.py   (KittiRasterizer)
    mask_bev/datasets/waymo/waymo_rasterizer.py   (WaymoRasterizer)
are imported UNMODIFIED from the checkout given on the command line.  Their ``import cv2`` (OpenCV is not installed) is
served by a stand-in module whose only function, ``drawContours``, is the fill rule of tests/box_rasterize_ref.py;
``matplotlib`` and ``torch_waymo`` (its ``SimplifiedFrame`` and the ``Type`` / ``Label`` / ``Box`` of its label protocol)
are minimal stand-ins; the KITTI label and frame types are the reference's own dataclasses.  The fixture therefore pins
the reference's OWN lines — label selection, instance numbering, the range skip, ``_box_to_points``, ``_map_to``, the
``np.intp`` truncation, the paint order, the image's axes — and NOT OpenCV's polygon fill.

Only inputs and recorded outputs are committed (tests/golden/box_rasterizer.npz): box tables, types, point counts, ranges,
the integer contours the reference handed to ``drawContours`` and the maps it returned.  The script ASSERTS that no corner
coordinate lies within 1e-9 of an integer before its truncation, so no last-bit difference of a cosine can move a vertex.
"""
import os
import sys
import types
from enum import IntEnum

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import box_rasterize_ref as BR  # noqa: E402

CONTOURS = []                                   # every contour the reference hands to drawContours, in call order


def _cv2_stand_in():
    cv2 = types.ModuleType('cv2')

    def drawContours(mask, contours, contour_idx, color, thickness):
        CONTOURS.append(np.array(contours[0], dtype=np.int64).reshape(4, 2))
        return BR.draw_contours_fill(mask, contours, contour_idx, color, thickness)

    cv2.drawContours = drawContours
    return cv2


def _torch_waymo_stand_in():
    tw, proto, lp = types.ModuleType('torch_waymo'), types.ModuleType('torch_waymo.protocol'), \
        types.ModuleType('torch_waymo.protocol.label_proto')

    class Type(IntEnum):
        TYPE_UNKNOWN, TYPE_VEHICLE, TYPE_PEDESTRIAN, TYPE_SIGN, TYPE_CYCLIST = 0, 1, 2, 3, 4

    class Box:
        def __init__(self, row):
            self.center_x, self.center_y, self.center_z, self.length, self.width, self.height, self.heading = row

    class Label:
        def __init__(self, box, type, num_lidar_points_in_box):
            self.box, self.type, self.num_lidar_points_in_box = box, type, num_lidar_points_in_box

    class SimplifiedFrame:
        def __init__(self, laser_labels):
            self.laser_labels = laser_labels

    tw.SimplifiedFrame, lp.Type, lp.Label, lp.Box = SimplifiedFrame, Type, Label, Box
    tw.protocol, proto.label_proto = proto, lp
    sys.modules.update({'torch_waymo': tw, 'torch_waymo.protocol': proto, 'torch_waymo.protocol.label_proto': lp})


if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.modules['cv2'] = _cv2_stand_in()
_torch_waymo_stand_in()
for _name in ('matplotlib', 'matplotlib.pyplot'):
    try:
        __import__(_name)
    except ImportError:
        sys.modules[_name] = types.ModuleType(_name)
sys.path.insert(0, sys.argv[1])
from mask_bev.datasets.kitti.kitti_dataset import KittiFrame, KittiLabel, KittiOccluded, KittiType  # noqa: E402
from mask_bev.datasets.kitti.kitti_rasterizer import KittiRasterizer  # noqa: E402
from mask_bev.datasets.waymo.waymo_rasterizer import WaymoRasterizer  # noqa: E402
from torch_waymo import SimplifiedFrame  # noqa: E402
from torch_waymo.protocol.label_proto import Box, Label, Type  # noqa: E402

VS = 0.5
Z_RANGE = (-3, 1)
CAR, VAN, TRUCK, PEDESTRIAN, CYCLIST = 0, 1, 2, 3, 5


def frames_for(x_range, y_range, rng):
    """The cases, described in CELL units on the grid of (x_range, y_range, VS) and converted to metres: a list of
    (name, boxes (n, 7), types (n))."""
    nx, ny = int((x_range[1] - x_range[0]) / VS), int((y_range[1] - y_range[0]) / VS)

    def box(cxc, cyc, lc, wc, deg):
        return [x_range[0] + cxc * VS, y_range[0] + cyc * VS, -1.0, lc * VS, wc * VS, 1.5, np.deg2rad(deg)]

    def cars(*rows):
        return np.array(rows, dtype=np.float64).reshape(-1, 7), np.full(len(rows), CAR, dtype=np.int64)

    f = []
    f.append(('axis_aligned', *cars(box(12.3, 8.4, 9.3, 4.2, 0.0))))
    f.append(('deg30', *cars(box(nx / 2 + 0.3, ny / 2 + 0.2, 10.7, 4.6, 30.0))))
    f.append(('deg89_9', *cars(box(nx / 2 - 3.6, ny / 2 + 0.4, 11.4, 4.3, 89.9))))
    f.append(('one_cell_wide', *cars(box(14.5, 10.45, 9.6, 0.5, 0.0), box(25.45, 9.3, 8.8, 0.5, 90.0),
                                     box(8.4, 16.3, 9.1, 0.45, 37.0))))
    f.append(('one_cell', *cars(box(5.5, 5.5, 0.3, 0.3, 20.0), box(20.45, 11.55, 0.25, 0.2, 0.0))))
    f.append(('overlap_later_wins', *cars(box(15.2, 11.3, 10.4, 4.4, 10.0), box(18.7, 12.6, 9.8, 4.1, -25.0))))
    f.append(('empty', np.zeros((0, 7)), np.zeros((0,), dtype=np.int64)))
    f.append(('cut_by_borders', *cars(box(1.2, ny / 2 + 0.3, 9.3, 4.2, 15.0), box(nx - 1.3, ny / 2 - 2.2, 9.3, 4.2, -20.0),
                                      box(nx / 2 + 0.4, 1.6, 9.3, 4.2, 70.0), box(nx / 2 - 4.3, ny - 1.2, 9.3, 4.2, 100.0))))
    # corners at -0.2 ... -0.9 cells, none at or below -1: truncation toward zero gives 0 where a floor would give -1, and the slanted edges
    # from such a corner reach other cells
    f.append(('negative_fraction', *cars(box(4.6, 1.75, 10.0, 4.0, 3.0), box(1.65, ny / 2 + 3.4, 4.4, 9.7, 4.0))))
    f.append(('wholly_outside', *cars(box(nx + 20.3, ny / 2 + 0.3, 9.3, 4.2, 30.0), box(nx / 2 + 0.3, ny + 30.4, 9.3, 4.2, 5.0))))
    n = 300
    # centres at or above the lower bounds, so the range skip keeps all 300: more than one staging pass of the kernel
    many = np.array([box(rng.uniform(0.1, nx + 4), rng.uniform(0.1, ny + 4), rng.uniform(2, 11), rng.uniform(0.3, 5),
                         rng.uniform(-180, 180)) for _ in range(n)])
    f.append(('many_300', many, np.full(n, CAR, dtype=np.int64)))
    # the range skip as it stands (kitti_rasterizer.py:46-48): a centre ABOVE the upper bounds is still painted where the box
    # reaches the grid; a centre below a lower bound is skipped but keeps its instance number
    f.append(('centre_above_upper_bound', *cars(box(nx + 1.3, ny / 2 + 0.4, 9.3, 4.2, 12.0), box(nx / 2 + 0.3, ny + 1.2, 9.3, 4.2, 80.0))))
    mixed = np.array([box(8.3, 7.4, 9.3, 4.2, 20.0), box(16.3, 14.4, 2.2, 1.6, 0.0), box(-1.4, 12.3, 9.3, 4.2, 5.0),
                      box(22.4, 9.3, 10.5, 4.9, -40.0), box(28.3, 18.2, 3.6, 1.2, 60.0), box(30.6, 6.3, 14.2, 5.3, 85.0)])
    f.append(('types_and_skip', mixed, np.array([CAR, PEDESTRIAN, CAR, VAN, CYCLIST, TRUCK], dtype=np.int64)))
    return f, (nx, ny)


def check_margin(raster, row):
    lab = types.SimpleNamespace(location=row[:3], dimensions=row[3:6], rotation_y=row[6], center_x=row[0], center_y=row[1],
                                center_z=row[2], length=row[3], width=row[4], height=row[5], heading=row[6])
    p = raster._box_to_points(lab)
    p[:, 0] = raster._map_to(p[:, 0], raster._x_range[0], raster._x_range[1], 0, raster._num_voxel_x)
    p[:, 1] = raster._map_to(p[:, 1], raster._y_range[0], raster._y_range[1], 0, raster._num_voxel_y)
    assert np.all(np.abs(p - np.round(p)) > 1e-9), (row, p)
    assert np.all(np.abs(p) < 2 ** 20)


def run_kitti(x_range, y_range, frames):
    r = KittiRasterizer(x_range, y_range, Z_RANGE, VS)
    maps, contours, counts = [], [], []
    for _, boxes, tps in frames:
        labels = [KittiLabel(KittiType(int(t)), 0.0, KittiOccluded.FullyVisible, 0.0, np.zeros(4), b[3:6].copy(), b[:3].copy(),
                             float(b[6])) for b, t in zip(boxes, tps)]
        for b in boxes:
            check_margin(r, b)
        del CONTOURS[:]
        out = r.get_mask(KittiFrame(None, [], labels, None))
        assert list(out.keys()) == [KittiType.Car]
        maps.append(out[KittiType.Car].astype(np.int32))
        contours += [c.copy() for c in CONTOURS]
        counts.append(len(CONTOURS))
    return np.stack(maps), np.array(contours, dtype=np.int32).reshape(-1, 4, 2), np.concatenate([[0], np.cumsum(counts)])


def run_waymo(x_range, y_range, frames, min_points):
    r = WaymoRasterizer(x_range, y_range, Z_RANGE, VS, min_points=min_points)
    maps, contours, counts = [], [], []
    for _, boxes, tps, npts in frames:
        labels = [Label(Box(b), Type(int(t)), int(c)) for b, t, c in zip(boxes, tps, npts)]
        for b in boxes:
            check_margin(r, b)
        del CONTOURS[:]
        out = r.get_mask(SimplifiedFrame(labels))
        assert list(out.keys()) == [Type.TYPE_VEHICLE]
        maps.append(out[Type.TYPE_VEHICLE].astype(np.int32))
        contours += [c.copy() for c in CONTOURS]
        counts.append(len(CONTOURS))
    return np.stack(maps), np.array(contours, dtype=np.int32).reshape(-1, 4, 2), np.concatenate([[0], np.cumsum(counts)])


def pack(out, key, frames):
    out[f'{key}_names'] = np.array([f[0] for f in frames])
    out[f'{key}_boxes'] = np.concatenate([f[1] for f in frames]).astype(np.float64)
    out[f'{key}_types'] = np.concatenate([f[2] for f in frames]).astype(np.int64)
    out[f'{key}_offsets'] = np.concatenate([[0], np.cumsum([len(f[1]) for f in frames])]).astype(np.int64)


def main():
    rng = np.random.default_rng(24)
    out = {'vs': np.array(VS), 'z_range': np.array(Z_RANGE, dtype=np.float64)}
    # two non-square KITTI grids: 40 x 24, and 70 x 130 (several tiles of the kernel, no multiple of 32 or 64)
    for key, x_range, y_range, want in (('a', (0, 20), (-6, 6), (40, 24)), ('b', (-10, 25), (-30, 35), (70, 130))):
        frames, grid = frames_for(x_range, y_range, rng)
        assert grid == want, grid
        maps, contours, coffs = run_kitti(x_range, y_range, frames)
        assert maps.shape == (len(frames), grid[1], grid[0])
        pack(out, key, frames)
        out[f'{key}_x_range'], out[f'{key}_y_range'] = np.array(x_range, dtype=np.float64), np.array(y_range, dtype=np.float64)
        out[f'{key}_maps'], out[f'{key}_contours'], out[f'{key}_contour_offsets'] = maps, contours, coffs
        names = [f[0] for f in frames]
        painted = {n: int((m > 0).sum()) for n, m in zip(names, maps)}
        assert painted['empty'] == 0 and painted['wholly_outside'] == 0 and painted['centre_above_upper_bound'] > 0
        assert sorted(np.unique(maps[names.index('types_and_skip')]).tolist()) == [0, 1, 3, 4]      # 2 skipped, never renumbered
        assert coffs[names.index('many_300') + 1] - coffs[names.index('many_300')] == 300
        print(key, grid, {n: painted[n] for n in names})
    # the falsy upper bound: x_range = (-8, 0) skips every box
    frames, grid = frames_for((-8, 0), (-6, 6), rng)
    frames = [f for f in frames if f[0] in ('axis_aligned', 'deg30', 'types_and_skip')]
    maps, contours, coffs = run_kitti((-8, 0), (-6, 6), frames)
    assert grid == (16, 24) and not maps.any() and len(contours) == 0
    pack(out, 'falsy', frames)
    out['falsy_x_range'], out['falsy_y_range'] = np.array([-8., 0.]), np.array([-6., 6.])
    out['falsy_maps'] = maps
    # Waymo on a SQUARE grid (the reference allocates its image as (nx, ny) and indexes it [y][x])
    x_range = y_range = (-12, 12)
    frames, grid = frames_for(x_range, y_range, rng)
    assert grid == (48, 48)
    wf = []
    for name, boxes, tps in frames:
        wt = np.where(np.isin(tps, [CAR, VAN, TRUCK]), 1, np.where(tps == PEDESTRIAN, 2, 4)).astype(np.int64)
        npts = rng.integers(0, 12, len(boxes)).astype(np.int64)
        if name == 'many_300':
            wt[rng.random(len(boxes)) < 0.2] = 3                                 # some signs in between
        else:
            npts[:] = np.maximum(npts, 5)
            if name == 'overlap_later_wins':
                npts[0] = 4                                                       # below min_points: the survivor becomes id 1
        wf.append((name, boxes, wt, npts))
    maps, contours, coffs = run_waymo(x_range, y_range, wf, min_points=5)
    pack(out, 'w', wf)
    out['w_num_points'] = np.concatenate([f[3] for f in wf])
    out['w_min_points'] = np.array(5)
    out['w_x_range'], out['w_y_range'] = np.array(x_range, dtype=np.float64), np.array(y_range, dtype=np.float64)
    out['w_maps'], out['w_contours'], out['w_contour_offsets'] = maps, contours, coffs
    print('w', grid, [int((m > 0).sum()) for m in maps])
    path = os.path.join(HERE, 'box_rasterizer.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
