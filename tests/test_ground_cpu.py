"""K35 without a GPU: the numpy restatement (tests/ground_ref.py) against a brute-force window and hand-worked answers, the
launcher's ``lift_settings``, and the declaration of the two entry points."""
import os
import re

import numpy as np
import pytest
import torch

from tests import ground_ref as G

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 9 (x) by 7 (y) cells of 1 m, one z cell of 4 m
RANGE, VOXEL, GRID = [0.0, 0.0, -3.0, 9.0, 7.0, 1.0], [1.0, 1.0, 4.0], [9, 7, 1]
INF = F(np.inf)


@pytest.mark.parametrize('radius', [0, 1, 3, 10])
def test_window_minimum_equals_the_double_loop(radius):
    rng = np.random.default_rng(35 + radius)
    z = rng.uniform(-2, 1, (7, 9)).astype(F)
    z[rng.uniform(0, 1, (7, 9)) < 0.6] = INF
    z[3, 4], z[3, 5] = F(-0.0), F(0.0)
    for grid in (z, np.full((7, 9), INF, dtype=F)):
        enc = G.encode(grid)
        got, want = G.window_min(enc, radius), G.window_min_brute(enc, radius)
        assert got.dtype == np.uint32 and np.array_equal(got, want)
        if radius == 10:                                   # larger than the grid: the grid's minimum everywhere
            assert np.all(G.decode(got).view(np.uint32) == np.array(grid.min(), dtype=F).view(np.uint32))
        if radius == 0:
            assert np.array_equal(got, enc)
    assert np.all(G.decode(G.window_min(G.encode(np.full((7, 9), INF, dtype=F)), radius)) == INF)


def test_encoding_orders_the_floats():
    z = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], dtype=F)
    e = G.encode(z)
    assert np.all(np.diff(e.astype(np.int64)) > 0)
    assert np.array_equal(G.decode(e).view(np.uint32), z.view(np.uint32))
    assert e[-1] == G.ENC_INF


def test_one_point_makes_one_cell_and_a_clipped_block():
    for (px, py), radius in (((4.5, 3.5), 2), ((0.5, 6.5), 1), ((8.5, 0.5), 3)):
        out = G.ground_map([np.array([[px, py, -1.5, 0.3]], dtype=F)], RANGE, VOXEL, GRID, radius)
        cx, cy = int(px), int(py)
        want_min = np.full((1, 7, 9), INF, dtype=F)
        want_min[0, cy, cx] = F(-1.5)
        want = np.full((1, 7, 9), INF, dtype=F)
        want[0, max(0, cy - radius):cy + radius + 1, max(0, cx - radius):cx + radius + 1] = F(-1.5)
        assert np.array_equal(out['cell_min'], want_min) and np.array_equal(out['ground'], want)
        assert int(np.isfinite(out['ground']).sum()) <= (2 * radius + 1) ** 2


def test_label_rule_equalities_signed_zero_and_floor():
    imap = np.zeros((1, 7, 9), dtype=np.int32)
    g = F(-1.5)
    clearance, max_height = F(0.25), F(2.0)               # sums exact in f32
    pts = np.array([[4.5, 3.5, -1.5, 0],                  # 0: the ground return itself
                    [4.5, 3.5, -1.25, 0],                 # 1: z == g + clearance: NOT labelled (strict)
                    [4.5, 3.5, np.nextafter(F(-1.25), INF), 0],   # 2: one ulp above: labelled
                    [4.5, 3.5, 0.5, 0],                   # 3: z == g + max_height: labelled
                    [4.5, 3.5, np.nextafter(F(0.5), INF), 0],     # 4: one ulp above the limit: not labelled
                    [4.5, 3.5, -2.5, 0]],                 # 5: below z_floor: in no cell, and under the ground: -1
                   dtype=F)
    gm = G.ground_map([pts], RANGE, VOXEL, GRID, 1, z_floor=-2.0)
    assert gm['cell_min'][0, 3, 4] == g and gm['ground'][0, 2, 3] == g and gm['ground'][0, 0, 0] == INF
    out = G.lift_ground([pts], imap, gm['ground'], RANGE, VOXEL, GRID, 1, clearance, max_height, z_bins=8)
    assert out['point_query'].tolist() == [-1, -1, 0, 0, -1, -1]
    assert out['counts'].tolist() == [[2]] and out['z_ground'][0, 0] == g
    assert out['z_extent'][0, 0, 0] == pts[2, 2] and out['z_extent'][0, 0, 1] == F(0.5)
    # without the floor the low return is the ground: every sum moves down by one metre
    low = G.ground_map([pts], RANGE, VOXEL, GRID, 1)
    assert low['cell_min'][0, 3, 4] == F(-2.5)
    out = G.lift_ground([pts], imap, low['ground'], RANGE, VOXEL, GRID, 1, clearance, max_height, z_bins=8)
    assert out['point_query'].tolist() == [0, 0, 0, -1, -1, -1]
    # an empty window labels nothing; max_height = +inf limits nothing
    far = np.array([[0.5, 0.5, 0.9, 0]], dtype=F)
    out = G.lift_ground([far], imap, gm['ground'], RANGE, VOXEL, GRID, 1, clearance, np.inf)
    assert out['point_query'].tolist() == [-1] and out['z_ground'].tolist() == [[0.0]] and not out['z_extent'].any()
    # -0.0 is below +0.0, whichever comes first
    for order in ([0.0, -0.0], [-0.0, 0.0]):
        two = np.array([[1.5, 1.5, order[0], 0], [1.5, 1.5, order[1], 0], [2.5, 1.5, 0.0, 0]], dtype=F)
        m = G.ground_map([two], RANGE, VOXEL, GRID, 1)
        assert np.signbit(m['cell_min'][0, 1, 1]) and not np.signbit(m['cell_min'][0, 1, 2])
        assert np.signbit(m['ground'][0, 1, 2]) and np.signbit(m['ground'][0, 2, 2]) and m['ground'][0, 1, 4] == INF
        assert m['ground'][0, 2, 3] == 0 and not np.signbit(m['ground'][0, 2, 3])       # only the +0.0 cell in reach


def test_lift_settings():
    from mask_bev_amd import evaluate
    from mask_bev_amd.predict import GroundSettings
    assert evaluate.lift_settings({}) is None and evaluate.lift_settings({'lift_ground': False, 'lift_ground_radius': 3}) is None
    s = evaluate.lift_settings({'lift_ground': True})
    assert s == GroundSettings(radius_m=1.6, clearance=0.3, max_height=None, z_floor=None)
    assert s.radius_cells(0.16) == 10 and s.radius_cells(0.25) == 7 and s.radius_cells(0.05) == 32 and s.radius_cells(1.6) == 1
    s = evaluate.lift_settings({'lift_ground': True, 'lift_ground_radius': 2.0, 'lift_ground_clearance': 0.2, 'lift_max_height': 3,
                                'lift_z_floor': -2.5, 'voxel_size': 0.1})
    assert s == GroundSettings(2.0, 0.2, 3.0, -2.5) and s.radius_cells(0.1) == 20
    assert evaluate.format_lift_settings(s, 0.1) == ('ground-aware lift: radius 2 m (20 cells), clearance 0.2 m, max height 3 m, '
                                                     'z floor -2.5 m')
    assert evaluate.format_lift_settings(GroundSettings(), 0.16) == 'ground-aware lift: radius 1.6 m (10 cells), clearance 0.3 m'
    with pytest.raises(ValueError, match='32 cells'):
        GroundSettings(radius_m=1.7).radius_cells(0.05)                # 34 cells
    with pytest.raises(ValueError, match='32 cells'):
        evaluate.lift_settings({'lift_ground': True, 'voxel_size': 0.04})


def test_entry_points_are_declared_and_bound():
    from mask_bev_amd import _lib, build, ops
    from mask_bev_amd._lib import MaskBevHipError
    with open(os.path.join(ROOT, 'include', 'maskbev_hip.h')) as fh:
        header = fh.read()
    for name in ('mbv_ground_map', 'mbv_ground_map_workspace_bytes', 'mbv_lift_instances_ground',
                 'mbv_lift_instances_ground_workspace_bytes'):
        assert name in _lib.SIGNATURES
        assert re.search(r'\b(int|size_t) ' + name + r'\(', header), name
    assert len(_lib.SIGNATURES['mbv_ground_map'][1]) == 25 and len(_lib.SIGNATURES['mbv_lift_instances_ground'][1]) == 33
    assert build.FILE_FLAGS['point_lift.hip'] == ['-ffp-contract=off']
    geom = ops.VoxelGeometry.from_ranges(RANGE, VOXEL)
    assert list(geom.grid) == GRID
    with pytest.raises(MaskBevHipError):
        ops.ground_map([torch.zeros(5, 4)], geom, 2)
    fields = [f for f in ops.PointInstances.__dataclass_fields__]
    assert fields[-1] == 'z_ground' and ops.PointInstances.__dataclass_fields__['z_ground'].default is None


def test_boxes3d_bottom_needs_a_ground():
    from mask_bev_amd.predict import Predictions
    p = Predictions(torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.bool), None, None, None,
                    None, (4, 4))
    with pytest.raises(ValueError, match="bottom='ground'"):
        p.boxes3d([torch.zeros(3, 4)], None, (0, 4), (0, 4), 1.0, bottom='ground')
    with pytest.raises(ValueError, match='bottom'):
        p.boxes3d([torch.zeros(3, 4)], None, (0, 4), (0, 4), 1.0, bottom='roof')
    with pytest.raises(ValueError, match='scans'):
        p.kitti_predictions((0, 4), (0, 4), 1.0, bottom='ground')
