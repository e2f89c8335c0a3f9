"""K38a without a GPU: the numpy restatement (tests/visibility_ref.py) against its plain-loop version and hand-worked answers,
the origin's cell, and the declaration of the entry points."""
import os

import numpy as np
import pytest

from tests import visibility_ref as V

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('where', sorted(V.ORIGINS))
@pytest.mark.parametrize('z_top', [-0.2, -1.25, 0.5])
def test_numpy_version_equals_the_plain_loops(where, z_top):
    origin = V.ORIGINS[where]
    ocx, ocy = V.origin_cell(V.RANGE, V.VOXEL, origin)
    for dim, prefilter in ((4, True), (3, False)):
        scans = V.scripted_scans(origin, dim)
        got = V.visibility_map(scans, V.RANGE, V.VOXEL, V.GRID, ocx, ocy, origin[2], z_top, prefilter)
        assert got.shape == (3, 37, 53) and got.dtype == np.uint8 and not got[1].any() and got.max() <= 3
        for b, s in enumerate(scans):
            want = V.plain_visibility(s, V.RANGE, V.VOXEL, V.GRID, ocx, ocy, origin[2], z_top, prefilter)
            assert np.array_equal(got[b], want)
        assert np.count_nonzero(got[0] & V.HIT) >= 5 and np.count_nonzero(got[2] & V.HIT) > 100


def test_origin_cells():
    assert V.origin_cell(V.RANGE, V.VOXEL, V.ORIGINS['inside']) == (20, 16)
    assert V.origin_cell(V.RANGE, V.VOXEL, V.ORIGINS['edge']) == (0, 22)
    assert V.origin_cell(V.RANGE, V.VOXEL, V.ORIGINS['outside']) == (-8, -6)
    # KITTI's x_range (0, 80): a sensor at x = 0 sits in column 0, just behind it in column -1
    assert V.origin_cell([0.0, -40.0, -3.0], [0.16, 0.16, 4.0], (0.0, 0.0, 0.0)) == (0, 250)
    assert V.origin_cell([0.0, -40.0, -3.0], [0.16, 0.16, 4.0], (-0.01, 0.0, 0.0))[0] == -1


def test_height_test_by_hand():
    scans = V.height_scans()
    run = lambda z_top, oz=0.0: V.visibility_map(scans, V.RANGE, V.VOXEL, V.GRID, 10, 10, oz, z_top)[0]
    vis = run(-0.5)
    # the ray to (10, 18): z_end = -1.0, n = 8: -1.0 * k <= -0.5 * 8 from k = 4 on, both sides equal at k = 4
    assert [int(vis[10, 10 + k]) for k in range(9)] == [0, 0, 0, 0, 1, 1, 1, 1, 2]
    # z_end = 0.25 > z_top certifies nothing, whatever k: 0.25 * k <= -4 never holds; the target is still HIT
    assert [int(vis[10 + k, 10]) for k in range(1, 9)] == [0] * 7 + [2]
    # origin_z <= z_top with the return below both: the whole ray, the origin's cell included
    vis = run(0.5)
    assert [int(vis[10, 10 + k]) for k in range(9)] == [1] * 8 + [2]
    assert all(int(vis[10 + k, 10]) & 1 for k in range(8))               # 0.25 * k <= 0.5 * 8 for k < 8
    # a NaN threshold certifies nothing
    assert not (run(np.nan) & V.PASSED).any() and np.count_nonzero(run(np.nan) & V.HIT) == 4
    # the same through the plain loops
    for z_top in (-0.5, 0.5, np.nan):
        assert np.array_equal(run(z_top), V.plain_visibility(scans[0], V.RANGE, V.VOXEL, V.GRID, 10, 10, 0.0, z_top))


def test_lowest_return_and_signed_zero_decide():
    a = V.cell_centre(30, 10, 0.0)
    pts = np.array([a, V.cell_centre(30, 10, -0.0), a], dtype=F)
    # origin_z = z_top = 0: rise = -0.0 - 0 = -0.0, rhs = 0 * n = 0: -0.0 * k <= 0 holds: the whole ray
    vis = V.visibility_map([pts], V.RANGE, V.VOXEL, V.GRID, 10, 10, 0.0, 0.0)[0]
    assert [int(v) for v in vis[10, 10:31]] == [1] * 20 + [2]
    # a second, lower return in the cell decides: with z_top = -0.5 the ray of z_end = -2 passes from k = 5 on (n = 20)
    pts = np.array([V.cell_centre(30, 10, -1.0), V.cell_centre(30, 10, -2.0)], dtype=F)
    vis = V.visibility_map([pts], V.RANGE, V.VOXEL, V.GRID, 10, 10, 0.0, -0.5)[0]
    assert [int(v) for v in vis[10, 10:31]] == [0] * 5 + [1] * 15 + [2]


def test_large_grid_rays_longer_than_two_wavefronts():
    scans, pc_range, voxel, grid = V.large_scans()
    got = V.visibility_map(scans, pc_range, voxel, grid, 0, 0, 0.0, -0.2)
    assert np.array_equal(got[0], V.plain_visibility(scans[0], pc_range, voxel, grid, 0, 0, 0.0, -0.2))
    diag = [int(got[0, k, k]) for k in range(256)]
    assert diag[0] & V.HIT and diag[255] == V.HIT and sum(d & V.PASSED for d in diag) > 128


def test_binding_table_header_and_flags():
    from mask_bev_amd import _lib, build, ops
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    names = ('mbv_visibility_map', 'mbv_visibility_map_workspace_bytes')
    for name in names:
        assert name in _lib.SIGNATURES and name + '(' in header
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [26, 3]
    assert build.FILE_FLAGS['visibility.hip'] == ['-ffp-contract=off'] and 'visibility.hip' in build.sources()
    assert hasattr(ops, 'visibility_map') and (ops.VIS_PASSED, ops.VIS_HIT) == (V.PASSED, V.HIT)

    class Geom:
        pc_range, voxel_size, grid = V.RANGE, V.VOXEL, V.GRID
    for origin in V.ORIGINS.values():
        assert ops.origin_cell(Geom, origin) == V.origin_cell(V.RANGE, V.VOXEL, origin)
    with pytest.raises(ValueError):
        ops.origin_cell(Geom, (1e9, 0.0, 0.0))
    with pytest.raises(ValueError):
        ops.origin_cell(Geom, (float('nan'), 0.0, 0.0))
