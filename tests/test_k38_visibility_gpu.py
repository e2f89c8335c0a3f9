"""K38a (mbv_visibility_map, csrc/visibility.hip) through the C ABI and ``ops.visibility_map``: ``vis`` equals the numpy
restatement (tests/visibility_ref.py) byte for byte, into an output and a workspace filled with garbage."""
import functools

import numpy as np
import pytest
import torch

from tests import visibility_ref as V

pytestmark = pytest.mark.gpu
F = np.float32
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
POISON = 0xa5


def _call(device, scans, pc_range, voxel, grid, ocx, ocy, origin_z, z_top, prefilter=True, dim=None):
    """→ (rc, vis (B, gy, gx) uint8 on the host); output and workspace poisoned."""
    from mask_bev_amd import _lib
    from mask_bev_amd.ops_core import _ptr, _stream
    lib = _lib.load()
    dim = dim or (scans[0].shape[1] if len(scans) else 4)
    lens = [len(s) for s in scans]
    pts = np.concatenate(scans).astype(F) if sum(lens) else np.zeros((0, dim), F)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to(device)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(device)
    gx, gy, gz = grid
    vis = torch.full((max(len(scans), 1), gy, gx), POISON, dtype=torch.uint8, device=device)
    nbytes = lib.mbv_visibility_map_workspace_bytes(len(scans), gx, gy)
    ws = torch.full((max(nbytes, 256),), 0x5a, dtype=torch.uint8, device=device)
    rc = lib.mbv_visibility_map(_ptr(d_pts) if sum(lens) else None, dim, sum(lens), _ptr(offs), len(scans), *pc_range, *voxel, gx,
                                gy, gz, 1 if prefilter else 0, ocx, ocy, float(origin_z), float(z_top), _ptr(vis), _ptr(ws),
                                ws.numel(), _stream())
    torch.cuda.synchronize()
    return rc, vis.cpu().numpy()[:len(scans)]


@functools.lru_cache(maxsize=None)
def _scripted_reference(where, dim, prefilter, z_top):
    origin = V.ORIGINS[where]
    ocx, ocy = V.origin_cell(V.RANGE, V.VOXEL, origin)
    ref = V.visibility_map(V.scripted_scans(origin, dim), V.RANGE, V.VOXEL, V.GRID, ocx, ocy, origin[2], z_top, prefilter)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize('where', sorted(V.ORIGINS))
@pytest.mark.parametrize('dim,prefilter', [(4, True), (3, False)])
def test_k38a_scripted_scans_on_an_odd_grid(device, where, dim, prefilter):
    """37 x 53, batch 3 with an empty scan; the origin inside, on an edge cell and outside the grid; targets in all octants,
    on the axes and diagonals and in the origin's cell; doubled returns, -0.0 / +0.0, NaN, rejected points; three z_top, one of
    them above origin_z (the whole ray)."""
    origin = V.ORIGINS[where]
    ocx, ocy = V.origin_cell(V.RANGE, V.VOXEL, origin)
    scans = V.scripted_scans(origin, dim)
    for z_top in (-0.2, -1.25, 0.5):
        rc, vis = _call(device, scans, V.RANGE, V.VOXEL, V.GRID, ocx, ocy, origin[2], z_top, prefilter)
        assert rc == 0
        ref = _scripted_reference(where, dim, prefilter, z_top)
        assert vis.dtype == np.uint8 and vis.tobytes() == ref.tobytes(), np.argwhere(vis != ref)[:8]
        assert not vis[1].any()


def test_k38a_height_test_boundaries(device):
    """z_end > z_top certifies nothing; a threshold mid-ray with both sides equal at k = 4; origin_z <= z_top certifies the
    whole ray; a NaN threshold certifies nothing; origin_z below every return."""
    scans = V.height_scans()
    for oz, z_top in ((0.0, -0.5), (0.0, 0.5), (0.0, np.nan), (-2.5, -0.5), (0.0, -3.0), (np.nan, 0.0)):
        rc, vis = _call(device, scans, V.RANGE, V.VOXEL, V.GRID, 10, 10, oz, z_top)
        ref = V.visibility_map(scans, V.RANGE, V.VOXEL, V.GRID, 10, 10, oz, z_top)
        assert rc == 0 and vis.tobytes() == ref.tobytes(), (oz, z_top)
    rc, vis = _call(device, scans, V.RANGE, V.VOXEL, V.GRID, 10, 10, 0.0, -0.5)
    assert [int(vis[0, 10, 10 + k]) for k in range(9)] == [0, 0, 0, 0, 1, 1, 1, 1, 2]
    assert [int(vis[0, 10 + k, 10]) for k in range(1, 9)] == [0] * 7 + [2]


def test_k38a_large_grid_corner_to_corner(device):
    """256 x 256: rays of 255 samples from a corner origin, and from an origin 300 cells outside the grid."""
    scans, pc_range, voxel, grid = V.large_scans()
    for ocx, ocy in ((0, 0), (255, 3), (-300, 128)):
        rc, vis = _call(device, scans, pc_range, voxel, grid, ocx, ocy, 0.0, -0.2)
        ref = V.visibility_map(scans, pc_range, voxel, grid, ocx, ocy, 0.0, -0.2)
        assert rc == 0 and vis.tobytes() == ref.tobytes(), (ocx, ocy, np.argwhere(vis != ref)[:8])
    assert np.count_nonzero(vis & V.PASSED) > 1000


def test_k38a_far_origin_takes_the_wide_integers(device):
    """An origin 2^20 cells away: n > 16384, the 64-bit line; only the last samples of a ray fall into the grid."""
    scans = V.height_scans()
    for ocx, ocy in ((-(1 << 20), 5), ((1 << 20), -(1 << 20)), (20000, 17)):
        rc, vis = _call(device, scans, V.RANGE, V.VOXEL, V.GRID, ocx, ocy, 0.0, 0.5)
        ref = V.visibility_map(scans, V.RANGE, V.VOXEL, V.GRID, ocx, ocy, 0.0, 0.5)
        assert rc == 0 and vis.tobytes() == ref.tobytes(), (ocx, ocy)
        assert np.count_nonzero(ref & V.PASSED) > 0


def test_k38a_empty_cases_and_error_codes(device):
    from mask_bev_amd import _lib
    from mask_bev_amd.ops_core import _ptr, _stream
    lib = _lib.load()
    empty = [np.zeros((0, 4), F), np.zeros((0, 4), F)]
    rc, vis = _call(device, empty, V.RANGE, V.VOXEL, V.GRID, 3, 3, 0.0, -0.2)
    assert rc == 0 and vis.shape == (2, 37, 53) and not vis.any()                       # total_points == 0: all zeros
    gx, gy, gz = V.GRID
    out = torch.full((1, gy, gx), POISON, dtype=torch.uint8, device=device)
    pts = torch.from_numpy(V.height_scans()[0]).to(device)
    offs = torch.tensor([0, pts.shape[0]], dtype=torch.int32, device=device)
    ws = torch.zeros((lib.mbv_visibility_map_workspace_bytes(1, gx, gy),), dtype=torch.uint8, device=device)

    def call(pts=pts, dim=4, n=pts.shape[0], offs=offs, batch=1, gx=gx, gy=gy, gz=gz, ocx=0, ocy=0, vis=out, ws=ws, ws_bytes=None):
        return lib.mbv_visibility_map(_ptr(pts), dim, n, _ptr(offs), batch, *V.RANGE, *V.VOXEL, gx, gy, gz, 1, ocx, ocy, 0.0, -0.2,
                                      _ptr(vis), _ptr(ws), ws.numel() if ws_bytes is None and ws is not None else (ws_bytes or 0),
                                      _stream())

    assert call(batch=0, vis=None, ws=None) == 0                                        # batch == 0: nothing is written
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    assert call() == 0 and call(ocx=1 << 20, ocy=-(1 << 20)) == 0
    for bad in (dict(batch=-1), dict(n=-1), dict(dim=2), dict(dim=5), dict(gx=0), dict(gy=0), dict(gz=0), dict(ocx=(1 << 20) + 1),
                dict(ocx=-(1 << 20) - 1), dict(ocy=(1 << 20) + 1), dict(ocy=-(1 << 20) - 1), dict(vis=None), dict(pts=None),
                dict(offs=None)):
        assert call(**bad) == BAD_ARG, bad
    assert call(batch=65536) == UNSUPPORTED and call(n=2 ** 31 - 1) == UNSUPPORTED
    assert call(gx=65537) == UNSUPPORTED and call(gy=65537) == UNSUPPORTED
    assert call(ws_bytes=ws.numel() - 1) == WORKSPACE and call(ws=None) == WORKSPACE
    assert call(n=0, pts=None, offs=None, ws=None) == 0                                 # no points: no workspace is needed
    assert lib.mbv_visibility_map_workspace_bytes(-1, gx, gy) == 0 and lib.mbv_visibility_map_workspace_bytes(65536, gx, gy) == 0
    assert lib.mbv_visibility_map_workspace_bytes(1, 0, gy) == 0 and lib.mbv_visibility_map_workspace_bytes(1, gx, 65537) == 0
    assert lib.mbv_visibility_map_workspace_bytes(3, gx, gy) >= 3 * gx * gy * 4
    torch.cuda.synchronize()


def test_ops_visibility_map(device):
    from mask_bev_amd import ops

    class Geom:
        pc_range, voxel_size, grid = V.RANGE, V.VOXEL, V.GRID
    for where, dim in (('inside', 4), ('outside', 3)):
        origin = V.ORIGINS[where]
        scans = V.scripted_scans(origin, dim)
        got = ops.visibility_map([torch.from_numpy(s).to(device) for s in scans], Geom, origin=origin, z_top=-1.25)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 37, 53)
        assert got.cpu().numpy().tobytes() == _scripted_reference(where, dim, True, -1.25).tobytes()
    with pytest.raises(ValueError):
        ops.visibility_map([], Geom)
