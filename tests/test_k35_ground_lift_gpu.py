"""K35 (csrc/point_lift.hip) through the C ABI and what is built on it: ``ops.ground_map``, ``ops.lift_instances(ground=)``,
``Predictions.lift`` / ``boxes3d`` with a ground, the launcher's ``lift_ground`` key.

K35a: ``cell_min`` and ``ground`` BIT-equal to the numpy restatement (tests/ground_ref.py), the +inf cells included, into
poisoned buffers between canaries; hostile points dropped as K1 and K31 drop them; two runs and a permuted run bit-equal.
K35b: labels, counts, the four z columns and ``z_ground`` equal to the restatement; a scene whose answer is known by
construction, on which the ground-aware lift scores PQ = SQ = RQ = 1 and the plain lift does not.  No tolerances."""
import numpy as np
import pytest
import torch

from tests import ground_ref as G
from tests import point_lift_ref as L
from tests.util_cfg import random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
F = np.float32
INF = F(np.inf)
POISON = 0x5a5a5a5a
PAD, CANARY = 256, 0xA5
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3

# the window passes of K35a work on tiles of TILE columns (by 16 and by TILE rows): a window that straddles a tile edge is
# where they can go wrong, hence the grids of (TILE - 1, TILE + 1) and (2 TILE + 3, TILE) cells next to the issue's list;
# (66, 132) has whole quads per row (the 16-byte path) and ragged tiles both ways
TILE = 64
GRIDS = [(1, 1), (1, 300), (300, 1), (37, 29), (130, 67), (257, 255), (TILE - 1, TILE + 1), (2 * TILE + 3, TILE), (66, 132)]
RADII = (0, 1, 7, 32)
VOXEL = [0.5, 0.75, 2.0]


def _geometry(gy, gx):
    """pc_range, voxel, grid of a (gy, gx) BEV grid with two z cells, off the origin."""
    x0, y0 = -3.0, 1.5
    return [x0, y0, -2.0, x0 + gx * VOXEL[0], y0 + gy * VOXEL[1], 2.0], VOXEL, [gx, gy, 2]


def _random_scans(rng_range, sizes, dim, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(rng_range[:3]), np.array(rng_range[3:])
    out = []
    for n in sizes:
        pts = rng.uniform(0, 1, (n, dim))
        pts[:, :3] = (lo + hi) / 2 + (pts[:, :3] * 2 - 1) * (hi - lo) / 2 * 1.05
        out.append(pts.astype(F))
    return out


def _guarded(device, nbytes, fill, offset=0):
    """``nbytes`` of device memory filled with ``fill`` between two canary zones → (raw, payload view (uint8)); ``offset``
    shifts the payload off its 256-byte alignment."""
    rounded = (nbytes + offset + 255) // 256 * 256
    raw = torch.full((rounded + 2 * PAD,), CANARY, dtype=torch.uint8, device=device)
    payload = raw[PAD + offset:PAD + offset + nbytes]
    payload.fill_(fill)
    return raw, payload


def _canaries_intact(raw, nbytes, offset=0):
    return bool((raw[:PAD + offset] == CANARY).all()) and bool((raw[PAD + offset + nbytes:] == CANARY).all())


def _raw_ground(lib, device, scans, geom, radius, z_floor=-np.inf, prefilter=True, dim=4, offset=0, ws_bytes=None, null=None):
    """mbv_ground_map into poisoned outputs and a poisoned workspace, all between canaries → (rc, cell_min, ground) on the
    host as float32 arrays; asserts the canaries."""
    from mask_bev_amd.ops_core import _ptr, _stream
    rng, voxel, grid = geom
    batch = len(scans)
    n = sum(s.shape[0] for s in scans)
    pts = torch.from_numpy(np.concatenate(scans).reshape(n, dim)).to(device) if n else torch.zeros((1, dim), device=device)
    offs = torch.tensor(np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]), dtype=torch.int32, device=device)
    cells = batch * grid[1] * grid[0]
    raw_min, cell_min = _guarded(device, 4 * cells, 0x5a, offset)
    raw_gnd, ground = _guarded(device, 4 * cells, 0x5a, offset)
    nbytes = lib.mbv_ground_map_workspace_bytes(batch, grid[0], grid[1])
    assert nbytes >= 8 * cells
    raw_ws, ws = _guarded(device, nbytes, 0x5a)
    rc = lib.mbv_ground_map(_ptr(pts), dim, n, _ptr(offs), batch, *rng, *voxel, *grid, 1 if prefilter else 0, radius, z_floor,
                            None if null == 'cell_min' else cell_min.data_ptr(), None if null == 'ground' else ground.data_ptr(),
                            ws.data_ptr(), nbytes if ws_bytes is None else ws_bytes, _stream())
    torch.cuda.synchronize()
    assert _canaries_intact(raw_min, 4 * cells, offset) and _canaries_intact(raw_gnd, 4 * cells, offset)
    assert _canaries_intact(raw_ws, nbytes)
    shape = (batch, grid[1], grid[0])
    as_f32 = lambda t: t.cpu().numpy().view(F).reshape(shape)
    return rc, as_f32(cell_min), as_f32(ground)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ------------------------------------------------------------------------------------------------ K35a
@pytest.mark.parametrize('gy,gx,dense', [(gy, gx, False) for gy, gx in GRIDS] + [(37, 29, True)])
def test_k35a_maps_equal_the_reference(device, gy, gx, dense):
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    geom = _geometry(gy, gx)
    n = 3 * gy * gx if dense else max(1, gy * gx // 20)                 # about 5 % of the cells occupied, or every cell thrice
    scans = _random_scans(geom[0], [n, 0, max(1, n // 2)], 4, 35 + gy + gx)        # B = 3, the middle scan empty
    enc = G.cell_minima(scans, *geom)
    assert np.all(enc[1] == G.ENC_INF) and (enc[0] != G.ENC_INF).any()
    for radius in RADII:
        rc, cell_min, ground = _raw_ground(lib, device, scans, geom, radius)
        assert rc == 0
        assert np.array_equal(_bits(cell_min), _bits(G.decode(enc))), radius
        assert np.array_equal(_bits(ground), _bits(G.decode(G.window_min(enc, radius)))), radius
        assert not (_bits(cell_min) == POISON).any() and not (_bits(ground) == POISON).any()
        if radius == 0:
            assert np.array_equal(_bits(ground), _bits(cell_min))
    # the wrapper: the same tensors
    out = ops.ground_map([torch.from_numpy(s).to(device) for s in scans], ops.VoxelGeometry(*geom), 7)
    assert out.radius == 7 and out.ground.shape == (3, gy, gx) and out.ground.dtype == torch.float32
    assert np.array_equal(_bits(out.cell_min.cpu().numpy()), _bits(G.decode(enc)))
    assert np.array_equal(_bits(out.ground.cpu().numpy()), _bits(G.decode(G.window_min(enc, 7))))


def _hostile_scans(geom, dim, seed):
    """Two scans around the range with planted points: every range limit and one ulp either side, outside the grid, NaN, inf."""
    rng_, _, _ = geom
    lo, hi = np.array(rng_[:3], dtype=F), np.array(rng_[3:], dtype=F)
    mid = ((lo + hi) / 2 + F(0.1)).astype(F)
    nan, inf = np.nan, np.inf
    planted = []
    for a in range(3):
        for limit in (lo[a], hi[a]):
            for v in (limit, np.nextafter(limit, -INF), np.nextafter(limit, INF)):
                p = mid.copy()
                p[a] = v
                planted.append(p)
    for a in range(3):
        for v in (nan, inf, -inf, hi[a] + 1.0, lo[a] - 1.0):
            p = mid.copy()
            p[a] = v
            planted.append(p)
    planted.append(np.array([mid[0], mid[1], -0.0], dtype=F))
    planted = np.array(planted, dtype=F)
    scans = _random_scans(rng_, [700, 300], dim, seed)
    rng = np.random.default_rng(seed)
    for s in scans:
        where = rng.choice(s.shape[0], planted.shape[0], replace=False)
        s[where, :3] = planted
    return scans


@pytest.mark.parametrize('z_floor', [-np.inf, -0.5])
@pytest.mark.parametrize('prefilter', [True, False])
@pytest.mark.parametrize('dim', [3, 4])
def test_k35a_hostile_points_are_dropped_as_k1_drops_them(device, dim, prefilter, z_floor):
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    geom = _geometry(12, 20)
    scans = _hostile_scans(geom, dim, 7 + dim)
    ref = G.ground_map(scans, *geom, radius=2, z_floor=z_floor, prefilter=prefilter)
    rc, cell_min, ground = _raw_ground(lib, device, scans, geom, 2, z_floor=z_floor, prefilter=prefilter, dim=dim)
    assert rc == 0
    assert np.array_equal(_bits(cell_min), _bits(ref['cell_min'])) and np.array_equal(_bits(ground), _bits(ref['ground']))
    assert np.isinf(cell_min).any() and np.isfinite(cell_min).any() and not np.isnan(cell_min).any()
    # the floor cuts, or does not
    below = sum(int((s[:, 2] < -0.5).sum()) for s in scans)
    assert below > 50 and (float(cell_min[np.isfinite(cell_min)].min()) >= -0.5) == (z_floor == -0.5)
    # the points that take part are the points K31 labels on a map that one query owns entirely, cut by the floor
    vg = ops.VoxelGeometry(*geom)
    dev_scans = [torch.from_numpy(s).to(device) for s in scans]
    lifted = ops.lift_instances(dev_scans, torch.zeros((2, 12, 20), dtype=torch.int32, device=device), vg, 1, prefilter=prefilter)
    occupied = np.zeros((2, 12, 20), dtype=bool)
    for b, (s, pq) in enumerate(zip(scans, lifted.per_scan())):
        ok, cx, cy = G.participating(s, *geom, prefilter, -np.inf)
        assert np.array_equal(pq.cpu().numpy() >= 0, ok) and 0 < ok.sum() < s.shape[0]
        with np.errstate(invalid='ignore'):
            part = ok & (s[:, 2] >= F(z_floor))
        occupied[b, cy[part], cx[part]] = True
    assert np.array_equal(np.isfinite(cell_min), occupied)


def test_k35a_is_deterministic_and_blind_to_the_order_of_points(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    geom = _geometry(130, 67)
    scans = _random_scans(geom[0], [3000, 0, 1700], 4, 11)
    for s in scans:                                    # ties and signed zeros: the minimum must not depend on arrival
        s[::7, 2] = F(-0.0)
        s[::5, 2] = F(0.0)
        s[::3, :2] = s[::3, :2].round()
    a = _raw_ground(lib, device, scans, geom, 7)
    b = _raw_ground(lib, device, scans, geom, 7)
    rng = np.random.default_rng(5)
    c = _raw_ground(lib, device, [s[rng.permutation(s.shape[0])] for s in scans], geom, 7)
    assert a[0] == b[0] == c[0] == 0
    for x, y, z in zip(a[1:], b[1:], c[1:]):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z))
    assert np.array_equal(_bits(a[2]), _bits(G.ground_map(scans, *geom, radius=7)['ground']))


@pytest.mark.parametrize('gy,gx,offset', [(66, 132, 0), (66, 132, 4), (37, 29, 0), (37, 29, 8)])
def test_k35a_writes_every_element_and_nothing_else(device, gy, gx, offset):
    """Outputs and workspace between canaries, pre-filled with a poison; with ``offset`` the outputs are not 16-byte aligned,
    so a grid of whole quads must take the dword path too.  No points at all: both maps are +inf."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    geom = _geometry(gy, gx)
    scans = _random_scans(geom[0], [gy * gx // 10, 5], 4, 3)
    ref = G.ground_map(scans, *geom, radius=32)
    rc, cell_min, ground = _raw_ground(lib, device, scans, geom, 32, offset=offset)          # asserts the canaries
    assert rc == 0 and np.array_equal(_bits(cell_min), _bits(ref['cell_min'])) and np.array_equal(_bits(ground), _bits(ref['ground']))
    assert not (_bits(cell_min) == POISON).any() and not (_bits(ground) == POISON).any()
    rc, cell_min, ground = _raw_ground(lib, device, [s[:0] for s in scans], geom, 3, offset=offset)
    assert rc == 0 and np.all(cell_min == INF) and np.all(ground == INF)


def test_k35a_error_codes(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    geom = _geometry(37, 29)
    scans = _random_scans(geom[0], [200, 100], 4, 1)
    nbytes = lib.mbv_ground_map_workspace_bytes(2, 29, 37)
    assert _raw_ground(lib, device, scans, geom, 32)[0] == 0
    assert _raw_ground(lib, device, scans, geom, 33)[0] == UNSUPPORTED
    assert _raw_ground(lib, device, scans, geom, -1)[0] == BAD_ARG
    assert _raw_ground(lib, device, scans, geom, 2, ws_bytes=nbytes - 1)[0] == WORKSPACE
    assert _raw_ground(lib, device, scans, geom, 2, null='ground')[0] == BAD_ARG
    assert _raw_ground(lib, device, scans, geom, 2, null='cell_min')[0] == BAD_ARG
    assert lib.mbv_ground_map_workspace_bytes(65536, 29, 37) == 0 and lib.mbv_ground_map_workspace_bytes(2, 0, 37) == 0
    assert lib.mbv_ground_map_workspace_bytes(0, 29, 37) == 0


# ------------------------------------------------------------------------------------------------ K35b
LRANGE, LVOXEL, LGRID = [-5.0, -4.5, -2.0, 5.0, 4.5, 2.0], [0.5, 0.75, 2.0], [20, 12, 2]     # K31's test grid
Z_FLOOR, CLEARANCE, MAX_HEIGHT, RADIUS = -1.0, 0.3, 1.5, 1


def _lift_case(q, seed):
    """Two scans on K31's grid, an instance map of q queries, and the reference ground of the scans.  In scan 0 every point
    of the cells x 0 .. 6, y 0 .. 5 lies below Z_FLOOR, so the windows inside that patch are empty although the cells hold
    points; query q - 1 owns cells in there only: all of its points are cut."""
    rng = np.random.default_rng(seed)
    scans = _random_scans(LRANGE, [1500, 700], 4, seed)
    ok, cx, cy = L.point_cells(scans[0], LRANGE, LVOXEL, LGRID, True)
    patch = ok & (cx <= 6) & (cy <= 5)
    scans[0][patch, 2] = rng.uniform(-1.9, -1.2, int(patch.sum())).astype(F)
    imap = rng.integers(-1, max(q - 1, 1), (2, 12, 20)).astype(np.int32)
    if q > 1:
        imap[0, 1:4, 1:5] = q - 1
    imap[:, 0, 19] = q                                     # values the kernel must never index with
    imap[:, 11, 0] = 2 ** 30
    ground = G.ground_map(scans, LRANGE, LVOXEL, LGRID, RADIUS, z_floor=Z_FLOOR)['ground']
    assert np.all(ground[0, 1:5, 1:6] == INF) and int((patch & (cx >= 1) & (cx <= 4) & (cy >= 1) & (cy <= 3)).sum()) > 5
    return scans, imap, ground


@pytest.mark.parametrize('q', [5, 1024])
def test_k35b_lift_equals_the_reference(device, q):
    from mask_bev_amd import _lib, ops
    from mask_bev_amd.ops_core import _ptr, _stream
    lib = _lib.load()
    scans, imap, ground = _lift_case(q, 35 + q)
    quantiles, z_bins = (0.1, 0.9), 64
    ref = G.lift_ground(scans, imap, ground, LRANGE, LVOXEL, LGRID, q, CLEARANCE, MAX_HEIGHT, z_bins, quantiles)
    plain = L.lift(scans, imap, LRANGE, LVOXEL, LGRID, q, z_bins, quantiles)
    # the cases are there: kept and cut points, a query cut entirely, points above the height limit
    cut = (plain['point_query'] >= 0) & (ref['point_query'] < 0)
    assert cut.sum() >= 100 and (ref['point_query'] >= 0).sum() >= 100
    assert plain['counts'][0, q - 1] > 5 and ref['counts'][0, q - 1] == 0
    assert not ref['z_extent'][0, q - 1].any() and ref['z_ground'][0, q - 1] == 0          # five zeros
    z_all = np.concatenate(scans)[:, 2]
    cells = [L.point_cells(s, LRANGE, LVOXEL, LGRID, True) for s in scans]
    g_all = np.concatenate([ground[b][cy, cx] for b, (_, cx, cy) in enumerate(cells)])       # (cell 0, 0 where not ok: never cut)
    with np.errstate(invalid='ignore'):
        assert (cut & (z_all > g_all + F(MAX_HEIGHT))).sum() >= 10 and (cut & (z_all <= g_all + F(CLEARANCE))).sum() >= 10

    # the C entry, into poisoned buffers
    n, batch = sum(s.shape[0] for s in scans), 2
    pts = torch.from_numpy(np.concatenate(scans)).to(device)
    offs = torch.tensor([0, scans[0].shape[0], n], dtype=torch.int32, device=device)
    tm, tg = torch.from_numpy(imap).to(device), torch.from_numpy(ground).to(device)
    pq = torch.full((n,), POISON, dtype=torch.int32, device=device)
    counts = torch.full((batch, q), POISON, dtype=torch.int32, device=device)
    ext = torch.full((batch, q, 4), POISON, dtype=torch.int32, device=device)
    zg = torch.full((batch, q), POISON, dtype=torch.int32, device=device)
    nbytes = lib.mbv_lift_instances_ground_workspace_bytes(batch, q, z_bins)
    assert nbytes > lib.mbv_lift_instances_workspace_bytes(batch, q, z_bins)
    ws = torch.full((nbytes,), 0x5a, dtype=torch.uint8, device=device)
    args = (_ptr(pts), 4, n, _ptr(offs), batch, *LRANGE, *LVOXEL, *LGRID, 1, _ptr(tm), q, z_bins, quantiles[0], quantiles[1],
            _ptr(tg), CLEARANCE, MAX_HEIGHT, _ptr(pq), _ptr(counts), _ptr(ext))
    rc = lib.mbv_lift_instances_ground(*args, _ptr(zg), _ptr(ws), nbytes, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(pq.cpu(), torch.from_numpy(ref['point_query']))
    assert torch.equal(counts.cpu(), torch.from_numpy(ref['counts']))
    assert np.array_equal(ext.cpu().numpy().view(F).view(np.uint32), _bits(ref['z_extent']))
    assert np.array_equal(zg.cpu().numpy().view(F).view(np.uint32), _bits(ref['z_ground']))
    assert int(counts.sum()) == int((pq >= 0).sum())
    assert lib.mbv_lift_instances_ground(*args, _ptr(zg), _ptr(ws), nbytes - 1, _stream()) == WORKSPACE
    assert lib.mbv_lift_instances_ground(*args, None, _ptr(ws), nbytes, _stream()) == BAD_ARG
    assert lib.mbv_lift_instances_ground(*args[:23], None, *args[24:], _ptr(zg), _ptr(ws), nbytes, _stream()) == BAD_ARG

    # the wrapper: a GroundMap made on the device gives the same, a tensor too; ground=None is today's call
    geom = ops.VoxelGeometry(LRANGE, LVOXEL, LGRID)
    dev_scans = [torch.from_numpy(s).to(device) for s in scans]
    gm = ops.ground_map(dev_scans, geom, RADIUS, z_floor=Z_FLOOR)
    assert np.array_equal(_bits(gm.ground.cpu().numpy()), _bits(ground))
    for g in (gm, tg):
        out = ops.lift_instances(dev_scans, tm, geom, q, z_bins=z_bins, quantiles=quantiles, ground=g, clearance=CLEARANCE,
                                 max_height=MAX_HEIGHT)
        assert torch.equal(out.point_query.cpu(), pq.cpu()) and torch.equal(out.counts.cpu(), counts.cpu())
        assert np.array_equal(_bits(torch.stack([out.z_min, out.z_max, out.z_lo, out.z_hi], -1).cpu().numpy()), _bits(ref['z_extent']))
        assert np.array_equal(_bits(out.z_ground.cpu().numpy()), _bits(ref['z_ground']))
    unlimited = ops.lift_instances(dev_scans, tm, geom, q, ground=gm, clearance=CLEARANCE)
    want = G.lift_ground(scans, imap, ground, LRANGE, LVOXEL, LGRID, q, CLEARANCE, np.inf)
    assert torch.equal(unlimited.point_query.cpu(), torch.from_numpy(want['point_query']))
    none = ops.lift_instances(dev_scans, tm, geom, q, z_bins=z_bins, quantiles=quantiles, ground=None)
    assert none.z_ground is None and torch.equal(none.point_query.cpu(), torch.from_numpy(plain['point_query']))
    assert torch.equal(none.counts.cpu(), torch.from_numpy(plain['counts']))
    assert np.array_equal(_bits(torch.stack([none.z_min, none.z_max, none.z_lo, none.z_hi], -1).cpu().numpy()), _bits(plain['z_extent']))


def test_k35b_equalities_of_the_label_rule(device):
    """The hand-worked cases of tests/test_ground_cpu.py on the device: z == g + clearance is not labelled, z == g + max_height
    is, a return below z_floor is no ground and lies under it."""
    from mask_bev_amd import ops
    rng_, voxel, grid = [0.0, 0.0, -3.0, 9.0, 7.0, 1.0], [1.0, 1.0, 4.0], [9, 7, 1]
    geom = ops.VoxelGeometry(rng_, voxel, grid)
    pts = np.array([[4.5, 3.5, -1.5, 0], [4.5, 3.5, -1.25, 0], [4.5, 3.5, np.nextafter(F(-1.25), INF), 0], [4.5, 3.5, 0.5, 0],
                    [4.5, 3.5, np.nextafter(F(0.5), INF), 0], [4.5, 3.5, -2.5, 0], [0.5, 0.5, 0.9, 0]], dtype=F)
    scans = [torch.from_numpy(pts).to(device)]
    imap = torch.zeros((1, 7, 9), dtype=torch.int32, device=device)
    gm = ops.ground_map(scans, geom, 1, z_floor=-2.0)
    assert float(gm.cell_min[0, 3, 4]) == -1.5 and float(gm.ground[0, 2, 3]) == -1.5 and float(gm.ground[0, 6, 8]) == np.inf
    out = ops.lift_instances(scans, imap, geom, 1, ground=gm, clearance=0.25, max_height=2.0)
    assert out.point_query.cpu().tolist() == [-1, -1, 0, 0, -1, -1, -1]          # the far point is its own ground
    out = ops.lift_instances([scans[0][:6]], imap, geom, 1, ground=gm, clearance=0.25, max_height=2.0)
    assert out.point_query.cpu().tolist() == [-1, -1, 0, 0, -1, -1] and out.counts.cpu().tolist() == [[2]]
    assert float(out.z_ground[0, 0]) == -1.5 and float(out.z_min[0, 0]) == float(pts[2, 2]) and float(out.z_max[0, 0]) == 0.5
    low = ops.ground_map(scans, geom, 1)
    out = ops.lift_instances([scans[0][:6]], imap, geom, 1, ground=low, clearance=0.25, max_height=2.0)
    assert out.point_query.cpu().tolist() == [0, 0, 0, -1, -1, -1] and float(out.z_ground[0, 0]) == -2.5
    two = torch.tensor([[1.5, 1.5, 0.0, 0], [1.5, 1.5, -0.0, 0], [2.5, 1.5, 0.0, 0]], device=device)
    m = ops.ground_map([two], geom, 1)
    sign = lambda t: bool(torch.signbit(t))
    assert sign(m.cell_min[0, 1, 1]) and not sign(m.cell_min[0, 1, 2]) and sign(m.ground[0, 1, 2]) and sign(m.ground[0, 2, 2])
    assert float(m.ground[0, 2, 3]) == 0 and not sign(m.ground[0, 2, 3]) and float(m.ground[0, 1, 4]) == np.inf


# ------------------------------------------------------------------------------------------------ the scene
VS, NXY = 0.25, 64
X_RANGE, Y_RANGE, Z_RANGE = (0.0, 16.0), (-8.0, 8.0), (-3.0, 1.0)
# footprints as (y0, y1, x0, x1) cells, ends exclusive: 8 x 18, 18 x 8, and 8 x 18 with its short end on the grid's border
FOOTPRINTS = [(10, 28, 8, 16), (40, 48, 10, 28), (14, 22, 46, 64)]
SCENE_RADIUS = 5                                                        # cells, >= half the short side of a footprint


@pytest.fixture(scope='module')
def scene():
    """Road: one return per cell at z = -1.70 +- 0.05, none under the footprints.  Cars: three returns per footprint cell with
    z in [-1.25, -0.20].  The instance map: every footprint grown by 3 cells.  Every window of radius 5 around a footprint
    cell reaches the road (the short side is 8 cells; the car on the border has its LONG axis across the border), so
    -1.75 <= g <= -1.65 everywhere: a road return has z <= -1.65 < g + 0.3, a car return z >= -1.25 > g + 0.3."""
    rng = np.random.default_rng(35)
    under = np.full((NXY, NXY), -1, dtype=np.int32)
    imap = np.full((1, NXY, NXY), -1, dtype=np.int32)
    for k, (y0, y1, x0, x1) in enumerate(FOOTPRINTS):
        imap[0, max(0, y0 - 3):min(NXY, y1 + 3), max(0, x0 - 3):min(NXY, x1 + 3)] = k
        under[y0:y1, x0:x1] = k
    pts, owner = [], []
    for cy in range(NXY):
        for cx in range(NXY):
            k = under[cy, cx]
            for _ in range(1 if k < 0 else 3):
                u, v = rng.uniform(0.2, 0.8, 2)
                z = rng.uniform(-1.75, -1.65) if k < 0 else rng.uniform(-1.25, -0.20)
                pts.append([X_RANGE[0] + (cx + u) * VS, Y_RANGE[0] + (cy + v) * VS, z, 0.5])
                owner.append(k)
    order = rng.permutation(len(pts))
    pts, owner = np.array(pts, dtype=F)[order], np.array(owner, dtype=np.int32)[order]
    assert np.all(pts[owner < 0, 2] <= F(-1.65)) and np.all(pts[owner < 0, 2] >= F(-1.75)) and np.all(pts[owner >= 0, 2] >= F(-1.25))
    words = np.where(owner >= 0, ((owner.astype(np.int64) + 1) << 16) | 10, 40).astype(np.int32)        # car | road
    return dict(points=pts, owner=owner, imap=imap, words=words)


def _scene_geometry():
    from mask_bev_amd import ops
    geom = ops.VoxelGeometry.from_ranges([X_RANGE[0], Y_RANGE[0], Z_RANGE[0], X_RANGE[1], Y_RANGE[1], Z_RANGE[1]], [VS, VS, 4.0])
    assert list(geom.grid) == [NXY, NXY, 1]
    return geom


def test_scene_ground_lift_labels_the_cars_and_only_the_cars(device, scene):
    from mask_bev_amd import ops
    from mask_bev_amd.metrics import DevicePanopticQuality, semantic_kitti_class_lut
    geom = _scene_geometry()
    scans = [torch.from_numpy(scene['points']).to(device)]
    imap = torch.from_numpy(scene['imap']).to(device)
    owner = torch.from_numpy(scene['owner'])
    gm = ops.ground_map(scans, geom, SCENE_RADIUS)
    lifted = ops.lift_instances(scans, imap, geom, 4, ground=gm, clearance=0.3)
    pq = lifted.point_query.cpu()
    assert bool((pq[owner < 0] == -1).all())                                   # every road point
    assert torch.equal(pq[owner >= 0], owner[owner >= 0])                      # every car point carries its query
    zg = lifted.z_ground.cpu()[0]
    assert bool(((zg[:3] >= -1.75) & (zg[:3] <= -1.65)).all()) and float(zg[3]) == 0.0
    assert lifted.counts.cpu()[0].tolist() == [3 * 8 * 18] * 3 + [0]
    # the restatement agrees, bit for bit
    ref_g = G.ground_map([scene['points']], geom.pc_range, geom.voxel_size, geom.grid, SCENE_RADIUS)
    assert np.array_equal(_bits(gm.ground.cpu().numpy()), _bits(ref_g['ground']))
    ref = G.lift_ground([scene['points']], scene['imap'], ref_g['ground'], geom.pc_range, geom.voxel_size, geom.grid, 4, 0.3)
    assert torch.equal(pq, torch.from_numpy(ref['point_query'])) and np.array_equal(_bits(zg.numpy()), _bits(ref['z_ground'][0]))
    # panoptic quality: exact with the ground, short of it without
    words = torch.from_numpy(scene['words']).to(device)
    query_class = torch.tensor([[1, 1, 1, 0]], dtype=torch.int32, device=device)
    results = []
    for labels in (lifted, ops.lift_instances(scans, imap, geom, 4)):
        metric = DevicePanopticQuality(2, semantic_kitti_class_lut(), min_points=1)
        metric.update(labels.point_query, query_class, words, [int(owner.shape[0])])
        results.append(metric.compute(reduce=False))
    with_ground, plain = results
    assert with_ground['pq'] == 1.0 and with_ground['sq'] == 1.0 and with_ground['rq'] == 1.0
    assert plain['sq'] < 1.0 and plain['pq'] < 1.0


def _scene_predictions(device, scene):
    from mask_bev_amd import batch as B
    from mask_bev_amd.predict import Predictions
    q = 4
    imap = torch.from_numpy(scene['imap']).to(device)
    maps = (imap + 1).permute(0, 2, 1).contiguous()                                 # (1, nx, ny), ids 1 .. 3
    labels, pm = B.instance_targets(maps, q, packed=True)
    scores = torch.tensor([[0.9, 0.8, 0.7, 0.0]], device=device)
    return Predictions(labels.to(torch.int32), scores, labels > 0, pm, None, None, imap, (NXY, NXY))


def test_scene_boxes_stand_on_the_ground(device, scene):
    from mask_bev_amd.predict import GroundSettings
    geom = _scene_geometry()
    p = _scene_predictions(device, scene)
    scans = [torch.from_numpy(scene['points']).to(device)]
    settings = GroundSettings(radius_m=SCENE_RADIUS * VS, clearance=0.3)
    assert settings.radius_cells(VS) == SCENE_RADIUS
    lifted = p.lift(scans, geom, ground=settings)
    out = p.boxes3d(scans, geom, X_RANGE, Y_RANGE, VS, ground=settings, bottom='ground')
    assert out['query'].cpu().tolist() == [0, 1, 2] and out['points'].cpu().tolist() == [3 * 8 * 18] * 3
    b3, zg, top = out['boxes3d'].cpu().numpy(), lifted.z_ground.cpu().numpy()[0, :3], lifted.z_max.cpu().numpy()[0, :3]
    assert np.array_equal(b3[:, 2], zg) and np.all((zg >= F(-1.75)) & (zg <= F(-1.65)))
    # h is the one f32 difference top - z_ground; adding it back to z_ground rounds once more: two half-ulps of values
    # below 2 m, 2^-24 each, bound what z_bottom + h can miss the highest kept return by
    assert np.array_equal(b3[:, 5], (top - zg).astype(F))
    assert np.all(np.abs((b3[:, 2] + b3[:, 5]).astype(np.float64) - top.astype(np.float64)) <= 2.0 ** -23)
    owner = scene['owner']
    want_top = np.array([scene['points'][owner == k, 2].max() for k in range(3)], dtype=F)
    assert np.array_equal(top, want_top)
    # bottom='points' with a ground: the lowest KEPT return; the plain lift reaches down to the road inside the mask
    kept = p.boxes3d(scans, geom, X_RANGE, Y_RANGE, VS, ground=settings)['boxes3d'].cpu().numpy()
    assert np.all(kept[:, 2] >= F(-1.25)) and np.array_equal(kept[:, 2], lifted.z_min.cpu().numpy()[0, :3])
    # the defaults: today's dictionary, key by key, from K31's own columns
    plain_lift = p.lift(scans, geom)
    assert plain_lift.z_ground is None
    plain = p.boxes3d(scans, geom, X_RANGE, Y_RANGE, VS)
    assert list(plain) == ['boxes', 'scores', 'scan', 'query', 'cells', 'boxes3d', 'points']
    bev = p.boxes(X_RANGE, Y_RANGE, VS)
    for key in ('boxes', 'scores', 'scan', 'query', 'cells'):
        assert torch.equal(plain[key], bev[key]), key
    b = bev['boxes']
    z, ztop = plain_lift.z_min[0, :3].to(b.device), plain_lift.z_max[0, :3].to(b.device)
    assert torch.equal(plain['boxes3d'], torch.stack([b[:, 0], b[:, 1], z, b[:, 2], b[:, 3], ztop - z, b[:, 4]], dim=1))
    assert torch.equal(plain['points'], plain_lift.counts.reshape(-1)[:3]) and bool((plain['boxes3d'][:, 2] < -1.6).all())
    dicts = p.kitti_predictions(X_RANGE, Y_RANGE, VS, scans=scans, module=geom, ground=settings, bottom='ground')
    assert len(dicts) == 1 and np.array_equal(dicts[0]['boxes3d'].cpu().numpy(), b3)
    assert torch.equal(p.kitti_predictions(X_RANGE, Y_RANGE, VS, scans=scans, module=geom)[0]['boxes3d'], plain['boxes3d'])
    with pytest.raises(ValueError, match="bottom='ground'"):
        p.boxes3d(scans, geom, X_RANGE, Y_RANGE, VS, bottom='ground')
    with pytest.raises(ValueError, match='32 cells'):
        p.lift(scans, geom, ground=GroundSettings(radius_m=8.5))


# ------------------------------------------------------------------------------------------------ the launcher
def test_launcher_writes_ground_aware_point_labels(device, tmp_path):
    """``write_point_labels`` with ``lift_ground: true`` writes ``pred.lift(..., ground=...)``; without the key, today's files."""
    from mask_bev_amd import batch as B
    from mask_bev_amd.evaluate import lift_settings, write_point_labels
    from mask_bev_amd.mask_bev_module import MaskBevModule
    kw = tiny_kwargs()
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    d = tmp_path / 'data' / 'sequences' / '08' / 'velodyne'
    d.mkdir(parents=True)
    scans = random_scans(kw, [1500, 1201], seed=3)
    files = []
    for i, s in enumerate(scans):
        s.numpy().tofile(d / f'{i:06d}.bin')
        files.append((d / f'{i:06d}.bin', None))
    part = [s.to(device) for s in scans]
    pred = model.predict(part)
    labelled = {}
    for name, extra in (('plain', {}), ('ground', {'lift_ground': True, 'lift_ground_radius': 1.0, 'lift_max_height': 2.0})):
        config = dict(kw, batch_size=2, **extra)
        settings = lift_settings(config)
        assert (settings is None) == (name == 'plain')
        paths = write_point_labels(model, config, device, files, tmp_path / name)
        lifted = pred.lift(part, model, ground=settings) if settings is not None else pred.lift(part, model)
        assert (lifted.z_ground is None) == (name == 'plain')
        labelled[name] = lifted.point_query.cpu().numpy().astype(np.int64)
        for s, path, want in zip(scans, paths, lifted.per_scan()):
            want = want.cpu().numpy().astype(np.int64)
            sem, inst = B.read_semantic_kitti_label(path)
            assert inst.shape[0] == s.shape[0] and np.array_equal(inst.astype(np.int64), want + 1)
            assert np.array_equal(sem, np.where(want >= 0, 10, 0))
    plain, ground = labelled['plain'], labelled['ground']
    assert (plain >= 0).sum() > 0 and np.all((ground == plain) | (ground == -1)) and (ground != plain).any()


def test_launcher_names_the_ground_settings(device, tmp_path, capsys):
    """``--test`` on ``dataset: kitti`` with ``kitti_3d: true``: with ``lift_ground: true`` one line names the settings in front
    of the AP block and the boxes stand on the estimated ground; without the key the output has no such line."""
    import os
    import shutil
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd.mask_bev_module import MaskBevModule
    sample = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kitti_object_sample')
    rng = np.random.default_rng(2)
    for k in ('velodyne', 'label_2', 'calib'):
        d = tmp_path / f'data_object_{k}' / 'training' / k
        d.mkdir(parents=True)
        for frame in (0, 1):
            if k == 'velodyne':
                rng.uniform([0, -10, -3, 0], [20, 10, 1, 1], (2000 + frame, 4)).astype(F).tofile(d / f'{frame:06d}.bin')
            else:
                shutil.copy(os.path.join(sample, k, '000000.txt'), d / f'{frame:06d}.txt')
    (tmp_path / 'val.txt').write_text('000000\n000001\n')
    (tmp_path / 'train.txt').write_text('000000\n000001\n')
    kw = dict(tiny_kwargs(), x_range=[0, 20], y_range=[-10, 10], z_range=[-3, 1], dataset='kitti', batch_size=1, kitti_3d=True)
    torch.manual_seed(0)
    model = MaskBevModule(**{k: v for k, v in kw.items() if k != 'kitti_3d'}).to(device)
    ck = tmp_path / 'ckpt'
    for name, extra in (('plain', {}), ('ground', {'lift_ground': True, 'lift_ground_radius': 1.0, 'lift_z_floor': -2.5})):
        (ck / name).mkdir(parents=True)
        launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'],
                                 ck / name / f'{name}-epoch=00-val_loss=1.000000.ckpt', 0, 'val_loss', 1.0)
        cfg = tmp_path / f'{name}.yml'
        cfg.write_text(yaml.safe_dump(dict(kw, **extra)))
        assert launcher.main(['--config', str(cfg), '--test', '--data-root', str(tmp_path), '--checkpoint-root', str(ck)]) == 0
        lines = capsys.readouterr().out.splitlines()
        named = [i for i, l in enumerate(lines) if l.startswith('ground-aware lift:')]
        bev = [i for i, l in enumerate(lines) if l.startswith('bev  AP:')]
        assert len(bev) == 2 and len([l for l in lines if l.startswith('3d   AP:')]) == 2
        if extra:
            assert len(named) == 1 and named[0] < bev[0]
            assert lines[named[0]] == 'ground-aware lift: radius 1 m (4 cells), clearance 0.3 m, z floor -2.5 m'
        else:
            assert named == []
