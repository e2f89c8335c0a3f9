"""K22 — SemanticKITTI scene → instance-id map on the device (csrc/rasterize.hip) against the numpy / scipy restatement
(tests/rasterize_ref.py) and the reference's recorded maps (tests/golden/rasterizer.npz).  Every comparison is exact:
the fixture's and the generated points keep away from cell edges and range bounds, so f64 rounding cannot move one."""
import numpy as np
import pytest
import torch

from tests import rasterize_ref as RR
from tests.test_rasterize_cpu import GOLDEN, load_case, restate

pytestmark = pytest.mark.gpu

BIG = ((-40, 40), (-40, 40), (-10, 10))


def _rasterizer(ranges, vs, **kw):
    from mask_bev_amd.rasterize import SemanticKittiRasterizer
    return SemanticKittiRasterizer(ranges[0], ranges[1], ranges[2], vs, **kw)


def _combined(poses, c):
    tf = np.linalg.inv(poses[c]) @ poses
    tf[:, 3, :] = [0, 0, 0, 1]
    return tf


class _Stub:
    pass


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'c_z', 'd', 'e'])
def test_fixture_cases(device, name):
    z = np.load(GOLDEN)
    points, labels, ranges, vs = load_case(z, name)
    poses, c = z['poses'], int(z['centre'])
    scene = RR.aggregate_scene(points, poses)
    settings = [(False, 1, f'{name}_map')] + ([(True, int(z['a_min_points']), 'a_map_unseen')] if name == 'a' else [])
    for remove_unseen, min_points, key in settings:
        want = restate(z, name, remove_unseen, min_points)
        r = _rasterizer(ranges, vs, remove_unseen=remove_unseen, min_points=min_points)
        centre = torch.from_numpy(labels[c].astype(np.int64)).to(device)
        # f32 per-scan points + one combined transform per scan
        got = r.rasterize([torch.from_numpy(p).to(device) for p in points],
                          [torch.from_numpy(i.astype(np.int64)).to(device) for i in labels], _combined(poses, c),
                          centre if remove_unseen else None, check_overflow=True)
        assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
        assert torch.equal(got.cpu().long(), torch.from_numpy(want))
        # the f64 world-frame scene as one scan
        got64 = r.rasterize(torch.from_numpy(scene).to(device), torch.from_numpy(np.concatenate(labels).astype(np.int64)).to(device),
                            np.linalg.inv(poses[c])[None], centre if remove_unseen else None, check_overflow=True)
        assert torch.equal(got64, got)
        # the reference's call on stand-in scan / scene objects
        scan, sc = _Stub(), _Stub()
        scan.velo_to_inv_pose, scan.inst_label = np.linalg.inv(poses[c]), labels[c]
        sc.point_cloud, sc.inst_label = scene, np.concatenate(labels)
        assert torch.equal(r.get_mask_around(scan, sc, device), got)
        if name != 'd':
            assert np.array_equal(got.cpu().numpy(), z[key])            # the reference's own recorded map


# ---------------------------------------------------------------------------------------------------------------
# K22b alone
# ---------------------------------------------------------------------------------------------------------------
def _pack(occ):
    """(S, nx, ny) {0, 1} -> (S, nx, ceil(ny / 32)) int32 bit images and (S, 4) bounding boxes."""
    s, nx, ny = occ.shape
    wpr = (ny + 31) // 32
    padded = np.zeros((s, nx, wpr * 32), dtype=np.uint64)
    padded[:, :, :ny] = occ
    words = (padded.reshape(s, nx, wpr, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    bbox = np.zeros((s, 4), dtype=np.int32)
    for i in range(s):
        xs, ys = np.nonzero(occ[i])
        bbox[i] = (xs.min(), ys.min(), xs.max(), ys.max()) if xs.size else (2 ** 31 - 1, 2 ** 31 - 1, -1, -1)
    return words.view(np.int32), bbox


def _paint(device, occ, ids, k, n_slots=None):
    from mask_bev_amd import ops
    words, bbox = _pack(occ)
    n = torch.tensor([len(ids) if n_slots is None else n_slots], dtype=torch.int32, device=device)
    got = ops.rasterize_paint(torch.from_numpy(words).to(device), torch.from_numpy(bbox).to(device),
                              torch.tensor(ids, dtype=torch.int32, device=device), n, occ.shape[2], k)
    return got.cpu().numpy()


@pytest.mark.parametrize('shape', [(70, 45), (64, 100), (50, 33), (37, 64)])
def test_morphology_random_blobs(device, shape):
    rng = np.random.default_rng(sum(shape))
    nx, ny = shape
    for k in range(1, 16, 2):
        occ = []
        for density in (0.05, 0.15, 0.3, 0.45, 0.6):
            o = np.zeros(shape, dtype=np.uint8)
            x0, y0 = int(rng.integers(0, nx // 2)), int(rng.integers(0, ny // 2))
            x1, y1 = int(rng.integers(x0 + 4, nx + 1)), int(rng.integers(y0 + 4, ny + 1))
            o[x0:x1, y0:y1] = rng.random((x1 - x0, y1 - y0)) < density
            occ.append(o)
        for edge in range(4):                                   # blobs on the four borders ...
            o = np.zeros(shape, dtype=np.uint8)
            sl = [(slice(0, 6), slice(5, ny - 5)), (slice(nx - 6, nx), slice(5, ny - 5)),
                  (slice(5, nx - 5), slice(0, 6)), (slice(5, nx - 5), slice(ny - 6, ny))][edge]
            o[sl] = rng.random(o[sl].shape) < 0.5
            occ.append(o)
        for cx, cy in ((0, 0), (0, ny - 5), (nx - 5, 0), (nx - 5, ny - 5)):      # ... and the four corners
            o = np.zeros(shape, dtype=np.uint8)
            o[cx:cx + 5, cy:cy + 5] = 1
            occ.append(o)
        occ = np.stack(occ)
        for s in range(len(occ)):                               # one at a time: no overlap hides a wrong cell
            if not occ[s].any():
                continue
            got = _paint(device, occ[s:s + 1], [s + 1], k)
            want = RR.paint_occupancies(occ[s:s + 1], [s + 1], k)
            assert np.array_equal(got, want), (shape, k, s)


def test_morphology_known_answers(device):
    o = np.zeros((3, 40, 50), dtype=np.uint8)
    o[0, 0:5, 0:5] = 1            # survives in the corner
    o[1, 17:22, 20:25] = 1        # vanishes inside
    o[2, 12:21, 30:39] = 1        # a 9 x 9 block survives
    got = _paint(device, o, [5, 6, 7], 9)
    want = np.zeros((40, 50), dtype=np.int64)
    want[0:5, 0:5] = 5
    want[12:21, 30:39] = 7
    assert np.array_equal(got, want)


def test_one_instance_fills_a_1024_grid(device):
    """The window (4 MB of cells = 128 KB of bits) does not fit the LDS images: the row-band path."""
    rng = np.random.default_rng(5)
    occ = (rng.random((1, 1024, 1024)) < 0.3).astype(np.uint8)
    occ[0, 300:420, 500:700] = 0                                # a hole the closing cannot fill
    occ[0, 0, 0] = occ[0, 1023, 1023] = 1
    for k in (9, 15):
        got = _paint(device, occ, [4242], k)
        assert np.array_equal(got, RR.paint_occupancies(occ, [4242], k)), k
    full = np.ones((1, 1024, 1024), dtype=np.uint8)
    assert (_paint(device, full, [9], 9) == 9).all()


def test_300_instances_and_unused_slots(device):
    rng = np.random.default_rng(6)
    ids = rng.choice(np.arange(1, 65536), 300, replace=False)
    occ = np.zeros((300, 200, 150), dtype=np.uint8)
    for s in range(300):
        x0, y0 = int(rng.integers(0, 180)), int(rng.integers(0, 130))
        sx, sy = int(rng.integers(6, 20)), int(rng.integers(6, 20))
        occ[s, x0:x0 + sx, y0:y0 + sy] = rng.random(occ[s, x0:x0 + sx, y0:y0 + sy].shape) < 0.7
    got = _paint(device, occ, ids.tolist(), 9)
    assert np.array_equal(got, RR.paint_occupancies(occ, ids, 9))
    got = _paint(device, occ, ids.tolist(), 9, n_slots=120)      # only the first 120 slots are in use
    assert np.array_equal(got, RR.paint_occupancies(occ[:120], ids[:120], 9))


# ---------------------------------------------------------------------------------------------------------------
# the whole path on made-up scenes
# ---------------------------------------------------------------------------------------------------------------
def _cell_points(rng, cells, ranges, vs, z=0.0):
    cells = np.asarray(cells, dtype=np.float64)
    off = rng.uniform(0.1, 0.9, cells.shape)
    xy = np.array([ranges[0][0], ranges[1][0]]) + (cells + off) * vs
    return np.hstack([xy, np.full((len(cells), 1), z), np.ones((len(cells), 1))]).astype(np.float32)


def _block_cells(x0, y0, sx, sy):
    return [(x, y) for x in range(x0, x0 + sx) for y in range(y0, y0 + sy)]


def test_overlap_highest_id_wins_independent_of_point_order(device):
    rng = np.random.default_rng(8)
    ranges, vs = ((-8, 8), (-8, 8), (-2, 2)), 0.16
    a, b = _block_cells(20, 20, 20, 12), _block_cells(34, 26, 20, 12)
    pts = np.concatenate([_cell_points(rng, a, ranges, vs), _cell_points(rng, b, ranges, vs)])
    inst = np.array([900] * len(a) + [31] * len(b), dtype=np.int64)
    r = _rasterizer(ranges, vs)
    maps = []
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(len(inst))
        maps.append(r.rasterize(torch.from_numpy(pts[perm]).to(device), torch.from_numpy(inst[perm]).to(device),
                                np.eye(4)[None], check_overflow=True))
    assert torch.equal(maps[0], maps[1]) and torch.equal(maps[0], maps[2])
    m = maps[0].cpu().numpy()
    assert (m[20:40, 20:32] == 900).all() and (m[34:54, 26:38][m[34:54, 26:38] != 900] == 31).all()
    assert (m[40:54, 26:38] == 31).all() and (m == 900).sum() == 240 and (m == 31).sum() == 240 - 6 * 6
    want = RR.get_mask_around(pts.astype(np.float64), inst, np.eye(4), *ranges, vs)
    assert np.array_equal(m, want)


def test_dropped_points_and_status_bits(device):
    from mask_bev_amd._lib import MaskBevHipError
    rng = np.random.default_rng(9)
    ranges, vs = ((-8, 8), (-8, 8), (-2, 2)), 0.16
    good = _cell_points(rng, _block_cells(30, 30, 12, 12), ranges, vs)
    bad = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1], [-8, 0, 0, 1], [8, 0, 0, 1], [0, -8, 0, 1],
                    [0, 8, 0, 1], [1, 1, -2, 1], [1, 1, 2, 1], [30, 0, 0, 1], [0, 0, 5, 1]], dtype=np.float32)
    unl = _cell_points(rng, _block_cells(60, 60, 10, 10), ranges, vs)
    pts = np.concatenate([good, bad, unl])
    inst = np.array([7] * len(good) + [8] * len(bad) + [0] * len(unl), dtype=np.int64)
    r = _rasterizer(ranges, vs)
    m = r.rasterize(torch.from_numpy(pts).to(device), torch.from_numpy(inst).to(device), np.eye(4)[None],
                    check_overflow=True).cpu().numpy()
    want = np.zeros((100, 100), dtype=np.int32)
    want[30:42, 30:42] = 7
    assert np.array_equal(m, want)
    # an id >= 65536
    pts2 = np.concatenate([pts, _cell_points(rng, _block_cells(70, 10, 10, 10), ranges, vs)])       # skipped points
    inst2 = np.concatenate([inst, [65536] * 50 + [-3] * 50])
    t2 = (torch.from_numpy(pts2).to(device), torch.from_numpy(inst2).to(device), np.eye(4)[None])
    assert np.array_equal(r.rasterize(*t2).cpu().numpy(), want)
    with pytest.raises(MaskBevHipError):
        r.rasterize(*t2, check_overflow=True)
    # more than max_instances instances: the smallest ids are kept, bit 0 is set
    cells = [_block_cells(5 + 14 * i, 10, 10, 10) for i in range(6)]
    pts3 = np.concatenate([_cell_points(rng, c, ranges, vs) for c in cells])
    inst3 = np.concatenate([[50 - i] * len(c) for i, c in enumerate(cells)]).astype(np.int64)
    few = _rasterizer(ranges, vs, max_instances=4)
    t3 = (torch.from_numpy(pts3).to(device), torch.from_numpy(inst3).to(device), np.eye(4)[None])
    m3 = few.rasterize(*t3).cpu().numpy()
    assert sorted(np.unique(m3).tolist()) == [0, 45, 46, 47, 48]
    with pytest.raises(IndexError):
        few.rasterize(*t3, check_overflow=True)
    assert sorted(np.unique(r.rasterize(*t3, check_overflow=True).cpu().numpy()).tolist()) == [0, 45, 46, 47, 48, 49, 50]


def make_big_scene(device, n_points=5_000_000, n_inst=60, labelled=0.03, seed=0, ranges=BIG, vs=0.16):
    """A scene of realistic size made on the device from a seed: 4 scans with their own poses, `labelled` of the points on
    `n_inst` car-sized instances (cell + offset in [0.1, 0.9] in the centre frame, taken back to the scan's frame and
    rounded to f32: at most 4e-6 m at 64 m, against a margin of 16 mm), the rest unlabelled anywhere."""
    g = torch.Generator(device=device).manual_seed(seed)
    rng = np.random.default_rng(seed)
    nx, ny = RR.grid_size(ranges[0], vs), RR.grid_size(ranges[1], vs)
    n_scans = 4
    per = n_points // n_scans
    tfs = []
    for s in range(n_scans):
        yaw, t = 0.05 * (s - 1.5), np.array([6.0 * (s - 1.5), 0.4 * s, 0.02 * s])
        m = np.eye(4)
        m[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
        m[:3, 3] = t
        tfs.append(m)
    tfs = np.stack(tfs)
    boxes = []
    for i in range(n_inst):
        sx, sy = (28, 12) if i % 2 else (12, 28)
        boxes.append((int(rng.integers(0, nx - sx)), int(rng.integers(0, ny - sy)), sx, sy))
    boxes_t = torch.tensor(boxes, dtype=torch.float64, device=device)
    ids = torch.from_numpy(rng.choice(np.arange(1, 65536), n_inst, replace=False)).to(device)
    lo = torch.tensor([ranges[0][0], ranges[1][0], ranges[2][0]], dtype=torch.float64, device=device)
    hi = torch.tensor([ranges[0][1], ranges[1][1], ranges[2][1]], dtype=torch.float64, device=device)
    points, inst = [], []
    for s in range(n_scans):
        pc = torch.rand((per, 4), generator=g, device=device, dtype=torch.float32)
        pc[:, :3] = (lo + (hi - lo) * (pc[:, :3].double() * 1.2 - 0.1)).float()
        lab = torch.zeros((per,), dtype=torch.int32, device=device)
        sel = torch.nonzero(torch.rand((per,), generator=g, device=device) < labelled).flatten()
        which = torch.randint(0, n_inst, (sel.numel(),), generator=g, device=device)
        u = torch.rand((sel.numel(), 4), generator=g, device=device, dtype=torch.float64)
        bx = boxes_t[which]
        cell = torch.floor(bx[:, :2] + u[:, :2] * bx[:, 2:])
        xy = lo[:2] + (cell + 0.1 + 0.8 * u[:, 2:]) * vs
        zc = torch.rand((sel.numel(), 1), generator=g, device=device, dtype=torch.float64) * 2 - 1
        centre = torch.cat([xy, zc, torch.ones_like(zc)], 1)
        local = centre @ torch.from_numpy(np.linalg.inv(tfs[s]).T).to(device)
        pc[sel, :3] = local[:, :3].float()
        lab[sel] = ids[which].to(torch.int32)
        points.append(pc)
        inst.append(lab)
    return points, inst, tfs


def test_realistic_scene(device):
    points, inst, tfs = make_big_scene(device)
    assert sum(p.shape[0] for p in points) >= 5_000_000
    r = _rasterizer(BIG, 0.16)
    got = r.rasterize(points, inst, tfs, check_overflow=True).cpu().numpy()
    lab_pts = [p[i != 0].cpu().numpy() for p, i in zip(points, inst)]
    lab_ids = np.concatenate([i[i != 0].cpu().numpy() for i in inst])
    assert 0.02 < len(lab_ids) / 5_000_000 < 0.04
    want = RR.get_mask_around(RR.aggregate_scene(lab_pts, tfs), lab_ids, np.eye(4), *BIG, 0.16)
    assert len(np.unique(want)) - 1 >= 50
    assert np.array_equal(got, want)


def test_scene_collate_equals_instance_map_collate(device):
    from mask_bev_amd import batch
    z = np.load(GOLDEN)
    points, labels, ranges, vs = load_case(z, 'a')
    poses, c = z['poses'], int(z['centre'])
    r = _rasterizer(ranges, vs)
    pc = points[c]
    sample = (pc, (points, labels, _combined(poses, c), None))
    for packed in (False, True):
        scans, (lab, masks) = batch.SceneCollate(r, 64, device, 5, packed)([sample, sample])
        scans2, (lab2, masks2) = batch.InstanceMapCollate(64, device, 5, packed)([(pc, z['a_map']), (pc, z['a_map'])])
        assert torch.equal(lab, lab2) and int(lab.sum()) == 2 * (len(np.unique(z['a_map'])) - 1)
        assert torch.equal(scans[0], scans2[0])
        if packed:
            assert torch.equal(masks.words, masks2.words)
        else:
            assert torch.equal(masks, masks2)


def test_training_step_on_a_scene_collate_batch(device):
    from mask_bev_amd import batch
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from tests.util_cfg import random_scans, tiny_kwargs
    torch.manual_seed(0)
    kw = tiny_kwargs(nx=80, ny=60, q=8)
    ranges, vs = (kw['x_range'], kw['y_range'], kw['z_range']), kw['voxel_size']
    r = _rasterizer(ranges, vs, morph_kernel_size=5)
    assert (r.nx, r.ny) == (80, 60)
    rng = np.random.default_rng(1)
    samples = []
    for b, pc in enumerate(random_scans(kw, [2500, 1999], seed=3)):
        cells = [_block_cells(10 + 20 * i, 8 + 12 * i + b, 12, 7) for i in range(3)]
        pts = np.concatenate([_cell_points(rng, cl, ranges, vs, z=-1.0) for cl in cells])
        inst = np.concatenate([[100 + i] * len(cl) for i, cl in enumerate(cells)])
        samples.append((pc, ([pts[::2], pts[1::2]], [inst[::2], inst[1::2]], np.stack([np.eye(4)] * 2), None)))
    scans, (labels, masks) = batch.SceneCollate(r, 8, device)(samples)
    assert labels.sum(1).tolist() == [3, 3] and tuple(masks.shape) == (2, 8, 60, 80)
    assert masks[:, :3].flatten(2).sum(2).eq(12 * 7).all()
    m = MaskBevModule(**kw).to(device).train()
    head = m._panoptic_head._panoptic_head
    head.num_points = 200
    head.point_seed = 3
    loss = m.training_step((scans, (labels, masks)), 0)
    m.scale_loss(loss).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss.detach()))


def test_outputs_and_workspace_stay_inside_their_buffers(device):
    """tests/test_guard_gpu.py's canaries around K22's output map and workspace: write-overruns only."""
    from mask_bev_amd import _lib, ops
    pad, canary = 256, 0xA5
    z = np.load(GOLDEN)

    def guarded(nbytes):
        rounded = (nbytes + 255) // 256 * 256
        raw = torch.full((rounded + 2 * pad,), canary, dtype=torch.uint8, device=device)
        return raw, raw[pad:pad + nbytes]

    def intact(raw, nbytes):
        return bool((raw[:pad] == canary).all()) and bool((raw[pad + nbytes:] == canary).all())

    for name, max_inst in (('b', 3), ('c', 7), ('a', 64)):
        points, labels, ranges, vs = load_case(z, name)
        poses, c = z['poses'], int(z['centre'])
        nx, ny = RR.grid_size(ranges[0], vs), RR.grid_size(ranges[1], vs)
        ws_bytes = _lib.load().mbv_rasterize_workspace_bytes(nx, ny, max_inst)
        raw_ws, ws = guarded(ws_bytes)
        raw_out, out = guarded(nx * ny * 4)
        offs = torch.from_numpy(z[f'{name}_offsets']).to(device)
        got, status, _ = ops.rasterize_scene(
            torch.from_numpy(np.concatenate(points)).to(device), torch.from_numpy(np.concatenate(labels).astype(np.int32)).to(device),
            offs, torch.from_numpy(_combined(poses, c)).to(device), None, *ranges, vs, nx, ny, 9, 1, max_inst,
            out=out.view(torch.int32).view(nx, ny), workspace=ws)
        torch.cuda.synchronize()
        assert intact(raw_ws, ws_bytes) and intact(raw_out, nx * ny * 4)
        assert int(status.item()) == 0
        assert np.array_equal(got.cpu().numpy(), z[f'{name}_map'])
