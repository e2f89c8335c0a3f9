"""K23 — training augmentations on the device (csrc/augment.hip) against the numpy restatement (tests/augment_ref.py):
the per-point op program, drops, shuffles and decimates, the instance-map warp, their agreement with K22 and K14, and the
launcher's use of the config's ``augmentations:`` list."""
import numpy as np
import pytest
import torch
import yaml

from tests import augment_ref as AR
from tests.test_augment_cpu import GENTLE

pytestmark = pytest.mark.gpu

# 0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099 points; batches of 1 to 4; an empty scan first, in the middle and last
BATCHES = [[1000], [0], [1], [0, 65, 4099], [63, 0, 257], [64, 256, 1, 0], [255, 4099], [4099, 1000, 257, 65]]
MAP_SHAPES = [(7, 5), (32, 32), (33, 64), (500, 500)]
ANGLES = [5.0, -3.7, 33.0, 90.0, 180.0]
# on 33 x 64 the origin's cell coordinates differ by a half: a 90 degree turn puts every source coordinate ON an integer
ANGLES_FOR = {(33, 64): [5.0, -3.7, 33.0, 91.3, 180.0]}
INF = float('inf')


def _A():
    from mask_bev_amd import augment
    return augment


def _scans(lengths, dim, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        pc = rng.uniform(-40, 40, (n, dim)).astype(np.float32)
        pc[:, 2] = rng.uniform(-3, 1, n)
        if dim == 4:
            pc[:, 3] = rng.uniform(0, 1, n)
        out.append(pc)
    return out


def _draws(lengths, ops_of, seed=0):
    A = _A()
    rng = np.random.default_rng(1000 + seed)
    return [A.SampleDraw(int(rng.integers(0, 1 << 64, dtype=np.uint64)), tuple(ops_of(b))) for b in range(len(lengths))]


def _apply(device, scans, draws, **kw):
    res = _A().DeviceAugmentation([]).apply([torch.from_numpy(s).to(device) for s in scans], draws=draws, **kw)
    return res, [v.cpu().numpy() for v in res.scans]


def _restate(scans, draws):
    return AR.augment_batch(scans, [(d.seed, list(d.ops)) for d in draws])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _ulp_diff(a, b):
    """Distance in f32 ulps between two arrays of finite floats of the same sign pattern."""
    ia, ib = _bits(a).astype(np.int64), _bits(b).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _flip(x, y):
    return _A().Op(1, 0, (-1. if x else 1., 0., 0., -1. if y else 1.))


def _jitter(mag, std, istd, lim=INF, ilim=INF):
    return _A().Op(2, 0, (mag, std, std, std, istd, lim, lim, lim, ilim))


def _drop(p):
    return _A().Op(3, _A().drop_threshold(p))


def _shuffle():
    return _A().Op(4)


def _decimate(k):
    return _A().Op(5, k)


# ---------------------------------------------------------------------------------------------------------------
# K23a
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [3, 4])
def test_flip_only_negates_columns_without_a_sync(device, dim, monkeypatch):
    for lengths in BATCHES:
        scans = _scans(lengths, dim)
        draws = _draws(lengths, lambda b: [_flip(b % 2 == 0, b % 3 != 0)] if b != 1 else [_flip(True, False), _flip(False, True)])
        with monkeypatch.context() as mp:                       # the no-removal path reads nothing back
            def no_sync(*a, **k):
                raise AssertionError('device -> host read on the no-removal path')
            for name in ('tolist', 'item', 'cpu', 'numpy'):
                mp.setattr(torch.Tensor, name, no_sync)
            res = _A().DeviceAugmentation([]).apply([torch.from_numpy(s).to(device) for s in scans], draws=draws)
        assert res.synced is False
        for b, (got, pc) in enumerate(zip(res.scans, scans)):
            want = pc.copy()
            sx, sy = np.diag(draws[b].matrix)
            want[:, 0] *= np.float32(sx)
            want[:, 1] *= np.float32(sy)
            assert got.shape == want.shape and np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (lengths, b)
        assert res.offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()


@pytest.mark.parametrize('dim', [3, 4])
def test_rotate_within_one_ulp_of_the_f64_restatement(device, dim):
    A = _A()
    for lengths in BATCHES:
        scans = _scans(lengths, dim, 1)
        draws = _draws(lengths, lambda b: [A.rotation_op([5.0, -3.7, 33.0, 180.0][b])] + ([A.rotation_op(90.0)] if b == 2 else []))
        res, got = _apply(device, scans, draws)
        assert res.synced is False
        for g, w, pc in zip(got, _restate(scans, draws), scans):
            assert g.shape == w.shape
            if len(g):
                print('rotate: max ulp', int(_ulp_diff(g[:, :2], w[:, :2]).max()))
                assert _ulp_diff(g[:, :2], w[:, :2]).max() <= 1           # double rounding only
            assert np.array_equal(_bits(g[:, 2:]), _bits(pc[:, 2:]))       # z, intensity untouched


@pytest.mark.parametrize('dim', [3, 4])
def test_jitter_against_the_restatement(device, dim):
    std, istd, mag = 0.05, 0.02, 1.5
    for lengths, lim, ilim in ((BATCHES[3], INF, INF), (BATCHES[7], 0.03, 0.01), (BATCHES[5], INF, 0.01)):
        scans = _scans(lengths, dim, 2)
        draws = _draws(lengths, lambda b: [_jitter(mag, std, istd, lim, ilim)] if b != 1 else [_flip(True, False), _jitter(mag, std, istd, lim, ilim)])
        res, got = _apply(device, scans, draws)
        for b, (g, w, pc) in enumerate(zip(got, _restate(scans, draws), scans)):
            assert g.shape == w.shape
            if not len(g):
                continue
            for c in range(dim):
                s = istd if c == 3 else std
                err = np.abs(g[:, c].astype(np.float64) - w[:, c])
                bound = 2.0 ** -22 * np.abs(w[:, c].astype(np.float64)) + 1e-5 * s * mag
                print(f'jitter c={c}: max err / bound', float((err / bound).max()))
                assert (err <= bound).all(), (lengths, b, c)
            if dim == 4:
                assert g[:, 3].min() >= 0 and g[:, 3].max() <= 1
            src = pc.copy()
            if b == 1:
                src[:, 0] = -src[:, 0]
            if lim != INF:                                                 # clipping is respected
                moved = np.abs(g[:, :3].astype(np.float64) - src[:, :3])
                assert (moved <= mag * lim + 2.0 ** -22 * np.abs(src[:, :3])).all()
                assert (moved > 0.9 * mag * lim).any()                     # and it does bite: std * 1 sigma > max_delta
            assert not np.array_equal(g[:, :3], src[:, :3])


def test_jitter_with_zero_std_changes_nothing(device):
    scans = _scans([257, 0, 1000], 4, 3)
    draws = _draws([257, 0, 1000], lambda b: [_jitter(1.5, 0.0, 0.0)])
    _, got = _apply(device, scans, draws)
    for g, pc in zip(got, scans):
        assert np.array_equal(_bits(g), _bits(pc))


def test_jitter_moments(device):
    n, sigma = 65536, 0.02
    pc = np.zeros((n, 4), dtype=np.float32)
    pc[:, 3] = 0.5
    draws = _draws([n], lambda b: [_jitter(1.0, sigma, sigma)], 5)
    _, (g,) = _apply(device, [pc], draws)
    for c in range(4):
        x = g[:, c].astype(np.float64) - (0.5 if c == 3 else 0.0)
        print(f'moments c={c}: mean {x.mean():.3e} var {x.var():.6e}')
        assert abs(x.mean()) <= 5 * sigma / np.sqrt(n)
        assert abs(x.var() - sigma ** 2) <= 5 * sigma ** 2 * np.sqrt(2.0 / n)


# ---------------------------------------------------------------------------------------------------------------
# K23b
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [3, 4])
def test_drop_keeps_exactly_the_restated_points(device, dim):
    for lengths in BATCHES:
        scans = _scans(lengths, dim, 4)
        probs = [0.3, 0.0, 1.0, 0.05]
        draws = _draws(lengths, lambda b: [_drop(probs[b])] + ([_drop(0.5)] if b == 0 else []))
        res, got = _apply(device, scans, draws)
        want = _restate(scans, draws)
        assert res.synced is True
        for b, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (lengths, b)
            if probs[b] == 0.0:
                assert len(g) == lengths[b]
            if probs[b] == 1.0:
                assert len(g) == 0
        counts = [len(w) for w in want]
        assert res.offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    if lengths == BATCHES[-1]:
        assert 0 < counts[0] < lengths[0]


@pytest.mark.parametrize('dim', [3, 4])
def test_shuffle_and_decimate(device, dim):
    for lengths in BATCHES:
        scans = _scans(lengths, dim, 6)
        programs = [[_shuffle()], [_flip(True, False)], [_drop(0.2), _decimate(3)], [_decimate(2), _shuffle(), _decimate(3)]]
        draws = _draws(lengths, lambda b: programs[b])
        res, got = _apply(device, scans, draws)
        want = _restate(scans, draws)
        for b, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (lengths, b)
        n0 = lengths[0]
        g0 = got[0]                                                         # a permutation of the scan
        assert len(g0) == n0 and np.array_equal(g0[np.lexsort(g0.T)], scans[0][np.lexsort(scans[0].T)])
        if n0 > 64:
            assert not np.array_equal(g0, scans[0])
        if len(lengths) > 1:                                                # no shuffle drawn: the order stays, next to a shuffled scan
            w1 = scans[1].copy()
            w1[:, 0] = -w1[:, 0]
            assert np.array_equal(_bits(got[1]), _bits(w1))
        if len(lengths) > 2:                                                # ceil(m / k) of the survivors, all of them survivors
            _, keep = AR.run_program(scans[2], draws[2].seed, list(draws[2].ops))
            assert len(got[2]) == -(-int(keep.sum()) // 3)
            surv = {r.tobytes() for r in scans[2][keep]}
            assert all(r.tobytes() in surv for r in got[2])
        if len(lengths) > 3:                                                # two decimates compose
            assert len(got[3]) == -(-(-(-lengths[3] // 2)) // 3)
        _, again = _apply(device, scans, draws)                             # run to run
        assert all(np.array_equal(_bits(a), _bits(g)) for a, g in zip(again, got))


def test_a_scan_gives_the_same_result_alone_and_inside_a_batch_of_four(device):
    lengths = [1000, 257, 4099, 65]
    scans = _scans(lengths, 4, 7)
    draws = _draws(lengths, lambda b: [_drop(0.1), _shuffle(), _jitter(1.0, 0.02, 0.01), _decimate(2)])
    _, got4 = _apply(device, scans, draws)
    want = _restate(scans, draws)
    for b in range(4):
        _, (alone,) = _apply(device, [scans[b]], [draws[b]])
        assert np.array_equal(_bits(alone), _bits(got4[b]))                 # the draws do not depend on the batch
        err = np.abs(got4[b].astype(np.float64) - want[b])
        assert got4[b].shape == want[b].shape and (err <= 2.0 ** -22 * np.abs(want[b]) + 1e-5 * 0.02).all()
        assert len(alone) == -(-int(AR.run_program(scans[b], draws[b].seed, list(draws[b].ops))[1].sum()) // 2)


@pytest.mark.parametrize('dim', [3, 4])
def test_reference_style_list_end_to_end(device, dim):
    A = _A()
    lengths = [4099, 1000, 257, 65]
    scans = _scans(lengths, dim, 8)
    spec = [dict(GENTLE[0], prob_drop=1), dict(GENTLE[1], prob_flip_y=1), dict(GENTLE[2], prob_shuffle=0.5),
            dict(GENTLE[3], rotate_prob=1), dict(GENTLE[4], prob_jitter=1)]
    aug = A.DeviceAugmentation(A.make_semantic_kitti_augmentation_list(spec), seed=11)
    draws = aug.draw(4)
    assert any(d.permutes for d in draws) and not all(d.permutes for d in draws)
    assert all([o.code for o in d.ops if o.code != 4] == [3, 1, 1, 2] for d in draws)
    res = aug.apply([torch.from_numpy(s).to(device) for s in scans], draws=draws)
    for b, (g, w) in enumerate(zip(res.scans, _restate(scans, draws))):
        g = g.cpu().numpy()
        assert g.shape == w.shape and 0.9 * lengths[b] < len(g) < lengths[b]
        err = np.abs(g.astype(np.float64) - w)
        std = np.array([0.02, 0.02, 0.02, 0.01])[:dim]
        assert (err <= 2.0 ** -22 * np.abs(w) + 1e-5 * std + 2.0 ** -23 * np.abs(w)).all()      # jitter's bound + the rotation's ulp
    # the same seed gives bit-identical outputs
    again = A.DeviceAugmentation(A.make_semantic_kitti_augmentation_list(spec), seed=11)
    res2 = again.apply([torch.from_numpy(s).to(device) for s in scans])
    assert res2.draws == draws and all(torch.equal(a, b) for a, b in zip(res.scans, res2.scans))


def test_refusals(device):
    A = _A()
    from mask_bev_amd._lib import MaskBevHipError
    aug = A.DeviceAugmentation([])
    with pytest.raises(MaskBevHipError):
        aug.apply([torch.zeros((5, 4))])
    with pytest.raises(ValueError):
        aug.apply([torch.zeros((5, 5), device=device)])
    with pytest.raises(ValueError):
        aug.apply([torch.zeros((5, 4), device=device)], instance_maps=torch.zeros((1, 4, 4), dtype=torch.int32, device=device),
                  draws=[A.SampleDraw(0, (_flip(True, False),))])           # no grid geometry given


# ---------------------------------------------------------------------------------------------------------------
# K23c
# ---------------------------------------------------------------------------------------------------------------
def _maps(shape, batch, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 5, (batch,) + shape).astype(np.int32) * rng.integers(1, 4000, (batch,) + shape).astype(np.int32)


@pytest.mark.parametrize('shape', MAP_SHAPES)
def test_warp_equals_the_restatement(device, shape):
    from mask_bev_amd import ops
    nx, ny = shape
    cx, cy = nx / 2, ny / 2
    mats = [np.eye(2), np.diag([-1., 1.]), np.diag([1., -1.]), np.diag([-1., -1.])] + [AR.rotation(t) for t in ANGLES_FOR.get(shape, ANGLES)]
    mats.append(AR.rotation(33.0) @ np.diag([1., -1.]))
    m = _maps(shape, len(mats), nx)
    want = []
    for a, mm in zip(mats, m):
        w, su, sv = AR.warp(mm, a, cx, cy)
        # the restated source coordinates keep away from the integers: f64 rounding cannot move a cell
        assert min(np.abs(su - np.rint(su)).min(), np.abs(sv - np.rint(sv)).min()) > 1e-9
        want.append(w)
    got = ops.warp_instance_maps(torch.from_numpy(m).to(device), torch.from_numpy(np.stack(mats)).to(device), cx, cy).cpu().numpy()
    for i in range(len(mats)):
        assert np.array_equal(got[i], want[i]), (shape, i)
    assert np.array_equal(got[0], m[0])                                      # identity
    assert np.array_equal(got[1], m[1][::-1]) and np.array_equal(got[2], m[2][:, ::-1])
    if nx == ny:
        assert np.array_equal(got[7], np.rot90(m[7], 1)) and np.array_equal(got[8], np.rot90(m[8], 2))
    if shape == (32, 32):                                                    # 33 degrees: the corners come from outside
        assert got[6][0, 0] == 0 and got[6][31, 31] == 0 and got[6][0, 31] == 0 and got[6][31, 0] == 0
    # an asymmetric range: everything mirrored in from outside the grid is 0
    off = ops.warp_instance_maps(torch.from_numpy(m[:1]).to(device), torch.from_numpy(np.diag([-1., 1.])[None]).to(device), 1.0, cy)
    assert np.array_equal(off[0].cpu().numpy(), AR.warp(m[0], np.diag([-1., 1.]), 1.0, cy)[0]) and not off[0, 2:].any()


# ---------------------------------------------------------------------------------------------------------------
# with K22 and K14
# ---------------------------------------------------------------------------------------------------------------
RANGES, VS = ((-8, 8), (-8, 8), (-2, 2)), 0.5


def _scene(seed=0):
    """Instances as blocks of cells, one point per cell at a cell-relative offset in [0.1, 0.9] (K22's tests' construction)."""
    rng = np.random.default_rng(seed)
    pts, inst = [], []
    for i, (x0, y0, sx, sy) in enumerate([(2, 3, 6, 5), (12, 20, 7, 6), (22, 4, 5, 9), (25, 25, 6, 6)]):
        cells = np.array([(x, y) for x in range(x0, x0 + sx) for y in range(y0, y0 + sy)], dtype=np.float64)
        xy = -8 + (cells + rng.uniform(0.1, 0.9, cells.shape)) * VS
        pts.append(np.hstack([xy, np.zeros((len(cells), 1)), np.ones((len(cells), 1))]).astype(np.float32))
        inst.append(np.full(len(cells), 300 + 7 * i, dtype=np.int64))
    return np.concatenate(pts), np.concatenate(inst)


def _rasterizer():
    from mask_bev_amd.rasterize import SemanticKittiRasterizer
    return SemanticKittiRasterizer(*RANGES, VS, morph_kernel_size=3)


def test_rasterising_the_transformed_scene_equals_warping_the_map(device):
    from mask_bev_amd import ops
    A = _A()
    pts, inst = _scene()
    r = _rasterizer()
    tp, ti = torch.from_numpy(pts).to(device), torch.from_numpy(inst).to(device)
    base = r.rasterize(tp, ti, np.eye(4)[None], check_overflow=True)
    assert len(torch.unique(base)) == 5
    for ops_ in ([_flip(True, False)], [_flip(False, True)], [_flip(True, True)], [A.rotation_op(90.0)],
                 [_flip(True, False), A.rotation_op(90.0)]):
        d = A.SampleDraw(1, tuple(ops_))
        res = A.DeviceAugmentation([], 0, RANGES[0], RANGES[1], VS).apply([tp], instance_maps=base[None],
                                                                           scene_transforms=[np.eye(4)[None]], draws=[d])
        assert np.array_equal(res.scene_transforms[0][0, 3], [0, 0, 0, 1])
        scene_map = r.rasterize(tp, ti, res.scene_transforms[0], check_overflow=True)
        assert torch.equal(scene_map, res.instance_maps[0]) and not torch.equal(scene_map, base)
        assert torch.equal(res.instance_maps[0], ops.warp_instance_maps(base[None], torch.from_numpy(d.matrix[None]).to(device), 16., 16.)[0])


def test_collates_with_an_augmentation_match_their_own_maps(device):
    from mask_bev_amd import batch
    A = _A()
    pts, inst = _scene(1)
    r = _rasterizer()
    spec = [{'name': 'drop', 'prob_drop': 1, 'per_point_drop_prob': 0.2}, {'name': 'flip', 'prob_flip_x': 0.5, 'prob_flip_y': 0.5},
            {'name': 'jitter', 'prob_jitter': 1, 'jitter_std': 0.01}]
    mk = lambda: A.DeviceAugmentation(A.make_semantic_kitti_augmentation_list(spec), 5, RANGES[0], RANGES[1], VS)
    pcs = _scans([1000, 257, 65], 4, 9)
    base = r.rasterize(torch.from_numpy(pts).to(device), torch.from_numpy(inst).to(device), np.eye(4)[None]).cpu().numpy()
    dev_pcs = [torch.from_numpy(p).to(device) for p in pcs]
    for packed in (False, True):
        # cached maps, K23c
        scans, (labels, masks) = batch.InstanceMapCollate(8, device, 0, packed, augmentation=mk())([(p, base) for p in pcs])
        ref = mk()
        draws = ref.draw(3)
        assert len({tuple(map(tuple, d.matrix)) for d in draws}) > 1         # the samples draw different flips
        res = ref.apply(dev_pcs, instance_maps=torch.from_numpy(base).to(device)[None].expand(3, -1, -1), draws=draws)
        lab2, masks2 = batch.instance_targets(res.instance_maps, 8, 0, packed)
        assert torch.equal(labels, lab2) and all(torch.equal(a, b) for a, b in zip(scans, res.scans))
        assert torch.equal(masks.words, masks2.words) if packed else torch.equal(masks, masks2)
        assert all(0.7 * len(p) < len(s) < len(p) for s, p in zip(scans, pcs)) and labels.sum(1).tolist() == [4, 4, 4]
        # scenes, rasterised after the transform: the same targets, since a flip of the scene is exact
        sample = lambda p: (p, ([pts[::2], pts[1::2]], [inst[::2], inst[1::2]], np.stack([np.eye(4)] * 2), None))
        scans3, (lab3, masks3) = batch.SceneCollate(r, 8, device, 0, packed, augmentation=mk())([sample(p) for p in pcs])
        assert torch.equal(lab3, labels) and all(torch.equal(a, b) for a, b in zip(scans3, scans))
        assert torch.equal(masks3.words, masks.words) if packed else torch.equal(masks3, masks)
    # augmentation=None: what the collate built before
    s0, (l0, m0) = batch.InstanceMapCollate(8, device)([(p, base) for p in pcs])
    l1, m1 = batch.instance_targets(torch.from_numpy(base).to(device)[None].expand(3, -1, -1).contiguous(), 8)
    assert torch.equal(l0, l1) and torch.equal(m0, m1) and all(torch.equal(a, b) for a, b in zip(s0, dev_pcs))


# ---------------------------------------------------------------------------------------------------------------
# the launcher
# ---------------------------------------------------------------------------------------------------------------
def test_launcher_augments_training_batches_only(device, tmp_path):
    from mask_bev_amd.datasets import SemanticKittiCacheBatches
    pts, inst = _scene(2)
    r = _rasterizer()
    base = r.rasterize(torch.from_numpy(pts).to(device), torch.from_numpy(inst).to(device), np.eye(4)[None]).cpu().numpy()
    seq = tmp_path / 'sequences' / '00'
    (seq / 'velodyne').mkdir(parents=True)
    (seq / 'mask_cache').mkdir()
    pcs = _scans([257, 1000], 4, 10)
    for i, pc in enumerate(pcs):
        pc.tofile(seq / 'velodyne' / f'{i:06d}.bin')
        np.save(seq / 'mask_cache' / f'{i:06d}.npy', base)
    config = yaml.safe_load("""
x_range: [-8, 8]
y_range: [-8, 8]
voxel_size: 0.5
num_queries: 8
batch_size: 2
shuffle_train: false
seed: 3
augmentations:
  - name: 'flip'
    prob_flip_x: 1
    prob_flip_y: 0
  - name: 'drop'
    prob_drop: 1
    per_point_drop_prob: 0.25
""")
    train = SemanticKittiCacheBatches(config, device, 0, 1, tmp_path, [0], augment=True)
    val = SemanticKittiCacheBatches(config, device, 0, 1, tmp_path, [0])
    assert train.augmentation is not None and len(train.augmentation.transforms) == 2 and val.augmentation is None
    torch.manual_seed(0)
    vs, (vl, vm) = val.batch(0, 0)
    torch.manual_seed(0)
    ts, (tl, tm) = train.batch(0, 0)
    torch.manual_seed(0)
    ts2, (_, tm2) = train.batch(0, 0)
    torch.manual_seed(0)
    ts3, _ = train.batch(1, 0)
    for v, t, t2, t3, pc in zip(vs, ts, ts2, ts3, pcs):
        assert sorted(map(tuple, v.cpu().numpy().tolist())) == sorted(map(tuple, pc.tolist()))       # validation: the file's points
        assert 0.5 * len(pc) < len(t) < len(pc)
        kept = {row.tobytes() for row in (v.cpu().numpy() * np.array([-1, 1, 1, 1], dtype=np.float32))}
        assert all(row.tobytes() in kept for row in t.cpu().numpy())                                # training: flipped survivors
        assert torch.equal(t, t2) and not (len(t) == len(t3) and torch.equal(t, t3))                # seeded by (epoch, batch)
    assert torch.equal(tl, vl) and torch.equal(tm, vm.flip(-1)) and torch.equal(tm, tm2) and not torch.equal(tm, vm)
