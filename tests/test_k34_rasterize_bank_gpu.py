"""K34 — ``mbv_rasterize_bank`` (csrc/rasterize.hip): the scenes of a whole batch rasterised in place from a scene bank on the
device, and what is built on it: ``SemanticKittiRasterizer.rasterize_bank``, ``batch.BankSceneCollate``,
``datasets.SemanticKittiSceneBatches`` and the launcher's ``semantic_kitti_targets: scenes``, ``--build-scene-bank`` and
``--build-mask-cache``.

Every comparison is exact.  The kernel is pinned bit for bit against ``SemanticKittiRasterizer.rasterize`` (K22) on the scans the
tables name; against the numpy restatement the points keep 0.15 m away from every cell edge, so neither the f32 storage
(2e-6 m at these coordinates) nor f64 rounding can move one."""
import numpy as np
import pytest
import torch

from tests import rasterize_ref as RR
from tests import scene_bank_util as U
from tests.util_cfg import tiny_kwargs

pytestmark = pytest.mark.gpu

RANGES = ((-12.0, 12.0), (-10.0, 10.0), (-3.0, 1.0))            # 48 x 40 cells of 0.5 m
VS = 0.5
CARS = [(-6.0, -4.0), (3.0, 5.0), (7.0, -5.0)]                  # in the frame of scan 0
N_SCANS = 8


def _rasterizer(**kw):
    from mask_bev_amd.rasterize import SemanticKittiRasterizer
    return SemanticKittiRasterizer(*RANGES, VS, **kw)


def _tf(s):
    """scan s → the frame of scan 0; scan 0's is the identity exactly."""
    return U.pose_2d(0.7 * s, 0.3 * s, 0.05 * s)


def _bank(device, scans):
    from mask_bev_amd.scene_bank import SceneBank
    return SceneBank(np.concatenate([p for p, _ in scans]), np.concatenate([i for _, i in scans]),
                     np.concatenate([[0], np.cumsum([len(i) for _, i in scans])]), device=device)


def _scans(seed=0, cars=CARS, n_car=(83, 97, 71)):
    """Eight scans of 251 … 400 points, every one labelled: the three cars seen from every scan."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(N_SCANS):
        pts = [U.into_frame(U.square(rng, c, 4.0, n), _tf(s)) for c, n in zip(cars, n_car)]
        ids = [np.full(n, i + 1, np.int32) for i, n in enumerate(n_car[:len(cars)])]
        out.append([np.concatenate(pts), np.concatenate(ids)])
    return out


def _add(scan, pts, ids):
    scan[0] = np.concatenate([scan[0], np.asarray(pts, np.float32).reshape(-1, 3)])
    scan[1] = np.concatenate([scan[1], np.asarray(ids, np.int32).reshape(-1)])


def _reference(r, bank, scans, tf, centre=None):
    """K22 on the listed scans of the bank: (map, status)."""
    from mask_bev_amd import ops
    if len(scans) == 0:
        pts, inst = torch.empty((0, 3), device=bank.device), torch.empty((0,), dtype=torch.int32, device=bank.device)
        offs, tf = [0, 0], np.eye(4)[None]
    else:
        pts, inst = [bank.scan(s)[0] for s in scans], [bank.scan(s)[1] for s in scans]
        offs = None
    c = None if centre is None else bank.scan(centre)[1]
    m = r.rasterize(pts, inst, tf, c, scan_offsets=offs)
    if len(scans):
        pts, inst = torch.cat(pts), torch.cat(inst)
        offs = np.concatenate([[0], np.cumsum([len(bank.scan(s)[1]) for s in scans])])
    _, st, _ = ops.rasterize_scene(pts, inst, torch.tensor(offs, dtype=torch.int32, device=bank.device),
                                   torch.from_numpy(np.ascontiguousarray(tf)).to(bank.device), c if r.remove_unseen else None,
                                   *RANGES, VS, r.nx, r.ny, r.morph_kernel_size, r.min_points, r.max_instances)
    return m, st


def _bank_call(r, bank, tables, **kw):
    from mask_bev_amd import ops
    maps, status, _ = ops.rasterize_bank(bank.points, bank.inst, *tables, *RANGES, VS, r.nx, r.ny, r.morph_kernel_size,
                                         r.min_points, r.max_instances, **kw)
    return maps, status


# ---------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 5])
def test_bit_equal_to_k22_in_one_call(device, k):
    """B = 3: non-contiguous segments without remove_unseen; remove_unseen with an id short of min_points and a present id
    without a kept point; no segment at all.  Points on the range bounds, NaN and inf; segments cut into several chunks."""
    scans = _scans()
    nxt = lambda v, to: np.nextafter(np.float32(v), np.float32(to))
    # scan 0 (identity transform): points exactly on a bound are not kept, their neighbours inside are
    _add(scans[0], [[12.0, 0.0, -1.0], [-12.0, 1.0, -1.0], [0.0, 10.0, -1.0], [0.0, -10.0, -1.0], [1.0, 1.0, 1.0], [1.0, 1.0, -3.0],
                    [nxt(12, 0), 0.0, -1.0], [nxt(-12, 0), 1.0, -1.0], [0.0, nxt(10, 0), -1.0], [np.nan, 0.0, -1.0],
                    [0.0, np.inf, -1.0], [0.0, 0.0, -np.inf]], [1, 1, 2, 2, 3, 3, 1, 1, 2, 2, 3, 3])
    rng = np.random.default_rng(11)
    # scan 4, the centre of sample 2: id 7 with 2 labels (< min_points), id 9 with 5 labels and every point out of range
    _add(scans[4], U.into_frame(U.square(rng, (-2.0, 6.0), 3.0, 2), _tf(4)), [7, 7])
    _add(scans[4], U.into_frame(U.square(rng, (50.0, 0.0), 3.0, 5), _tf(4)), [9] * 5)
    _add(scans[5], U.into_frame(U.square(rng, (-2.0, 6.0), 3.0, 60), _tf(5)), [7] * 60)        # id 7 seen well from scan 5
    _add(scans[7], U.into_frame(U.square(rng, (-8.0, 6.0), 3.0, 50), _tf(7)), [11] * 50)       # id 11: not in the centre scan
    bank = _bank(device, scans)
    assert bank.points.shape[0] % 4 != 0 and any(int(o) % 4 for o in bank.scan_offsets[1:-1])
    assert all(200 <= len(i) <= 400 for _, i in scans)
    seen, unseen = _rasterizer(morph_kernel_size=k, remove_unseen=True, min_points=3), _rasterizer(morph_kernel_size=k, min_points=3)
    shift = U.pose_2d(1.0, -0.5, 0.1)
    scenes = [([0, 2, 3, 6], np.stack([_tf(s) for s in (0, 2, 3, 6)]), 0),
              ([3, 4, 5, 7], np.stack([shift @ _tf(s) for s in (3, 4, 5, 7)]), 4),
              ([], np.zeros((0, 4, 4)), 4)]
    tables = list(seen.bank_tables(bank, scenes))
    assert tables[5].tolist() == [len(scans[0][1]), len(scans[4][1]), len(scans[4][1])]
    tables[5][0] = -1                                                  # sample 1: remove_unseen off
    maps, status = _bank_call(seen, bank, tables)
    want = [_reference(unseen, bank, *scenes[0][:2]), _reference(seen, bank, *scenes[1]), _reference(seen, bank, *scenes[2])]
    for b in range(3):
        assert torch.equal(maps[b], want[b][0]), b
        assert torch.equal(status[b:b + 1], want[b][1]), b
    assert status.tolist() == [0, 0, 0]
    got = maps.cpu().numpy()
    assert set(np.unique(got[0])) == {0, 1, 2, 3} and set(np.unique(got[1])) == {0, 1, 2, 3} and not got[2].any()
    if k == 1:
        assert got[0][47, 20] == 1 and got[0][0, 22] == 1 and got[0][24, 39] == 2        # the neighbours of the bounds
    # with remove_unseen off for sample 2 as well, ids 7 and 11 appear: the centre scan is what removed them
    both = unseen.rasterize_bank(bank, scenes)
    assert torch.equal(both[0], maps[0]) and torch.equal(both[1], _reference(unseen, bank, *scenes[1][:2])[0])
    assert {7, 11} <= set(np.unique(both[1].cpu().numpy())) and not both[2].any()
    assert torch.equal(seen.rasterize_bank(bank, scenes[1:])[0], maps[1])
    # several chunks per segment, chunk edges off the quad grid; and twice the same call
    for chunk in (4, 64, 100):
        m2, s2 = _bank_call(seen, bank, tables, chunk_points=chunk)
        assert torch.equal(m2, maps) and torch.equal(s2, status), chunk
    m3, s3 = _bank_call(seen, bank, tables, out=torch.full_like(maps, 77))
    assert torch.equal(m3, maps) and torch.equal(s3, status)


def test_agrees_with_the_numpy_restatement(device):
    """Three instances that no closing can join, points at cell centres ± 0.2 cell, spread over non-contiguous scans."""
    rng = np.random.default_rng(3)
    blocks = {4: (3, 4, 9, 8), 9: (20, 25, 10, 7), 300: (34, 6, 11, 12)}          # id: x0, y0, cells along x, along y
    chosen, tfs = [1, 4, 5], {s: _tf(s) for s in range(7)}
    scans = [[np.zeros((0, 3), np.float32), np.zeros((0,), np.int32)] for _ in range(7)]
    for s in (0, 2, 3, 6):                                                     # scans the scene does not name
        _add(scans[s], U.into_frame(U.square(rng, (0.0, 0.0), 6.0, 200), tfs[s]), [50] * 200)
    for ident, (x0, y0, w, h) in blocks.items():
        cells = np.stack(np.meshgrid(np.arange(x0, x0 + w), np.arange(y0, y0 + h), indexing='ij'), -1).reshape(-1, 2)
        cells = cells[rng.random(len(cells)) < 0.8]                            # holes for the closing to fill
        for rep in range(3):
            xy = (cells + 0.5 + (rng.random(cells.shape) - 0.5) * 0.4) * VS + [RANGES[0][0], RANGES[1][0]]
            world = np.concatenate([xy, np.full((len(xy), 1), -1.0)], 1)
            _add(scans[chosen[rep]], U.into_frame(world, tfs[chosen[rep]]), [ident] * len(xy))
    assert all(200 <= len(scans[s][1]) <= 400 for s in range(7))
    bank = _bank(device, scans)
    tf = np.stack([tfs[s] for s in chosen])
    r = _rasterizer(morph_kernel_size=5)
    scene = RR.aggregate_scene([scans[s][0] for s in chosen], tf)
    want, masks = RR.get_mask_around(scene, np.concatenate([scans[s][1] for s in chosen]), np.eye(4), *RANGES, VS,
                                     morph_kernel_size=5, return_masks=True)
    stack = np.stack([masks[i] for i in sorted(masks)]).astype(np.int64)
    assert sorted(masks) == [4, 9, 300] and stack.sum(0).max() == 1 and stack.any((1, 2)).all()      # disjoint: no paint order
    got = r.rasterize_bank(bank, [(chosen, tf, None)], check_overflow=True)
    assert tuple(got.shape) == (1, 48, 40) and got.dtype == torch.int32
    assert np.array_equal(got[0].cpu().numpy(), want)


def test_reads_only_its_segments(device):
    """Car points between the named scans and after the last one, where the expected map is empty: they change nothing."""
    rng = np.random.default_rng(5)
    base = _scans(seed=2, cars=CARS[:2], n_car=(120, 131))
    named = [0, 2, 4]
    tf = np.stack([_tf(s) for s in named])
    r = _rasterizer(morph_kernel_size=5)
    results = []
    for version, (where, ident, n) in enumerate([((7.0, -5.0), 5, 150), ((-7.0, 6.0), 6, 222)]):
        scans = [[p.copy(), i.copy()] for p, i in base[:6]]
        for s in (1, 3, 5):                                        # a car of their own, seen from the frame before them
            scans[s] = [U.into_frame(U.square(rng, where, 4.0, n), _tf(s - 1)), np.full(n, ident, np.int32)]
        bank = _bank(device, scans)
        want = _reference(r, bank, named, tf)[0]
        decoyed = _reference(r, bank, [0, 1, 2, 4], np.stack([_tf(s) for s in (0, 0, 2, 4)]))[0]
        assert (decoyed == ident).any() and not (want == ident).any()       # they WOULD paint cells that stay empty
        got = r.rasterize_bank(bank, [(named, tf, None), (named[::-1], tf[::-1], None)])
        assert torch.equal(got[0], want) and torch.equal(got[1], want)
        results.append(got)
    assert torch.equal(results[0], results[1]) and set(np.unique(results[0].cpu().numpy())) == {0, 1, 2}


def test_status_bits_per_sample(device):
    from mask_bev_amd._lib import MaskBevHipError
    scans = _scans(seed=4)[:3]
    scans[1] = [scans[1][0][scans[1][1] != 2], scans[1][1][scans[1][1] != 2]]         # two instances only
    wide = scans[2][1].copy()
    wide[wide == 3] = 70000                                                       # not a 16-bit id
    scans[2] = [scans[2][0], wide]
    bank = _bank(device, scans)
    r = _rasterizer(morph_kernel_size=5, max_instances=2)
    scenes = [([s], _tf(s)[None], None) for s in range(3)]
    maps, status = _bank_call(r, bank, r.bank_tables(bank, scenes))
    for b in range(3):
        m, st = _reference(r, bank, *scenes[b][:2])
        assert torch.equal(maps[b], m) and torch.equal(status[b:b + 1], st), b
    assert status.tolist() == [1, 0, 2]
    got = maps.cpu().numpy()
    assert [sorted(np.unique(g).tolist()) for g in got] == [[0, 1, 2], [0, 1, 3], [0, 1, 2]]
    with pytest.raises(IndexError, match='max_instances'):
        r.rasterize_bank(bank, scenes[:2], check_overflow=True)
    with pytest.raises(MaskBevHipError, match='65535'):
        r.rasterize_bank(bank, scenes[1:], check_overflow=True)
    assert torch.equal(r.rasterize_bank(bank, scenes[1:2], check_overflow=True)[0], maps[1])


def test_arguments(device):
    from mask_bev_amd import _lib, ops
    from mask_bev_amd._lib import MaskBevHipError
    lib = _lib.load()
    none = [None] * 2
    assert lib.mbv_rasterize_bank(*none, 0, *none, 0, None, None, 0, 0, *none, 0, 0., 0., 0., 0., 0., 0., 0., 0, 0, 0, 0, 0, 0,
                                  *none, None, 0, None) == 0                  # B = 0: before any pointer is checked
    assert lib.mbv_rasterize_bank_workspace_bytes(0, 48, 40, 16) == 0 and lib.mbv_rasterize_bank_workspace_bytes(2, 48, 0, 16) == 0
    one, three = lib.mbv_rasterize_workspace_bytes(48, 40, 16), lib.mbv_rasterize_bank_workspace_bytes(3, 48, 40, 16)
    assert 0 < one <= three <= 3 * one
    bank = _bank(device, _scans(seed=6)[:2])
    r = _rasterizer(morph_kernel_size=5)
    tables = list(r.bank_tables(bank, [([0, 1], np.stack([_tf(0), _tf(1)]), None)]))
    n = bank.points.shape[0]
    for change in ({0: np.array([0, n - 3])}, {1: np.array([5, n])}, {0: np.array([-1, 0])}, {2: np.array([0, 3])},
                   {4: np.array([n]), 5: np.array([1])}):
        bad = [change.get(i, t) for i, t in enumerate(tables)]
        with pytest.raises(MaskBevHipError, match='MBV_ERR_BAD_ARG'):
            _bank_call(r, bank, bad)
    with pytest.raises(MaskBevHipError, match='MBV_ERR_BAD_ARG'):
        _bank_call(r, bank, tables, chunk_points=6)
    with pytest.raises(MaskBevHipError):
        ops.rasterize_bank(bank.points[1:], bank.inst[1:], *tables, *RANGES, VS, r.nx, r.ny)       # not 16-byte aligned
    with pytest.raises(MaskBevHipError, match='no CPU fallback'):
        r.rasterize_bank(bank.to('cpu'), [([0], _tf(0)[None], None)])
    with pytest.raises(ValueError, match='centre scan'):
        _rasterizer(remove_unseen=True).rasterize_bank(bank, [([0], _tf(0)[None], None)])
    with pytest.raises(IndexError):
        r.rasterize_bank(bank, [([2], _tf(0)[None], None)])
    assert tuple(_bank_call(r, bank, r.bank_tables(bank, [([0], _tf(0)[None], None)]))[0].shape) == (1, 48, 40)


# ---------------------------------------------------------------------------------------------------------------
# the collate
# ---------------------------------------------------------------------------------------------------------------
def test_bank_collate_equals_scene_collate(device):
    from mask_bev_amd import augment as A
    from mask_bev_amd import batch
    banks = {'a': _bank(device, _scans(seed=8)), 3: _bank(device, _scans(seed=9, cars=CARS[:2], n_car=(140, 111)))}
    r = _rasterizer(morph_kernel_size=5)
    rng = np.random.default_rng(2)
    pcs = [rng.standard_normal((n, 4)).astype(np.float32) * 4 for n in (300, 257, 201, 333)]
    picks = [('a', [0, 2, 5], 2), (3, [1, 2], 1), ('a', [6, 7], 7), (3, [0, 3, 4, 7], 3)]
    bank_samples, scene_samples = [], []
    for pc, (key, scans, centre) in zip(pcs, picks):
        tf = np.stack([np.linalg.inv(_tf(centre)) @ _tf(s) for s in scans])
        bank_samples.append((pc, (key, np.array(scans), tf, centre)))
        scene_samples.append((pc, ([banks[key].scan(s)[0] for s in scans], [banks[key].scan(s)[1] for s in scans], tf, None)))
    spec = [{'name': 'flip', 'prob_flip_x': 0.5, 'prob_flip_y': 0.5}, {'name': 'rotate', 'rotate_prob': 1, 'rotation_range': 30}]
    mk = lambda: A.DeviceAugmentation(A.make_semantic_kitti_augmentation_list(spec), 5, RANGES[0], RANGES[1], VS)
    plain = None
    for packed in (False, True):
        for aug in (None, mk):
            a = None if aug is None else aug()
            b = None if aug is None else aug()
            if a is not None:
                a.reseed(5, 0, 1, 2)
                b.reseed(5, 0, 1, 2)
            s1, (l1, m1) = batch.BankSceneCollate(r, banks, 8, device, 0, packed, augmentation=a)(bank_samples)
            s2, (l2, m2) = batch.SceneCollate(r, 8, device, 0, packed, augmentation=b)(scene_samples)
            assert torch.equal(l1, l2) and l1.sum(1).tolist() == [3, 2, 3, 2]
            assert all(torch.equal(x, y) for x, y in zip(s1, s2))
            assert torch.equal(m1.words, m2.words) if packed else torch.equal(m1, m2)
            if not packed:
                assert tuple(m1.shape) == (4, 8, 40, 48) and bool(m1[:, :2].flatten(2).any(2).all())
                if aug is None:
                    plain = m1
                else:
                    assert not torch.equal(m1, plain)                    # the augmentation moved the targets
    # one sequence in the batch: the maps come straight from the one call
    s3, (l3, m3) = batch.BankSceneCollate(r, banks, 8, device)([bank_samples[0], bank_samples[2]])
    assert torch.equal(m3, plain[[0, 2]]) and l3.sum(1).tolist() == [3, 3]
    # metadata rides along
    assert batch.BankSceneCollate(r, banks, 8, device)([s + ('meta',) for s in bank_samples])[2] == ['meta'] * 4


# ---------------------------------------------------------------------------------------------------------------
# readers and launcher: a tree as downloaded, no mask cache
# ---------------------------------------------------------------------------------------------------------------
def _tree(root, kw, seqs=((8, 4),), seed=3):
    """Sequences of scans of 300 points with two cars each, on the tiny model's 80 x 80 grid of 0.25 m cells."""
    rng = np.random.default_rng(seed)
    half = (kw['x_range'][1], kw['y_range'][1])
    for seq, n in seqs:
        poses, scans, words = U.drive(rng, n, [(4.0, 3.5), (-3.0, -4.5)], 3.5, half)
        U.write_sequence(root / 'sequences' / f'{seq:02d}', poses, scans, words)


def _config(kw, **more):
    cfg = dict(dict(kw, dataset='semantic-kitti', batch_size=2, val_sequences=[8], train_sequences=[8]), **more)
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}


def test_readers_give_equal_targets(device, tmp_path):
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd.datasets import SemanticKittiCacheBatches, SemanticKittiSceneBatches
    kw = tiny_kwargs()
    _tree(tmp_path, kw, seqs=((0, 4), (8, 2)))
    cfg = _config(kw, train_sequences=[0, 8], shuffle_train=False, remove_unseen=True, min_num_points=3)
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(cfg))
    assert launcher.main(['--config', str(tmp_path / 'tiny.yml'), '--data-root', str(tmp_path), '--build-mask-cache']) is None
    cache = SemanticKittiCacheBatches(cfg, device, 0, 1, tmp_path, [0, 8])
    scenes = SemanticKittiSceneBatches(cfg, device, 0, 1, tmp_path, [0, 8])
    assert len(cache) == len(scenes) == 3 and [f for f, _ in scenes.files] == [f for f, _ in cache.files]
    assert all(m is None for _, m in scenes.files)
    for i in range(3):                                      # two batches of sequence 00, one of sequence 08
        (_, (l1, m1)), (_, (l2, m2)) = cache.batch(0, i), scenes.batch(0, i)
        assert torch.equal(l1, l2) and torch.equal(m1, m2) and l1.sum(1).tolist() == [2, 2]


def test_launcher_trains_and_tests_without_a_mask_cache(device, tmp_path, capsys, monkeypatch):
    import re
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd import datasets
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.scene_bank import SceneBank
    kw = tiny_kwargs()
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    data = tmp_path / 'data'
    _tree(data, kw)
    seq = data / 'sequences' / '08'
    assert not (seq / 'mask_cache').exists()
    ck = tmp_path / 'ckpt' / 'tiny'
    ck.mkdir(parents=True)
    launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'], ck / 'tiny-epoch=00-val_loss=9.000000.ckpt', 0,
                             'val_loss', 9.0)
    cfg = _config(kw, panoptic_min_points=1)
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(dict(cfg, semantic_kitti_targets='scenes')))
    (tmp_path / 'default.yml').write_text(yaml.safe_dump(cfg))
    common = ['--data-root', str(data), '--checkpoint-root', str(tmp_path / 'ckpt')]
    # the default key: today's reader, today's error
    with pytest.raises(ValueError, match=re.escape('no (velodyne/*.bin, mask_cache/*.npy) pairs')):
        launcher.main(['--config', str(tmp_path / 'default.yml'), '--train', '--max-steps', '2', '--max-epochs', '1'] + common)
    capsys.readouterr()
    # --train
    assert launcher.main(['--config', str(tmp_path / 'tiny.yml'), '--train', '--max-steps', '2', '--max-epochs', '1'] + common) == 0
    out = capsys.readouterr().out
    got = re.search(r'epoch 0: train_loss (\S+) val_loss (\S+)', out)
    assert got and np.isfinite(float(got.group(1))) and np.isfinite(float(got.group(2))), out
    assert re.search(r'scene bank of sequence 08 built: 4 scans, 800 points, 12840 bytes', out)
    # --test --write-labels
    out_dir = tmp_path / 'out'
    assert launcher.main(['--config', str(tmp_path / 'tiny.yml'), '--test', '--write-labels', str(out_dir)] + common) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len([l for l in lines if l.startswith('val_loss ')]) == 1 and np.isfinite(float([l for l in lines if l.startswith('val_loss ')][0].split()[1]))
    assert len([l for l in lines if l.startswith('layer ')]) == 10, lines
    assert len([l for l in lines if l.startswith('point PQ')]) == 1
    for i in range(4):
        words = np.fromfile(str(out_dir / 'sequences' / '08' / 'predictions' / f'{i:06d}.label'), '<u4')
        assert len(words) == 300
    # --build-scene-bank
    assert launcher.main(['--config', str(tmp_path / 'tiny.yml'), '--build-scene-bank'] + common) is None
    bank = SceneBank.load(SceneBank.default_path(data, 8), device, num_scans=4)
    assert bank.points.shape[0] == 800
    # --build-mask-cache: one file per scan, equal to rasterize_bank's map, in the reference's dtype
    assert launcher.main(['--config', str(tmp_path / 'tiny.yml'), '--build-mask-cache'] + common) is None
    s = datasets.SceneSequence(data, 8, seq, device)
    r = datasets.scene_rasterizer(cfg)
    want = r.rasterize_bank(s.bank, [(*s.scene(k, cfg), k) for k in range(4)]).cpu().numpy()
    files = sorted((seq / 'mask_cache').glob('*.npy'))
    assert [f.name for f in files] == [f'{i:06d}.npy' for i in range(4)]
    for f, m in zip(files, want):
        got = np.load(f)
        assert got.dtype == np.int64 and got.shape == (80, 80) and np.array_equal(got, m)
        assert sorted(np.unique(got).tolist()) == [0, 1, 2]
    # a second run rewrites nothing; --overwrite rewrites all four
    saved = []
    monkeypatch.setattr(np, 'save', lambda path, array: saved.append(path))
    assert launcher.main(['--config', str(tmp_path / 'tiny.yml'), '--build-mask-cache'] + common) is None
    assert saved == []
    assert launcher.main(['--config', str(tmp_path / 'tiny.yml'), '--build-mask-cache', '--overwrite'] + common) is None
    assert len(saved) == 4
    monkeypatch.undo()
    # and the old reader trains from that cache
    assert launcher.main(['--config', str(tmp_path / 'default.yml'), '--train', '--max-steps', '1', '--max-epochs', '1'] + common) == 0
    assert re.search(r'epoch 0: train_loss (\S+)', capsys.readouterr().out)
