"""K24 — KITTI / Waymo box tables → instance-id maps on the device (csrc/box_rasterize.hip) against the integer fill rule
restated in numpy (tests/box_rasterize_ref.py), bit for bit: the kernel on every golden case in batches of three, the two
rasteriser classes against the maps recorded from the reference, ``BoxCollate`` with and without augmentation, the
``global_noise`` point pass, and the entry point's argument checks."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import box_rasterize_ref as BR
from tests.test_boxes_cpu import frame_rows, golden, kitti_rasterizer, selected, waymo_rasterizer

pytestmark = pytest.mark.gpu

GARBAGE = -1234567


@pytest.fixture(scope='module')
def cases():
    """Per grid: the rasteriser, and per frame the vertices and ids the product paints and the oracle's (nx, ny) map."""
    from mask_bev_amd import rasterize
    g = golden()
    out = {'g': g}
    for key in ('a', 'b', 'w'):
        r = waymo_rasterizer(g) if key == 'w' else kitti_rasterizer(g, key)
        frames = []
        for f in range(len(g[f'{key}_names'])):
            boxes, ids = selected(g, key, f)
            verts = rasterize.box_vertices(boxes, r.x_range, r.y_range, r.nx, r.ny)
            frames.append((verts, ids, BR.rasterize_boxes(verts, ids, r.nx, r.ny)))
        out[key] = (r, frames)
    return out


def _launch(device, frames, nx, ny):
    from mask_bev_amd import ops_rasterize
    verts = np.concatenate([f[0] for f in frames])
    ids = np.concatenate([f[1] for f in frames]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(f[1]) for f in frames])])
    out = torch.full((len(frames), nx, ny), GARBAGE, dtype=torch.int32, device=device)       # every cell must be written
    got = ops_rasterize.rasterize_boxes(torch.from_numpy(verts).to(device), torch.from_numpy(ids).to(device), offsets, nx, ny,
                                        out=out)
    assert got is out
    return out.cpu().numpy()


@pytest.mark.parametrize('key', ['a', 'b'])
def test_kernel_equals_the_oracle_on_every_case(device, cases, key):
    """40 x 24 and 70 x 130 (non-square; the second spans 5 x 3 tiles and is no multiple of 16, 32 or 64), B = 3: every
    window of three consecutive cases, so each case is first, middle and last, the empty frame included; 300 boxes in one
    frame take two staging passes."""
    r, frames = cases[key]
    names = cases['g'][f'{key}_names'].tolist()
    n = len(frames)
    for i in range(n):
        trio = [frames[(i + k) % n] for k in range(3)]
        got = _launch(device, trio, r.nx, r.ny)
        for k in range(3):
            assert np.array_equal(got[k], trio[k][2]), (names[(i + k) % n], 'in window', i)
    # ids are painted as they are given: large, negative and 0 (a later 0 erases what lies under it, as an overwrite does)
    verts = np.concatenate([frames[names.index('overlap_later_wins')][0], frames[names.index('deg30')][0]])
    ids = np.array([2 ** 31 - 1, 0, -5], dtype=np.int32)
    got = _launch(device, [(verts, ids, None)], r.nx, r.ny)[0]
    assert np.array_equal(got, BR.rasterize_boxes(verts, ids, r.nx, r.ny)) and (got == 2 ** 31 - 1).any() and (got == -5).any()


def test_kernel_all_frames_empty_and_one_launch_for_many(device, cases):
    r, frames = cases['b']
    empty = (np.zeros((0, 4, 2), dtype=np.int32), np.zeros((0,), dtype=np.int32), None)
    assert not _launch(device, [empty, empty], r.nx, r.ny).any()
    got = _launch(device, frames, 70, 130)                                # B = 13 in one launch
    assert all(np.array_equal(got[k], frames[k][2]) for k in range(len(frames)))
    # a grid of one tile row and a single column / row
    for nx, ny in ((1, 130), (70, 1), (17, 65)):
        got = _launch(device, frames[:3], nx, ny)
        assert all(np.array_equal(got[k], BR.rasterize_boxes(frames[k][0], frames[k][1], nx, ny)) for k in range(3))


def test_rasterizer_classes_equal_the_golden_maps(device, cases):
    from mask_bev_amd import rasterize
    g = cases['g']
    for key in ('a', 'b', 'falsy'):
        r = kitti_rasterizer(g, key)
        r.device = device
        n = len(g[f'{key}_names'])
        rows = [frame_rows(g, key, f) for f in range(n)]
        maps = r.rasterize_batch([b for b, _ in rows], [t for _, t in rows])
        assert maps.shape == (n, r.nx, r.ny) and maps.dtype == torch.int32 and maps.is_cuda
        assert np.array_equal(maps.transpose(1, 2).cpu().numpy(), g[f'{key}_maps'])
    r = waymo_rasterizer(g)
    r.device = device
    n = len(g['w_names'])
    rows = [frame_rows(g, 'w', f) for f in range(n)]
    counts = [g['w_num_points'][int(g['w_offsets'][f]):int(g['w_offsets'][f + 1])] for f in range(n)]
    maps = r.rasterize_batch([b for b, _ in rows], [t for _, t in rows], counts)
    assert np.array_equal(maps.transpose(1, 2).cpu().numpy(), g['w_maps'])
    # get_mask, the reference's call
    f = g['a_names'].tolist().index('types_and_skip')
    boxes, tps = frame_rows(g, 'a', f)
    frame = types.SimpleNamespace(labels=[types.SimpleNamespace(type=int(t), location=b[:3], dimensions=b[3:6], rotation_y=b[6])
                                          for b, t in zip(boxes, tps)])
    r = kitti_rasterizer(g, 'a')
    r.device = device
    out = r.get_mask(frame)
    assert list(out) == [rasterize.KITTI_CAR] and np.array_equal(out[0].cpu().numpy(), g['a_maps'][f])
    f = g['w_names'].tolist().index('many_300')
    boxes, tps = frame_rows(g, 'w', f)
    frame = types.SimpleNamespace(laser_labels=[
        types.SimpleNamespace(type=int(t), num_lidar_points_in_box=int(c),
                              box=types.SimpleNamespace(center_x=b[0], center_y=b[1], center_z=b[2], length=b[3], width=b[4],
                                                        height=b[5], heading=b[6])) for b, t, c in zip(boxes, tps, counts[f])])
    r = waymo_rasterizer(g)
    r.device = device
    out = r.get_mask(frame)
    assert list(out) == [rasterize.WAYMO_TYPE_VEHICLE] and np.array_equal(out[1].cpu().numpy(), g['w_maps'][f])


def _samples(g, key, names, seed=0):
    """(point cloud, car-like boxes) samples of the named frames, as the launcher makes them."""
    rng = np.random.default_rng(seed)
    all_names = g[f'{key}_names'].tolist()
    out = []
    for k, name in enumerate(names):
        boxes, tps = frame_rows(g, key, all_names.index(name))
        pc = rng.uniform(-20, 20, (100 + 37 * k, 4)).astype(np.float32)
        out.append((pc, boxes[np.isin(tps, (0, 1, 2))]))
    return out


@pytest.mark.parametrize('packed', [False, True])
def test_box_collate_equals_targets_of_the_golden_maps(device, cases, packed):
    from mask_bev_amd import batch as B
    g = cases['g']
    names = ['overlap_later_wins', 'empty', 'types_and_skip', 'cut_by_borders']
    r = kitti_rasterizer(g, 'b')
    samples = _samples(g, 'b', names)
    collate = B.BoxCollate(r, 6, device, packed=packed)
    pcs, (labels, masks) = collate(samples)
    all_names = g['b_names'].tolist()
    ref = torch.from_numpy(np.stack([g['b_maps'][all_names.index(n)].T for n in names])).to(device)
    want_labels, want_masks = B.instance_targets(ref, 6, packed=packed)
    assert torch.equal(labels, want_labels) and labels.sum(1).tolist() == [2, 0, 3, 4] and labels.max() == B.CAR
    if packed:
        assert torch.equal(masks.words, want_masks.words) and (masks.h, masks.w) == (130, 70)
    else:
        assert masks.shape == (4, 6, 130, 70) and torch.equal(masks, want_masks)
        assert torch.equal(masks[2, 1], torch.from_numpy(g['b_maps'][all_names.index('types_and_skip')] == 3).to(device).float())
    assert all(torch.equal(p.cpu(), torch.from_numpy(s[0])) for p, s in zip(pcs, samples))
    with_meta = collate([(s[0], s[1], {'k': k}) for k, s in enumerate(samples)])
    assert with_meta[2] == [{'k': k} for k in range(4)]
    # the range filter sits behind the augmentation, where the reference's pipeline has it
    ranges = ((-10, 25), (-30, 0))
    keep = [B.object_range_mask(s[1], *ranges) for s in samples]
    assert 0 < sum(int(k.sum()) for k in keep) < 9
    got = B.BoxCollate(r, 6, device, object_range=ranges)(samples)[1]
    want = B.BoxCollate(r, 6, device)([(s[0], s[1][k]) for s, k in zip(samples, keep)])[1]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[0].sum() < labels.sum()


def test_box_collate_with_flip_and_rotation(device, cases):
    """The masks are those of the oracle run on the augmented boxes; the points are K23's for the same draws."""
    from mask_bev_amd import augment as A, batch as B, rasterize
    g = cases['g']
    names = ['deg30', 'types_and_skip', 'overlap_later_wins']
    r = kitti_rasterizer(g, 'b')
    samples = _samples(g, 'b', names, seed=4)

    def make():
        return A.DeviceAugmentation(A.make_kitti_augmentation_list(
            [{'name': 'flip', 'prob_flip_y': 1.0}, {'name': 'rotate', 'rotate_prob': 1.0, 'rotation_range': [5, 25]}]), seed=11)

    pcs, (labels, masks) = B.BoxCollate(r, 5, device, augmentation=make())(samples)
    draws = make().draw(len(samples))
    assert all([op.code for op in d.ops] == [A.OP_LINEAR, A.OP_LINEAR] for d in draws)
    maps = []
    for (_, boxes), d in zip(samples, draws):
        moved = A.transform_boxes(boxes, d.ops)
        kept, ids = r._select(moved)
        maps.append(BR.rasterize_boxes(rasterize.box_vertices(kept, r.x_range, r.y_range, r.nx, r.ny), ids, r.nx, r.ny))
    assert not np.array_equal(maps[0], cases['b'][1][g['b_names'].tolist().index('deg30')][2])          # it did move
    want_labels, want_masks = B.instance_targets(torch.from_numpy(np.stack(maps)).to(device), 5)
    assert torch.equal(labels, want_labels) and torch.equal(masks, want_masks) and masks.sum() > 0
    k23 = A.DeviceAugmentation([]).apply([torch.from_numpy(s[0]).to(device) for s in samples], draws=draws)
    assert all(torch.equal(p, q) for p, q in zip(pcs, k23.scans)) and k23.boxes is None
    assert not torch.equal(pcs[0].cpu(), torch.from_numpy(samples[0][0]))


def test_global_noise_point_pass(device):
    """v' = (f32)((f64)v * s + t) per coordinate: compared against the f64 expression rounded to f32, 1 ulp allowed (the
    kernel rounds the product to f64 before the sum: a double rounding of at most one f32 ulp)."""
    from mask_bev_amd import augment as A
    rng = np.random.default_rng(6)
    for dim, lengths in ((4, [1000, 0, 257]), (3, [65])):
        scans = [np.concatenate([rng.uniform(-70, 70, (n, 3)), rng.uniform(0, 1, (n, dim - 3))], axis=1).astype(np.float32)
                 for n in lengths]
        draws = [A.SampleDraw(int(rng.integers(0, 1 << 62)), (A.Op(A.OP_GLOBAL_NOISE, 0, (float(rng.uniform(0.95, 1.05)),
                                                                   *[float(v) for v in rng.standard_normal(3) * 0.2])),))
                 for _ in lengths]
        dev_scans = [torch.from_numpy(s).to(device) for s in scans]
        boxes = [np.array([[10., -3., -1., 4., 1.8, 1.5, 0.4]])] * len(lengths)
        res = A.DeviceAugmentation([]).apply(dev_scans, draws=draws, boxes=boxes)
        assert not res.synced
        for s, d, out, b in zip(scans, draws, res.scans, res.boxes):
            scale, t = d.ops[0].p[0], np.array(d.ops[0].p[1:4])
            want = (s[:, :3].astype(np.float64) * scale + t).astype(np.float32)
            got = out.cpu().numpy()
            assert got.shape == s.shape
            ulps = np.abs(got[:, :3].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            same_sign = np.signbit(got[:, :3]) == np.signbit(want)
            assert np.all(same_sign | (np.abs(want) < 1e-30)) and (ulps[same_sign].max() if ulps.size else 0) <= 1
            assert np.array_equal(got[:, 3:], s[:, 3:])                                  # intensity untouched
            assert np.array_equal(b, [[10. * scale + t[0], -3. * scale + t[1], -1. * scale + t[2], 4. * scale, 1.8 * scale,
                                       1.5 * scale, 0.4]])
        with pytest.raises(ValueError, match='global_noise'):
            A.DeviceAugmentation([], x_range=(-8, 8), y_range=(-8, 8), voxel_size=1.0).apply(
                dev_scans, draws=draws, instance_maps=torch.zeros((len(lengths), 16, 16), dtype=torch.int32, device=device))
        with pytest.raises(ValueError, match='global_noise'):
            A.DeviceAugmentation([]).apply(dev_scans, draws=draws, scene_transforms=[np.eye(4)[None]] * len(lengths))
    # in a list with the other ops, in op order: a rotation, then the noise
    rot = A.rotation_op(17.0)
    noise = A.Op(A.OP_GLOBAL_NOISE, 0, (1.03, 0.1, -0.2, 0.05))
    s = scans[0]
    res = A.DeviceAugmentation([]).apply([torch.from_numpy(s).to(device)], draws=[A.SampleDraw(1, (rot, noise))])
    a = np.array(rot.p).reshape(2, 2)
    xy = (s[:, :2].astype(np.float64) @ a.T).astype(np.float32).astype(np.float64)
    want = np.concatenate([xy, s[:, 2:3].astype(np.float64)], axis=1) * 1.03 + [0.1, -0.2, 0.05]
    assert np.allclose(res.scans[0].cpu().numpy()[:, :3], want, rtol=0, atol=2e-5)


def test_bad_arguments_launch_nothing(device, cases):
    from mask_bev_amd import _lib
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd import ops_rasterize
    lib = _lib.load()
    r, frames = cases['a']
    verts = torch.from_numpy(frames[0][0]).to(device)
    ids = torch.from_numpy(frames[0][1].astype(np.int32)).to(device)
    offs = torch.tensor([0, 1], dtype=torch.int32, device=device)
    out = torch.full((1, r.nx, r.ny), GARBAGE, dtype=torch.int32, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                           # noqa: E731
    good = [p(verts), p(ids), p(offs), 1, r.nx, r.ny, p(out), stream]
    bad = {0: None, 1: None, 2: None, 6: None}
    calls = [good[:k] + [v] + good[k + 1:] for k, v in bad.items()]
    calls += [good[:3] + [b] + good[4:] for b in (0, -1, 65536)]
    calls += [good[:4] + [nx, ny] + good[6:] for nx, ny in ((0, r.ny), (r.nx, 0), (-3, r.ny), (1 << 14, 1 << 14))]
    calls.append([ctypes.c_void_p(verts.data_ptr() + 4)] + good[1:])       # vertices not 16-byte aligned
    for args in calls:
        assert lib.mbv_rasterize_boxes(*args) == -1                       # MBV_ERR_BAD_ARG
    torch.cuda.synchronize(device)
    assert bool((out == GARBAGE).all())                                   # nothing was launched
    assert lib.mbv_rasterize_boxes(*good) == 0
    assert np.array_equal(out[0].cpu().numpy(), frames[0][2])
    # the wrapper's own checks
    with pytest.raises(ValueError):
        ops_rasterize.rasterize_boxes(verts, ids, [0, 2], r.nx, r.ny)
    with pytest.raises(ValueError):
        ops_rasterize.rasterize_boxes(verts, ids, [1, 1], r.nx, r.ny)
    with pytest.raises(MaskBevHipError):
        ops_rasterize.rasterize_boxes(verts.to(torch.int64), ids, [0, 1], r.nx, r.ny)
    with pytest.raises(MaskBevHipError):
        ops_rasterize.rasterize_boxes(verts, ids, [0, 1], r.nx, r.ny, out=out.to(torch.int64))
    with pytest.raises(MaskBevHipError):
        ops_rasterize.rasterize_boxes(verts.cpu(), ids, [0, 1], r.nx, r.ny)


def test_launcher_kitti_batches(device, tmp_path, capsys):
    """``dataset: kitti``: the launcher's batch source over a KITTI object tree holding the sample frame twice, with the
    keys of the reference's configs/training/kitti files; ``object_sample`` / ``object_noise`` are left out with one line."""
    import shutil
    import yaml
    from mask_bev_amd.datasets import KittiObjectBatches
    from mask_bev_amd import batch as B, rasterize
    from tests.test_boxes_cpu import SAMPLE
    import os
    rng = np.random.default_rng(2)
    for k, sub in (('velodyne', 'velodyne'), ('label_2', 'label_2'), ('calib', 'calib')):
        d = tmp_path / f'data_object_{k}' / 'training' / sub
        d.mkdir(parents=True)
        for frame in (0, 1):
            if k == 'velodyne':
                rng.uniform(-40, 80, (300 + frame, 4)).astype(np.float32).tofile(d / f'{frame:06d}.bin')
            else:
                shutil.copy(os.path.join(SAMPLE, sub, '000000.txt'), d / f'{frame:06d}.txt')
    (tmp_path / 'train.txt').write_text('000000\n000001\n')
    (tmp_path / 'val.txt').write_text('000001\n')
    config = yaml.safe_load("""
dataset: kitti
x_range: [0, 80]
y_range: [-40, 40]
z_range: [-3, 1]
voxel_size: 0.1
num_queries: 45
batch_size: 2
remove_unseen: True
min_num_points: 1
shuffle_train: False
filter_difficulty: True
seed: 420
augmentations:
  - name: 'object_sample'
    dataset_root: '~/Datasets/KITTI'
    num_sample: 5
  - name: 'object_noise'
  - name: 'flip'
    prob_flip_y: 1
  - name: 'global_noise'
    prob_aug: 0.5
""")
    train = KittiObjectBatches(config, device, 0, 1, tmp_path, 'train', augment=True)
    assert 'training without object_sample, object_noise' in capsys.readouterr().out
    val = KittiObjectBatches(dict(config, batch_size=1), device, 0, 1, tmp_path, 'val')
    assert len(train) == 1 and len(val) == 1 and val.augmentation is None and len(train.augmentation.transforms) == 2
    pcs, (labels, masks) = val.batch(0, 0)
    assert pcs[0].shape == (301, 4) and masks.shape == (1, 45, 800, 800) and labels.shape == (1, 45)
    # the sample frame: Car, Van, Truck, Car are car-like; the last fails the difficulty filter; all three others lie in range
    lab = B.kitti_labels_to_velodyne(B.read_kitti_label(os.path.join(SAMPLE, 'label_2', '000000.txt')),
                                     B.read_kitti_calib(os.path.join(SAMPLE, 'calib', '000000.txt')))
    boxes = lab['boxes'][:3]
    verts = rasterize.box_vertices(boxes, (0, 80), (-40, 40), 800, 800)
    want = BR.rasterize_boxes(verts, [1, 2, 3], 800, 800)
    assert labels[0].tolist() == [1, 1, 1] + [0] * 42
    for q in range(3):
        assert np.array_equal(masks[0, q].cpu().numpy(), (want == q + 1).T)
    tp, (tl, tm) = train.batch(0, 0)
    assert tm.shape == (2, 45, 800, 800) and tl.sum(1).tolist() == [3, 3] and not torch.equal(tm[1], masks[0])
