"""K28 — KITTI object augmentations on the device (csrc/object_augment.hip) against the numpy f64 restatement
(tests/object_augment_ref.py), bit for bit: membership and move, the shapes of a batch, pasting, the bank's builder, the
reference's configuration-01 list through ``DeviceAugmentation`` and ``BoxCollate``, and the launcher's new key."""
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as AR
from tests import object_augment_ref as OR
from tests.test_object_augment_cpu import CONFIG_01, spaced_boxes

pytestmark = pytest.mark.gpu

MOVE, REMOVE = OR.MOVE, OR.REMOVE
CHAIN_SEED = 15         # chosen on the host so that the batch covers the list (asserted in the test)


def _OA():
    from mask_bev_amd import object_augment
    return object_augment


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def points_around(rng, boxes, per_box, dim, reach=1.5):
    """``per_box`` points per box, uniform in the box's frame within ``reach`` x its half extents (and below / above it)."""
    out = []
    for b in np.asarray(boxes, dtype=np.float64).reshape(-1, 7):
        u = rng.uniform(-reach, reach, (per_box, 2)) * [b[3] / 2, b[4] / 2]
        c, s = np.cos(b[6]), np.sin(b[6])
        p = np.zeros((per_box, 4))
        p[:, 0], p[:, 1] = b[0] + c * u[:, 0] - s * u[:, 1], b[1] + s * u[:, 0] + c * u[:, 1]
        p[:, 2] = b[2] + rng.uniform(-0.3, 1.3, per_box) * b[5]
        p[:, 3] = rng.uniform(0, 1, per_box)
        out.append(p)
    pts = np.concatenate(out) if out else np.zeros((0, 4))
    return np.ascontiguousarray(pts[rng.permutation(len(pts))][:, :dim], dtype=np.float32)


def noise_for(rng, n):
    return rng.uniform(-0.15, 0.15, n), rng.normal(scale=0.25, size=(n, 3))


def run_kernel(device, scans, frames, bank=None):
    """frames: per scan (boxes, rot, loc, flags, pasted bank indices) → (list of output scans, offsets, counts)."""
    from mask_bev_amd import ops_augment
    OA = _OA()
    tables = [OA.box_table(b, r, t, f) for b, r, t, f, _ in frames]
    segments, paste_offsets = [], [0]
    for *_, pasted in frames:
        segments += [(int(bank.offsets[k]), int(bank.offsets[k + 1] - bank.offsets[k])) for k in pasted]
        paste_offsets.append(len(segments))
    points = torch.from_numpy(np.concatenate(scans)).to(device)
    out, offs, counts = ops_augment.object_augment(
        points, np.concatenate([[0], np.cumsum([len(s) for s in scans])]), torch.from_numpy(np.concatenate(tables)).to(device),
        np.concatenate([[0], np.cumsum([len(t) for t in tables])]), None if bank is None else bank.device_points(device),
        segments or None, paste_offsets)
    offs, counts = offs.cpu().numpy(), counts.cpu().numpy()
    assert out.shape[0] == len(points) + sum(c for _, c in segments)
    out = out.cpu().numpy()
    return [out[offs[b]:offs[b + 1]] for b in range(len(scans))], offs, counts


def restate(scans, frames, bank=None):
    return [OR.scan(s, b, r, t, f, [bank.sample_points(k) for k in pasted]) for s, (b, r, t, f, pasted) in zip(scans, frames)]


def assert_same(got, want, what=''):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (what, b, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w)), (what, b)


# ---------------------------------------------------------------------------------------------------------------
def test_membership_and_move(device):
    rng = np.random.default_rng(0)
    boxes = np.array([[10.0, 3.0, -1.6, 4.2, 1.8, 1.5, 0.6],           # 0 and 1 overlap: 0 wins
                      [11.0, 4.0, -1.7, 4.0, 1.9, 1.6, -0.4],
                      [25.0, -8.0, -1.5, 3.9, 1.7, 1.4, -2.5],
                      [18.0, 12.0, -1.8, 4.5, 2.0, 1.7, 2.9],
                      [30.0, 5.0, -1.5, 3.5, 1.6, 1.5, 1.2],           # 4: the identity noise
                      [8.0, -4.0, -1.5, 4.0, 2.0, 1.5, 0.0]])          # 5: axis-aligned, dyadic
    rot, loc = noise_for(rng, 6)
    rot[4], loc[4] = 0.0, 0.0
    flags = np.full(6, MOVE)
    cx, cy, cz = 8.0, -4.0, -1.5
    e = 2.0 ** -10
    faces = np.array([[cx + 2, cy, cz + 0.5], [cx - 2, cy, cz + 0.5], [cx, cy + 1, cz + 0.5], [cx, cy - 1, cz + 0.5],
                      [cx, cy, cz], [cx, cy, cz + 1.5], [cx + 2, cy + 1, cz + 1.5]])
    inner = np.array([[cx + 2 - e, cy, cz + 0.5], [cx - 2 + e, cy, cz + 0.5], [cx, cy + 1 - e, cz + 0.5],
                      [cx, cy - 1 + e, cz + 0.5], [cx, cy, cz + e], [cx, cy, cz + 1.5 - e], [cx + 2 - e, cy + 1 - e, cz + 1.5 - e]])
    for dim in (3, 4):
        pts = points_around(rng, boxes, 331, dim)
        planted = np.zeros((14, dim), dtype=np.float32)
        planted[:, :3] = np.concatenate([faces, inner])
        scan = np.concatenate([pts, planted])                            # 2 000 points
        assert len(scan) == 2000 and np.array_equal(planted[:, :3].astype(np.float64), np.concatenate([faces, inner]))
        frame = (boxes, rot, loc, flags, [])
        (got,), offs, counts = run_kernel(device, [scan], [frame])
        (want,) = restate([scan], [frame])
        assert offs.tolist() == [0, 2000] and counts.tolist() == [2000]
        assert_same([got], [want], f'dim {dim}')
        # on a face: outside, so untouched; just inside: moved
        assert np.array_equal(_bits(got[-14:-7]), _bits(planted[:7]))
        assert (got[-7:, :3] != planted[7:, :3]).any(1).all()
        # the restatement's own picture: both yaw signs hold points, the overlap goes to box 0, the identity box's points
        # stay where they are, every point outside all boxes stays bit for bit
        first = OR.first_box(scan, boxes)
        assert all((first == j).sum() > 50 for j in range(6))
        both = OR.inside(scan, boxes[0]) & OR.inside(scan, boxes[1])
        assert both.sum() > 5 and (first[both] == 0).all()
        only0 = OR.move(scan, boxes[:1], rot[:1], loc[:1], flags[:1])
        assert np.array_equal(_bits(got[both]), _bits(only0[both]))
        assert np.array_equal(_bits(got[first == -1]), _bits(scan[first == -1]))
        assert np.abs(got[first == 4] - scan[first == 4]).max() <= 2.0 ** -20 and (got[first == 2] != scan[first == 2]).any()
        if dim == 4:
            assert np.array_equal(_bits(got[:, 3]), _bits(scan[:, 3]))    # intensity untouched
        # with the remove bit on box 2 its points are gone, the others keep their order
        flags2 = flags.copy()
        flags2[2] |= REMOVE
        (got2,), offs2, _ = run_kernel(device, [scan], [(boxes, rot, loc, flags2, [])])
        assert_same([got2], restate([scan], [(boxes, rot, loc, flags2, [])]), 'remove')
        assert offs2[1] == 2000 - (first == 2).sum() and np.array_equal(_bits(got2), _bits(got[first != 2]))


@pytest.mark.parametrize('dim', [3, 4])
def test_batch_shapes(device, dim):
    from mask_bev_amd._lib import MaskBevHipError
    rng = np.random.default_rng(1)
    many = spaced_boxes(rng, 129, pitch=6.0)
    lengths = [0, 1, 255, 257, 1000]
    tables = [spaced_boxes(rng, 3), np.zeros((0, 7)), spaced_boxes(rng, 5), many[:128], spaced_boxes(rng, 2)]
    scans, frames = [], []
    for n, boxes in zip(lengths, tables):
        src = boxes if len(boxes) else spaced_boxes(rng, 2)
        scans.append(points_around(rng, src, -(-n // len(src)), dim, reach=1.2)[:n].reshape(n, dim))
        rot, loc = noise_for(rng, len(boxes))
        flags = np.full(len(boxes), MOVE) | (rng.random(len(boxes)) < 0.3) * REMOVE
        if n == 1000:
            flags[0] |= REMOVE
        frames.append((boxes, rot, loc, flags, []))
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [3], [0], [1, 0]):
        s, f = [scans[k] for k in order], [frames[k] for k in order]
        got, offs, counts = run_kernel(device, s, f)
        want = restate(s, f)
        assert_same(got, want, str(order))
        assert offs.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        assert counts.tolist() == [len(w) for w in want]
    kept = [len(w) for w in restate(scans, frames)]
    assert kept[1] == 1 and kept[3] < 257 and 0 < kept[4] < 1000           # no boxes: untouched; 128 boxes remove some
    # 129 boxes in one scan are refused; nothing is written
    rot, loc = noise_for(rng, 129)
    with pytest.raises(MaskBevHipError, match='UNSUPPORTED'):
        run_kernel(device, [scans[3]], [(many, rot, loc, np.full(129, MOVE), [])])


def _bank(rng):
    """5 samples of 5 to 300 points, each inside its own box."""
    OA = _OA()
    boxes = spaced_boxes(rng, 5)
    counts = [5, 17, 64, 300, 129]
    pts = [points_around(rng, boxes[k:k + 1], c, 4, reach=0.95) for k, c in enumerate(counts)]
    for p, b in zip(pts, boxes):
        p[:, 2] = (b[2] + rng.uniform(0.05, 0.95, len(p)) * b[5]).astype(np.float32)
    return OA.ObjectBank(np.concatenate(pts), np.concatenate([[0], np.cumsum(counts)]), boxes)


@pytest.mark.parametrize('dim', [3, 4])
def test_paste(device, dim):
    rng = np.random.default_rng(2)
    bank = _bank(rng)
    assert all((OR.first_box(bank.sample_points(k), bank.boxes[k:k + 1]) == 0).all() for k in range(5))
    labels = [np.array([[-10.0, 0.0, -1.6, 4.0, 1.8, 1.5, 0.3], [-10.0, 8.0, -1.6, 4.0, 1.8, 1.5, -0.3]]),
              np.array([[-12.0, -5.0, -1.6, 4.0, 1.8, 1.5, 1.0]])]
    pasted = [[3, 0, 4], []]
    scans, frames = [], []
    for lab, ks in zip(labels, pasted):
        boxes = np.concatenate([lab, bank.boxes[ks]])
        pc = points_around(rng, np.concatenate([lab, bank.boxes]), 60, dim)      # scene points inside every bank box too
        if ks:
            b = bank.boxes[ks[0]]
            above = np.zeros((2, dim), dtype=np.float32)
            above[:, :3] = [[b[0], b[1], b[2] + b[5] + 0.25], [b[0], b[1], b[2] + 0.5 * b[5]]]
            pc = np.concatenate([pc, above])
        rot, loc = noise_for(rng, len(boxes))
        flags = np.full(len(boxes), MOVE)
        flags[len(lab):] |= REMOVE
        scans.append(pc)
        frames.append((boxes, rot, loc, flags, ks))
    got, offs, counts = run_kernel(device, scans, frames, bank)
    want = restate(scans, frames, bank)
    assert_same(got, want, f'dim {dim}')
    # order: the kept scene points, then samples 3, 0, 4; offsets and counts say so
    gone = np.zeros(len(scans[0]), dtype=bool)
    for k in pasted[0]:
        gone |= OR.inside(scans[0], bank.boxes[k])
    kept0 = int((~gone).sum())
    assert gone.sum() > 30 and counts.tolist() == [kept0 + 300 + 5 + 129, len(scans[1])]
    assert offs.tolist() == [0, counts[0], counts[0] + counts[1]]
    # removal looks at all three coordinates: of the two planted points the one above the box's top stays
    assert not gone[-2] and gone[-1]
    moved = OR.move(scans[0], *frames[0][:4])
    assert np.array_equal(_bits(got[0][:kept0]), _bits(moved[~gone]))
    start = kept0
    for k in pasted[0]:
        src = bank.sample_points(k)[:, :dim]
        seg = got[0][start:start + len(src)]
        j = 2 + pasted[0].index(k)
        only = OR.move(src, frames[0][0][j:j + 1], frames[0][1][j:j + 1], frames[0][2][j:j + 1], [MOVE])
        assert np.array_equal(_bits(seg), _bits(only)) and (seg[:, :3] != src[:, :3]).any()     # it follows its own box
        if dim == 4:
            assert np.array_equal(_bits(seg[:, 3]), _bits(src[:, 3]))
        start += len(src)
    # the second scan pastes nothing: in a bank box it loses no point
    assert len(got[1]) == len(scans[1])
    # a scan gives the same rows alone and inside the batch, first or last
    for b in (0, 1):
        (alone,), _, _ = run_kernel(device, [scans[b]], [frames[b]], bank)
        assert np.array_equal(_bits(alone), _bits(got[b]))
    swapped, _, _ = run_kernel(device, scans[::-1], frames[::-1], bank)
    assert_same(swapped, want[::-1], 'swapped')
    # only pasted points: a scan without scene points
    empty = np.zeros((0, dim), dtype=np.float32)
    got_e, offs_e, _ = run_kernel(device, [empty, empty], [frames[0], frames[1]], bank)
    assert_same(got_e, restate([empty, empty], frames, bank), 'empty scene')
    assert offs_e.tolist() == [0, 434, 434]


def test_bank_build(device):
    from mask_bev_amd import batch as B, ops_augment
    from tests.test_boxes_cpu import SAMPLE
    OA = _OA()
    lab = B.kitti_labels_to_velodyne(B.read_kitti_label(os.path.join(SAMPLE, 'label_2', '000000.txt')),
                                     B.read_kitti_calib(os.path.join(SAMPLE, 'calib', '000000.txt')))
    boxes = lab['boxes'][:6]                                                 # Car, Van, Truck, Car, Pedestrian, Cyclist
    rng = np.random.default_rng(3)
    inside_counts = [9, 4, 5, 0, 7, 7]
    pts = [points_around(rng, boxes, 40, 4, reach=3.0)]
    pts[0] = pts[0][OR.first_box(pts[0], boxes) == -1]                       # the background: outside every box
    for b, c in zip(boxes, inside_counts):
        p = points_around(rng, b[None], c, 4, reach=0.9)
        p[:, 2] = (b[2] + rng.uniform(0.1, 0.9, c) * b[5]).astype(np.float32)
        pts.append(p)
    points = np.concatenate(pts)
    points = points[rng.permutation(len(points))]
    want = OR.first_box(points, boxes)
    assert [(want == k).sum() for k in range(len(boxes))] == inside_counts and (want == -1).sum() > 50
    got = ops_augment.points_in_boxes(torch.from_numpy(points).to(device), torch.from_numpy(OA.box_table(boxes)).to(device))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    got3 = ops_augment.points_in_boxes(torch.from_numpy(np.ascontiguousarray(points[:, :3])).to(device),
                                       torch.from_numpy(OA.box_table(boxes)).to(device))
    assert np.array_equal(got3.cpu().numpy(), want)
    # two frames: 4 points are too few, 5 are enough; the points keep their order within a sample
    bank = OA.ObjectBank.build([(points, boxes), (torch.from_numpy(points[::-1].copy()), boxes)], device=device)
    keep = [k for k, c in enumerate(inside_counts) if c >= 5]
    assert len(bank) == 2 * len(keep) and np.array_equal(bank.boxes, np.concatenate([boxes[keep], boxes[keep]]))
    assert np.diff(bank.offsets).tolist() == [inside_counts[k] for k in keep] * 2
    for i, k in enumerate(keep):
        assert np.array_equal(bank.sample_points(i), points[want == k])
        assert np.array_equal(bank.sample_points(len(keep) + i), points[::-1][want[::-1] == k])
    assert len(OA.ObjectBank.build([(points, boxes)], min_points=10, device=device)) == 0
    assert len(OA.ObjectBank.build([(points, np.zeros((0, 7)))], device=device)) == 0


# ---------------------------------------------------------------------------------------------------------------
def chain_case():
    """Four frames of spaced labels, a bank beside them, scans with points in and around every label and bank box."""
    OA = _OA()
    rng = np.random.default_rng(5)
    grid = spaced_boxes(rng, 25, pitch=7.0)
    grid[:, 1] *= 0.9
    bank_boxes, label_pool = grid[:10], grid[10:]
    counts = rng.integers(5, 120, 10)
    pts = [points_around(rng, bank_boxes[k:k + 1], int(c), 4, reach=0.9) for k, c in enumerate(counts)]
    for p, b in zip(pts, bank_boxes):
        p[:, 2] = (b[2] + rng.uniform(0.1, 0.9, len(p)) * b[5]).astype(np.float32)
    bank = OA.ObjectBank(np.concatenate(pts), np.concatenate([[0], np.cumsum(counts)]), bank_boxes)
    labels = [label_pool[:6], label_pool[6:9], np.zeros((0, 7)), label_pool[9:15]]
    scans = [points_around(rng, grid, n, 4) for n in (40, 33, 21, 52)]
    return bank, labels, scans


def restate_points(pc, draw):
    """tests/augment_ref.py over one scan, with ``global_noise`` (which it does not know) done here: the ops before it, the
    scale and shift in f64 with one rounding each and an f32 store, the ops after it — every op in its own slot."""
    ops = [(o.code, o.arg, o.p) for o in draw.ops]
    vals, keep = np.array(pc, dtype=np.float32), np.ones(len(pc), dtype=bool)
    cut = [s for s, o in enumerate(ops) if o[0] == 6] + [len(ops)]
    begin = 0
    for end in cut:
        vals, k = AR.run_program(vals, draw.seed, [(0, 0, ())] * begin + ops[begin:end])
        keep &= k
        if end < len(ops):
            p = ops[end][2]
            for c in range(3):
                vals[:, c] = (vals[:, c].astype(np.float64) * p[0] + p[1 + c]).astype(np.float32)
        begin = end + 1
    idx = np.flatnonzero(keep)
    if any(o[0] in (AR.OP_SHUFFLE, AR.OP_DECIMATE) for o in ops):
        idx = idx[np.argsort(AR.draw(draw.seed, AR.ORDER_SLOT, idx, 0, 0) >> 6, kind='stable')]
    return vals[idx]


def test_configuration_01_chain(device):
    from mask_bev_amd import augment as A, batch as B, rasterize
    OA = _OA()
    bank, labels, scans = chain_case()
    aug = A.DeviceAugmentation(OA.make_kitti_object_augmentation_list(CONFIG_01, bank), seed=CHAIN_SEED)
    dev_scans = [torch.from_numpy(s).to(device) for s in scans]
    res = aug.apply(dev_scans, boxes=labels)
    assert type(res) is A.ObjectAugmentedBatch and res.synced and len(res.objects) == 4 and len(res) == 7
    # the host decisions, replayed from the same seed: all object draws of the batch come before the point draws
    rng = np.random.default_rng(np.random.SeedSequence([CHAIN_SEED]))
    staged, moved = [], []
    for f, lab, pc in zip(res.objects, labels, scans):
        boxes, pasted, rot, loc, flags = OR.frame(rng, lab, bank.boxes, 15, {})
        assert f.pasted == pasted and np.array_equal(f.table, OA.box_table(boxes, rot, loc, flags))
        staged.append(OR.scan(pc, boxes, rot, loc, flags, [bank.sample_points(k) for k in pasted]))
        moved.append(OR.moved_boxes(boxes, rot, loc))
    again = A.DeviceAugmentation(OA.make_kitti_object_augmentation_list(CONFIG_01, bank), seed=CHAIN_SEED)
    assert OA.draw_frames(again.transforms[:2], again._rng, labels)[0].pasted == res.objects[0].pasted
    assert again.draw(4) == res.draws
    # the seed was chosen so that the batch covers the list: pastes, an empty frame, and every point op at least once
    codes = {o.code for d in res.draws for o in d.ops}
    assert codes >= {1, 2, 3, 4, 6} and sum(len(f.pasted) for f in res.objects) >= 3 and res.objects[2].n_labels == 0
    assert any(any(o.code == 1 and abs(o.p[0]) != 1 for o in d.ops) for d in res.draws)        # a rotation, not only flips
    for b, (g, d) in enumerate(zip(res.scans, res.draws)):
        g, w = g.cpu().numpy(), restate_points(staged[b], d)
        assert g.shape == w.shape, b
        # K23's rule for a list with a rotation and a jitter (test_reference_style_list_end_to_end): the jitter's f32
        # normal, 2^-22 |w| + 1e-5 std, and the rotation's double rounding, one f32 ulp = 2^-23 |w| — which global_noise,
        # standing between the two here, passes on scaled by at most 1.05 and rounds once more: 2 ulps in all
        std = np.array([0.01, 0.01, 0.01, 0.01])
        err = np.abs(g.astype(np.float64) - w)
        print('chain: max err / bound', float((err / (2.0 ** -22 * np.abs(w) + 1e-5 * std + 2.0 ** -22 * np.abs(w) + 1e-300)).max()))
        assert (err <= 2.0 ** -22 * np.abs(w) + 1e-5 * std + 2.0 ** -22 * np.abs(w)).all(), b
        assert np.array_equal(res.boxes[b], A.transform_boxes(moved[b], d.ops)), b
    # BoxCollate: one non-empty mask per in-range box, pasted ones included
    xr, yr = (0, 80), (-40, 40)
    rast = rasterize.KittiRasterizer(xr, yr, (-3, 1), 0.16, device=device)
    aug.reseed(CHAIN_SEED)
    collate = B.BoxCollate(rast, 32, device, augmentation=aug, object_range=(xr, yr))
    pcs, (lab, masks) = collate(list(zip(scans, labels)))
    assert all(torch.equal(a, b) for a, b in zip(pcs, res.scans))
    for b in range(4):
        n_in = int(B.object_range_mask(res.boxes[b], xr, yr).sum())
        assert int(lab[b].sum()) == n_in
        assert bool((masks[b, :n_in].flatten(1).sum(1) > 0).all()) and not bool(masks[b, n_in:].any())
    assert sum(int(B.object_range_mask(r, xr, yr).sum()) for r in res.boxes) > sum(len(x) for x in labels)
    # refusals
    with pytest.raises(ValueError, match='instance maps or scene'):
        aug.apply(dev_scans, instance_maps=torch.zeros(4, 8, 8, dtype=torch.int32, device=device), boxes=labels)
    with pytest.raises(ValueError, match='boxes='):
        aug.apply(dev_scans)
    # a list without object transforms is untouched by all this
    plain = A.DeviceAugmentation(A.make_kitti_augmentation_list(CONFIG_01[2:]), seed=4)
    out = plain.apply(dev_scans, boxes=labels)
    assert type(out) is A.AugmentedBatch and len(out.boxes[0]) == 6


def test_launcher_with_device_object_augmentation(device, tmp_path, capsys):
    """tests/test_k24_boxes_gpu.py::test_launcher_kitti_batches' scenario with ``device_object_augmentation: true``: the
    bank is built from the training split, the list holds both object transforms, nothing is left out."""
    import shutil
    import yaml
    from mask_bev_amd.datasets import KittiObjectBatches, build_object_bank
    from mask_bev_amd import batch as B
    from tests.test_boxes_cpu import SAMPLE
    OA = _OA()
    lab = B.kitti_labels_to_velodyne(B.read_kitti_label(os.path.join(SAMPLE, 'label_2', '000000.txt')),
                                     B.read_kitti_calib(os.path.join(SAMPLE, 'calib', '000000.txt')))
    rng = np.random.default_rng(2)
    for k, sub in (('velodyne', 'velodyne'), ('label_2', 'label_2'), ('calib', 'calib')):
        d = tmp_path / f'data_object_{k}' / 'training' / sub
        d.mkdir(parents=True)
        for frame in (0, 1):
            if k == 'velodyne':
                pc = np.concatenate([rng.uniform(-40, 80, (300 + frame, 4)).astype(np.float32),
                                     points_around(rng, lab['boxes'][:3], 30, 4, reach=0.8)])
                pc.tofile(d / f'{frame:06d}.bin')
            else:
                shutil.copy(os.path.join(SAMPLE, sub, '000000.txt'), d / f'{frame:06d}.txt')
    (tmp_path / 'train.txt').write_text('000000\n000001\n')
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
device_object_augmentation: true
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
    config['object_bank'] = str(tmp_path / 'bank' / 'samples.npz')
    with pytest.raises(FileNotFoundError, match='build-object-bank'):
        KittiObjectBatches(config, device, 0, 1, tmp_path, 'train', augment=True)
    path = build_object_bank(config, device, tmp_path)
    assert str(path) == config['object_bank'] and 'object bank:' in capsys.readouterr().out
    bank = OA.ObjectBank.load(path)
    assert 2 <= len(bank) <= 6 and (np.diff(bank.offsets) >= 5).all()
    train = KittiObjectBatches(config, device, 0, 1, tmp_path, 'train', augment=True)
    assert 'training without' not in capsys.readouterr().out
    kinds = [type(t) for t in train.augmentation.transforms]
    assert kinds[:2] == [OA.ObjectSample, OA.ObjectNoise] and len(kinds) == 4
    pcs, (labels, masks) = train.batch(0, 0)
    assert len(pcs) == 2 and all(p.dim() == 2 and p.shape[1] == 4 and p.shape[0] > 300 for p in pcs)
    assert masks.shape == (2, 45, 800, 800) and labels.shape == (2, 45) and all(3 <= int(v) <= 45 for v in labels.sum(1))
    pcs2, (labels2, masks2) = train.batch(0, 0)                            # a pure function of (seed, rank, epoch, batch index)
    assert torch.equal(masks, masks2) and all(a.shape == b.shape for a, b in zip(pcs, pcs2))
