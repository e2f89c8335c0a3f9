"""Host side of the KITTI object augmentations (mask_bev_amd/object_augment.py): the collision rule against the float64
rotated-box intersection area of tests/kitti_eval_ref.py, the sequential noise search and ``object_sample`` against the
restatement (tests/object_augment_ref.py), the bank's file, and how the lists are built."""
import numpy as np
import pytest

from tests import kitti_eval_ref as KR
from tests import object_augment_ref as OR

# configs/training/kitti/01_kitti_point_mask_lower_lr_finer.yml, ``augmentations:``, verbatim
CONFIG_01 = [
    {'name': 'object_sample', 'dataset_root': 'data/KITTI', 'num_sample': 15},
    {'name': 'object_noise'},
    {'name': 'flip', 'prob_flip_x': 0, 'prob_flip_y': 0.5},
    {'name': 'rotate', 'rotate_prob': 0.1, 'rotation_range': 2.5},
    {'name': 'global_noise', 'prob_aug': 0.5},
    {'name': 'drop', 'prob_drop': 0.1, 'per_point_drop_prob': 0.05},
    {'name': 'shuffle', 'prob_shuffle': 0.5},
    {'name': 'jitter', 'prob_jitter': 0.25, 'jitter_std': 0.01, 'intensity_std': 0.01},
]


def _OA():
    from mask_bev_amd import object_augment
    return object_augment


def random_boxes(rng, n, spread=20.0):
    b = np.zeros((n, 7))
    b[:, 0], b[:, 1] = rng.uniform(5, 5 + spread, n), rng.uniform(-spread / 2, spread / 2, n)
    b[:, 2] = rng.uniform(-2, -1.5, n)
    b[:, 3], b[:, 4], b[:, 5] = rng.uniform(3, 5, n), rng.uniform(1.5, 2.2, n), rng.uniform(1.4, 2, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def spaced_boxes(rng, n, pitch=8.0):
    """n boxes on a grid of ``pitch`` metres: no two collide (the longest diagonal is below 5.5 m)."""
    b = random_boxes(rng, n)
    side = int(np.ceil(np.sqrt(n)))
    b[:, 0], b[:, 1] = 6 + pitch * (np.arange(n) % side), pitch * (np.arange(n) // side) - pitch * side / 2
    return b


def small_bank(rng, n=12, points=6):
    OA = _OA()
    boxes = spaced_boxes(rng, n)
    pts = rng.uniform(-1, 1, (n * points, 4)).astype(np.float32)
    return OA.ObjectBank(pts, np.arange(n + 1) * points, boxes)


# ------------------------------------------------------------------------------------------------ collision rule
def _segment_distance(p, a, b):
    ab, ap = b - a, p - a
    t = np.clip(np.dot(ap, ab) / np.dot(ab, ab), 0, 1)
    return float(np.linalg.norm(ap - t * ab))


def _gap(p, q):
    """Distance between two convex quadrilaterals that do not overlap: the least corner-to-edge distance."""
    return min(min(_segment_distance(p[i], q[k], q[(k + 1) % 4]), _segment_distance(q[i], p[k], p[(k + 1) % 4]))
               for i in range(4) for k in range(4))


def test_collision_rule_against_the_intersection_area():
    OA = _OA()
    rng = np.random.default_rng(7)
    n = 2000
    a = np.zeros((n, 7))
    a[:, 3], a[:, 4], a[:, 6] = rng.uniform(2, 5, n), rng.uniform(1, 2.5, n), rng.uniform(-np.pi, np.pi, n)
    b = np.zeros((n, 7))
    b[:, 0], b[:, 1] = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    b[:, 3], b[:, 4], b[:, 6] = rng.uniform(2, 5, n), rng.uniform(1, 2.5, n), rng.uniform(-np.pi, np.pi, n)
    fa, fb = OA.footprints(a), OA.footprints(b)
    got = [OA.collides(fa[i:i + 1], fb[i:i + 1])[0, 0] for i in range(n)]
    excluded, hits = 0, 0
    for i in range(n):
        area = float(KR.intersection_area(a[i, [0, 1, 3, 4, 6]], b[i, [0, 1, 3, 4, 6]]))
        if 0 < area < 1e-9 or (area == 0 and _gap(fa[i], fb[i]) < 1e-9):
            excluded += 1
            continue
        hits += area > 0
        assert bool(got[i]) == (area > 0), (i, area)
        assert OR.collide(fa[i], fb[i]) == (area > 0), (i, area)           # the restatement follows the same rule
    assert excluded <= 0.01 * n
    assert 0.15 * n < hits < 0.85 * n                                       # both answers are well represented


def test_collision_rule_planted_cases():
    OA = _OA()
    box = lambda cx, cy, l, w, th: [cx, cy, 0, l, w, 1, th]                # noqa: E731
    cases = {
        'inside': (box(0, 0, 6, 4, 0.3), box(0.2, -0.1, 1, 0.5, -1.0), True),
        'cross': (box(0, 0, 6, 1, 0), box(0, 0, 6, 1, np.pi / 2), True),   # no corner of either inside the other
        'identical': (box(1, 2, 4, 2, 0.7), box(1, 2, 4, 2, 0.7), True),
        'touching_x': (box(1, 0.5, 2, 1, 0), box(3, 0.5, 2, 1, 0), False),  # share the edge x = 2
        'touching_y': (box(1, 0.5, 2, 1, 0), box(1, 1.5, 2, 1, 0), False),  # share the edge y = 1
        'apart': (box(0, 0, 2, 1, 0.4), box(10, 0, 2, 1, -0.4), False),
        'hulls_only': (box(0, 0, 6, 0.5, np.pi / 4), box(2.5, -2.5, 1, 1, 0), False),   # hulls overlap, boxes do not
    }
    for name, (p, q, want) in cases.items():
        fp, fq = OA.footprints([p]), OA.footprints([q])
        assert bool(OA.collides(fp, fq)[0, 0]) is want, name
        assert bool(OA.collides(fq, fp)[0, 0]) is want, name
        assert OR.collide(fp[0], fq[0]) is want, name
    # the cross: every corner of each lies outside the other
    fp, fq = OA.footprints([cases['cross'][0]])[0], OA.footprints([cases['cross'][1]])[0]
    assert not any(OR._strictly_inside(fp, c) for c in fq) and not any(OR._strictly_inside(fq, c) for c in fp)
    # a matrix: each entry is the pair's answer
    boxes = random_boxes(np.random.default_rng(1), 9, spread=10)
    f = OA.footprints(boxes)
    m = OA.collides(f[:4], f)
    assert m.shape == (4, 9) and all(bool(m[i, j]) == OR.collide(f[i], f[j]) for i in range(4) for j in range(9))
    # the footprint's corners are those the rasteriser draws (cell size 1, origin 0: the vertices truncated)
    from mask_bev_amd import rasterize
    assert np.array_equal(rasterize.box_vertices(boxes, (0, 64), (-32, 32), 64, 64),
                          np.intp(f + [0, 32]).astype(np.int32))
    assert np.allclose(f, [OR.corners(b) for b in boxes], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the noise search
def test_noise_search_equals_the_restatement():
    OA = _OA()
    boxes = random_boxes(np.random.default_rng(3), 8, spread=12)             # crowded: some tries collide
    noise = OA.ObjectNoise(translation_std=[1.0, 1.0, 0.25], num_try=20)
    rot, loc, sel = noise.search(np.random.default_rng(11), boxes)
    r_rot, r_loc, r_sel = OR.object_noise(np.random.default_rng(11), boxes, (1.0, 1.0, 0.25), num_try=20)
    assert np.array_equal(sel, r_sel) and np.array_equal(rot, r_rot) and np.array_equal(loc, r_loc)
    assert sel.any() and (np.abs(rot[sel]) <= 0.15707963267).all() and (loc[sel, 2] != 0).all()
    # not every box took its first try: the collision test decided something
    first_rot = np.random.default_rng(11)
    first_rot.normal(size=(8, 20, 3))
    assert not np.array_equal(rot, first_rot.uniform(-0.15707963267, 0.15707963267, size=(8, 20))[:, 0])
    # every moved box is free of every other final footprint
    frame = OA.ObjectFrame(boxes)
    noise.run(np.random.default_rng(11), frame)
    assert frame.noise and np.array_equal(frame.rot, rot)
    final = [OR.corners(b) for b in frame.moved_boxes]
    for i in np.flatnonzero(sel):
        assert not any(OR.collide(final[i], final[k]) for k in range(8) if k != i), i
    assert np.array_equal(frame.moved_boxes, OR.moved_boxes(boxes, r_rot, r_loc))
    assert np.array_equal(frame.moved_boxes[~sel], boxes[~sel])
    # the defaults are the reference's
    d = OA.ObjectNoise()
    assert d._translation_std.tolist() == [0.25] * 3 and d._rot_range == (-0.15707963267, 0.15707963267) and d._num_try == 100
    with pytest.raises(NotImplementedError, match='global_rot_range'):
        OA.ObjectNoise(global_rot_range=[-0.1, 0.1])
    OA.ObjectNoise(global_rot_range=[0.0, 0.0])


def test_walled_in_box_stays_and_zero_tries_move_nothing():
    OA = _OA()
    box = lambda cx, cy, l, w: [cx, cy, -1.5, l, w, 1.5, 0.0]               # noqa: E731
    # a 4 x 2 box in a slot 0.1 m wider than itself on every side, between four walls that collide with nothing
    boxes = np.array([box(0, 0, 4, 2), box(12.1, 0, 20, 60), box(-12.1, 0, 20, 60), box(0, 11.1, 4, 20), box(0, -11.1, 4, 20)])
    f = OA.footprints(boxes)
    assert not (OA.collides(f, f) & ~np.eye(5, dtype=bool)).any()
    frame = OA.ObjectFrame(boxes)
    OA.ObjectNoise(translation_std=[5.0, 5.0, 5.0], num_try=3).run(np.random.default_rng(0), frame)
    assert not frame.selected[0] and frame.rot[0] == 0 and (frame.loc[0] == 0).all()
    assert np.array_equal(frame.moved_boxes[0], boxes[0])
    row = frame.table[0]
    assert row[8:13].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and row[13] == OA.FLAG_MOVE     # identity, still claims its points
    assert np.array_equal(OR.object_noise(np.random.default_rng(0), boxes, (5.0, 5.0, 5.0), num_try=3)[2], frame.selected)
    # num_try = 0
    frame = OA.ObjectFrame(boxes)
    OA.ObjectNoise(num_try=0).run(np.random.default_rng(0), frame)
    assert not frame.selected.any() and not frame.rot.any() and not frame.loc.any()
    assert np.array_equal(frame.moved_boxes, boxes)
    # no boxes: untouched, nothing drawn
    rng = np.random.default_rng(5)
    frame = OA.ObjectFrame(np.zeros((0, 7)))
    OA.ObjectNoise().run(rng, frame)
    assert frame.table.shape == (0, 14) and rng.integers(0, 1 << 30) == np.random.default_rng(5).integers(0, 1 << 30)


# ------------------------------------------------------------------------------------------------ object_sample
def test_object_sample_count_acceptance_and_determinism():
    OA = _OA()
    bank = small_bank(np.random.default_rng(4), n=12)
    labels = np.array([[-20.0, 0, -1.5, 4, 2, 1.5, 0.2]])                   # far from every bank entry
    sample = OA.ObjectSample('unused', 15, bank=bank)
    counts = set()
    for seed in range(40):
        got = sample.choose(np.random.default_rng(seed), labels)
        assert got == OR.object_sample(np.random.default_rng(seed), labels, bank.boxes, 15), seed
        # the count rule and the acceptance order, replayed: spaced entries collide only with themselves
        rng = np.random.default_rng(seed)
        count = sum(int(rng.integers(0, 15)) for _ in range(3)) % 15
        picks = [int(rng.integers(0, 12)) for _ in range(count)]
        assert got == list(dict.fromkeys(picks)), seed                      # a repeated pick is rejected, not retried
        counts.add(count)
    assert len(counts) > 8 and max(counts) <= 14
    # an entry placed on top of a label is never accepted
    on_top = np.concatenate([bank.boxes[3:4] + [0.3, 0.2, 0, 0, 0, 0, 0.1], labels])
    taken = [k for seed in range(60) for k in sample.choose(np.random.default_rng(seed), on_top)]
    assert 3 not in taken and {0, 1, 2, 4, 5} <= set(taken)
    # frames: accepted boxes are appended in order, with the remove bit; the same seed gives the same batch
    both = [sample, OA.ObjectNoise()]
    a = OA.draw_frames(both, np.random.default_rng(9), [labels, on_top, np.zeros((0, 7))])
    b = OA.draw_frames(both, np.random.default_rng(9), [labels, on_top, np.zeros((0, 7))])
    assert all(np.array_equal(x.table, y.table) and x.pasted == y.pasted for x, y in zip(a, b))
    assert any(f.pasted for f in a)
    rng = np.random.default_rng(9)
    for f, lab in zip(a, [labels, on_top, np.zeros((0, 7))]):
        boxes, pasted, rot, loc, flags = OR.frame(rng, lab, bank.boxes, 15, {})
        assert f.pasted == pasted and np.array_equal(f.boxes, boxes) and f.n_labels == len(lab)
        assert np.array_equal(f.table[:, 13], flags) and np.array_equal(f.rot, rot) and np.array_equal(f.loc, loc)
        assert np.array_equal(f.boxes[len(lab):], bank.boxes[pasted])
    with pytest.raises(ValueError):
        OA.draw_frames([OA.ObjectNoise(), sample], np.random.default_rng(1), [labels] * 8)      # sample after noise


# ------------------------------------------------------------------------------------------------ the bank's file
def test_object_bank_round_trip_and_missing_file(tmp_path):
    OA = _OA()
    bank = small_bank(np.random.default_rng(6), n=5, points=7)
    path = OA.ObjectBank.default_path(tmp_path)
    assert path == tmp_path / 'samples.npz'
    bank.save(path)
    back = OA.ObjectBank.load(path)
    assert len(back) == 5 and back.points.dtype == np.float32 and back.offsets.dtype == np.int32 and back.boxes.dtype == np.float64
    assert np.array_equal(back.points, bank.points) and np.array_equal(back.offsets, bank.offsets)
    assert np.array_equal(back.boxes, bank.boxes) and np.array_equal(back.sample_points(2), bank.points[14:21])
    assert OA.ObjectSample(str(tmp_path), 3).bank.boxes.shape == (5, 7)     # the default location
    other = tmp_path / 'other'
    other.mkdir()
    with pytest.raises(FileNotFoundError, match='build-object-bank') as e:
        OA.ObjectSample(str(other), 3)
    assert 'samples.pkl' not in str(e.value)
    (other / 'samples.pkl').write_bytes(b'\x80\x04N.')
    with pytest.raises(FileNotFoundError, match='samples.pkl.*not read.*--build-object-bank'):
        OA.ObjectSample(str(other), 3)
    with pytest.raises(ValueError):
        OA.ObjectBank(bank.points, bank.offsets[:-1], bank.boxes)


# ------------------------------------------------------------------------------------------------ lists
def test_object_list_accepts_the_reference_configuration():
    from mask_bev_amd import augment as A
    OA = _OA()
    bank = small_bank(np.random.default_rng(8))
    ts = OA.make_kitti_object_augmentation_list(CONFIG_01, bank)
    assert [type(t) for t in ts] == [OA.ObjectSample, OA.ObjectNoise, A.KittiFlip, A.RandomRotate, A.GlobalNoise,
                                     A.RandomDropPoints, A.ShufflePoints, A.JitterPoints]
    assert ts[0].bank is bank and ts[0]._num_sample == 15
    assert OA.object_transforms(ts) == ts[:2] and OA.stage_bank(ts) is bank
    assert ts[0].draw(np.random.default_rng(0)) == [] and ts[1].draw(np.random.default_rng(0)) == []
    # an object transform after a point transform, or inside rand_augment
    with pytest.raises(ValueError, match='before every point transform'):
        OA.make_kitti_object_augmentation_list([CONFIG_01[2], CONFIG_01[1]], bank)
    with pytest.raises(ValueError, match='before every point transform'):
        OA.make_kitti_object_augmentation_list([CONFIG_01[1], CONFIG_01[2], CONFIG_01[0]], bank)
    with pytest.raises(ValueError, match='rand_augment'):
        OA.make_kitti_object_augmentation_list(
            [{'name': 'rand_augment', 'num_augments': 1, 'magnitude': 1, 'transforms': [CONFIG_01[1], CONFIG_01[2]]}], bank)
    with pytest.raises(ValueError, match='object_sample before object_noise'):
        OA.make_kitti_object_augmentation_list([CONFIG_01[1], CONFIG_01[0]], bank)
    # the reference's import path
    from mask_bev.augmentations import kitti_mask_augmentations as KA
    assert KA.BoxNoise is OA.ObjectNoise and KA.ObjectSample is OA.ObjectSample
    # a list without object transforms comes out as the old factory builds it
    plain = OA.make_kitti_object_augmentation_list(CONFIG_01[2:])
    assert [type(t) for t in plain] == [type(t) for t in A.make_kitti_augmentation_list(CONFIG_01[2:])]


def test_old_factories_still_raise():
    from mask_bev_amd import augment as A
    for make in (A.make_kitti_augmentation_list, A.make_waymo_augmentation_list, A.make_semantic_kitti_augmentation_list):
        with pytest.raises(NotImplementedError, match='samples.pkl'):
            make([CONFIG_01[0]])
        with pytest.raises(NotImplementedError, match='collision search'):
            make([CONFIG_01[1]])


def test_apply_refuses_object_transforms_on_maps_and_scenes():
    """The checks of ``DeviceAugmentation.apply`` that come before anything touches a device."""
    import torch
    from mask_bev_amd import augment as A
    from mask_bev_amd._lib import MaskBevHipError
    OA = _OA()
    aug = A.DeviceAugmentation([OA.ObjectNoise()], seed=1)
    with pytest.raises(MaskBevHipError):
        aug.apply([torch.zeros(5, 4)], boxes=[np.zeros((0, 7))])              # no CPU fallback
    assert aug.draw(2)[0].ops == ()                                          # an object transform draws no point op
    fake = torch.zeros(5, 4, device='meta')
    for kw in (dict(instance_maps=torch.zeros(1, 4, 4, dtype=torch.int32, device='meta')), dict(scene_transforms=[np.eye(4)[None]])):
        with pytest.raises(ValueError, match='instance maps or scene'):
            aug._object_frames(1, kw.get('instance_maps'), kw.get('scene_transforms'), [np.zeros((0, 7))], None)
    with pytest.raises(ValueError, match='boxes='):
        aug._object_frames(1, None, None, None, None)
    assert A.DeviceAugmentation([A.KittiFlip()], seed=1)._object_frames(1, None, None, None, None) is None
    del fake
