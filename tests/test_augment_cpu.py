"""Host side of the K23 augmentations (mask_bev_amd/augment.py) and the numpy restatement the GPU tests compare against
(tests/augment_ref.py): config parsing, the reference's magnitude rules, seeded host draws, composed matrices, the warp rule
against numpy's own flips and rot90."""
import inspect

import numpy as np
import pytest
import torch

from tests import augment_ref as AR

GENTLE = [  # configs/training/semantic_kitti/01_point_mask_data_aug_gentle.yml of the reference, `augmentations:`
    {'name': 'drop', 'prob_drop': 0.5, 'per_point_drop_prob': 0.05},
    {'name': 'flip', 'prob_flip_x': 0, 'prob_flip_y': 0.5},
    {'name': 'shuffle', 'prob_shuffle': 0},
    {'name': 'rotate', 'rotate_prob': 0.5, 'rotation_range': 5},
    {'name': 'jitter', 'prob_jitter': 0.5, 'jitter_std': 0.02, 'intensity_std': 0.01},
]


def _always(name, **kw):
    from mask_bev_amd import augment as A
    return A.make_augmentation(dict(name=name, **kw))


def _rng(seed=0):
    return np.random.default_rng(seed)


def test_config_parsing_and_defaults():
    from mask_bev_amd import augment as A
    ts = A.make_semantic_kitti_augmentation_list(GENTLE)
    assert [type(t) for t in ts] == [A.RandomDropPoints, A.Flip, A.ShufflePoints, A.RandomRotate, A.JitterPoints]
    assert ts[3]._rotation_range == (-5, 5)
    assert ts[4]._jitter_std == (0.02, 0.02, 0.02) and ts[4]._max_delta is None and ts[4]._intensity_max_delta is None
    f = A.make_augmentation({'name': 'flip'})
    assert (f._prob_flip_x, f._prob_flip_y) == (0.5, 0.5)
    assert A.make_augmentation({'name': 'shuffle'})._prob_shuffle == 0.5
    assert A.make_augmentation({'name': 'rotate', 'rotate_prob': 1, 'rotation_range': [-3, 7]})._rotation_range == (-3, 7)
    j = A.make_augmentation({'name': 'jitter', 'prob_jitter': 1, 'jitter_std': [1, 2, 3], 'max_delta': 0.5})
    assert j._jitter_std == (1, 2, 3) and j._max_delta == (0.5, 0.5, 0.5) and j._intensity_std == 0.0
    # the reference's keyword names, class by class
    for cls, names in ((A.Flip, ['prob_flip_x', 'prob_flip_y']), (A.ShufflePoints, ['prob_shuffle']),
                       (A.RandomRotate, ['rotate_prob', 'rotation_range']), (A.DecimatePoints, ['prob_decimate', 'keep_every']),
                       (A.JitterPoints, ['prob_jitter', 'jitter_std', 'max_delta', 'intensity_std', 'intensity_max_delta']),
                       (A.RandomDropPoints, ['prob_drop', 'per_point_drop_prob'])):
        assert list(inspect.signature(cls.__init__).parameters)[1:] == names
    with pytest.raises(TypeError):
        A.make_augmentation({'name': 'flip', 'prob': 1})


def test_alias_module_exports_the_reference_names():
    from mask_bev.augmentations import semantic_kitti_mask_augmentations as M
    from mask_bev_amd import augment as A
    assert M.make_augmentation is A.make_augmentation
    assert M.make_semantic_kitti_augmentation_list is A.make_semantic_kitti_augmentation_list


def test_errors():
    from mask_bev_amd import augment as A
    with pytest.raises(NotImplementedError):
        A.make_augmentation({'name': 'cut_pc', 'prob_cut': 0.5})
    with pytest.raises(NotImplementedError):
        A.make_augmentation({'name': 'mirror'})
    with pytest.raises(NotImplementedError):
        A.make_augmentation({})
    with pytest.raises(ValueError):
        A.make_augmentation({'name': 'decimate', 'prob_decimate': 1, 'keep_every': 0})
    d = A.make_augmentation({'name': 'decimate', 'prob_decimate': 1, 'keep_every': 2})
    with pytest.raises(ValueError):
        d.draw(_rng(), 0.4)                                   # int(2 * 0.4) = 0


def test_magnitude_rules():
    from mask_bev_amd import augment as A
    # flip, shuffle: the probability scales
    assert _always('flip', prob_flip_x=0.5, prob_flip_y=0.5).draw(_rng(), 0) == []
    assert len(_always('flip', prob_flip_x=0.5, prob_flip_y=0.5).draw(_rng(), 2)) == 2
    assert _always('shuffle', prob_shuffle=0.5).draw(_rng(), 0) == []
    assert _always('shuffle', prob_shuffle=0.5).draw(_rng(), 2) == [A.Op(A.OP_SHUFFLE)]
    # rotate: the range scales, the probability does not
    assert _always('rotate', rotate_prob=1, rotation_range=10).draw(_rng(), 0) == [A.rotation_op(0.0)]
    thetas = []
    for s in range(200):
        (op,) = _always('rotate', rotate_prob=1, rotation_range=10).draw(_rng(s), 0.5)
        thetas.append(np.rad2deg(np.arctan2(op.p[2], op.p[0])))
    assert max(np.abs(thetas)) <= 5 and max(np.abs(thetas)) > 4
    # decimate: int(keep_every * magnitude)
    assert _always('decimate', prob_decimate=1, keep_every=3).draw(_rng(), 1.5) == [A.Op(A.OP_DECIMATE, 4)]
    # jitter: the noise scales (the magnitude travels in p[0]); no max_delta = +inf
    (op,) = _always('jitter', prob_jitter=1, jitter_std=0.02, intensity_std=0.01).draw(_rng(), 1.5)
    assert op.p == (1.5, 0.02, 0.02, 0.02, 0.01) + (float('inf'),) * 4
    (op,) = _always('jitter', prob_jitter=1, jitter_std=0.02, max_delta=[1, 2, 3], intensity_max_delta=0.1).draw(_rng())
    assert op.p == (1.0, 0.02, 0.02, 0.02, 0.0, 1.0, 2.0, 3.0, 0.1)
    # drop: per_point_drop_prob scales; T = ceil(p * 2^24) clamped
    assert _always('drop', prob_drop=1, per_point_drop_prob=0.05).draw(_rng(), 2) == [A.Op(A.OP_DROP, A.drop_threshold(0.1))]
    assert A.drop_threshold(0) == 0 and A.drop_threshold(1) == 1 << 24 and A.drop_threshold(3.5) == 1 << 24
    assert A.drop_threshold(0.05) == int(np.ceil(0.05 * 2 ** 24)) and A.drop_threshold(2.0 ** -30) == 1


def test_rand_augment_draws_with_replacement():
    from mask_bev_amd import augment as A
    ra = A.make_augmentation({'name': 'rand_augment', 'num_augments': 4, 'magnitude': 1.5, 'transforms': [
        {'name': 'rotate', 'rotate_prob': 1, 'rotation_range': 10}, {'name': 'decimate', 'prob_decimate': 1, 'keep_every': 2}]})
    assert isinstance(ra, A.RandAugment)
    seen_repeat = False
    for s in range(20):
        ops = ra.draw(_rng(s))
        assert len(ops) == 4
        codes = [o.code for o in ops]
        seen_repeat |= codes.count(A.OP_DECIMATE) >= 2 or codes.count(A.OP_LINEAR) >= 2
        assert all(o.arg == 3 for o in ops if o.code == A.OP_DECIMATE)               # int(2 * 1.5)
    assert seen_repeat
    one = A.make_augmentation({'name': 'rand_augment', 'num_augments': 3, 'magnitude': 1, 'transforms': [
        {'name': 'drop', 'prob_drop': 1, 'per_point_drop_prob': 0.1}]})
    assert [o.code for o in one.draw(_rng())] == [A.OP_DROP] * 3
    too_many = A.DeviceAugmentation([A.make_augmentation({'name': 'rand_augment', 'num_augments': 9, 'magnitude': 1,
                                                          'transforms': [{'name': 'shuffle', 'prob_shuffle': 1}]})])
    with pytest.raises(ValueError):
        too_many.draw(1)


def test_host_draws_are_seeded():
    from mask_bev_amd import augment as A
    ts = A.make_semantic_kitti_augmentation_list(GENTLE)
    a, b = A.DeviceAugmentation(ts, 7), A.DeviceAugmentation(ts, 7)
    da, db = a.draw(16), b.draw(16)
    assert da == db and len({d.seed for d in da}) == 16 and all(0 <= d.seed < 1 << 64 for d in da)
    assert len({d.ops for d in da}) > 4                                              # the samples do differ
    assert A.DeviceAugmentation(ts, 8).draw(16) != da
    a.reseed(7, 0, 3, 11)
    b.reseed(7, 0, 3, 11)
    d1 = a.draw(4)
    assert d1 == b.draw(4)
    a.reseed(7, 1, 3, 11)
    assert a.draw(4) != d1
    rec = A.pack_records(da)
    assert rec.dtype.itemsize == 656 and rec.tobytes() == A.pack_records(db).tobytes()
    assert rec['n_ops'].tolist() == [len(d.ops) for d in da]
    assert [(int(r['seed_hi']) << 32) | int(r['seed_lo']) for r in rec] == [d.seed for d in da]
    assert A.batch_mode(da) == 1 and A.batch_mode([A.SampleDraw(1, (A.rotation_op(3.0),))]) == 0
    assert A.batch_mode([A.SampleDraw(1, (A.Op(A.OP_DROP, 5),)), A.SampleDraw(2, (A.Op(A.OP_SHUFFLE),))]) == 2


def test_composed_matrix_depends_on_op_order():
    from mask_bev_amd import augment as A
    flip_x, rot = A.Op(A.OP_LINEAR, 0, (-1., 0., 0., 1.)), A.rotation_op(30.0)
    r, f = AR.rotation(30.0), np.diag([-1., 1.])
    fr = A.SampleDraw(0, (flip_x, rot)).matrix
    rf = A.SampleDraw(0, (rot, flip_x)).matrix
    assert np.array_equal(fr, r @ f) and np.array_equal(rf, f @ r) and not np.allclose(fr, rf)
    # and that is what the restated point program does
    p = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    got, _ = AR.run_program(p, 0, [tuple(flip_x), tuple(rot)])
    assert np.allclose(got[0, :2], fr @ p[0, :2], rtol=1e-6) and got[0, 2] == 3.0
    assert np.array_equal(A.SampleDraw(0, (A.Op(A.OP_SHUFFLE), A.Op(A.OP_DROP, 3))).matrix, np.eye(2))


@pytest.mark.parametrize('shape', [(6, 4), (7, 5), (32, 32)])
def test_restated_warp_of_a_flip_is_a_reversed_axis(shape):
    m = np.random.default_rng(0).integers(1, 99, shape).astype(np.int32)
    cx, cy = shape[0] / 2, shape[1] / 2                                               # a symmetric range
    assert np.array_equal(AR.warp(m, np.diag([-1., 1.]), cx, cy)[0], m[::-1])
    assert np.array_equal(AR.warp(m, np.diag([1., -1.]), cx, cy)[0], m[:, ::-1])
    assert np.array_equal(AR.warp(m, np.diag([-1., -1.]), cx, cy)[0], m[::-1, ::-1])
    assert np.array_equal(AR.warp(m, np.eye(2), cx, cy)[0], m)
    # an asymmetric range mirrors about the origin's cell: cells from outside arrive as 0
    got = AR.warp(m, np.diag([-1., 1.]), 1.0, cy)[0]
    assert np.array_equal(got[:2], m[:2][::-1]) and not got[2:].any()


@pytest.mark.parametrize('n', [8, 33])
def test_restated_warp_at_right_angles_is_rot90(n):
    m = np.random.default_rng(1).integers(1, 99, (n, n)).astype(np.int32)
    c = n / 2
    assert np.array_equal(AR.warp(m, AR.rotation(90.0), c, c)[0], np.rot90(m, 1))
    assert np.array_equal(AR.warp(m, AR.rotation(180.0), c, c)[0], np.rot90(m, 2))
    assert np.array_equal(AR.warp(m, AR.rotation(-90.0), c, c)[0], np.rot90(m, -1))
    # consistent with the points: the cell of a rotated point holds the value of the cell of the point
    r = AR.rotation(90.0)
    p = np.array([1.3, -2.6])
    cell = lambda q: tuple(np.floor(q + c).astype(int))
    assert AR.warp(m, r, c, c)[0][cell(r @ p)] == m[cell(p)]


def test_restated_hash_known_values():
    """pcg_hash as csrc/rng.hpp has it: three values worked out by hand from the formula in maskbev_hip.h."""
    def by_hand(v):
        s = (v * 747796405 + 2891336453) % 2 ** 32
        w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) % 2 ** 32
        return (w >> 22) ^ w
    for v in (0, 1, 0xFFFFFFFF, 123456789):
        assert int(AR.pcg(v)) == by_hand(v)
    assert np.array_equal(AR.pcg(np.array([0, 1, 5])), [by_hand(0), by_hand(1), by_hand(5)])
    n = AR.normal(99, 4, np.arange(65536), 0)
    assert np.abs(n).max() <= 5.78 and abs(n.mean()) < 5 / 256 and abs(n.var() - 1) < 5 * np.sqrt(2 / 65536)


def test_collates_without_an_augmentation_keep_their_defaults():
    from mask_bev_amd import batch
    sig = inspect.signature(batch.InstanceMapCollate.__init__).parameters
    assert list(sig)[1:] == ['num_queries', 'device', 'min_num_inst_pixels', 'packed', 'augmentation']
    assert sig['augmentation'].default is None
    sig = inspect.signature(batch.SceneCollate.__init__).parameters
    assert list(sig)[1:] == ['rasterizer', 'num_queries', 'device', 'min_num_inst_pixels', 'packed', 'augmentation']
    assert sig['augmentation'].default is None
    assert batch.InstanceMapCollate(8, 'cpu').augmentation is None and batch.SceneCollate(None, 8, 'cpu').augmentation is None


def test_cpu_tensors_and_bad_dims_are_refused():
    from mask_bev_amd import augment as A
    from mask_bev_amd._lib import MaskBevHipError
    aug = A.DeviceAugmentation(A.make_semantic_kitti_augmentation_list(GENTLE), 0)
    with pytest.raises(MaskBevHipError):
        aug.apply([torch.zeros((5, 4))])


def test_launcher_builds_the_augmentation_from_the_config():
    from mask_bev_amd.datasets import build_augmentation
    from mask_bev_amd import augment as A
    cfg = {'x_range': [-40, 40], 'y_range': [-40, 40], 'voxel_size': 0.16, 'seed': 3}
    assert build_augmentation(cfg) is None and build_augmentation(dict(cfg, augmentations=[])) is None
    aug = build_augmentation(dict(cfg, augmentations=GENTLE))
    assert isinstance(aug, A.DeviceAugmentation) and len(aug.transforms) == 5 and aug.voxel_size == 0.16
