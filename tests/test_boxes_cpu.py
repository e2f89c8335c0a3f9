"""Host side of the box datasets (K24's surroundings), no GPU: the fill-rule oracle against the golden maps and against a
brute-force check of itself, ``rasterize.box_vertices`` against the reference's recorded contours, the KITTI readers on
the sample frame, the box half of the augmentations against a restatement of the reference's lines, and the augmentations
that are not provided."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import box_rasterize_ref as BR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SAMPLE = os.path.join(GOLDEN, 'kitti_object_sample')


def golden():
    return np.load(os.path.join(GOLDEN, 'box_rasterizer.npz'))


def frame_rows(g, key, f):
    a, b = int(g[f'{key}_offsets'][f]), int(g[f'{key}_offsets'][f + 1])
    return g[f'{key}_boxes'][a:b], g[f'{key}_types'][a:b]


def frame_contours(g, key, f):
    a, b = int(g[f'{key}_contour_offsets'][f]), int(g[f'{key}_contour_offsets'][f + 1])
    return g[f'{key}_contours'][a:b]


def _R():
    from mask_bev_amd import rasterize
    return rasterize


def kitti_rasterizer(g, key):
    return _R().KittiRasterizer(tuple(g[f'{key}_x_range']), tuple(g[f'{key}_y_range']), tuple(g['z_range']), float(g['vs']))


def waymo_rasterizer(g):
    return _R().WaymoRasterizer(tuple(g['w_x_range']), tuple(g['w_y_range']), tuple(g['z_range']), float(g['vs']),
                                min_points=int(g['w_min_points']))


def selected(g, key, f):
    """The boxes the product paints in frame f and their ids."""
    boxes, types = frame_rows(g, key, f)
    if key == 'w':
        a, b = int(g['w_offsets'][f]), int(g['w_offsets'][f + 1])
        return waymo_rasterizer(g)._select(boxes, types, g['w_num_points'][a:b])
    return kitti_rasterizer(g, key)._select(boxes, types)


# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['a', 'b', 'w'])
def test_oracle_and_selection_reproduce_the_golden_maps(key):
    """Label selection, numbering and range skip of the product + its vertices + the oracle's fill = the maps the reference
    returned (through the stand-in cv2 whose fill is the oracle's: this pins the reference's own lines, not OpenCV)."""
    g = golden()
    names = g[f'{key}_names'].tolist()
    r = waymo_rasterizer(g) if key == 'w' else kitti_rasterizer(g, key)
    assert len(names) == 13 and g[f'{key}_maps'].shape == (13, r.ny, r.nx)
    for f, name in enumerate(names):
        boxes, ids = selected(g, key, f)
        verts = _R().box_vertices(boxes, r.x_range, r.y_range, r.nx, r.ny)
        assert verts.dtype == np.int32 and np.array_equal(verts, frame_contours(g, key, f)), name
        m = BR.rasterize_boxes(verts, ids, r.nx, r.ny)
        assert np.array_equal(m.T, g[f'{key}_maps'][f]), name            # the reference's image is [y-cell][x-cell]


def test_golden_cases_are_what_they_claim():
    g = golden()
    for key in ('a', 'b'):
        names = g[f'{key}_names'].tolist()
        maps = g[f'{key}_maps']
        area = {n: int((maps[i] > 0).sum()) for i, n in enumerate(names)}
        assert area['empty'] == 0 and area['wholly_outside'] == 0 and area['one_cell'] == 2
        assert area['centre_above_upper_bound'] > 0                      # the quirk: painted where it reaches the grid
        c = frame_contours(g, key, names.index('one_cell'))
        assert all(len({tuple(v) for v in quad}) == 1 for quad in c)     # four vertices in one cell
        c = frame_contours(g, key, names.index('negative_fraction'))
        assert (c == 0).any() and not (c < 0).any()                      # (-1, 0) truncates to 0, a floor would give -1
        two = maps[names.index('overlap_later_wins')]
        v1 = BR.box_cells(frame_contours(g, key, names.index('overlap_later_wins'))[0], maps.shape[2], maps.shape[1])
        assert (v1.T & (two == 2)).any()                                 # cells of box 1 that box 2 took
        assert sorted(np.unique(maps[names.index('types_and_skip')]).tolist()) == [0, 1, 3, 4]
        assert len(frame_contours(g, key, names.index('many_300'))) == 300             # all painted: two staging passes
    assert not g['falsy_maps'].any()
    for f in range(len(g['falsy_names'])):
        boxes, ids = selected(g, 'falsy', f)
        assert len(ids) == 0                                             # x_range[1] = 0 is falsy: every box is skipped
    # Waymo: a box below min_points leaves, the next becomes id 1
    names = g['w_names'].tolist()
    assert np.unique(g['w_maps'][names.index('overlap_later_wins')]).tolist() == [0, 1]


def test_box_vertices_refuses_what_the_kernel_cannot_hold():
    bv = _R().box_vertices
    ok = [[10., 0., 0., 4., 1.8, 1.5, 0.3]]
    assert bv(ok, (0, 80), (-40, 40), 800, 800).shape == (1, 4, 2)
    assert bv(np.zeros((0, 7)), (0, 80), (-40, 40), 800, 800).shape == (0, 4, 2)
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            bv([[bad, 0., 0., 4., 1.8, 1.5, 0.3]], (0, 80), (-40, 40), 800, 800)
    with pytest.raises(ValueError):
        bv([[2e5, 0., 0., 4., 1.8, 1.5, 0.3]], (0, 80), (-40, 40), 800, 800)          # 2e6 cells > 2^20
    # truncation toward zero, not a floor
    v = bv([[0.05, 0.05, 0., 0.16, 0.16, 1.5, 0.]], (0, 10), (0, 10), 100, 100)          # corners at -0.3 and 1.3 cells
    assert sorted(np.unique(v).tolist()) == [0, 1]


def test_rasterizers_need_a_device_and_device_tensors():
    import torch
    from mask_bev_amd import ops_rasterize
    from mask_bev_amd._lib import MaskBevHipError
    r = _R().KittiRasterizer((0, 20), (-6, 6), (-3, 1), 0.5, device='cpu')
    assert (r.nx, r.ny) == (40, 24)
    with pytest.raises(MaskBevHipError):
        r.rasterize_batch([np.zeros((0, 7))])
    with pytest.raises(MaskBevHipError):
        ops_rasterize.rasterize_boxes(torch.zeros((1, 4, 2), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32),
                                      [0, 1], 8, 8)
    assert _R().KittiRasterizer((0, 80), (-40, 40), (-3, 1), 0.1).nx == 800


# ---------------------------------------------------------------------------------------------------------
# the oracle itself, brute force
# ---------------------------------------------------------------------------------------------------------
def _pip_fraction(verts, px, py):
    """Closed point-in-polygon with rationals: on an edge, or an odd number of crossings of the ray towards +x, each
    crossing located by its exact intersection abscissa."""
    p = (Fraction(px), Fraction(py))
    odd = False
    for e in range(4):
        (ax, ay), (bx, by) = [tuple(Fraction(int(c)) for c in verts[k % 4]) for k in (e, e + 1)]
        if (bx - ax) * (p[1] - ay) == (by - ay) * (p[0] - ax) and min(ax, bx) <= p[0] <= max(ax, bx) \
                and min(ay, by) <= p[1] <= max(ay, by):
            return True
        if (ay > p[1]) != (by > p[1]):
            x_at = ax + (p[1] - ay) * (bx - ax) / (by - ay)
            if p[0] < x_at:
                odd = not odd
    return odd


def _segment_distance_chebyshev_le_half(a, b, c):
    """Is cell c within Chebyshev distance 1/2 of the segment a-b?  Exact: the distance is convex and piecewise linear in
    the segment parameter, so its minimum is at an end or where |dx(t)| = |dy(t)| or one of them is 0."""
    a, b, c = [tuple(Fraction(int(v)) for v in p) for p in (a, b, c)]
    d = (b[0] - a[0], b[1] - a[1])
    ts = [Fraction(0), Fraction(1)]
    ex, ey = a[0] - c[0], a[1] - c[1]
    for sx, sy, k in ((d[0], d[1], 0), (d[0], -d[1], 1)):                # ex + t dx = ±(ey + t dy)
        den = sx - sy
        if den != 0:
            ts.append((ey - ex) / den if k == 0 else (-ey - ex) / den)
    for comp, dc in ((ex, d[0]), (ey, d[1])):
        if dc != 0:
            ts.append(-comp / dc)
    best = min(max(abs(ex + t * d[0]), abs(ey + t * d[1])) for t in ts if 0 <= t <= 1)
    return best <= Fraction(1, 2)


def test_oracle_brute_force_on_random_quadrilaterals():
    rng = np.random.default_rng(7)
    n_folded = 0
    for k in range(200):
        if k % 2 == 0:                                                   # what the product makes: a truncated rectangle
            th = rng.uniform(-math.pi, math.pi)
            c, l, w = rng.uniform(2, 10, 2), rng.uniform(0.2, 9), rng.uniform(0.2, 5)
            d, n = np.array([math.cos(th), math.sin(th)]), np.array([-math.sin(th), math.cos(th)])
            quad = np.array([c + d * l / 2 + n * w / 2, c - d * l / 2 + n * w / 2, c - d * l / 2 - n * w / 2,
                             c + d * l / 2 - n * w / 2])
            verts = np.trunc(quad).astype(np.int64)
            if k % 4 == 0:
                verts = verts[::-1].copy()                               # the other orientation
        else:                                                            # anything: folded, degenerate, repeated vertices
            verts = rng.integers(-2, 12, (4, 2))
            n_folded += 1
        gx, gy = np.meshgrid(np.arange(-4, 15), np.arange(-4, 15), indexing='ij')
        inside = BR.inside_closed(verts, gx, gy)
        want = np.array([[_pip_fraction(verts, int(x), int(y)) for y in range(-4, 15)] for x in range(-4, 15)])
        assert np.array_equal(inside, want), verts
        for e in range(4):
            a, b = verts[e], verts[(e + 1) % 4]
            cells = BR.line_cells(a, b)
            assert len(cells) == max(abs(int(b[0] - a[0])), abs(int(b[1] - a[1]))) + 1
            assert tuple(cells[0]) == tuple(a) and tuple(cells[-1]) == tuple(b)
            for c in cells:
                assert _segment_distance_chebyshev_le_half(a, b, c), (a, b, c)
        # the painted set is I ∪ L clipped, nothing else
        m = BR.box_cells(verts, 12, 11)
        lines = np.zeros_like(m)
        for e in range(4):
            for x, y in BR.line_cells(verts[e], verts[(e + 1) % 4]):
                if 0 <= x < 12 and 0 <= y < 11:
                    lines[x, y] = True
        assert np.array_equal(m, inside[4:16, 4:15] | lines)
    assert n_folded == 100


# ---------------------------------------------------------------------------------------------------------
# readers
# ---------------------------------------------------------------------------------------------------------
def test_kitti_readers_parse_the_sample_frame():
    from mask_bev_amd import batch as B
    lab = B.read_kitti_label(os.path.join(SAMPLE, 'label_2', '000000.txt'))
    names = [_R().KITTI_TYPES[t] for t in lab['type']]
    assert names == ['Car', 'Van', 'Truck', 'Car', 'Pedestrian', 'Cyclist']          # the two DontCare lines are gone
    assert lab['occluded'].tolist() == [0, 1, 2, 2, 0, 3] and lab['truncated'].tolist() == [0.0, 0.1, 0.4, 0.62, 0.0, 0.0]
    assert lab['bbox'].shape == (6, 4) and lab['bbox'][0].tolist() == [587.01, 173.33, 614.12, 200.12]
    assert lab['dimensions'][2].tolist() == [2.85, 2.63, 12.34] and lab['location'][1].tolist() == [-16.53, 2.39, 58.49]
    assert lab['rotation_y'].tolist() == [-1.59, 1.57, -1.56, 1.33, 0.01, -1.20] and lab['alpha'][0] == -1.58
    cal = B.read_kitti_calib(os.path.join(SAMPLE, 'calib', '000000.txt'))
    assert sorted(cal) == ['P0', 'P1', 'P2', 'P3', 'R0_rect', 'Tr_imu_to_velo', 'Tr_velo_to_cam']
    assert all(m.shape == (4, 4) and m[3].tolist() == [0, 0, 0, 1] for m in cal.values())
    assert cal['Tr_velo_to_cam'][0].tolist() == [7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03]
    assert cal['R0_rect'][:3, 3].tolist() == [0, 0, 0] and cal['R0_rect'][1, 1] == 9.999421e-01 and cal['P2'][0, 3] == 44.85728

    velo = B.kitti_labels_to_velodyne(lab, cal)
    c2v = np.linalg.inv(cal['Tr_velo_to_cam'])
    for k in range(6):
        h, w, l = lab['dimensions'][k]
        assert velo['dimensions'][k].tolist() == [l, h, w]                            # dimensions[[2, 0, 1]]
        want = (c2v @ np.array([*lab['location'][k], 1.0]))[:3]
        assert np.array_equal(velo['location'][k], want)
        yaw = -lab['rotation_y'][k] - np.pi / 2
        assert velo['rotation_y'][k] == np.arctan2(np.sin(yaw), np.cos(yaw)) and -np.pi <= velo['rotation_y'][k] <= np.pi
        assert np.array_equal(velo['boxes'][k], [*want, l, h, w, velo['rotation_y'][k]])
    assert 46 < velo['location'][0][0] < 48 and abs(velo['location'][0][1] - 0.65) < 0.5      # the car ahead, 47 m out
    assert np.array_equal(velo['type'], lab['type'])

    ok = B.is_difficulty_valid(lab['occluded'], lab['truncated'])
    assert ok.tolist() == [True, True, True, False, True, False]          # 0.62 > 0.5 largely occluded; occlusion unknown
    inside = B.object_range_mask(velo['boxes'], (0, 50), (-40, 40))
    assert inside.tolist() == [True, False, False, True, True, True]
    kept = B.select_labels(velo, ok & inside)
    assert kept['boxes'].shape == (2, 7) and kept['type'].tolist() == [0, 3]
    assert np.array_equal(B.object_range_mask([[50., -40., 0, 1, 1, 1, 0]], (0, 50), (-40, 40)), [True])   # closed ranges
    empty = B.read_kitti_label(os.devnull)
    assert empty['type'].shape == (0,) and B.kitti_labels_to_velodyne(empty, cal)['boxes'].shape == (0, 7)


# ---------------------------------------------------------------------------------------------------------
# boxes under the augmentations: the reference's lines, restated
# ---------------------------------------------------------------------------------------------------------
def _reference_flip_y(boxes):
    """kitti_mask_augmentations.py:67-71."""
    out = boxes.copy()
    out[:, 1] = -out[:, 1]
    out[:, 6] = -out[:, 6]
    return out


def _reference_rotate(boxes, theta_deg):
    """kitti_mask_augmentations.py:101-106,118-123."""
    c, s = np.cos(np.deg2rad(theta_deg)), np.sin(np.deg2rad(theta_deg))
    R = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    out = boxes.copy()
    for k in range(len(out)):
        out[k, :3] = (R @ np.array([*boxes[k, :3], 1]).T).T[:3]
        out[k, 6] = boxes[k, 6] + np.deg2rad(theta_deg)
    return out


def _reference_global_noise(boxes, scale, noise):
    """kitti_mask_augmentations.py:209-214."""
    out = boxes.copy()
    for k in range(len(out)):
        out[k, :3] *= scale
        out[k, 3:6] *= scale
        out[k, :3] += noise
    return out


def _boxes(n=9, seed=3):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(0, 70, n), rng.uniform(-40, 40, n), rng.uniform(-2, 0, n), rng.uniform(3, 5, n),
                            rng.uniform(1.5, 2, n), rng.uniform(1.4, 2, n), rng.uniform(-np.pi, np.pi, n)])


def test_boxes_follow_flips_rotations_and_global_noise():
    from mask_bev_amd import augment as A
    boxes = _boxes()
    flip = A.KittiFlip(prob_flip_y=1.0).draw(np.random.default_rng(0))
    assert len(flip) == 1 and flip[0].p == (1., 0., 0., -1.)
    assert np.array_equal(A.transform_boxes(boxes, flip), _reference_flip_y(boxes))
    rot = A.RandomRotate(1.0, 30).draw(np.random.default_rng(5))
    rng = np.random.default_rng(5)
    assert rng.uniform(0, 1) < 1.0
    theta = rng.uniform(-30, 30)                                          # the same draws, in the reference's order
    assert rot == [A.rotation_op(theta)]
    got, want = A.transform_boxes(boxes, rot), _reference_rotate(boxes, theta)
    assert np.array_equal(got[:, 2:], want[:, 2:]) and np.allclose(got[:, :2], want[:, :2], rtol=0, atol=1e-13)
    noise_op = A.GlobalNoise(prob_aug=0.0, trans_std=0.2, scale_delta=0.05).draw(np.random.default_rng(9))   # always applied
    rng = np.random.default_rng(9)
    noise = rng.standard_normal((3,)) * 0.2
    scale = rng.uniform(1 - 0.05, 1 + 0.05)
    assert noise_op == [A.Op(A.OP_GLOBAL_NOISE, 0, (scale, *noise))]
    assert np.array_equal(A.transform_boxes(boxes, noise_op), _reference_global_noise(boxes, scale, noise))
    # composed, in op order; the composed matrix of the draw moves the centres
    ops = flip + rot + noise_op + rot
    want = _reference_rotate(_reference_global_noise(_reference_rotate(_reference_flip_y(boxes), theta), scale, noise), theta)
    assert np.allclose(A.transform_boxes(boxes, ops), want, rtol=0, atol=1e-12)
    m = A.SampleDraw(0, tuple(flip + rot)).matrix
    assert np.allclose(A.transform_boxes(boxes, flip + rot)[:, :2], boxes[:, :2] @ m.T, rtol=0, atol=1e-12)
    # the input is not modified; an empty table stays empty
    assert np.array_equal(boxes, _boxes()) and A.transform_boxes(np.zeros((0, 7)), ops).shape == (0, 7)
    # Waymo: center_y mirrored, heading left alone (waymo_mask_augmentations.py:54-59); two uniforms drawn
    rng_a, rng_b = np.random.default_rng(1), np.random.default_rng(1)
    wflip = A.WaymoFlip(prob_flip_y=1.0).draw(rng_a)
    rng_b.uniform(0, 1), rng_b.uniform(0, 1)
    assert rng_a.uniform(0, 1) == rng_b.uniform(0, 1)
    got = A.transform_boxes(boxes, wflip)
    assert np.array_equal(got[:, 1], -boxes[:, 1]) and np.array_equal(np.delete(got, 1, axis=1), np.delete(boxes, 1, axis=1))
    # an x flip (SemanticKITTI's Flip) mirrors the heading about the y axis; a bare linear op follows the direction vector
    xf = A.Flip(1.0, 0.0).draw(np.random.default_rng(0))
    assert np.allclose(A.transform_boxes(boxes, xf)[:, 6], np.pi - boxes[:, 6])
    bare = [A.Op(A.OP_LINEAR, 0, rot[0].p)]
    d = A.transform_boxes(boxes, bare)[:, 6] - (boxes[:, 6] + np.deg2rad(theta))
    assert np.allclose(np.arctan2(np.sin(d), np.cos(d)), 0, atol=1e-12)


def test_kitti_and_waymo_augmentation_lists():
    from mask_bev_amd import augment as A
    from mask_bev.augmentations import kitti_mask_augmentations as KA, waymo_mask_augmentations as WA
    spec = [{'name': 'flip', 'prob_flip_y': 0.5}, {'name': 'rotate', 'rotate_prob': 0.5, 'rotation_range': 20},
            {'name': 'global_noise', 'prob_aug': 0.5, 'trans_std': 0.1, 'scale_delta': 0.02},
            {'name': 'drop', 'prob_drop': 0.5, 'per_point_drop_prob': 0.05}]
    ts = KA.make_kitti_augmentation_list(spec)
    assert [type(t) for t in ts] == [A.KittiFlip, A.RandomRotate, A.GlobalNoise, A.RandomDropPoints]
    assert KA.make_kitti_augmentation_list is A.make_kitti_augmentation_list
    assert type(KA.make_augmentation({'name': 'flip'})) is A.KittiFlip
    ra = A.make_kitti_augmentation_list([{'name': 'rand_augment', 'num_augments': 2, 'magnitude': 0.5,
                                          'transforms': [{'name': 'flip'}, {'name': 'shuffle'}]}])[0]
    assert type(ra) is A.RandAugment and type(ra._transforms[0]) is A.KittiFlip
    for make in (A.make_kitti_augmentation_list, A.make_waymo_augmentation_list):
        with pytest.raises(ValueError, match='Cannot flip in x'):
            make([{'name': 'flip', 'prob_flip_x': 0.5}])
    ws = WA.make_waymo_augmentation_list([s for s in spec if s['name'] != 'global_noise'])
    assert [type(t) for t in ws] == [A.WaymoFlip, A.RandomRotate, A.RandomDropPoints]
    assert type(WA.make_augmentation({'name': 'flip'})) is A.WaymoFlip
    with pytest.raises(NotImplementedError, match='rand augment'):
        A.make_waymo_augmentation_list([{'name': 'rand_augment', 'num_augments': 1, 'magnitude': 1, 'transforms': []}])
    with pytest.raises(NotImplementedError):
        A.make_waymo_augmentation_list([{'name': 'global_noise', 'prob_aug': 1}])
    with pytest.raises(NotImplementedError):
        A.make_semantic_kitti_augmentation_list([{'name': 'global_noise', 'prob_aug': 1}])


@pytest.mark.parametrize('make', ['kitti', 'waymo', 'semantic_kitti'])
def test_unsupported_augmentations_raise(make):
    from mask_bev_amd import augment as A
    make = getattr(A, f'make_{make}_augmentation_list')
    with pytest.raises(NotImplementedError, match='samples.pkl'):
        make([{'name': 'object_sample', 'dataset_root': '~/Datasets/KITTI', 'num_sample': 5}])
    with pytest.raises(NotImplementedError, match='collision search'):
        make([{'name': 'object_noise'}])
    with pytest.raises(NotImplementedError, match='cut_pc'):
        make([{'name': 'cut_pc'}])
    with pytest.raises(NotImplementedError, match='no_such_thing is not implemented'):
        make([{'name': 'no_such_thing'}])


def test_global_noise_record_and_existing_records():
    from mask_bev_amd import augment as A
    assert A.OP_GLOBAL_NOISE == 6 and A.OP_DECIMATE == 5
    d = [A.SampleDraw(5, (A.rotation_op(12.0), A.Op(A.OP_GLOBAL_NOISE, 0, (1.01, 0.1, -0.2, 0.3))))]
    rec = A.pack_records(d)
    assert rec[0]['n_ops'] == 2 and rec[0]['ops'][1]['code'] == 6
    assert rec[0]['ops'][1]['p'].tolist() == [1.01, 0.1, -0.2, 0.3, 0, 0, 0, 0, 0]
    # the heading rule of a linear op is host-side only: the record of a rotation holds the matrix and nothing else
    assert rec[0]['ops'][0]['p'][4:].tolist() == [0, 0, 0, 0, 0] and rec[0]['ops'][0]['arg'] == 0
    assert not d[0].permutes and not d[0].removes and A.batch_mode(d) == 0
    assert np.allclose(d[0].matrix, np.array(A.rotation_op(12.0).p).reshape(2, 2))
    assert A.AugmentedBatch._fields[-1] == 'boxes' and A.AugmentedBatch._field_defaults == {'boxes': None}
