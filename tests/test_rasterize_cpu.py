"""K22 on the host side: the numpy / scipy restatement (tests/rasterize_ref.py) against the reference's recorded maps
(tests/golden/rasterizer.npz, made by the reference's own class — see make_golden_rasterizer.py), known answers of the
border rule, ``scans_in_range`` and the argument errors of ``SemanticKittiRasterizer``."""
import os

import numpy as np
import pytest
import torch

from tests import rasterize_ref as RR

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'rasterizer.npz')


def load_case(z, name):
    offs = z[f'{name}_offsets']
    pts, inst = z[f'{name}_points'], z[f'{name}_inst']
    points = [pts[offs[s]:offs[s + 1]] for s in range(len(offs) - 1)]
    labels = [inst[offs[s]:offs[s + 1]] for s in range(len(offs) - 1)]
    ranges = [tuple(float(v) for v in r) for r in z[f'{name}_ranges']]
    return points, labels, ranges, float(z[f'{name}_vs'])


def restate(z, name, remove_unseen=False, min_points=1, return_masks=False):
    points, labels, ranges, vs = load_case(z, name)
    poses, c = z['poses'], int(z['centre'])
    scene = RR.aggregate_scene(points, poses)
    return RR.get_mask_around(scene, np.concatenate(labels), np.linalg.inv(poses[c]), *ranges, vs, centre_inst=labels[c],
                              remove_unseen=remove_unseen, min_points=min_points, return_masks=return_masks)


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'c_z', 'e'])
def test_restatement_equals_the_reference_map(name):
    z = np.load(GOLDEN)
    assert np.array_equal(restate(z, name), z[f'{name}_map'])
    if name == 'a':
        assert np.array_equal(restate(z, 'a', True, int(z['a_min_points'])), z['a_map_unseen'])
        assert not np.array_equal(z['a_map_unseen'], z['a_map'])


def test_fixture_shapes_and_content():
    z = np.load(GOLDEN)
    assert z['a_map'].shape == (500, 500) and z['b_map'].shape == (100, 120)
    assert len(np.unique(z['a_map'])) - 1 >= 30 and not z['e_map'].any()
    m = z['c_map']                                   # cut on every side, and a corner cell is painted
    assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and m[0, 0] != 0


def test_touching_pairs_differ_only_where_two_instances_claim_a_cell():
    z = np.load(GOLDEN)
    mine, masks = restate(z, 'd', return_masks=True)
    ref = z['d_map']
    claims = sum(v.astype(np.int64) for v in masks.values())
    multi, fg = claims > 1, claims > 0
    assert 0 < multi.sum() <= 0.10 * fg.sum()
    assert np.array_equal(mine[~multi], ref[~multi])
    for x, y in zip(*np.nonzero(multi)):
        assert masks[int(ref[x, y])][x, y]
        assert mine[x, y] == max(i for i, v in masks.items() if v[x, y])          # the highest id wins


def _block(shape, x0, y0, s):
    occ = np.zeros(shape, dtype=np.uint8)
    occ[x0:x0 + s, y0:y0 + s] = 1
    return occ


def test_border_rule_known_answers():
    corner, inside, big = _block((40, 50), 0, 0, 5), _block((40, 50), 17, 20, 5), _block((40, 50), 12, 20, 9)
    assert np.array_equal(RR.close_open(corner, 9), corner)             # outside the grid counts as set for an erosion
    assert not RR.close_open(inside, 9).any()
    assert np.array_equal(RR.close_open(big, 9), big)
    near = _block((40, 60), 10, 5, 9) | _block((40, 60), 10, 18, 9)     # 4 empty cells between the blocks
    far = _block((40, 60), 10, 5, 9) | _block((40, 60), 10, 23, 9)      # 9
    joined = RR.close_open(near, 9)
    assert joined[10:19, 5:27].all() and joined.sum() == 9 * 22
    assert np.array_equal(RR.close_open(far, 9), far)


def test_scans_in_range_known_answers():
    from mask_bev_amd.rasterize import scans_in_range
    poses = np.tile(np.eye(4), (21, 1, 1))
    poses[:, 0, 3] = np.arange(21) * 10.0                 # a straight line along x, 10 m apart
    got = scans_in_range(poses, 10, (-40, 40), (-40, 40))
    assert got.tolist() == list(range(3, 18))             # |dx| < 80 strictly: 80 m away is out
    assert scans_in_range(poses, 10, (-40, 40), (-40, 40), scaling=1).tolist() == [7, 8, 9, 10, 11, 12, 13]
    assert scans_in_range(poses, 0, (-40, 40), (-40, 40)).tolist() == list(range(0, 8))
    turned = poses.copy()
    turned[10, :3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]                 # the centre scan looks along +y
    assert scans_in_range(turned, 10, (-20, 20), (-40, 40)).tolist() == list(range(3, 18))
    assert scans_in_range(turned, 10, (-40, 40), (-20, 20)).tolist() == list(range(7, 14))
    v2c = np.array([[0., -1, 0, 0.1], [0, 0, -1, 0.2], [1, 0, 0, 0.3], [0, 0, 0, 1]])
    cam = v2c @ poses @ np.linalg.inv(v2c)
    assert scans_in_range(cam, 10, (-40, 40), (-40, 40), velo_to_cam=v2c).tolist() == list(range(3, 18))


def test_rasterizer_argument_errors():
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.rasterize import SemanticKittiRasterizer
    for k in (0, 8, 33, -3):
        with pytest.raises(ValueError):
            SemanticKittiRasterizer((-40, 40), (-40, 40), (-10, 10), 0.16, morph_kernel_size=k)
    r = SemanticKittiRasterizer((-40, 40), (-40, 40), (-10, 10), 0.16)
    assert (r.nx, r.ny, r.morph_kernel_size, r.remove_unseen, r.min_points) == (500, 500, 9, False, 1)
    pts, inst = torch.zeros((5, 4)), torch.zeros((5,), dtype=torch.int32)
    with pytest.raises(MaskBevHipError):
        r.rasterize([pts], [inst], np.eye(4)[None])
    with pytest.raises(MaskBevHipError):
        r.rasterize(pts, inst, np.eye(4)[None])
    with pytest.raises(MaskBevHipError):
        r.rasterize_batch([([pts], [inst], np.eye(4)[None])])
    ru = SemanticKittiRasterizer((-40, 40), (-40, 40), (-10, 10), 0.16, remove_unseen=True, min_points=3)
    with pytest.raises(ValueError):
        ru.rasterize([pts], [inst], np.eye(4)[None])
