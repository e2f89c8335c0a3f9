"""The oracle of K30a / K30b (tests/min_area_rect_ref.py) against known answers and a brute-force scan of directions, and the
host side of the feature: the three symbols in the header and the binding table, the wrappers' refusal of CPU tensors, the
``method`` argument of ``Predictions.boxes``.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import min_area_rect_ref as R
from tests.test_predict_cpu import _pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('mbv_largest_component_workspace_bytes', 'mbv_largest_component', 'mbv_min_area_boxes')


# ------------------------------------------------------------------------------------------------ the oracle
def test_known_answers_of_the_rectangle():
    n, hull, box = R.min_area_box(R.block())
    assert (n, hull) == (147, 4) and box.tolist() == [14.0, 8.0, 21.0, 7.0, 0.0]             # the same as K25
    n, hull, box = R.min_area_box(R.line())
    assert (n, hull) == (35, 2) and box.tolist() == [7.0, 20.0, 1.0, 35.0, 0.0]
    n, hull, box = R.min_area_box(R.single())
    assert (n, hull) == (1, 1) and box.tolist() == [35.0, 39.0, 1.0, 1.0, 0.0]
    n, hull, box = R.min_area_box(R.ell())
    assert (n, hull) == (225, 5) and box.tolist() == [17.0, 17.0, 25.0, 25.0, 0.0]
    n, hull, box = R.min_area_box(np.zeros((40, 36), dtype=bool))
    assert (n, hull) == (0, 0) and not box.any()


def test_canonical_direction_and_the_tie_rule():
    assert R.canonical(0, 1) == (1, 0) and R.canonical(-1, 0) == (1, 0) and R.canonical(0, -5) == (5, 0)
    assert R.canonical(1, 1) == (1, 1) and R.canonical(-1, 1) == (1, 1) and R.canonical(1, -1) == (1, 1)
    assert R.canonical(-2, 1) == (2, -1) and R.canonical(2, -1) == (2, -1) and R.canonical(1, -2) == (2, 1)
    for ex in range(-4, 5):
        for ey in range(-4, 5):
            if (ex, ey) != (0, 0):
                cx, cy = R.canonical(ex, ey)
                assert cx > 0 and -cx < cy <= cx and cx * cx + cy * cy == ex * ex + ey * ey
    # the symmetric diamond: (2, 1) and (2, -1) tie in area and in |ey| / ex; ey >= 0 wins
    n, hull, box = R.min_area_box(R.diamond())
    assert hull == 4 and box[4] == pytest.approx(np.arctan2(1.0, 2.0), abs=1e-15) and box[0] == pytest.approx(30.0, abs=1e-12)
    assert box[1] == pytest.approx(33.0, abs=1e-12)
    # collinear cells on a diagonal: the direction of the segment
    m = np.eye(12, dtype=bool)
    n, hull, box = R.min_area_box(m)
    assert (n, hull) == (12, 2) and box[4] == pytest.approx(np.pi / 4) and box[3] == pytest.approx(np.sqrt(2.0))
    assert box[2] == pytest.approx(11 * np.sqrt(2.0) + np.sqrt(2.0))
    n, hull, box = R.min_area_box(m[::-1])                                                    # the other diagonal: the same canonical direction
    assert hull == 2 and box[4] == pytest.approx(np.pi / 4) and box[2] == pytest.approx(np.sqrt(2.0))


def test_rectangle_holds_every_cell_and_beats_a_scan_of_directions():
    """For the rotated rectangles of the GPU test: every cell centre lies inside the oracle's rectangle, and its
    through-centres area is no larger than that of any direction of a 0.25 degree scan."""
    for name, mask in R.rotated_rectangles().items():
        n, hull, box = R.min_area_box(mask)
        assert n > 200 and hull >= 4 and -np.pi / 4 < box[4] <= np.pi / 4, name
        ys, xs = np.nonzero(mask)
        c, s = np.cos(box[4]), np.sin(box[4])
        cell = abs(c) + abs(s)
        u = (xs - box[0]) * c + (ys - box[1]) * s
        v = (ys - box[1]) * c - (xs - box[0]) * s
        assert np.abs(u).max() <= (box[2] - cell) / 2 + 1e-9 and np.abs(v).max() <= (box[3] - cell) / 2 + 1e-9, name
        area = float(R.through_centres_area(mask))
        assert area == pytest.approx((box[2] - cell) * (box[3] - cell), rel=1e-12), name
        scan = np.deg2rad(np.arange(0.0, 90.0, 0.25))
        pu = xs[None] * np.cos(scan)[:, None] + ys[None] * np.sin(scan)[:, None]
        pv = ys[None] * np.cos(scan)[:, None] - xs[None] * np.sin(scan)[:, None]
        brute = ((pu.max(1) - pu.min(1)) * (pv.max(1) - pv.min(1))).min()
        assert area <= brute * (1 + 1e-12), (name, area, brute)


def test_known_answers_of_the_components():
    # the issue's example: a 30 x 9 rectangle at 7 degrees on 64 x 64 plus two stray cells
    clean = R.rect(64, 64, 32, 32, 30, 9, 7.0)
    noisy = clean.copy()
    noisy[2, 60] = noisy[61, 3] = True
    kept, n, comps = R.largest_component(noisy)
    assert comps == 3 and n == int(clean.sum()) and np.array_equal(kept, clean)
    assert np.allclose(R.min_area_box(kept)[2], R.min_area_box(clean)[2])
    # corners connect; equal sizes: the lower raster index wins
    m = np.zeros((8, 8), dtype=bool)
    m[1:3, 1:3] = m[3:5, 3:5] = True
    assert R.largest_component(m)[1:] == (8, 1)
    m = np.zeros((8, 9), dtype=bool)
    m[5:7, 0:2] = m[1:3, 6:8] = True
    kept, n, comps = R.largest_component(m)
    assert (n, comps) == (4, 2) and kept[1:3, 6:8].all() and not kept[5:7].any()
    checker = (np.add.outer(np.arange(7), np.arange(9)) % 2).astype(bool)
    assert R.largest_component(checker)[1:] == (int(checker.sum()), 1)
    assert R.largest_component(np.zeros((3, 3), dtype=bool))[1:] == (0, 0)


# ------------------------------------------------------------------------------------------------ the host side
def test_symbols_in_the_header_and_the_binding_table():
    from mask_bev_amd import _lib, ops
    with open(os.path.join(ROOT, 'include', 'maskbev_hip.h')) as fh:
        header = fh.read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r'\b(int|int64_t)\s+' + name + r'\s*\(', header), name
    assert len(_lib.SIGNATURES['mbv_largest_component'][1]) == 12 and len(_lib.SIGNATURES['mbv_min_area_boxes'][1]) == 10
    assert callable(ops.largest_component) and callable(ops.min_area_boxes)
    from mask_bev_amd import build
    assert {'mask_components.hip', 'min_area_rect.hip'} <= set(build.sources())


def test_wrappers_refuse_cpu_tensors():
    from mask_bev_amd import ops
    from mask_bev_amd._lib import MaskBevHipError
    pm = ops.PackedMasks(torch.zeros((2, ((8 * 8 + 63) // 64) * 2), dtype=torch.int32), 8, 8)
    with pytest.raises(MaskBevHipError):
        ops.largest_component(pm, torch.tensor([0, 1]))
    with pytest.raises(MaskBevHipError):
        ops.min_area_boxes(pm, torch.tensor([0, 1]))


def _cpu_predictions():
    from mask_bev_amd import ops
    from mask_bev_amd.predict import Predictions
    b, q, h, w = 1, 2, 8, 8
    dense = torch.zeros(b * q, h, w, dtype=torch.bool)
    dense[0, 2:5, 1:7] = True
    return Predictions(torch.ones(b, q, dtype=torch.int32), torch.full((b, q), 0.9), torch.ones(b, q, dtype=torch.bool),
                       ops.PackedMasks(_pack(dense), h, w), None, None, None, (h, w))


def test_unknown_box_method_is_a_value_error():
    from mask_bev_amd import kitti_eval as KE
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.predict import BOX_METHODS
    assert BOX_METHODS == ('moment', 'min_area_rect')
    p = _cpu_predictions()
    for call in (lambda: p.boxes((0, 8), (0, 8), 1.0, method='nope'),
                 lambda: p.kitti_predictions((0, 8), (0, 8), 1.0, method='nope'),
                 lambda: KE.mask_to_pred(p, (0, 8), (0, 8), 1.0, method='nope')):
        with pytest.raises(ValueError):
            call()
    for method in BOX_METHODS:                                         # known methods get as far as the kernels: no CPU fallback
        with pytest.raises(MaskBevHipError):
            p.boxes((0, 8), (0, 8), 1.0, method=method)


def test_launcher_refuses_an_unknown_kitti_box_method(tmp_path):
    from mask_bev_amd.evaluate import kitti_bev_evaluation
    with pytest.raises(ValueError):
        kitti_bev_evaluation(None, dict(kitti_box_method='nope'), 'cpu', tmp_path)
    with pytest.raises(ValueError):
        kitti_bev_evaluation(None, {}, 'cpu', tmp_path, box_method='nope')
