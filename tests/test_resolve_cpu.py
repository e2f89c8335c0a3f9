"""K42 without a GPU: hand-worked answers of the plain-loop restatement (tests/resolve_ref.py) on a 1 x 12 strip, the settings
record, the binding table and the new fields of ``Predictions``."""
import os

import pytest
import torch

from tests import resolve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nms(spans, scores, labels=None, iou=(1, 2), same_label=True, keep=None):
    masks = R.strip(*spans)
    keep = [True] * len(spans) if keep is None else keep
    labels = [1] * len(spans) if labels is None else labels
    return R.nms(R.self_overlap(masks, keep), scores, labels, keep, iou, same_label)


def test_chain_is_not_transitive():
    """A = [0, 8), B = [2, 10), C = [4, 12): A~B and B~C share 6 of 10 cells, A~C 4 of 12.  At 1/2 A suppresses B, and B, being
    suppressed, suppresses nobody: C survives."""
    inter = R.self_overlap(R.strip((0, 8), (2, 10), (4, 12)), [True] * 3)
    assert inter == [[8, 6, 4], [6, 8, 6], [4, 6, 8]]
    keep1, by = _nms([(0, 8), (2, 10), (4, 12)], [0.9, 0.8, 0.7])
    assert keep1 == [True, False, True] and by == [-1, 0, -1]
    # the order is the scores', not the indices': with C strongest, C suppresses B and A survives
    keep1, by = _nms([(0, 8), (2, 10), (4, 12)], [0.7, 0.8, 0.9])
    assert keep1 == [True, False, True] and by == [-1, 2, -1]


def test_equality_suppresses():
    """[0, 8) against [0, 4): 4 of 8 cells, exactly 1/2."""
    assert _nms([(0, 8), (0, 4)], [0.9, 0.8], iou=(1, 2)) == ([True, False], [-1, 0])
    assert _nms([(0, 8), (0, 4)], [0.9, 0.8], iou=(51, 100)) == ([True, True], [-1, -1])
    assert _nms([(0, 8), (0, 8)], [0.9, 0.8], iou=(1, 1)) == ([True, False], [-1, 0])         # num == den: only identical masks


def test_ties_labels_and_non_kept():
    assert _nms([(0, 8), (0, 8)], [0.5, 0.5]) == ([True, False], [-1, 0])                      # equal scores: the smaller q wins
    assert _nms([(0, 8), (0, 8)], [0.9, 0.8], labels=[1, 2]) == ([True, True], [-1, -1])       # different labels: both stay
    assert _nms([(0, 8), (0, 8)], [0.9, 0.8], labels=[1, 2], same_label=False) == ([True, False], [-1, 0])
    # a query that is not kept neither suppresses nor is suppressed, and its row of the table is zero
    keep = [False, True, True]
    inter = R.self_overlap(R.strip((0, 8), (0, 8), (0, 8)), keep)
    assert inter == [[0, 0, 0], [0, 8, 8], [0, 8, 8]]
    assert _nms([(0, 8), (0, 8), (0, 8)], [0.9, 0.8, 0.7], keep=keep) == ([False, True, False], [-1, -1, 1])


def test_empty_mask_survives_nms_and_falls_to_min_cells():
    masks = R.strip((0, 8), None)
    out = R.resolve(masks, [0.9, 0.8], [1, 1], [True, True], [[0] * 8 + [-1] * 4])
    assert out['keep1'] == [True, True] and out['suppressed_by'] == [-1, -1]                    # union with itself is 0: not suppressed
    assert out['owned'] == [8, 0] and out['keep'] == [True, False]
    out = R.resolve(masks, [0.9, 0.8], [1, 1], [True, True], [[0] * 8 + [-1] * 4], min_cells=0)
    assert out['keep'] == [True, True]                                                          # 0 * 5 >= 4 * 0


def test_overlap_filter_at_four_fifths():
    """owned 4 of area 5 stays (4 * 5 >= 4 * 5); owned 3 of area 4 goes (15 < 16) and its cells become -1, not the neighbour's."""
    imap = [[0, 0, 0, 0, 1, 1, 1, 2, 2, -1, 7, -5]]
    keep2, owned, new = R.overlap_filter(imap, [5, 4, 2], [True, True, False], (4, 5), 1)
    assert owned == [4, 3, 0] and keep2 == [True, False, False]
    assert new == [[0, 0, 0, 0, -1, -1, -1, -1, -1, -1, 7, -5]]        # a query outside keep is cleared too; other values stay
    keep2, owned, new = R.overlap_filter(imap, [5, 4, 2], [True, True, False], None, 1)
    assert keep2 == [True, True, False] and new[0][4:7] == [1, 1, 1]
    assert R.overlap_filter(imap, [5, 4, 2], [True, True, False], None, 4)[0] == [True, False, False]
    # the composition hands the rebuilt map through: a function of keep1, or the map
    out = R.resolve(R.strip((0, 5), (4, 8), (7, 9)), [0.9, 0.8, 0.7], [1, 1, 1], [True, True, False], lambda k1: imap)
    assert out['keep'] == [True, False, False] and out['instance_map'] == [[0, 0, 0, 0, -1, -1, -1, -1, -1, -1, 7, -5]]


def test_resolve_settings_validation():
    from mask_bev_amd.predict import ResolveSettings
    s = ResolveSettings()
    assert (s.nms_iou, s.min_overlap, s.min_cells, s.same_label, s.exclusive) == ((1, 2), (4, 5), 1, True, False)
    assert ResolveSettings(nms_iou=None, min_overlap=None, min_cells=0).nms_iou is None
    assert ResolveSettings(nms_iou=[65535, 65535]).nms_iou == (65535, 65535)
    for bad in (dict(nms_iou=(0, 2)), dict(nms_iou=(3, 2)), dict(nms_iou=(1, 65536)), dict(nms_iou=0.5), dict(nms_iou=(0.5, 1)),
                dict(min_overlap=(0, 1)), dict(min_overlap=(2, 1)), dict(min_overlap=(1, 2, 3)), dict(min_cells=-1),
                dict(min_cells=1.5), dict(min_cells=None)):
        with pytest.raises(ValueError):
            ResolveSettings(**bad)


def test_launcher_keys():
    from mask_bev_amd.evaluate import format_resolve_settings, resolve_settings
    from mask_bev_amd.predict import ResolveSettings
    assert resolve_settings(dict()) is None and resolve_settings(dict(predict_resolve=False, predict_min_cells=3)) is None
    assert resolve_settings(dict(predict_resolve=True)) == ResolveSettings()
    got = resolve_settings(dict(predict_resolve=True, predict_nms_iou=[2, 3], predict_min_overlap=None, predict_min_cells=4,
                                predict_exclusive_masks=True))
    assert got == ResolveSettings(nms_iou=(2, 3), min_overlap=None, min_cells=4, exclusive=True)
    with pytest.raises(ValueError):
        resolve_settings(dict(predict_resolve=True, predict_nms_iou=[3, 2]))
    assert format_resolve_settings(ResolveSettings()) == 'resolved predictions: nms_iou 1/2, min_overlap 4/5, min_cells 1'
    assert format_resolve_settings(got) == 'resolved predictions: nms_iou 2/3, min_overlap off, min_cells 4, exclusive masks'


def test_binding_table_header_and_sources():
    from mask_bev_amd import _lib, build, ops
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    for name, n_args in (('mbv_mask_self_overlap', 7), ('mbv_mask_nms', 12), ('mbv_overlap_filter', 13)):
        assert name in _lib.SIGNATURES and name + '(' in header
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert 'resolve.hip' in build.sources() and 'resolve.hip' not in build.FILE_FLAGS       # integers only: the common flags
    assert _lib.ABI_VERSION == 59
    for name in ('mask_self_overlap', 'mask_nms', 'overlap_filter'):
        assert hasattr(ops, name)
    with pytest.raises(ops.MaskBevHipError):                               # no CPU fallback
        ops.mask_nms(torch.zeros((1, 2, 2), dtype=torch.int32), torch.zeros((1, 2)), torch.zeros((1, 2), dtype=torch.int32),
                     torch.zeros((1, 2), dtype=torch.bool))


def test_predictions_fields_and_arguments():
    import inspect
    from mask_bev_amd import predict as P
    from mask_bev_amd.mask_bev_module import MaskBevModule
    z = torch.zeros((1, 2), dtype=torch.int32)
    old = P.Predictions(z, z.float(), z.bool(), None, None, None, None, (4, 4))           # the eight positional fields of before
    assert old.suppressed_by is None and old.owned is None and old.clone().owned is None
    new = P.Predictions(z, z.float(), z.bool(), None, None, None, None, (4, 4), z + 3, z + 5)
    c = new.clone()
    assert torch.equal(c.suppressed_by, z + 3) and torch.equal(c.owned, z + 5) and c.owned is not new.owned
    assert torch.equal(new.cpu().owned, z + 5)
    for fn in (P.extract_instances, P.predict, MaskBevModule.predict, P.GraphedPredictStep.__init__):
        assert inspect.signature(fn).parameters['resolve'].default is None
    assert 'mask_scores' in P.Predictions.__doc__ and 'UNRESOLVED' in P.Predictions.__doc__
    with pytest.raises(ValueError):                                        # resolve needs the masks and the map
        P._resolve_settings(P.ResolveSettings(), True, False)
    with pytest.raises(TypeError):
        P._resolve_settings(dict(), True, True)
