"""K30a (largest 8-connected component of a packed mask) and K30b (minimum-area rectangle of a packed mask) through the C
ABI, against the exact oracle of tests/min_area_rect_ref.py; their composition behind ``Predictions.boxes(method=
'min_area_rect')``; capture into a HIP graph.

K30a: the output words, n and the component count are exact (``torch.equal``).  K30b: n and the hull's vertex count exact, the
box within the project's f32 bar relative to the largest reference value (the device arithmetic is float64 with one rounding
per operation and one rounding to f32 at the store); no case excluded.  theta lies in (-pi/4, pi/4], the upper end read as
the f32 value the store rounds pi/4 to.

Grids: 40 x 36, 64 x 64, 33 x 100 (rows straddle words), 33 x 33 (the spiral), 1 x 40, 40 x 1, 1 x 1, and two larger ones:
160 x 160, the smallest round size at which each of the three Bernoulli masks falls into at least 20 components (at p = 0.6
the listed grids give fewer than ten), and 130 x 1000, the smallest at which K30a's planes leave LDS for the workspace."""
import numpy as np
import pytest
import torch

from tests import f64_bars
from tests import min_area_rect_ref as R
from tests.test_predict_cpu import _pack
from tests.util_cfg import random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
MODULE = 'test_k30_min_area_rect_gpu'
_CACHE = {}


def _cases(h, w):
    """Per grid, computed once and left unchanged: names, the dense masks, the packed words with garbage in the tail bits, and
    the oracle's answers for K30a and for K30b on both the masks and their kept components."""
    if (h, w) not in _CACHE:
        masks = {f'c:{k}': v for k, v in R.component_masks(h, w).items()}
        masks.update({f'r:{k}': v for k, v in R.rectangle_masks(h, w).items()})
        names = list(masks)
        words = _pack(torch.from_numpy(np.stack([masks[n] for n in names])))
        tail = torch.zeros(words.shape[1] * 32, dtype=torch.bool)
        tail[h * w:] = True                                            # bits beyond the map set to garbage: never cells
        words = words | _pack(tail.view(1, 1, -1))
        comp = [R.largest_component(masks[n]) for n in names]
        kept_words = _pack(torch.from_numpy(np.stack([c[0] for c in comp])))
        _CACHE[(h, w)] = dict(names=names, masks=masks, words=words, comp=comp, kept_words=kept_words,
                              box=[R.min_area_box(masks[n]) for n in names], kept_box=[R.min_area_box(c[0]) for c in comp])
    return _CACHE[(h, w)]


def _order(k):
    return list(reversed(range(k))) + [0, k + 5, -1]                   # any order, repeats, rows outside the table


def _check_boxes(capsys, tag, names, order, got, want, bad):
    n, hull, box = (t.cpu() for t in got)
    assert n.dtype == torch.int32 and hull.dtype == torch.int32 and box.dtype == torch.float32
    assert tuple(box.shape) == (len(order), 5)
    total = 0
    for j, i in enumerate(order):
        inside = 0 <= i < len(names)
        rn, rh, rb = want[i] if inside else (0, 0, np.zeros(5))
        name = names[i] if inside else f'row {i}'
        assert (int(n[j]), int(hull[j])) == (rn, rh), (tag, name)
        if rn == 0:
            assert not box[j].any(), (tag, name)
            continue
        assert -np.pi / 4 < float(box[j, 4]) <= float(np.float32(np.pi / 4)), (tag, name)
        e = float(np.abs(box[j].double().numpy() - rb).max() / np.abs(rb).max())
        f64_bars.check(capsys, MODULE, f'{tag} {name}', e, f64_bars.F32_BAR, bad)
        total += 1
    return total


# ------------------------------------------------------------------------------------------------ K30a
@pytest.mark.parametrize('h,w', R.GRIDS)
def test_k30a_largest_component(device, h, w):
    from mask_bev_amd import ops
    c = _cases(h, w)
    names, order = c['names'], _order(len(c['names']))
    pm = ops.PackedMasks(c['words'].to(device), h, w)
    kept, n, comps = ops.largest_component(pm, torch.tensor(order, device=device))
    assert (kept.h, kept.w) == (h, w) and kept.words.dtype == torch.int32 and n.dtype == torch.int32 and comps.dtype == torch.int32
    want_words = torch.zeros((len(order), c['words'].shape[1]), dtype=torch.int32)
    want_n, want_c = torch.zeros(len(order), dtype=torch.int32), torch.zeros(len(order), dtype=torch.int32)
    for j, i in enumerate(order):
        if 0 <= i < len(names):
            want_words[j], want_n[j], want_c[j] = c['kept_words'][i], c['comp'][i][1], c['comp'][i][2]
    miss = [names[i] if 0 <= i < len(names) else i for j, i in enumerate(order)
            if not torch.equal(kept.words[j].cpu(), want_words[j])]
    assert not miss, miss
    assert torch.equal(kept.words.cpu(), want_words) and torch.equal(n.cpu(), want_n) and torch.equal(comps.cpu(), want_c)
    by_name = {k: c['comp'][i] for i, k in enumerate(names)}
    if min(h, w) >= 2 and 'c:checkerboard' in by_name:
        assert by_name['c:checkerboard'][2] == 1
    if 'c:corner' in by_name:
        assert by_name['c:corner'][2] == 1 and by_name['c:equal'][1:] == (20, 2) and by_name['c:strays'][2] == 3
        assert by_name['c:equal'][0][3:8].any() and not by_name['c:equal'][0][20:24].any()      # the lower raster index won
    if 'c:ring' in by_name:
        assert by_name['c:ring'][2] == 2
    if (h, w) == (160, 160):
        assert all(by_name[f'c:bernoulli{p:g}'][2] >= 20 for p in (0.3, 0.45, 0.6))
    if (h, w) == (33, 33):
        assert by_name['c:spiral'][1:] == (int(c['masks']['c:spiral'].sum()), 1) and by_name['c:spiral'][1] > 500
    # no row to do
    kept, n, comps = ops.largest_component(pm, torch.zeros((0,), dtype=torch.int64, device=device))
    assert tuple(kept.words.shape) == (0, c['words'].shape[1]) and n.numel() == 0 and comps.numel() == 0


# ------------------------------------------------------------------------------------------------ K30b
@pytest.mark.parametrize('h,w', R.GRIDS)
def test_k30b_min_area_boxes(device, capsys, h, w):
    from mask_bev_amd import ops
    c = _cases(h, w)
    names, order = c['names'], _order(len(c['names']))
    rows = torch.tensor(order, device=device)
    bad = []
    pm = ops.PackedMasks(c['words'].to(device), h, w)
    got = ops.min_area_boxes(pm, rows)
    total = _check_boxes(capsys, f'K30b {h}x{w}', names, order, got, c['box'], bad)
    # the composition by hand: K30a's output is K30b's input
    kept, n_kept, _ = ops.largest_component(pm, rows)
    got2 = ops.min_area_boxes(kept, torch.arange(len(order), device=device))
    want2 = [c['kept_box'][i] if 0 <= i < len(names) else (0, 0, np.zeros(5)) for i in order]
    total += _check_boxes(capsys, f'K30a+b {h}x{w}', [names[i] if 0 <= i < len(names) else f'row {i}' for i in order],
                          list(range(len(order))), got2, want2, bad)
    assert torch.equal(got2[0], n_kept)
    assert not bad, bad
    box = got[2].cpu()
    if (h, w) == (40, 36):                                             # the exact lists
        assert total >= 2 * 14
        for name, want in (('r:block', [14.0, 8.0, 21.0, 7.0, 0.0]), ('r:line', [7.0, 20.0, 1.0, 35.0, 0.0]),
                           ('r:single', [35.0, 39.0, 1.0, 1.0, 0.0]), ('r:ell', [17.0, 17.0, 25.0, 25.0, 0.0])):
            assert box[order.index(names.index(name))].tolist() == want, name
    if (h, w) == (64, 64):
        assert sum(k.startswith('r:rect') for k in names) == 12
        j = order.index(names.index('r:diamond'))                      # the tie: (2, 1) and (2, -1); ey >= 0 wins
        assert int(got[1][j]) == 4 and float(box[j, 4]) == pytest.approx(np.arctan2(1.0, 2.0), rel=1e-6)   # not its negative
        assert box[j, :2].tolist() == [30.0, 33.0]
    n0 = ops.min_area_boxes(pm, torch.zeros((0,), dtype=torch.int32, device=device))
    assert n0[0].numel() == 0 and tuple(n0[2].shape) == (0, 5)


# ------------------------------------------------------------------------------------------------ composition and interface
def test_predictions_boxes_by_method(device):
    from mask_bev_amd import ops, rasterize
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(0)
    kw = tiny_kwargs()
    m = MaskBevModule(**kw).to(device)
    m.log_scalars = False
    p = m.predict([x.to(device) for x in random_scans(kw, [2500, 1800], seed=5)])
    b, q = p.keep.shape
    p.keep = torch.ones_like(p.keep)
    p.keep[0, 1] = False
    p.masks.words[3].zero_()                                           # one kept mask is empty
    ranges = (kw['x_range'], kw['y_range'], kw['voxel_size'])
    default, moment = p.boxes(*ranges), p.boxes(*ranges, method='moment')
    assert set(default) == set(moment) and all(torch.equal(default[k], moment[k]) for k in default)
    out = p.boxes(*ranges, method='min_area_rect')
    rows = torch.nonzero(p.keep.reshape(-1)).flatten()
    kept, n_kept, comps = ops.largest_component(p.masks, rows)
    n, hull, cells = ops.min_area_boxes(kept, torch.arange(rows.numel(), device=device))
    full = torch.nonzero(n > 0).flatten()
    assert 0 < full.numel() < rows.numel() and torch.equal(n, n_kept)
    assert torch.equal(out['boxes'], rasterize.boxes_from_cells(cells[full], kw['x_range'], kw['y_range'], 80, 80))
    assert torch.equal(out['cells'], n_kept[full]) and torch.equal(out['scan'] * q + out['query'], rows[full])
    assert torch.equal(out['scores'], p.scores.reshape(-1)[rows[full]])
    assert bool((out['boxes'][:, 2] >= out['boxes'][:, 3]).all()) and bool(torch.isfinite(out['boxes']).all())
    assert bool((out['cells'] <= moment['cells']).all()) and torch.equal(out['query'], moment['query'])
    rz = rasterize.KittiRasterizer(kw['x_range'], kw['y_range'], kw['z_range'], kw['voxel_size'])
    per_scan = p.kitti_predictions(rz, method='min_area_rect')
    assert torch.equal(torch.cat([d['boxes'] for d in per_scan]), out['boxes'])
    from mask_bev_amd import kitti_eval as KE
    assert torch.equal(torch.cat([d['boxes'] for d in KE.mask_to_pred(p, rz, method='min_area_rect')]), out['boxes'])
    with pytest.raises(ValueError):
        p.boxes(*ranges, method='nope')


def test_stray_cells_stretch_the_moment_box_only(device, capsys):
    """A hand-made Predictions: query 0 a 30 x 9 rectangle at 7 degrees on 64 x 64, query 1 the same plus two stray cells."""
    from mask_bev_amd import ops
    from mask_bev_amd.predict import Predictions
    clean = R.rect(64, 64, 32, 32, 30, 9, 7.0)
    noisy = clean.copy()
    noisy[2, 60] = noisy[61, 3] = True
    words = _pack(torch.from_numpy(np.stack([clean, noisy]))).to(device)
    ones = torch.ones((1, 2), device=device)
    p = Predictions(ones.int(), ones * 0.9, ones.bool(), ops.PackedMasks(words, 64, 64), None, None, None, (64, 64))
    ranges = ((0.0, 64.0), (0.0, 64.0), 1.0)
    mar, mom = p.boxes(*ranges, method='min_area_rect'), p.boxes(*ranges)
    assert mar['cells'].tolist() == [int(clean.sum())] * 2 and mom['cells'].tolist() == [int(clean.sum()), int(clean.sum()) + 2]
    bad = []
    e = float((mar['boxes'][1, 2:4] - mar['boxes'][0, 2:4]).abs().max() / mar['boxes'][0, 2:4].abs().max())
    f64_bars.check(capsys, MODULE, 'extents with strays vs clean, min_area_rect', e, f64_bars.F32_BAR, bad)
    assert not bad, bad
    with capsys.disabled():
        print(f'\n[{MODULE}] l x w: min_area_rect clean {mar["boxes"][0, 2:4].tolist()} strays {mar["boxes"][1, 2:4].tolist()}; '
              f'moment clean {mom["boxes"][0, 2:4].tolist()} strays {mom["boxes"][1, 2:4].tolist()}', end='')
    assert bool((mom['boxes'][1, 2:4] > mom['boxes'][0, 2:4]).all())


def test_capture_and_replay(device, capsys):
    """K30a + K30b recorded into one graph and replayed on a second input: the second input's oracle result."""
    from mask_bev_amd import ops
    h, w = 33, 100                                                     # rows straddle words
    c = _cases(h, w)
    names = c['names']
    k = len(names)
    first = c['words'].to(device)
    second = c['words'].flip(0).contiguous().to(device)                # map i of the second input is map k - 1 - i of the first
    static = first.clone()
    rows = torch.arange(k, device=device)
    pm = ops.PackedMasks(static, h, w)

    def run():
        kept, n, comps = ops.largest_component(pm, rows)
        return kept.words, n, comps, ops.min_area_boxes(kept, rows)

    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    kept_words, n, comps, boxes = out
    back = list(reversed(range(k)))
    assert torch.equal(kept_words.cpu(), c['kept_words'][back])
    assert n.cpu().tolist() == [c['comp'][i][1] for i in back] and comps.cpu().tolist() == [c['comp'][i][2] for i in back]
    bad = []
    _check_boxes(capsys, 'replay', [names[i] for i in back], list(range(k)), boxes, [c['kept_box'][i] for i in back], bad)
    assert not bad, bad


def test_launcher_kitti_box_method(device, tmp_path):
    """``evaluate.kitti_bev_evaluation`` over a small KITTI object tree with an untrained tiny model: the
    configuration's ``kitti_box_method`` selects the boxes, the default is ``moment``, and the block keeps its four lines."""
    import os
    import shutil
    from mask_bev_amd.evaluate import kitti_bev_evaluation
    from mask_bev_amd.mask_bev_module import MaskBevModule
    sample = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'kitti_object_sample')
    rng = np.random.default_rng(2)
    for k in ('velodyne', 'label_2', 'calib'):
        d = tmp_path / f'data_object_{k}' / 'training' / k
        d.mkdir(parents=True)
        for frame in (0, 1):
            if k == 'velodyne':
                rng.uniform([0, -10, -3, 0], [20, 10, 1, 1], (2000 + frame, 4)).astype(np.float32).tofile(d / f'{frame:06d}.bin')
            else:
                shutil.copy(os.path.join(sample, k, '000000.txt'), d / f'{frame:06d}.txt')
    (tmp_path / 'val.txt').write_text('000000\n000001\n')
    torch.manual_seed(0)
    kw = dict(tiny_kwargs(), x_range=(0, 20), y_range=(-10, 10))
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    config = dict(kw, dataset='kitti', batch_size=2)
    default = kitti_bev_evaluation(model, config, device, tmp_path)
    moment = kitti_bev_evaluation(model, dict(config, kitti_box_method='moment'), device, tmp_path)
    assert str(default) == str(moment) and np.array_equal(default.raw['stats'], moment.raw['stats'])
    by_key = kitti_bev_evaluation(model, dict(config, kitti_box_method='min_area_rect'), device, tmp_path)
    by_arg = kitti_bev_evaluation(model, config, device, tmp_path, box_method='min_area_rect')
    assert str(by_key) == str(by_arg) and np.array_equal(by_key.raw['stats'], by_arg.raw['stats'])
    lines = by_key.splitlines()
    assert len(lines) == 4 and lines[0] == 'Car AP(Average Precision)@0.70:' and lines[2] == 'Car AP(Average Precision)@0.50:'
    assert all(l.startswith('bev  AP:') and len(l.split(',')) == 3 for l in (lines[1], lines[3]))
    with pytest.raises(ValueError):
        kitti_bev_evaluation(model, dict(config, kitti_box_method='nope'), device, tmp_path)
