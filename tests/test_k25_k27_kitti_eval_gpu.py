"""K25 (oriented box of a packed mask), K26 (rotated-box overlap over ragged frames), K27 (KITTI tp / fp / fn) and the
evaluator on them, through the C ABI, against the numpy oracle of tests/kitti_eval_ref.py and the values recorded from
the reference's own protocol functions (tests/golden/kitti_eval.npz).

K25: n and the five moments exact, the box within the project's f32 bar (the device arithmetic is float64 with one
rounding).  K26: exactly 0 where the oracle is exactly 0, otherwise within max(4e-6, 4 x the float32 oracle's own error)
relative to the largest reference value; no pair excluded.  K27: the sums exact, thresholds and APs to 1e-6."""
import os

import numpy as np
import pytest
import torch

from tests import f64_bars
from tests import kitti_eval_ref as R
from tests.test_kitti_eval_cpu import MIN_OVERLAPS, golden, golden_frames
from tests.test_predict_cpu import _pack
from tests.util_cfg import random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
MODULE = 'test_k25_k27_kitti_eval_gpu'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, 'tests', 'golden', 'kitti_object_sample')


# ------------------------------------------------------------------------------------------------ K25
def _rect(h, w, cx, cy, length, width, deg):
    """Cells whose centre lies in the rectangle (numpy paint)."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.deg2rad(deg)
    u = (xs - cx) * np.cos(a) + (ys - cy) * np.sin(a)
    v = (ys - cy) * np.cos(a) - (xs - cx) * np.sin(a)
    return (np.abs(u) <= length / 2) & (np.abs(v) <= width / 2)


def _k25_masks(h, w):
    m = {}
    m['empty'] = np.zeros((h, w), dtype=bool)
    m['single'] = np.zeros((h, w), dtype=bool)
    m['single'][h - 1, w - 1] = True                                   # the last pixel of the map
    m['line'] = np.zeros((h, w), dtype=bool)
    m['line'][3:h - 2, 7] = True                                       # one cell wide
    m['block'] = np.zeros((h, w), dtype=bool)
    m['block'][5:12, 4:25] = True
    m['square'] = np.zeros((h, w), dtype=bool)
    m['square'][6:16, 9:19] = True                                     # isotropic
    m['full'] = np.ones((h, w), dtype=bool)
    m['blobs'] = _rect(h, w, 8, 8, 9, 4, 20) | _rect(h, w, w - 9, h - 8, 7, 5, -50)
    return m


def _k25_cases():
    cases = []
    for h, w in ((40, 36), (64, 64)):
        masks = _k25_masks(h, w)
        for k, deg in enumerate(np.arange(12) * 15 + 7.0 if (h, w) == (64, 64) else ()):
            masks[f'rect{deg:g}'] = _rect(h, w, w / 2 + 0.3 * k, h / 2 - 0.2 * k, 30 + k, 8 + (k % 5), deg)    # aspect >= 2.5
        cases.append((h, w, masks))
    cases.append((33, 100, {'rect': _rect(33, 100, 50.2, 16.4, 60, 9, 12), 'full': np.ones((33, 100), dtype=bool)}))
    return cases


def test_k25_fit_boxes(device, capsys):
    from mask_bev_amd import ops
    bad, total = [], 0
    for h, w, masks in _k25_cases():
        names = list(masks)
        dense = torch.from_numpy(np.stack([masks[n] for n in names]))
        words = _pack(dense)
        npix, nwords = h * w, words.shape[1]
        tail = torch.zeros(nwords * 32, dtype=torch.bool)
        tail[npix:] = True                                             # bits beyond the map set to garbage: never cells
        words = words | _pack(tail.view(1, 1, -1))
        pm = ops.PackedMasks(words.to(device), h, w)
        order = list(reversed(range(len(names)))) + [0, len(names) + 5, -1]        # any order, repeats, rows outside the table
        n, mom, box = ops.fit_boxes(pm, torch.tensor(order, device=device))
        assert n.dtype == torch.int32 and mom.dtype == torch.int64 and box.dtype == torch.float32
        assert tuple(mom.shape) == (len(order), 5) and tuple(box.shape) == (len(order), 5)
        refs = {i: R.fit_box(masks[names[i]]) for i in range(len(names))}
        for j, i in enumerate(order):
            rn, rm, rb = refs[i] if 0 <= i < len(names) else (0, [0] * 5, np.zeros(5))
            assert int(n[j]) == rn, (h, w, i)
            assert torch.equal(mom[j].cpu(), torch.tensor(rm, dtype=torch.int64)), (h, w, i)
            if rn == 0:
                assert not box[j].any()
                continue
            e = float(np.abs(box[j].double().cpu().numpy() - rb).max() / np.abs(rb).max())
            f64_bars.check(capsys, MODULE, f'K25 {h}x{w} {names[i]}', e, f64_bars.F32_BAR, bad)
            total += 1
        for name in ('square', 'full'):
            if name in names and (name == 'square' or h == w):         # isotropic: theta is exactly 0
                j = order.index(names.index(name))
                assert float(box[j, 4]) == 0.0 and float(box[j, 2]) == float(box[j, 3])
        if 'block' in names:
            j = order.index(names.index('block'))
            assert box[j].tolist() == [14.0, 8.0, 21.0, 7.0, 0.0]
    assert not bad, bad
    assert total >= 24
    # no row to fit
    n, mom, box = ops.fit_boxes(pm, torch.zeros((0,), dtype=torch.int64, device=device))
    assert n.numel() == 0 and tuple(box.shape) == (0, 5)


# ------------------------------------------------------------------------------------------------ K26
def _k26_tables():
    rng = np.random.default_rng(26)
    sizes = [(0, 5), (3, 0), (1, 1), (7, 13), (65, 70), (6, 6)]

    def rand(n):
        return np.stack([rng.uniform(-80, 80, n), rng.uniform(-80, 80, n), rng.uniform(0.5, 6, n), rng.uniform(0.5, 6, n),
                         rng.uniform(-np.pi, np.pi, n)], axis=1).reshape(n, 5)

    a, b = [rand(n) for n, _ in sizes], [rand(k) for _, k in sizes]
    # dense enough to overlap: the query boxes of the two large frames sit near boxes of the first table
    for f in (3, 4):
        n, k = sizes[f]
        for j in range(k):
            b[f][j, :2] = a[f][j % n, :2] + rng.uniform(-2, 2, 2)
    # the closed forms, planted in the last frame (6 x 6): pair (i, i)
    box = np.array([12.5, -33.25, 4.5, 1.75, 0.4])
    a[5][0], b[5][0] = [3, 4, 4, 2, 0], [4, 4.5, 2, 3, 0]                         # axis-aligned: they share a 2 x 2 square
    a[5][1], b[5][1] = box, box                                                    # identical
    a[5][2], b[5][2] = box, box + [30, 0, 0, 0, 0.7]                               # disjoint
    a[5][3], b[5][3] = [12.6, -33.2, 1.0, 0.5, 0.4], box                           # inside
    a[5][4], b[5][4] = box, box + [0, 0, 0, 0, np.pi / 2]                          # a cross
    a[5][5], b[5][5] = [0, 0, 4, 1, np.deg2rad(30)], [1.5, 1.0, 0.4, 0.4, 0]       # the sign of the angle
    a32 = [x.astype(np.float32) for x in a]
    b32 = [x.astype(np.float32) for x in b]
    return sizes, a32, b32


@pytest.fixture(scope='module')
def k26_refs():
    sizes, a, b = _k26_tables()
    inter64 = [R.rotate_iou(x, y, 2, np.float64) for x, y in zip(a, b)]
    inter32 = [R.rotate_iou(x, y, 2, np.float32) for x, y in zip(a, b)]
    return sizes, a, b, inter64, inter32


def test_k26_rotate_iou(device, capsys, k26_refs):
    from mask_bev_amd import ops
    sizes, a, b, inter64, inter32 = k26_refs
    ta, tb = torch.from_numpy(np.concatenate(a)).to(device), torch.from_numpy(np.concatenate(b)).to(device)
    off_a = np.concatenate([[0], np.cumsum([n for n, _ in sizes])])
    off_b = np.concatenate([[0], np.cumsum([k for _, k in sizes])])
    bad, offsets = [], None
    for criterion in (-1, 0, 1, 2):
        got, offsets = ops.rotate_iou(ta, tb, off_a, off_b, criterion=criterion, offsets=offsets)
        assert got.dtype == torch.float32 and got.numel() == sum(n * k for n, k in sizes) == offsets.total
        assert offsets.pairs.tolist() == np.concatenate([[0], np.cumsum([n * k for n, k in sizes])]).tolist()
        ref64 = np.concatenate([R.overlap_from_intersection(i, x, y, criterion).reshape(-1) for i, x, y in zip(inter64, a, b)])
        ref32 = np.concatenate([R.overlap_from_intersection(i, x, y, criterion).reshape(-1) for i, x, y in zip(inter32, a, b)])
        g = got.cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(g))
        zero = ref64 == 0
        assert (~zero).sum() >= 60 and zero.sum() >= 1000 and np.all(g[zero] == 0), (criterion, np.flatnonzero(zero & (g != 0))[:5])
        bar = f64_bars.f32_bar(torch.from_numpy(ref32.astype(np.float64)), torch.from_numpy(ref64))
        f64_bars.check(capsys, MODULE, f'K26 criterion {criterion}', f64_bars.err(torch.from_numpy(g), torch.from_numpy(ref64)),
                       bar, bad)
        # the planted closed forms, pair (i, i) of the last frame
        last = g[offsets.pairs[5]:].reshape(6, 6)
        if criterion == 2:
            assert last[0, 0] == pytest.approx(4.0, abs=2e-5) and last[2, 2] == 0 and last[5, 5] > 0.1
            assert last[3, 3] == pytest.approx(0.5, abs=1e-5) and last[4, 4] == pytest.approx(1.75 ** 2, abs=2e-5)
        if criterion == -1:
            assert last[0, 0] == pytest.approx(4.0 / (8 + 6 - 4), abs=4e-6) and last[1, 1] == pytest.approx(1.0, abs=4e-6)
        if criterion == 0:
            assert last[4, 4] == pytest.approx(1.75 / 4.5, abs=4e-6) and last[3, 3] == pytest.approx(1.0, abs=4e-6)
    assert not bad, bad
    # one frame without offsets; an empty table
    got, o = ops.rotate_iou(ta[:4], tb[:9])
    assert np.array_equal(got.cpu().numpy().reshape(4, 9), ops.rotate_iou(ta[:4], tb[:9], [0, 4], [0, 9])[0].cpu().numpy().reshape(4, 9))
    got, o = ops.rotate_iou(ta[:0], tb[:9])
    assert got.numel() == 0 and o.total == 0
    with pytest.raises(ValueError):
        ops.rotate_iou(ta, tb, [0, 3], off_b)


# ------------------------------------------------------------------------------------------------ K27 and the evaluator
@pytest.fixture(scope='module')
def oracle_eval():
    g = golden()
    frames = golden_frames(g)
    overlaps = [R.rotate_iou(dt['boxes'], gt['bev']) for gt, dt in frames]
    return g, frames, overlaps, R.eval_class(frames, overlaps, 0, (0, 1, 2), MIN_OVERLAPS)


def _product_inputs(frames, device):
    labels = [gt for gt, _ in frames]
    preds = [dict(boxes=torch.from_numpy(dt['boxes']).float().to(device), score=torch.from_numpy(dt['score']).float().to(device),
                  type=torch.from_numpy(dt['type'])) for _, dt in frames]
    return labels, preds


def test_k27_statistics_equal_the_oracle(device, oracle_eval):
    from mask_bev_amd import ops
    g, frames, overlaps, res = oracle_eval
    allov = np.concatenate([ov.reshape(-1) for ov in overlaps])
    assert np.abs(allov - 0.5).min() > 1e-3 and np.abs(allov - 0.7).min() > 1e-3          # the precondition
    dt = torch.from_numpy(g['dt_boxes']).float().to(device)
    gt = torch.from_numpy(g['gt_boxes']).float().to(device)
    ov, offs = ops.rotate_iou(dt, gt, g['dt_offsets'], g['gt_offsets'])
    assert np.abs(ov.cpu().numpy() - allov).max() < 1e-5
    scores = torch.from_numpy(g['dt_scores']).float().to(device)
    for d in range(3):
        ig = torch.from_numpy(g[f'ignored_gt_{d}'].astype(np.int32)).to(device)
        idt = torch.from_numpy(g[f'ignored_dt_{d}'].astype(np.int32)).to(device)
        for k, mo in enumerate(MIN_OVERLAPS):
            stats, tps, flags = ops.kitti_statistics(ov, offs, ig, idt, scores, mo, None, compute_fp=False, collect_scores=True)
            want = []
            for f, ((gtd, dtd), o) in enumerate(zip(frames, overlaps)):
                a, b = int(g['gt_offsets'][f]), int(g['gt_offsets'][f + 1])
                c, e = int(g['dt_offsets'][f]), int(g['dt_offsets'][f + 1])
                want.append(R.compute_statistics(o, g[f'ignored_gt_{d}'][a:b], g[f'ignored_dt_{d}'][c:e], dtd['score'], mo))
            assert stats.dtype == torch.int64 and stats.cpu().tolist() == [[sum(w[0] for w in want), 0, sum(w[2] for w in want)]]
            got_scores = np.sort(tps.cpu().numpy()[flags.cpu().numpy() != 0].astype(np.float64))
            assert np.array_equal(got_scores, np.sort(np.concatenate([np.array(w[3], dtype=np.float64) for w in want])))
            t = int(g['num_thresholds'][d, k])
            th = torch.from_numpy(g['thresholds'][d, k, :t].astype(np.float32)).to(device)
            stats = ops.kitti_statistics(ov, offs, ig, idt, scores, mo, th, compute_fp=True)
            assert torch.equal(stats.cpu(), torch.from_numpy(g['stats'][d, k, :t]))
            assert torch.equal(stats.cpu(), torch.from_numpy(res['stats'][(d, k)]))


def test_eval_kitti_equals_the_oracle_and_the_reference(device, oracle_eval):
    from mask_bev_amd import kitti_eval as KE
    g, frames, _, res = oracle_eval
    labels, preds = _product_inputs(frames, device)
    got = KE.eval_class(labels, preds, [0], (0, 1, 2))
    assert got['precision'].shape == (1, 3, 2, 41) and np.array_equal(got['num_valid_gt'][0], g['num_valid_gt'])
    assert np.array_equal(got['num_thresholds'][0], g['num_thresholds'])
    assert np.array_equal(got['stats'][0], g['stats'])
    for d in range(3):
        for k in range(2):
            assert np.array_equal(got['stats'][0, d, k, :len(res['stats'][(d, k)])], res['stats'][(d, k)])
    assert np.abs(got['thresholds'][0] - g['thresholds']).max() <= 1e-6
    assert np.abs(got['precision'][0] - g['precision']).max() <= 1e-6
    assert np.abs(KE.get_mAP(got['precision'])[0] - g['ap']).max() <= 1e-6
    assert np.abs(KE.get_mAP(got['precision'])[0] - R.get_map(res['precision'])).max() <= 1e-6
    text = KE.eval_kitti(labels, preds)
    lines = text.splitlines()
    assert lines[0] == 'Car AP(Average Precision)@0.70:' and lines[2] == 'Car AP(Average Precision)@0.50:'
    assert lines[1] == 'bev  AP:' + ', '.join(f'{v:.2f}' for v in g['ap'][:, 0]) and lines[3].startswith('bev  AP:')
    assert text.metrics['Car']['bev_ap@0.50']['hard'] == pytest.approx(g['ap'][2, 1], abs=1e-6)
    # numpy predictions are uploaded; the alias module's rotate_iou_gpu_eval is K26
    again = KE.eval_kitti(labels, [dict(boxes=dt['boxes'], score=dt['score'], type=dt['type']) for _, dt in frames])
    assert str(again) == str(text)
    from mask_bev.evaluation.rotate_iou import rotate_iou_gpu_eval
    gt0, dt0 = frames[0]
    ov = rotate_iou_gpu_eval(dt0['boxes'], gt0['bev'])
    assert ov.dtype == np.float64 and np.abs(ov - R.rotate_iou(dt0['boxes'], gt0['bev'])).max() < 1e-5


# ------------------------------------------------------------------------------------------------ round trip
def test_round_trip_paint_fit_evaluate(device, capsys):
    """The sample label through K24 → K14 → K25 → metres: every fitted box equals the oracle's fit of the same mask, its
    centre lies within one cell of the label's, and eval_kitti of those boxes against those labels equals the oracle's."""
    from mask_bev_amd import batch as B, kitti_eval as KE, ops, rasterize
    from mask_bev_amd.predict import unpack_bits
    lab = B.kitti_labels_to_velodyne(B.read_kitti_label(os.path.join(SAMPLE, 'label_2', '000000.txt')),
                                     B.read_kitti_calib(os.path.join(SAMPLE, 'calib', '000000.txt')))
    x_range, y_range, vs, q = (0, 80), (-40, 40), 0.1, 12
    r = rasterize.KittiRasterizer(x_range, y_range, (-3, 1), vs, device=device)
    car_like = np.isin(lab['type'], rasterize.KITTI_CAR_LIKE) & B.object_range_mask(lab['boxes'], x_range, y_range)
    boxes7 = lab['boxes'][car_like]
    maps = r.rasterize_batch([boxes7])
    labels, pm = B.instance_targets(maps, q, packed=True)
    rows = torch.nonzero(labels.reshape(-1)).flatten()
    assert rows.numel() == len(boxes7) >= 3
    n, mom, cell = ops.fit_boxes(pm, rows)
    dense = unpack_bits(pm.words[rows], pm.h, pm.w).cpu().numpy()
    metres = rasterize.boxes_from_cells(cell, x_range, y_range, r.nx, r.ny)
    bad = []
    for j in range(rows.numel()):
        rn, rm, rb = R.fit_box(dense[j])
        assert int(n[j]) == rn > 0 and mom[j].cpu().tolist() == rm
        e = float(np.abs(cell[j].double().cpu().numpy() - rb).max() / np.abs(rb).max())
        f64_bars.check(capsys, MODULE, f'round trip box {j}', e, f64_bars.F32_BAR, bad)
        got = metres[j].double().cpu().numpy()
        assert abs(got[0] - boxes7[j, 0]) <= vs and abs(got[1] - boxes7[j, 1]) <= vs and got[2] >= got[3]
        iou = float(R.rotate_iou(got[None], boxes7[j:j + 1, [0, 1, 3, 4, 6]])[0, 0])
        with capsys.disabled():
            print(f'\n[{MODULE}] round trip box {j}: IoU with the label\'s box {iou:.4f} '
                  f'(l, w {got[2]:.3f}, {got[3]:.3f} vs {boxes7[j, 3]:.3f}, {boxes7[j, 4]:.3f})', end='')
    assert not bad, bad
    scores = np.array([0.9, 0.8, 0.7, 0.6, 0.5][:rows.numel()], dtype=np.float32)
    preds = [dict(boxes=metres, score=torch.from_numpy(scores).to(device), type=np.zeros(rows.numel(), dtype=np.int64))]
    text = KE.eval_kitti([lab], preds)
    frames = [(dict(lab, bev=lab['boxes'][:, [0, 1, 3, 4, 6]]),
               dict(type=np.zeros(rows.numel(), dtype=np.int64), score=scores.astype(np.float64), boxes=metres.double().cpu().numpy()))]
    ov = [R.rotate_iou(frames[0][1]['boxes'], frames[0][0]['bev'])]
    assert np.abs(ov[0] - 0.5).min() > 1e-3 and np.abs(ov[0] - 0.7).min() > 1e-3
    res = R.eval_class(frames, ov, 0, (0, 1, 2), MIN_OVERLAPS)
    for d in range(3):
        for k in range(2):
            assert np.array_equal(text.raw['stats'][0, d, k, :len(res['stats'][(d, k)])], res['stats'][(d, k)])
    assert np.abs(text.raw['precision'][0] - res['precision']).max() <= 1e-6
    assert np.abs(text.raw['thresholds'][0] - res['thresholds']).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ Predictions
def test_predictions_boxes_and_kitti_predictions(device):
    from mask_bev_amd import ops, rasterize
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(0)
    kw = tiny_kwargs()
    m = MaskBevModule(**kw).to(device)
    m.log_scalars = False
    p = m.predict([x.to(device) for x in random_scans(kw, [2500, 1800], seed=5)])
    b, q = p.keep.shape
    p.keep = torch.ones_like(p.keep)                                   # an untrained head keeps what it likes: keep most rows
    p.keep[0, 1] = False
    p.keep[1, q - 1] = False
    p.masks.words[3].zero_()                                           # and one kept mask is empty
    areas = ops.fit_boxes(p.masks, torch.arange(b * q, device=device))[0].view(b, q)
    want_rows = torch.nonzero((p.keep & (areas > 0)).reshape(-1)).flatten()
    assert 0 < want_rows.numel() == int(p.keep.sum()) - int((areas[p.keep] == 0).sum()) < b * q - 2
    out = p.boxes(kw['x_range'], kw['y_range'], kw['voxel_size'])
    r = want_rows.numel()
    assert tuple(out['boxes'].shape) == (r, 5) and out['boxes'].dtype == torch.float32 and out['boxes'].is_cuda
    assert out['scores'].dtype == torch.float32 and tuple(out['scores'].shape) == (r,)
    assert torch.equal(out['scan'] * q + out['query'], want_rows) and torch.equal(out['cells'], areas.reshape(-1)[want_rows])
    assert bool((out['boxes'][:, 2] >= out['boxes'][:, 3]).all()) and bool(torch.isfinite(out['boxes']).all())
    assert torch.equal(out['scores'], p.scores.reshape(-1)[want_rows])
    nx = ny = 80
    direct = rasterize.boxes_from_cells(ops.fit_boxes(p.masks, want_rows)[2], kw['x_range'], kw['y_range'], nx, ny)
    assert torch.equal(out['boxes'], direct)
    lo, hi = kw['x_range']
    assert bool(((out['boxes'][:, 0] > lo) & (out['boxes'][:, 0] < hi)).all())
    # a rasteriser in place of the ranges; the per-scan form
    rz = rasterize.KittiRasterizer(kw['x_range'], kw['y_range'], kw['z_range'], kw['voxel_size'])
    assert torch.equal(p.boxes(rz)['boxes'], out['boxes'])
    per_scan = p.kitti_predictions(rz)
    assert len(per_scan) == b and sum(d['boxes'].shape[0] for d in per_scan) == r
    assert torch.equal(torch.cat([d['boxes'] for d in per_scan]), out['boxes'])
    assert all(d['type'].dtype == torch.int64 and not d['type'].any() and d['score'].shape[0] == d['boxes'].shape[0]
               for d in per_scan)
    with pytest.raises(ValueError):
        p.boxes((0, 10), (0, 10), 0.5)


# ------------------------------------------------------------------------------------------------ the launcher's hook
def test_launcher_kitti_bev_evaluation(device, tmp_path):
    """``evaluate.kitti_bev_evaluation`` over a KITTI object tree holding the sample frame twice, with an untrained
    tiny model: predict → boxes → protocol end to end; the block has the reference's lines for Car at 0.7 and 0.5."""
    import shutil
    from mask_bev_amd.evaluate import kitti_bev_evaluation
    from mask_bev_amd.mask_bev_module import MaskBevModule
    rng = np.random.default_rng(2)
    for k in ('velodyne', 'label_2', 'calib'):
        d = tmp_path / f'data_object_{k}' / 'training' / k
        d.mkdir(parents=True)
        for frame in (0, 1, 2):
            if k == 'velodyne':
                pts = rng.uniform([0, -10, -3, 0], [20, 10, 1, 1], (2000 + frame, 4)).astype(np.float32)
                pts.tofile(d / f'{frame:06d}.bin')
            else:
                shutil.copy(os.path.join(SAMPLE, k, '000000.txt'), d / f'{frame:06d}.txt')
    (tmp_path / 'val.txt').write_text('000000\n000001\n000002\n')
    torch.manual_seed(0)
    kw = dict(tiny_kwargs(), x_range=(0, 20), y_range=(-10, 10))
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    config = dict(kw, dataset='kitti', batch_size=2)
    out = kitti_bev_evaluation(model, config, device, tmp_path)
    lines = out.splitlines()
    assert len(lines) == 4 and lines[0] == 'Car AP(Average Precision)@0.70:' and lines[2] == 'Car AP(Average Precision)@0.50:'
    assert all(l.startswith('bev  AP:') and len(l.split(',')) == 3 for l in (lines[1], lines[3]))
    assert set(out.metrics['Car']) == {'bev_ap@0.70', 'bev_ap@0.50'}
    assert all(0.0 <= v <= 100.0 for m in out.metrics['Car'].values() for v in m.values())
    assert out.raw['num_valid_gt'][0].tolist() == [3 * v for v in (out.raw['num_valid_gt'][0] // 3).tolist()]
