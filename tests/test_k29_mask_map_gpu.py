"""K29 — COCO mask AP on the device: K29a pairwise popcounts of bit-packed masks against integer sums of the dense masks
(exact, outputs between sentinels), K29b per-image matching against the oracle's ``coco_evaluate_image`` (exact),
``DeviceMaskMeanAveragePrecision`` from logits against the oracle's ``coco_mask_map`` (1e-12), the module's metric slot
against the host class, and the launcher's ``--test`` report."""
import re

import numpy as np
import pytest
import torch
import yaml

from oracle import metrics_oracle as MO
from tests.mask_map_ref import RANK_NONE, image_dict, integer_tables, oracle_state
from tests.util_cfg import random_gt, random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 64            # int32 words on each side of an output: 256 bytes, the payload stays 256-byte aligned
KEYS = ('map', 'map_50', 'map_75', 'map_small', 'map_medium', 'map_large', 'mar_1', 'mar_10', 'mar_100', 'mar_small',
        'mar_medium', 'mar_large')


def _between_sentinels(shape, device):
    n = int(np.prod(shape))
    raw = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.int32, device=device)
    return raw, raw[PAD:PAD + n].view(shape)


def _sentinels_intact(raw):
    return bool((raw[:PAD] == SENTINEL).all()) and bool((raw[-PAD:] == SENTINEL).all())


def _overlap_case(name):
    g = torch.Generator().manual_seed(29)
    if name == 'tail_bit':                  # 37 x 45 = 1665 cells: 27 groups of 64, 54 words, ONE bit in the last group
        n, q, ng, h, w = 3, 5, 4, 37, 45
        pred, gt = torch.rand(n, q, h, w, generator=g) > 0.5, torch.rand(n, ng, h, w, generator=g) > 0.6
        pred[0, 1] = False                  # an empty prediction
        pred[1, 2] = True                   # a full one
        gt[2] = False                       # an image whose ground truth is all padding
        gt[0, 3] = False
    elif name == 'tile_edges':              # 130 predictions: three tiles of 64; 376 words: three chunks of 128
        n, q, ng, h, w = 2, 130, 7, 100, 120
        pred, gt = torch.rand(n, q, h, w, generator=g) > 0.7, torch.rand(n, ng, h, w, generator=g) > 0.5
        gt[:, 5:] = False
    else:                                   # 'split': 1126 words: two splits of the contraction; 40 ground truths: two tiles
        n, q, ng, h, w = 1, 3, 40, 180, 200
        pred, gt = torch.rand(n, q, h, w, generator=g) > 0.5, torch.rand(n, ng, h, w, generator=g) > 0.5
        gt[0, 10:33] = False
    return pred, gt


@pytest.mark.parametrize('name', ['tail_bit', 'tile_edges', 'split'])
def test_pairwise_overlap_is_exact_and_stays_inside_its_outputs(device, name):
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    pred, gt = _overlap_case(name)
    n, q, h, w = pred.shape
    ng = gt.shape[1]
    if name == 'tail_bit':
        assert lib.mbv_packed_mask_words(h, w) == 54 and h * w % 64 == 1
    p64, g64 = pred.flatten(2).long(), gt.flatten(2).long()
    want_inter = torch.einsum('nqk,ngk->nqg', p64, g64).to(torch.int32)
    want_pa, want_ga = p64.sum(2).to(torch.int32), g64.sum(2).to(torch.int32)
    pp = ops.pack_binary_masks(pred.flatten(0, 1).float().to(device))
    gp = ops.pack_binary_masks(gt.flatten(0, 1).float().to(device))
    raws, outs = zip(*[_between_sentinels(s, device) for s in ((n, q, ng), (n, q), (n, ng))])
    rc = lib.mbv_pairwise_mask_overlap(ops._ptr(pp.words), ops._ptr(gp.words), n, q, ng, pp.words.shape[1],
                                       ops._ptr(outs[0]), ops._ptr(outs[1]), ops._ptr(outs[2]), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert all(_sentinels_intact(r) for r in raws)
    assert torch.equal(outs[0].cpu(), want_inter) and torch.equal(outs[1].cpu(), want_pa)
    assert torch.equal(outs[2].cpu(), want_ga)
    # the wrapper gives the same tables
    inter, pa, ga = ops.pairwise_mask_overlap(pp, gp, n)
    assert torch.equal(inter.cpu(), want_inter) and torch.equal(pa.cpu(), want_pa) and torch.equal(ga.cpu(), want_ga)


def test_pairwise_overlap_without_pairs_and_beyond_its_limits(device):
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    null = ops._ptr(None)
    for n, q, ng in ((0, 5, 4), (3, 0, 4), (3, 5, 0), (0, 0, 0)):
        assert lib.mbv_pairwise_mask_overlap(null, null, n, q, ng, 54, null, null, null, ops._stream()) == 0
    assert lib.mbv_pairwise_mask_overlap(null, null, 1, 1025, 4, 54, null, null, null, ops._stream()) == -3
    assert lib.mbv_pairwise_mask_overlap(null, null, 1, 4, 1025, 54, null, null, null, ops._stream()) == -3
    assert lib.mbv_pairwise_mask_overlap(null, null, 1, 4, 4, 54, null, null, null, ops._stream()) == -1
    torch.cuda.synchronize()


def _table_images(q):
    rng = np.random.default_rng(100 + q)
    # image 1 of the long case: all 130 detections in class 0, more than the 100 the protocol keeps
    tables = [integer_tables(rng, q, 9, labels_below=1 if (i == 1 and q > 100) else 3, no_object=(i == 2)) for i in range(3)]
    if q > 100:
        tables[1][5][2:5] = 0               # ... and three real ground truths of that class
    tables[0][4][3] = 7                     # a predicted label outside 0 .. L-1
    tables[1][5][1] = 5                     # a ground-truth label outside it
    tables[1][4][0] = -1
    return tables


@pytest.mark.parametrize('q', [130, 12])
def test_coco_match_equals_the_oracle(device, q):
    """Every (image, class, area range): rank, matched bits, ignored bits and the counted ground truths equal the oracle's
    ``coco_evaluate_image`` on the IoUs of the same integer tables."""
    from mask_bev_amd import ops
    from mask_bev_amd.metrics import DeviceMaskMeanAveragePrecision as Metric
    num_labels = 3
    tables = _table_images(q)
    stack = [torch.from_numpy(np.stack([t[i] for t in tables])) for i in range(6)]
    inter, pa, ga, sc, pl, gl = [x.to(device) for x in stack]
    thrs = torch.from_numpy(np.linspace(0.5, 0.95, 10)).to(device)
    areas = torch.tensor([[lo, hi] for lo, hi in MO.COCO_AREAS.values()], dtype=torch.float64, device=device)
    assert torch.equal(thrs.cpu(), Metric.IOU_THRS)
    rank, matched, ignored, npig = ops.coco_match(inter.int(), pa.int(), ga.int(), sc, pl.int(), gl.int(), num_labels, thrs,
                                                  areas, 100)
    seen_cut = seen_match = False
    for i, t in enumerate(tables):
        w_rank, w_matched, w_ignored, w_npig = oracle_state(image_dict(*t), num_labels)
        assert np.array_equal(rank[i].cpu().numpy(), w_rank), i
        assert np.array_equal(matched[i].cpu().numpy(), w_matched), i
        assert np.array_equal(ignored[i].cpu().numpy(), w_ignored), i
        assert np.array_equal(npig[i].cpu().numpy(), w_npig), i
        in_range = (t[4] >= 0) & (t[4] < num_labels)
        seen_cut |= bool((w_rank[in_range] == RANK_NONE).any())
        seen_match |= bool(w_matched.any())
    assert seen_match and seen_cut == (q > 100)          # the cases do match, and the long one is cut at max_det


def _logit_batch(seed, device):
    """B = 2, Q = 6 logits at 10 x 12 for a 40 x 48 grid, G = 5 with two padding slots: three queries follow a ground truth
    (block-aligned rectangles, so the interpolated logit is far from 0 inside them), three are noise."""
    g = torch.Generator().manual_seed(seed)
    b, q, ng, h, w, s = 2, 6, 5, 10, 12, 4
    low = torch.zeros(b, ng, h, w)
    for i in range(b):
        for j in range(ng - 2):
            y0, x0 = int(torch.randint(0, h - 4, (1,), generator=g)), int(torch.randint(0, w - 4, (1,), generator=g))
            low[i, j, y0:y0 + int(torch.randint(2, 5, (1,), generator=g)), x0:x0 + int(torch.randint(2, 5, (1,), generator=g))] = 1
    gt = low.repeat_interleave(s, 2).repeat_interleave(s, 3)
    logits = torch.randn(b, q, h, w, generator=g) * 3
    logits[:, :3] = (low[:, :3] * 2 - 1) * 6 + torch.randn(b, 3, h, w, generator=g)
    scores = torch.rand(b, q, generator=g)
    pred_labels = torch.randint(0, 2, (b, q), generator=g)
    pred_labels[:, :3] = 1
    gt_labels = torch.tensor([[1, 1, 1, 0, 0]] * b)
    return [x.to(device) for x in (logits, scores, pred_labels, gt, gt_labels)]


def test_metric_from_logits_equals_the_oracle(device):
    from mask_bev_amd import ops
    from mask_bev_amd.metrics import DeviceMaskMeanAveragePrecision
    from mask_bev_amd.predict import unpack_bits
    dense, packed = DeviceMaskMeanAveragePrecision(num_labels=2), DeviceMaskMeanAveragePrecision(num_labels=2)
    images = []
    for seed in (1, 2):
        logits, scores, pred_labels, gt, gt_labels = _logit_batch(seed, device)
        b, q = scores.shape
        dense.update(logits, scores, pred_labels, gt, gt_labels)
        packed.update(logits, scores, pred_labels, ops.pack_binary_masks(gt.flatten(0, 1)), gt_labels)
        # the oracle takes the IoUs of K21's own masks: a pixel whose interpolated logit is near 0 cannot make the sides differ
        keep = torch.ones((b, q), dtype=torch.bool, device=device)
        pm = ops.extract_masks(logits.float(), scores, keep, gt.shape[-2:], masks=True, instance_map=False)['masks']
        pred = unpack_bits(pm.words, pm.h, pm.w).view(b, q, pm.h, pm.w).cpu()
        for i in range(b):
            images.append(dict(ious=MO.pairwise_mask_iou(pred[i], gt[i].cpu() > 0.5), scores=scores[i].double().cpu().numpy(),
                               pred_labels=pred_labels[i].cpu().numpy(), pred_areas=pred[i].flatten(1).sum(1).double().numpy(),
                               gt_labels=gt_labels[i].cpu().numpy(), gt_areas=gt[i].flatten(1).sum(1).double().cpu().numpy()))
    assert len(dense.state) == 2 and all(x.is_cuda for x in dense.state[0])
    ref = MO.coco_mask_map(images)
    got, got_packed = dense.compute(), packed.compute()
    assert tuple(got) == KEYS and ref['map'] > 0 and ref['map_50'] > 0
    for k in KEYS:
        assert got[k] == pytest.approx(ref[k], abs=1e-12), k
        assert got_packed[k] == got[k], k
    dense.reset()
    assert dense.state == []


def test_module_validation_feeds_the_device_metric(device):
    """The `map_metric` slot filled with the device class through two validation steps; its logged values agree with the
    host class fed the same batches (that one thresholds torch's own interpolation: 2e-2, as for K15's IoUs)."""
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.metrics import DeviceMaskMeanAveragePrecision
    torch.manual_seed(0)
    kw = tiny_kwargs(nx=96, ny=96, q=8)
    m = MaskBevModule(**kw).to(device).eval()
    m.log_scalars = False
    m._panoptic_head._panoptic_head.num_points = 500
    batches = []
    for s in (0, 1):
        scans = [x.to(device) for x in random_scans(kw, [3000, 2500], seed=s)]
        labels, gt = random_gt(kw, 2, 3, seed=10 + s)
        batches.append((scans, (labels.to(device), gt.to(device))))
    logged = {}
    for mode in ('device', True):
        m.enable_metrics(layers=(0, 9), train=False, mask_map=mode)
        with torch.no_grad():
            for i, batch in enumerate(batches):
                assert torch.isfinite(m.validation_step(batch, i))
        metric = m._val_metric_per_layer[9][1]
        if mode == 'device':
            assert isinstance(metric, DeviceMaskMeanAveragePrecision) and len(metric.state) == 2 and metric.num_labels >= 2
        m.logged.clear()
        m.on_validation_epoch_end()
        logged[mode] = dict(m.logged)
        if mode == 'device':
            assert metric.state == []
    for layer in (0, 9):
        for k in KEYS:
            v = logged['device'][f'val_mAP_{layer}_{k}']
            assert v == -1.0 or 0.0 <= v <= 1.0, (layer, k, v)
            assert abs(v - logged[True][f'val_mAP_{layer}_{k}']) <= 2e-2, (layer, k)
        assert f'val_mIoU_layer_{layer}' in logged['device'] and f'val_cls_mAP_layer_{layer}' in logged['device']


def test_launcher_test_run_reports_the_metrics_of_every_layer(tmp_path, capsys):
    import train_mask_bev_amd as launcher
    from mask_bev_amd import synthetic
    root = tmp_path / 'data'
    seq = root / 'sequences' / '08'
    (seq / 'velodyne').mkdir(parents=True)
    (seq / 'mask_cache').mkdir()
    rng = np.random.default_rng(0)
    for f in range(2):
        pts = rng.uniform([-12, -12, -3, 0], [12, 12, 1, 1], (3000, 4)).astype(np.float32)
        pts.tofile(seq / 'velodyne' / f'{f:06d}.bin')
        imap = np.zeros((96, 96), dtype=np.int32)
        for k in range(3):
            y0, x0 = rng.integers(0, 80, 2)
            imap[y0:y0 + 12, x0:x0 + 9] = k + 1
        np.save(seq / 'mask_cache' / f'{f:06d}.npy', imap)
    kw = dict(synthetic.module_kwargs('smoke_96', 2, compute_dtype='bf16'), dataset='semantic-kitti', synthetic_points=6000,
              x_range=[-12, 12], y_range=[-12, 12], z_range=[-3, 1], train_sequences=[8], val_sequences=[8])
    cfg = tmp_path / 'smoke_96.yml'
    cfg.write_text(yaml.safe_dump(kw))
    ck = tmp_path / 'ckpt'
    assert launcher.main(['--config', str(cfg), '--train', '--synthetic', '--max-epochs', '1', '--steps-per-epoch', '2',
                          '--checkpoint-root', str(ck)]) == 0
    capsys.readouterr()
    assert launcher.main(['--config', str(cfg), '--test', '--data-root', str(root), '--checkpoint-root', str(ck)]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    at = [i for i, line in enumerate(lines) if line.startswith('val_loss ')]
    assert len(at) == 1 and np.isfinite(float(lines[at[0]].split()[1]))
    report = lines[at[0] + 1:]
    assert len(report) == 10
    for layer, line in enumerate(report):
        got = re.fullmatch(rf'layer {layer}: map (\S+) map_50 (\S+) map_75 (\S+) mar_100 (\S+) mIoU (\S+) cls_AP (\S+)', line)
        assert got, line
        values = [float(v) for v in got.groups()]
        assert all(v == -1.0 or 0.0 <= v <= 1.0 for v in values), line
