"""K32 (panoptic tp / fp / fn, IoU sums and confusion per frame, csrc/panoptic.hip) through the C ABI, and what is built on
it: ``ops.panoptic_frames``, ``metrics.DevicePanopticQuality``, ``Predictions.panoptic_points`` / ``panoptic_bev`` and the
launcher's ``point PQ`` line.

The kernel: every output EQUAL to the numpy restatement (tests/panoptic_ref.py) into poisoned outputs and workspace, the f64
IoU sums within 1e-12 relative and bit-equal between two runs; the degenerate calls and the limits."""
import re

import numpy as np
import pytest
import torch
import yaml

from tests import panoptic_ref as R
from tests.util_cfg import random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
POISON = 0x5a5a5a5a
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3


def _raw(lib, device, pq, gw, lengths, qc, lut, C, max_gt, min_points):
    """mbv_panoptic_frames into poisoned buffers (outputs and workspace) → (rc, dict of host arrays)."""
    from mask_bev_amd.ops_core import _ptr, _stream
    frames, P = qc.shape
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32, device=device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    tpq, tgw, tqc, tlut = t(pq), t(gw), t(qc), t(lut)
    full = lambda shape, dtype: torch.full(shape, POISON, dtype=dtype, device=device)
    out = dict(stats=full((frames, C, 3), torch.int32), iou=full((frames, C), torch.int64).view(torch.float64),
               confusion=full((frames, C, C), torch.int64), n_gt=full((frames,), torch.int32),
               gt_key=full((frames, max_gt), torch.int32), gt_area=full((frames, max_gt), torch.int32),
               pred_area=full((frames, max(P, 1)), torch.int32))
    nbytes = lib.mbv_panoptic_frames_workspace_bytes(frames, P, max_gt, C)
    ws = torch.full((max(nbytes, 256),), 0x5a, dtype=torch.uint8, device=device)
    rc = lib.mbv_panoptic_frames(_ptr(tpq), _ptr(tgw), pq.shape[0], _ptr(offs), frames, _ptr(tqc), P, _ptr(tlut), lut.shape[0],
                                 C, max_gt, min_points, _ptr(out['stats']), _ptr(out['iou']), _ptr(out['confusion']),
                                 _ptr(out['n_gt']), _ptr(out['gt_key']), _ptr(out['gt_area']), _ptr(out['pred_area']), _ptr(ws),
                                 ws.numel(), _stream())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host['pred_area'] = host['pred_area'][:, :P]
    return rc, host


def _assert_equal(got, ref):
    for k in ('stats', 'confusion', 'n_gt', 'gt_key', 'gt_area', 'pred_area'):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    assert np.all(np.abs(got['iou'] - ref['iou']) <= 1e-12 * np.abs(ref['iou'])), (got['iou'], ref['iou'])


@pytest.mark.parametrize('max_gt', [8, 64])
@pytest.mark.parametrize('C', [2, 3])
@pytest.mark.parametrize('P', [1, 7, 1024])
def test_k32_equals_the_restatement(device, P, C, max_gt):
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    pq, gw, lengths, qc, lut = R.planted_case(P, C)
    ref = R.frames(pq, gw, lengths, qc, lut, C, max_gt, R.MIN_POINTS)
    # the cases are there, by the reference alone
    tp, fp, fn = ref['stats'].sum((0, 1))
    assert tp > 0 and fp > 0 and fn > 0 and ref['ignored'] >= 100 and ref['in_pair'] >= 100
    big = R.element_classes(pq[-1000:], gw[-1000:], qc[3], lut, C)
    first = np.flatnonzero((big[0] == 1) & (big[1] == 0))
    assert len(set(first // 256)) == 2                                  # a segment fed by two blocks of one frame
    assert ref['n_gt'].tolist()[:3] == [0, 1, 5] and 8 < ref['n_gt'][3] < 64
    if max_gt == 8:                                                     # the overflowing frame: zeros, and n_gt says so
        assert not ref['stats'][3].any() and not ref['iou'][3].any() and ref['pred_area'][3].any() == (P >= 1)
    sem = (gw.view(np.uint32) & 0xffff).astype(np.int64)
    assert (sem >= lut.shape[0]).any() and {-1, -7, C} <= set(lut[sem[sem < lut.shape[0]]].tolist())
    assert {P, 2 ** 30, -5} <= set(pq.tolist()) and {0, 65535} <= set((gw.view(np.uint32) >> 16).tolist())
    if P >= 7:
        assert {0, C, -3} <= set(qc[2].tolist()) and ((ref['pred_area'] == 0) & (qc >= 1) & (qc < C)).any()
    rc, got = _raw(lib, device, pq, gw, lengths, qc, lut, C, max_gt, R.MIN_POINTS)
    assert rc == 0
    _assert_equal(got, ref)
    rc2, again = _raw(lib, device, pq, gw, lengths, qc, lut, C, max_gt, R.MIN_POINTS)
    assert rc2 == 0 and all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)
    # the wrapper: the same, from lengths and from device offsets
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32, device=device)
    for where in (lengths, offs):
        out = ops.panoptic_frames(t(pq), t(gw), where, t(qc), t(lut), C, max_gt=max_gt, min_points=R.MIN_POINTS)
        _assert_equal(dict(stats=out.frame_stats.cpu().numpy(), iou=out.frame_iou.cpu().numpy(),
                           confusion=out.confusion.cpu().numpy(), n_gt=out.n_gt.cpu().numpy(), gt_key=out.gt_key.cpu().numpy(),
                           gt_area=out.gt_area.cpu().numpy(), pred_area=out.pred_area.cpu().numpy()), ref)


def test_k32_degenerate_calls_and_limits(device):
    from mask_bev_amd import _lib
    from mask_bev_amd.ops_core import _ptr, _stream
    lib = _lib.load()
    C, P, max_gt = 3, 7, 64
    pq, gw, lengths, qc, lut = R.planted_case(P, C)
    # no frame: MBV_OK before any pointer is looked at
    assert lib.mbv_panoptic_frames(None, None, 0, None, 0, None, P, None, 0, C, max_gt, 5, None, None, None, None, None, None,
                                   None, None, 0, _stream()) == 0
    # all frames empty: zeros everywhere, keys -1
    rc, got = _raw(lib, device, pq[:0], gw[:0], [0, 0, 0], qc[:3], lut, C, max_gt, 5)
    assert rc == 0 and not got['stats'].any() and not got['iou'].any() and not got['confusion'].any()
    assert not got['n_gt'].any() and not got['gt_area'].any() and not got['pred_area'].any() and (got['gt_key'] == -1).all()
    # no query: every element is class 0 on the prediction side
    ref = R.frames(pq, gw, lengths, qc[:, :0], lut, C, max_gt, 5)
    rc, got = _raw(lib, device, pq, gw, lengths, qc[:, :0], lut, C, max_gt, 5)
    assert rc == 0 and ref['stats'][..., 2].any() and not ref['stats'][..., :2].any()
    _assert_equal(got, ref)
    # an empty table: everything is ignored
    ref = R.frames(pq, gw, lengths, qc, lut[:0], C, max_gt, 5)
    rc, got = _raw(lib, device, pq, gw, lengths, qc, lut[:0], C, max_gt, 5)
    assert rc == 0 and not ref['confusion'].any()
    _assert_equal(got, ref)

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    tpq, tgw, tqc, tlut = t(pq), t(gw), t(np.zeros((4, 1030), dtype=np.int32)), t(lut)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32, device=device)
    bufs = [torch.empty((4 * 64 * 8,), dtype=torch.int64, device=device) for _ in range(7)]      # room for any output
    ws = torch.empty((1 << 20,), dtype=torch.uint8, device=device)

    def call(P=7, C=3, max_gt=64, min_points=5, frames=4, total=pq.shape[0], ws_bytes=None, words=tgw, lut_len=lut.shape[0]):
        rc = lib.mbv_panoptic_frames(_ptr(tpq), _ptr(words), total, _ptr(offs), frames, _ptr(tqc), P, _ptr(tlut), lut_len, C,
                                     max_gt, min_points, *[_ptr(b) for b in bufs], _ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc

    assert call() == 0
    assert call(P=1025) == UNSUPPORTED and call(C=17) == UNSUPPORTED and call(max_gt=1025) == UNSUPPORTED
    assert call(frames=65536) == UNSUPPORTED and call(total=2 ** 31 - 1) == UNSUPPORTED
    assert call(max_gt=0) == BAD_ARG and call(C=0) == BAD_ARG and call(min_points=-1) == BAD_ARG and call(P=-1) == BAD_ARG
    assert call(total=-1) == BAD_ARG and call(lut_len=-1) == BAD_ARG and call(words=None) == BAD_ARG
    assert call(ws_bytes=16) == WORKSPACE
    assert lib.mbv_panoptic_frames_workspace_bytes(4, 1025, 64, 3) == 0 and lib.mbv_panoptic_frames_workspace_bytes(4, 7, 0, 3) == 0
    assert lib.mbv_panoptic_frames_workspace_bytes(4, 7, 64, 17) == 0
    assert lib.mbv_panoptic_frames_workspace_bytes(4, 7, 64, 3) >= 4 * (2 * 3 * 8192 + 64 * 7 * 4)


def test_device_panoptic_quality_over_two_updates(device):
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.metrics import DevicePanopticQuality, panoptic_quality
    C, P = 3, 7
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    a = R.planted_case(P, C, seed=0)
    b = R.planted_case(P, C, seed=1)
    metric = DevicePanopticQuality(C, a[4], min_points=R.MIN_POINTS, max_gt=64)
    assert metric.compute()['frames'] == 0 and metric.compute()['pq'] == 0.0
    for pq, gw, lengths, qc, lut in (a, b):
        metric.update(t(pq), t(qc), t(gw), lengths)
    ref = R.frames(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), a[2] + b[2], np.concatenate([a[3], b[3]]), a[4], C,
                   64, R.MIN_POINTS)
    want = panoptic_quality(ref['stats'][..., 0].sum(0), ref['stats'][..., 1].sum(0), ref['stats'][..., 2].sum(0),
                            ref['iou'].sum(0), ref['confusion'].sum(0))
    got = metric.compute()
    assert got['frames'] == 8 and got['per_class']['tp'] == want['per_class']['tp'] and sum(want['per_class']['tp']) > 0
    assert got['per_class']['fp'] == want['per_class']['fp'] and got['per_class']['fn'] == want['per_class']['fn']
    for k in ('pq', 'sq', 'rq', 'iou'):
        assert got[k] == pytest.approx(want[k], rel=1e-12) and got['per_class'][k] == pytest.approx(want['per_class'][k], rel=1e-12)
    assert 0 < got['pq'] < 1 and 0 < got['iou'] < 1
    metric.reset()
    assert metric.compute()['frames'] == 0
    small = DevicePanopticQuality(C, a[4], min_points=R.MIN_POINTS, max_gt=8)
    small.update(t(a[0]), t(a[3]), t(a[1]), a[2])
    with pytest.raises(MaskBevHipError, match='1 of 4 frames'):
        small.compute()


def _tiny_model(device):
    from mask_bev_amd.mask_bev_module import MaskBevModule
    kw = tiny_kwargs()
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    return kw, model


def _words_from_queries(point_query, erase=None):
    """The ``.label`` words that make the prediction itself the ground truth: car (10), instance query + 1; class 0 (40)
    elsewhere, and where ``erase`` is the query."""
    q = point_query.to(torch.int64)
    thing = (q >= 0) if erase is None else ((q >= 0) & (q != erase))
    return torch.where(thing, ((q + 1) << 16) | 10, torch.full_like(q, 40)).to(torch.int32)


def test_predictions_panoptic_points_and_bev(device):
    from mask_bev_amd.metrics import DevicePanopticQuality, semantic_kitti_class_lut
    kw, model = _tiny_model(device)
    scans = [s.to(device) for s in random_scans(kw, [1500, 1201], seed=3)]
    pred = model.predict(scans)
    lifted = pred.lift(scans, model)
    owners = torch.nonzero(lifted.counts.reshape(-1) > 0).flatten().tolist()
    assert owners, 'no query owns a point: the test needs another seed'
    n_seg = len(owners)
    metric = DevicePanopticQuality(2, semantic_kitti_class_lut(), min_points=1)
    pred.panoptic_points(lifted, [_words_from_queries(p) for p in lifted.per_scan()], metric)
    got = metric.compute()
    assert got['pq'] == 1.0 and got['sq'] == 1.0 and got['rq'] == 1.0 and got['iou'] == 1.0 and got['frames'] == 2
    assert got['per_class']['tp'][1] == n_seg and got['per_class']['fp'][1] == 0 and got['per_class']['fn'][1] == 0
    # one instance erased from the ground truth of its scan: that prediction is a false positive
    b, q = divmod(owners[0], pred.labels.shape[1])
    metric.reset()
    pred.panoptic_points(lifted, [_words_from_queries(p, erase=q if i == b else None) for i, p in enumerate(lifted.per_scan())],
                         metric)
    got = metric.compute()
    assert got['per_class']['tp'][1] == n_seg - 1 and got['per_class']['fp'][1] == 1 and got['per_class']['fn'][1] == 0
    with pytest.raises(Exception):
        pred.panoptic_points(lifted, [torch.zeros(3, dtype=torch.int32, device=device)] * 2, metric)
    # the BEV side: cells as elements, the map itself as the ground truth (0 = background, id = query + 1)
    cells = torch.bincount((pred.instance_map.reshape(-1) + 1).long(), minlength=2)[1:]
    n_bev = int((cells > 0).sum())
    assert n_bev > 0
    bev = DevicePanopticQuality(2, np.arange(2), min_points=1)
    gt = pred.instance_map + 1
    rec = pred.panoptic_bev(gt, bev)
    got = bev.compute()
    assert got['pq'] == 1.0 and got['per_class']['tp'][1] == int(rec.n_gt.sum()) > 0
    assert got['per_class']['fp'][1] == 0 and got['per_class']['fn'][1] == 0
    gone = int(gt[0].max()) if int(gt[0].max()) > 0 else None
    if gone is not None:
        bev.reset()
        erased = gt.clone()
        erased[0][erased[0] == gone] = 0
        pred.panoptic_bev(erased, bev)
        got = bev.compute()
        assert got['per_class']['fp'][1] == 1 and got['per_class']['fn'][1] == 0 and got['pq'] < 1.0


def test_launcher_prints_point_pq(device, tmp_path, capsys):
    """``--test`` on ``dataset: semantic-kitti``: with ``labels/NNNNNN.label`` next to every validated scan one ``point PQ``
    line whose tp, fp and fn are the restatement's on the same predictions; without the files no such line."""
    import train_mask_bev_amd as launcher
    from mask_bev_amd.evaluate import semantic_kitti_label_path
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.metrics import semantic_kitti_class_lut
    kw, model = _tiny_model(device)
    seq = tmp_path / 'data' / 'sequences' / '08'
    (seq / 'velodyne').mkdir(parents=True)
    (seq / 'mask_cache').mkdir()
    scans = random_scans(kw, [1500, 1201, 900, 700], seed=3)
    for i, s in enumerate(scans):
        s.numpy().tofile(seq / 'velodyne' / f'{i:06d}.bin')
        imap = np.zeros((80, 80), dtype=np.int32)
        imap[10:22, 10:19], imap[40:52, 30:39] = 1, 2
        np.save(seq / 'mask_cache' / f'{i:06d}.npy', imap)
    cfg = dict(kw, dataset='semantic-kitti', batch_size=2, val_sequences=[8], train_sequences=[8], panoptic_min_points=1)
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}
    ck = tmp_path / 'ckpt' / 'tiny'
    ck.mkdir(parents=True)
    path = ck / 'tiny-epoch=00-val_loss=1.000000.ckpt'
    launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'], path, 0, 'val_loss', 1.0)
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(cfg))
    argv = ['--config', str(tmp_path / 'tiny.yml'), '--test', '--data-root', str(tmp_path / 'data'), '--checkpoint-root',
            str(tmp_path / 'ckpt')]
    assert launcher.main(argv) == 0
    assert not [l for l in capsys.readouterr().out.splitlines() if l.startswith('point PQ')]
    # the model as the launcher loads it, its predictions, and a ground truth made from them: scan 0's first owner erased
    loaded = MaskBevModule.from_config(dict(cfg, checkpoint=str(path))).to(device)
    loaded.log_scalars = False
    loaded.flatten_parameters()
    files = [(seq / 'velodyne' / f'{i:06d}.bin', None) for i in range(4)]
    assert semantic_kitti_label_path(files[2][0]) == seq / 'labels' / '000002.label'
    (seq / 'labels').mkdir()
    per, classes = [], []
    for start in (0, 2):
        part = [s.to(device) for s in scans[start:start + 2]]
        pred = loaded.predict(part)
        per += [p.cpu() for p in pred.lift(part, loaded).per_scan()]
        classes.append(pred.query_classes().cpu().numpy())
    classes = np.concatenate(classes)
    owners = sorted(set(per[0][per[0] >= 0].tolist()))
    assert owners
    words = [_words_from_queries(p, erase=owners[0] if i == 0 else None).numpy() for i, p in enumerate(per)]
    for i, w in enumerate(words):
        w.view(np.uint32).astype('<u4').tofile(seq / 'labels' / f'{i:06d}.label')
    assert launcher.main(argv) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('point PQ')]
    assert len(lines) == 1
    got = re.fullmatch(r'point PQ (\S+) SQ (\S+) RQ (\S+) IoU (\S+) \(car; tp (\d+) fp (\d+) fn (\d+)\)', lines[0])
    assert got, lines[0]
    ref = R.frames(np.concatenate([p.numpy() for p in per]).astype(np.int32), np.concatenate(words), [len(p) for p in per], classes,
                   semantic_kitti_class_lut(), 2, 256, 1)
    tp, fp, fn = ref['stats'][:, 1].sum(0).tolist()
    assert [int(got.group(k)) for k in (5, 6, 7)] == [tp, fp, fn] and tp > 0 and fp == 1 and fn == 0
    assert 0.0 < float(got.group(1)) < 1.0 and float(got.group(2)) == 1.0
