"""DeviceMaskMeanAveragePrecision on the host: ``compute()`` on states built from the oracle's per-image evaluation
equals the oracle's whole COCO accumulation, in one process and with the state split over two gloo ranks; the
``mask_map`` switch of ``enable_metrics``."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import metrics_oracle as MO
from tests.mask_map_ref import image_dict, integer_tables, oracle_state
from tests.util_cfg import tiny_kwargs

NUM_LABELS = 3


def _random_images(trial, g):
    """The cases of test_mask_map_matches_coco_protocol_oracle (tests/test_host_cpu.py); trial 4: 130 detections an image,
    more than the 100 the protocol keeps."""
    imgs = []
    for _ in range(3):
        q, ng = (130, 9) if trial == 4 else (12, 9)
        iou = torch.rand(q, ng, generator=g, dtype=torch.float64)
        iou[iou < 0.45] = 0
        iou[:, -2:] = 0
        if trial == 1:
            iou = (iou * 4).round() / 4
        im = dict(ious=iou, scores=torch.rand(q, generator=g, dtype=torch.float32).double(),
                  pred_labels=torch.randint(0, 2, (q,), generator=g),
                  pred_areas=torch.rand(q, generator=g, dtype=torch.float64) * 12000,
                  gt_labels=torch.cat([torch.ones(ng - 2, dtype=torch.long), torch.zeros(2, dtype=torch.long)]),
                  gt_areas=torch.cat([torch.rand(ng - 2, generator=g, dtype=torch.float64) * 12000,
                                      torch.zeros(2, dtype=torch.float64)]))
        imgs.append({k: v.numpy() for k, v in im.items()})
    return imgs


def _tables_images():
    """Integer tables with score ties, IoU ties at the thresholds and areas on the range borders; one image has no object."""
    rng = np.random.default_rng(5)
    return [image_dict(*integer_tables(rng, 130 if i == 0 else 12, 9, no_object=(i == 2))) for i in range(3)]


def _all_cases():
    g = torch.Generator().manual_seed(0)
    return [_random_images(trial, g) for trial in range(5)] + [_tables_images()]


def _append(metric, imgs):
    for im in imgs:
        rank, matched, ignored, npig = oracle_state(im, NUM_LABELS)
        metric.append_state(torch.from_numpy(im['scores']).float(), torch.from_numpy(np.asarray(im['pred_labels'])),
                            torch.from_numpy(rank), torch.from_numpy(matched), torch.from_numpy(ignored),
                            torch.from_numpy(npig))


def test_compute_matches_the_coco_protocol_oracle():
    from mask_bev_amd.metrics import DeviceMaskMeanAveragePrecision
    for case, imgs in enumerate(_all_cases()):
        m = DeviceMaskMeanAveragePrecision()
        _append(m, imgs)
        got, ref = m.compute(), MO.coco_mask_map(imgs)
        assert list(got.keys()) == list(ref.keys())
        assert any(v > 0 for v in ref.values())
        for k in ref:
            assert got[k] == pytest.approx(ref[k], abs=1e-12), (case, k)
        m.reset()
        assert m.state == [] and set(m.compute().values()) == {-1.0}


def _gloo_worker(rank, world, rdv, out):
    dist.init_process_group('gloo', init_method=f'file://{rdv}', rank=rank, world_size=world)
    from mask_bev_amd.metrics import DeviceMaskMeanAveragePrecision
    res = []
    for imgs in _all_cases():
        imgs = imgs + imgs[:1]                               # four images: two per rank, in the order one process sees
        m = DeviceMaskMeanAveragePrecision()
        _append(m, imgs[2 * rank:2 * rank + 2])
        res.append(m.compute())
    out[rank] = res
    dist.destroy_process_group()


def test_compute_gathers_the_state_of_two_gloo_ranks():
    from mask_bev_amd.metrics import DeviceMaskMeanAveragePrecision
    fd, rdv = tempfile.mkstemp(prefix='mbv_gloo_rdv_')
    os.close(fd)
    os.unlink(rdv)
    try:
        out = mp.Manager().dict()
        mp.spawn(_gloo_worker, args=(2, rdv, out), nprocs=2, join=True)
    finally:
        if os.path.exists(rdv):
            os.unlink(rdv)
    for case, imgs in enumerate(_all_cases()):
        m = DeviceMaskMeanAveragePrecision()
        _append(m, imgs + imgs[:1])
        single = m.compute()
        ref = MO.coco_mask_map(imgs + imgs[:1])
        for k in ref:
            assert single[k] == pytest.approx(ref[k], abs=1e-12), (case, k)
            assert out[0][case][k] == single[k] and out[1][case][k] == single[k], (case, k)


def test_enable_metrics_mask_map_switch():
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.metrics import DeviceMaskMeanAveragePrecision, MaskMeanAveragePrecision
    m = MaskBevModule(**tiny_kwargs(nx=40, ny=40, q=4))
    m.enable_metrics(layers=(0, 9), train=False, mask_map='device')
    assert m._train_metric_per_layer == {} and sorted(m._val_metric_per_layer) == [0, 9]
    assert all(type(v[1]) is DeviceMaskMeanAveragePrecision for v in m._val_metric_per_layer.values())
    assert m._val_metric_per_layer[0][1] is not m._val_metric_per_layer[9][1]
    m.enable_metrics(layers=(9,), val=False, mask_map=True)
    assert type(m._train_metric_per_layer[9][1]) is MaskMeanAveragePrecision
    m.enable_metrics(layers=(9,), val=False)
    assert m._train_metric_per_layer[9][1] is None
    with pytest.raises(ValueError):
        m.enable_metrics(mask_map='host')
