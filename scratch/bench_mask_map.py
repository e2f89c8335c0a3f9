#!/usr/bin/env python3
"""What the COCO mask-AP metric costs per validation step at the headline workload (semantic_kitti_512, B = 4, Q = 100,
bf16, eval mode, eager): one ``validation_step`` with no metric objects, with the host-side ``MaskMeanAveragePrecision``
on decoder layer 9 and on all ten layers, and with ``DeviceMaskMeanAveragePrecision`` (K29) on layer 9 and on all ten.
The variants alternate inside every round; a step is timed by the host clock around work that ends in a device
synchronise (the host-side class synchronises by itself, the others do not).  Also: the K29a and K29b calls alone on the
tensors of that step (HIP events; K29a = area pre-pass + fill + tile kernel), and ``compute()`` of either class on the
state of the timed steps.  Prints one JSON object; --out writes it to a file as well.

    python scratch/bench_mask_map.py [--rounds 5] [--out bench_mask_map.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mask_bev_amd import ops, synthetic                                     # noqa: E402
from mask_bev_amd.mask_bev_module import MaskBevModule                      # noqa: E402
from mask_bev_amd.metrics import DeviceMaskMeanAveragePrecision             # noqa: E402

WORKLOAD, BATCH = 'semantic_kitti_512', 4
VARIANTS = (('none', None, ()), ('host_layer9', True, (9,)), ('host_10_layers', True, tuple(range(10))),
            ('device_layer9', 'device', (9,)), ('device_10_layers', 'device', tuple(range(10))))


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(ms[0]), 'max_ms': float(ms[-1]), 'runs': len(ms)}


def events_ms(fn, runs=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mask_map.py needs an MI355X')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = MaskBevModule(**synthetic.module_kwargs(WORKLOAD, BATCH, compute_dtype='bf16')).to(dev).eval()
    model.log_scalars = False
    model.flatten_parameters()
    batches = [synthetic.make_batch(WORKLOAD, BATCH, 0, s, dev) for s in range(2)]

    def set_variant(mask_map, layers):
        model._val_metric_per_layer.clear()
        if layers:
            model.enable_metrics(layers=layers, train=False, mask_map=mask_map)
            for layer in layers:                    # the mask AP alone: the other two slots cost the same in every variant
                model._val_metric_per_layer[layer] = (None, model._val_metric_per_layer[layer][1], None)

    def step(i):
        with torch.no_grad():
            loss = model.validation_step(batches[i % len(batches)], i)
        torch.cuda.synchronize()
        return loss

    times = {name: [] for name, _, _ in VARIANTS}
    compute_ms = {}
    for rnd in range(-1, args.rounds):              # round -1 warms every variant up
        for name, mask_map, layers in VARIANTS:
            set_variant(mask_map, layers)
            t0 = time.perf_counter()
            step(rnd + 1)
            dt = (time.perf_counter() - t0) * 1e3
            if rnd >= 0:
                times[name].append(dt)
            if rnd == args.rounds - 1 and layers == (9,):
                metric = model._val_metric_per_layer[9][1]
                t0 = time.perf_counter()
                numbers = metric.compute()
                torch.cuda.synchronize()
                compute_ms[name] = {'ms': (time.perf_counter() - t0) * 1e3, 'images': BATCH, 'map': numbers['map']}
    result = {'workload': WORKLOAD, 'batch': BATCH, 'dtype': 'bf16', 'device': torch.cuda.get_device_name(0),
              'validation_step': {k: stats(v) for k, v in times.items()}, 'compute_after_one_step': compute_ms}

    # the two kernels alone, on the tensors of one step's last decoder layer
    with torch.no_grad():
        scans, (labels_gt, masks_gt) = batches[0]
        cls, masks, _ = model(scans)
    logits, sm = masks[9].float().contiguous(), cls[9].float().softmax(-1)
    scores, pred_labels = sm[..., 0].contiguous(), cls[9].argmax(-1).to(torch.int32)
    b, q = scores.shape
    gt = masks_gt if isinstance(masks_gt, ops.PackedMasks) else ops.pack_binary_masks(masks_gt.float().flatten(0, 1))
    keep = torch.ones((b, q), dtype=torch.bool, device=dev)
    extract = lambda: ops.extract_masks(logits, scores, keep, (gt.h, gt.w), masks=True, instance_map=False)['masks']  # noqa: E731
    pred = extract()
    inter, pa, ga = ops.pairwise_mask_overlap(pred, gt, b)
    metric = DeviceMaskMeanAveragePrecision(num_labels=int(cls[9].shape[-1]))
    thrs, areas = metric._constants(dev)
    gl = labels_gt.to(torch.int32)
    result['kernels'] = {
        'shape': {'images': b, 'queries': q, 'gt_slots': int(ga.shape[1]), 'grid': [int(gt.h), int(gt.w)],
                  'words': int(gt.words.shape[1]), 'non_empty_gt': int((ga > 0).sum())},
        'k21_extract_masks_call': events_ms(extract),
        'k29a_pairwise_mask_overlap_call': events_ms(lambda: ops.pairwise_mask_overlap(pred, gt, b)),
        'k29b_coco_match_call': events_ms(lambda: ops.coco_match(inter, pa, ga, scores, pred_labels, gl, metric.num_labels,
                                                                  thrs, areas, 100)),
    }
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
