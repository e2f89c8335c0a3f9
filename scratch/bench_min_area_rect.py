#!/usr/bin/env python3
"""K30a + K30b next to K25 (``fit_boxes``) on the same rows, at the KITTI shape: a 496 x 432 (ny, nx) grid
([0, 69.12] x [-39.68, 39.68] m on 0.16 m cells), 200 queries.  The kept rows are the car-like boxes of the committed sample
label (tests/golden/kitti_object_sample) painted by K24 and packed by K14, each with two stray cells set far from the car (so
the bounding box K30a repacks is most of the map and its planes live in the workspace); ``--clean`` leaves the strays out
(planes in LDS).  Two row sets: the kept rows alone, and all 200 rows (the rest are empty maps).  HIP events around eager
calls, the three alternating in the same run, ``--runs`` each after 20 warm-up runs.  Prints one JSON object; --out writes it
to a file as well.

    python scratch/bench_min_area_rect.py [--runs 200] [--clean] [--out bench_min_area_rect.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mask_bev_amd import batch as B, ops, rasterize      # noqa: E402

SAMPLE = os.path.join(ROOT, 'tests', 'golden', 'kitti_object_sample')


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {'median_us': float(np.median(ms)) * 1e3, 'min_us': float(ms[0]) * 1e3, 'p90_us': float(ms[int(0.9 * (len(ms) - 1))]) * 1e3}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=200)
    ap.add_argument('--clean', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X')
    dev = torch.device('cuda', 0)
    x_range, y_range, vs, q = (0, 69.12), (-39.68, 39.68), 0.16, 200
    lab = B.kitti_labels_to_velodyne(B.read_kitti_label(os.path.join(SAMPLE, 'label_2', '000000.txt')),
                                     B.read_kitti_calib(os.path.join(SAMPLE, 'calib', '000000.txt')))
    r = rasterize.KittiRasterizer(x_range, y_range, (-3, 1), vs, device=dev)
    car_like = np.isin(lab['type'], rasterize.KITTI_CAR_LIKE) & B.object_range_mask(lab['boxes'], x_range, y_range)
    labels, pm = B.instance_targets(r.rasterize_batch([lab['boxes'][car_like]]), q, packed=True)
    kept = torch.nonzero(labels.reshape(-1)).flatten()
    h, w = pm.h, pm.w
    if not args.clean:
        for p in (2 * w + (w - 4), (h - 3) * w + 3):                   # cells (2, w - 4) and (h - 3, 3) of every kept map
            pm.words[kept, p // 32] |= (1 << (p % 32))
    every = torch.arange(pm.words.shape[0], device=dev)
    res = {'grid_hw': [h, w], 'queries': q, 'kept_rows': int(kept.numel()), 'strays': not args.clean, 'runs': args.runs,
           'device': torch.cuda.get_device_name(0)}
    for tag, rows in (('kept_rows', kept), ('all_rows', every)):
        ar = torch.arange(rows.numel(), device=dev)
        state = {}

        def k30a():
            state['kept'] = ops.largest_component(pm, rows)

        fns = {'fit_boxes': lambda: ops.fit_boxes(pm, rows), 'largest_component': k30a,
               'min_area_boxes': lambda: ops.min_area_boxes(state['kept'][0], ar)}
        for _ in range(20):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ev = {k: [] for k in fns}
        for _ in range(args.runs):
            for k, fn in fns.items():                                  # alternating: the same machine state for all three
                ev[k].append(timed(fn))
        res[tag] = {k: stats(v) for k, v in ev.items()}
        res[tag]['cells'] = ops.fit_boxes(pm, rows)[0].tolist()[:8]
        res[tag]['kept_cells'] = state['kept'][1].tolist()[:8]
        res[tag]['components'] = state['kept'][2].tolist()[:8]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
