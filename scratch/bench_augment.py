#!/usr/bin/env python3
"""K23 at the bench batch: 4 x 120 000-point scans, 500 x 500 instance maps, the reference's
01_point_mask_data_aug_gentle list with every transform firing (shuffle off, as that file has it; once more with it on).
HIP events around eager calls, 200 runs after 20 warm-up runs; the numpy restatement (tests/augment_ref.py) timed on the
host in the same run.  Prints one JSON object; --out writes it to a file as well.

    python scratch/bench_augment.py [--runs 200] [--out bench_augment.json]
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

from mask_bev_amd import augment as A      # noqa: E402
from tests import augment_ref as AR        # noqa: E402

GENTLE = [{'name': 'drop', 'prob_drop': 1, 'per_point_drop_prob': 0.05}, {'name': 'flip', 'prob_flip_x': 0, 'prob_flip_y': 1},
          {'name': 'shuffle', 'prob_shuffle': 0}, {'name': 'rotate', 'rotate_prob': 1, 'rotation_range': 5},
          {'name': 'jitter', 'prob_jitter': 1, 'jitter_std': 0.02, 'intensity_std': 0.01}]


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(ms[0]), 'p90_ms': float(ms[int(0.9 * (len(ms) - 1))]), 'max_ms': float(ms[-1])}


def time_device(fn, runs, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return {'device': stats(ev), 'host_wall': stats(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=200)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--grid', type=int, default=500)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_augment.py needs an MI355X: a CPU run says nothing about the device')
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    half = args.grid * 0.16 / 2
    scans_np = []
    for _ in range(args.batch):
        pc = rng.uniform(-half, half, (args.points, 4)).astype(np.float32)
        pc[:, 2] = rng.uniform(-3, 1, args.points)
        pc[:, 3] = rng.uniform(0, 1, args.points)
        scans_np.append(pc)
    maps_np = (rng.integers(0, 40, (args.batch, args.grid, args.grid)) * (rng.random((args.batch, args.grid, args.grid)) < 0.05)).astype(np.int32)
    scans = [torch.from_numpy(p).to(dev) for p in scans_np]
    maps = torch.from_numpy(maps_np).to(dev)
    res = {'batch': args.batch, 'points_per_scan': args.points, 'grid': args.grid, 'runs': args.runs}

    def variant(spec, seed):
        aug = A.DeviceAugmentation(A.make_semantic_kitti_augmentation_list(spec), seed, (-half, half), (-half, half), 0.16)
        draws = aug.draw(args.batch)
        return aug, draws

    no_removal = [dict(GENTLE[0], prob_drop=0)] + GENTLE[1:]
    with_shuffle = GENTLE[:2] + [dict(GENTLE[2], prob_shuffle=1)] + GENTLE[3:]
    for name, spec in (('all_ops_drop_compaction', GENTLE), ('no_removal', no_removal), ('all_ops_with_shuffle_sort', with_shuffle)):
        aug, draws = variant(spec, 1)
        res[name] = time_device(lambda: aug.apply(scans, instance_maps=maps, draws=draws), args.runs)
        res[name]['mode'] = A.batch_mode(draws)
        res[name]['including_host_draw'] = time_device(lambda: aug.apply(scans, instance_maps=maps), args.runs)['host_wall']
    # the pieces of the all-ops path
    aug, draws = variant(GENTLE, 1)
    from mask_bev_amd import ops
    points = torch.cat(scans)
    offs = torch.tensor(np.arange(args.batch + 1) * args.points, dtype=torch.int32, device=dev)
    for mode, spec in ((0, no_removal), (1, GENTLE), (2, with_shuffle)):
        _, d = variant(spec, 1)
        rec = torch.from_numpy(A.pack_records(d).view(np.uint8).reshape(-1)).to(dev)
        ws = torch.empty(max(256, ops._lib.load().mbv_augment_workspace_bytes(points.shape[0], args.batch, mode)), dtype=torch.uint8, device=dev)
        res[f'mbv_augment_points_mode{mode}'] = time_device(lambda: ops.augment_points(points, offs, rec, mode, ws), args.runs)['device']
    mats = torch.from_numpy(np.stack([d.matrix for d in draws])).to(dev)
    res['mbv_warp_instance_maps'] = time_device(lambda: ops.warp_instance_maps(maps, mats, args.grid / 2, args.grid / 2), args.runs)['device']
    # the numpy restatement on the host (points + maps), 5 runs
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        AR.augment_batch(scans_np, [(d.seed, list(d.ops)) for d in draws])
        for b, d in enumerate(draws):
            AR.warp(maps_np[b], d.matrix, args.grid / 2, args.grid / 2)
        host.append((time.perf_counter() - t0) * 1e3)
    res['numpy_restatement_host'] = stats(host)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
