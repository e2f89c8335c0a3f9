#!/usr/bin/env python3
"""K28 at the KITTI workload: 4 scans of ~120 000 points, 10 labelled boxes and 14 pasted samples of ~300 points per scan,
every box perturbed.  Three figures, each the median of 5 timed runs after 3 warm-up runs: the object stage alone
(``mbv_object_augment``, HIP events), K23 alone on the same batch (the reference's configuration-01 point list with every
transform firing), and the numpy restatement of the object stage on the host (tests/object_augment_ref.py).  Prints one
JSON object; --out writes it to a file as well.

    python scratch/bench_object_augment.py [--out bench_object_augment.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mask_bev_amd import augment as A, object_augment as OA, ops_augment    # noqa: E402
from tests import object_augment_ref as OR                                  # noqa: E402

POINT_LIST = [{'name': 'flip', 'prob_flip_x': 0, 'prob_flip_y': 1}, {'name': 'rotate', 'rotate_prob': 1, 'rotation_range': 2.5},
              {'name': 'global_noise', 'prob_aug': 0.5}, {'name': 'drop', 'prob_drop': 1, 'per_point_drop_prob': 0.05},
              {'name': 'shuffle', 'prob_shuffle': 1}, {'name': 'jitter', 'prob_jitter': 1, 'jitter_std': 0.01, 'intensity_std': 0.01}]


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(ms[0]), 'max_ms': float(ms[-1]), 'runs': len(ms)}


def time_device(fn, runs=5, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b))
    return stats(ev)


def grid_boxes(rng, n, x0, pitch=7.0):
    b = np.zeros((n, 7))
    b[:, 0], b[:, 1] = x0 + pitch * (np.arange(n) % 6), pitch * (np.arange(n) // 6) - 14
    b[:, 2], b[:, 3], b[:, 4], b[:, 5] = -1.7, rng.uniform(3.5, 4.5, n), rng.uniform(1.6, 2.0, n), rng.uniform(1.4, 1.7, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--labels', type=int, default=10)
    ap.add_argument('--pasted', type=int, default=14)
    ap.add_argument('--sample-points', type=int, default=300)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_object_augment.py needs an MI355X: a CPU run says nothing about the device')
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    boxes = grid_boxes(rng, args.labels + args.pasted, 5.0)                      # labels first, then the pasted boxes
    bank_boxes = boxes[args.labels:]
    pts = []
    for b in bank_boxes:
        u = rng.uniform(-0.9, 0.9, (args.sample_points, 2)) * [b[3] / 2, b[4] / 2]
        c, s = np.cos(b[6]), np.sin(b[6])
        p = np.stack([b[0] + c * u[:, 0] - s * u[:, 1], b[1] + s * u[:, 0] + c * u[:, 1],
                      b[2] + rng.uniform(0.1, 0.9, args.sample_points) * b[5], rng.uniform(0, 1, args.sample_points)], -1)
        pts.append(p.astype(np.float32))
    bank = OA.ObjectBank(np.concatenate(pts), np.arange(args.pasted + 1) * args.sample_points, bank_boxes)
    scans_np, frames = [], []
    for _ in range(args.batch):
        pc = np.stack([rng.uniform(0, 70, args.points), rng.uniform(-35, 35, args.points), rng.uniform(-3, 1, args.points),
                       rng.uniform(0, 1, args.points)], -1).astype(np.float32)
        scans_np.append(pc)
        f = OA.ObjectFrame(boxes[:args.labels])
        for k in range(args.pasted):
            f.paste(bank, k)
        OA.ObjectNoise().run(rng, f)
        frames.append(f)
    scans = [torch.from_numpy(p).to(dev) for p in scans_np]
    commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    res = {'batch': args.batch, 'points_per_scan': args.points, 'labels_per_scan': args.labels, 'pasted_per_scan': args.pasted,
           'points_per_sample': args.sample_points, 'parent_commit': commit or None, 'device': torch.cuda.get_device_name(0)}

    # the object stage alone: the C entry point on resident buffers
    points = torch.cat(scans)
    tables = torch.from_numpy(np.concatenate([f.table for f in frames])).to(dev)
    scan_offs = np.arange(args.batch + 1) * args.points
    box_offs = np.arange(args.batch + 1) * len(boxes)
    segs = [(int(bank.offsets[k]), int(bank.offsets[k + 1] - bank.offsets[k])) for f in frames for k in f.pasted]
    paste_offs = np.arange(args.batch + 1) * args.pasted
    bank_dev = bank.device_points(dev)

    def stage():
        return ops_augment.object_augment(points, scan_offs, tables, box_offs, bank_dev, segs, paste_offs)
    out, out_offs, _ = stage()
    res['object_stage_device'] = time_device(stage)
    res['rows_out'] = [int(v) for v in np.diff(out_offs.cpu().numpy())]

    # ... with the host work of apply(): tables, upload, the one sync
    aug = A.DeviceAugmentation([], seed=1)
    wall = []
    for _ in range(8):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        OA.run_frames(scans, frames, bank)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res['object_stage_host_wall'] = stats(wall[3:])

    # K23 alone on the same batch
    paug = A.DeviceAugmentation(A.make_kitti_augmentation_list(POINT_LIST), seed=1)
    draws = paug.draw(args.batch)
    res['k23_mode'] = A.batch_mode(draws)
    res['k23_alone_device'] = time_device(lambda: paug.apply(scans, draws=draws))

    # the numpy restatement of the object stage on the host
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        for pc, f in zip(scans_np, frames):
            OR.scan(pc, f.boxes, f.rot, f.loc, f.table[:, 13].astype(np.int64), [bank.sample_points(k) for k in f.pasted])
        host.append((time.perf_counter() - t0) * 1e3)
    res['numpy_restatement_host'] = stats(host)
    want = OR.scan(scans_np[0], frames[0].boxes, frames[0].rot, frames[0].loc, frames[0].table[:, 13].astype(np.int64),
                   [bank.sample_points(k) for k in frames[0].pasted])
    res['first_scan_equals_restatement'] = bool(np.array_equal(out[:len(want)].cpu().numpy().view(np.int32), want.view(np.int32)))
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
