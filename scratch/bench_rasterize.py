#!/usr/bin/env python3
"""K22 timing (a measurement helper; bench.py is the product benchmark): a 5 M-point scene (4 scans, 3 % labelled, ~60
instances) on a 500 x 500 grid.  K22a (binning) and K22b (morphology + paint) are timed separately with device events
after warm-up, median of --iters, next to the numpy / scipy restatement (tests/rasterize_ref.py) on the labelled points
of the same scene, with the thread count it ran on.  Prints one JSON line.

    python scratch/bench_rasterize.py [--iters 30] [--points 5000000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mask_bev_amd import ops  # noqa: E402
from tests import rasterize_ref as RR  # noqa: E402
from tests.test_k22_rasterize_gpu import BIG, make_big_scene  # noqa: E402


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--points', type=int, default=5_000_000)
    ap.add_argument('--max-instances', type=int, default=1024)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a CPU run says nothing about these times'
    dev = torch.device('cuda:0')
    vs = 0.16
    points, inst, tfs = make_big_scene(dev, args.points)
    pts, lab = torch.cat(points), torch.cat(inst)
    offs = torch.tensor(np.concatenate([[0], np.cumsum([p.shape[0] for p in points])]), dtype=torch.int32, device=dev)
    tf = torch.from_numpy(tfs).to(dev)
    nx, ny = RR.grid_size(BIG[0], vs), RR.grid_size(BIG[1], vs)
    n = int(lab.numel())
    n_lab = int((lab != 0).sum())
    res = {'points': n, 'labelled': n_lab, 'grid': [nx, ny], 'max_instances': args.max_instances, 'iters': args.iters}
    for f64 in (False, True):
        p = pts.double() if f64 else pts
        state = {}

        def run(phases):
            m, _, ws = ops.rasterize_scene(p, lab, offs, tf, None, *BIG, vs, nx, ny, 9, 1, args.max_instances, phases,
                                           out=state.get('out'), workspace=state.get('ws'))
            state['out'], state['ws'] = m, ws
        run(3)
        key = 'f64' if f64 else 'f32'
        res[f'{key}_k22a_ms'] = timed(lambda: run(1), args.iters)
        res[f'{key}_k22b_ms'] = timed(lambda: run(2), args.iters)
        res[f'{key}_whole_ms'] = timed(lambda: run(3), args.iters)
        # what K22a has to read: the label stream twice (presence pass + binning pass) and the labelled points twice
        elem = 8 if f64 else 4
        need = 2 * (4 * n + 4 * elem * n_lab)
        res[f'{key}_k22a_bytes_needed'] = need
        res[f'{key}_k22a_fraction_of_8TBps'] = need / (res[f'{key}_k22a_ms'][0] * 1e-3) / 8e12
        # the same scene read in full once (labels + every point), the figure a one-pass streaming kernel would be held to
        res[f'{key}_scene_bytes'] = (4 + 4 * elem) * n
    res['instances'] = int(torch.unique(state['out']).numel()) - 1
    lab_pts = [q[i != 0].cpu().numpy() for q, i in zip(points, inst)]
    lab_ids = np.concatenate([i[i != 0].cpu().numpy() for i in inst])
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = RR.get_mask_around(RR.aggregate_scene(lab_pts, tfs), lab_ids, np.eye(4), *BIG, vs)
        cpu.append((time.perf_counter() - t0) * 1e3)
    res['cpu_restatement_labelled_points_only_ms'] = statistics.median(cpu)
    res['cpu_threads'] = int(os.environ.get('OMP_NUM_THREADS', 0)) or torch.get_num_threads()
    res['equal_to_restatement'] = bool(np.array_equal(state['out'].cpu().numpy(), want))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
