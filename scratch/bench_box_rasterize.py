#!/usr/bin/env python3
"""K24 at 800 x 800, B = 4, 20 boxes per frame (the KITTI configuration: [0, 80] x [-40, 40] m on 0.1 m cells), next to a
``torch.zeros`` of the same (4, 800, 800) int32 tensor in the same run, the two alternating.  HIP events around eager
calls, 200 runs each after 20 warm-up runs; also ``KittiRasterizer.rasterize_batch`` (host corners + upload + launch).
Prints one JSON object; --out writes it to a file as well.

    python scratch/bench_box_rasterize.py [--runs 200] [--out bench_box_rasterize.json]
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

from mask_bev_amd import ops_rasterize, rasterize      # noqa: E402


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(ms[0]), 'p90_ms': float(ms[int(0.9 * (len(ms) - 1))]), 'max_ms': float(ms[-1])}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(24)
    batch, per_frame = 4, 20
    r = rasterize.KittiRasterizer((0, 80), (-40, 40), (-3, 1), 0.1, device=dev)
    boxes = [np.column_stack([rng.uniform(2, 78, per_frame), rng.uniform(-38, 38, per_frame), np.full(per_frame, -1.0),
                              rng.uniform(3.5, 4.5, per_frame), rng.uniform(1.6, 2.0, per_frame), np.full(per_frame, 1.5),
                              rng.uniform(-np.pi, np.pi, per_frame)]) for _ in range(batch)]
    verts = torch.from_numpy(np.concatenate([rasterize.box_vertices(b, r.x_range, r.y_range, r.nx, r.ny) for b in boxes])).to(dev)
    ids = torch.from_numpy(np.tile(np.arange(1, per_frame + 1, dtype=np.int32), batch)).to(dev)
    offs = torch.arange(0, batch * per_frame + 1, per_frame, dtype=torch.int32, device=dev)
    out = torch.empty((batch, r.nx, r.ny), dtype=torch.int32, device=dev)
    fns = {'mbv_rasterize_boxes': lambda: ops_rasterize.rasterize_boxes(verts, ids, offs, r.nx, r.ny, out=out),
           'torch_zeros': lambda: torch.zeros((batch, r.nx, r.ny), dtype=torch.int32, device=dev),
           'rasterize_batch': lambda: r.rasterize_batch(boxes)}
    for _ in range(20):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    wall = {k: [] for k in fns}
    for _ in range(args.runs):
        for k, fn in fns.items():                       # alternating: the same machine state for all three
            e, w = timed(fn)
            ev[k].append(e)
            wall[k].append(w)
    painted = int((out > 0).sum())
    res = {'shape': [batch, r.nx, r.ny], 'boxes_per_frame': per_frame, 'runs': args.runs, 'painted_cells': painted,
           'output_bytes': out.numel() * 4, 'device': torch.cuda.get_device_name(0),
           **{k: {'device': stats(ev[k]), 'host_wall': stats(wall[k])} for k in fns}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
