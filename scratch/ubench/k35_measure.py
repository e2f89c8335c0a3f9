"""K35 measurement: K31's lift, K35a's ``mbv_ground_map`` and K35b's ground lift through the C ABI on preallocated buffers, at
the bench shape — B = 4 scans of 120 k points, the ``semantic_kitti_512`` geometry (512 x 512 cells), 100 queries, radius 10.

    python scratch/ubench/k35_measure.py [--root DIR] [--out FILE] [--calls N] [--windows N]

``--root DIR``: import ``mask_bev_amd`` from DIR instead of this tree (a checkout of the parent commit, built there, gives the
parent's K31 time; the K35 entries are skipped where the library lacks them).  Device events around ``--calls`` back-to-back
calls, ``--windows`` windows after a warm-up window; the median window is reported per call.  Prints one JSON line with the
times and the bytes each launch must move (computed from the shapes).  Per-kernel times: run it under
``rocprofv3 --kernel-trace --stats -- python scratch/ubench/k35_measure.py --calls 20 --windows 2``."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

parser = argparse.ArgumentParser()
parser.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
parser.add_argument('--out', default=None)
parser.add_argument('--calls', type=int, default=200)
parser.add_argument('--windows', type=int, default=9)
args = parser.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

from mask_bev_amd import _lib                                              # noqa: E402
from mask_bev_amd.ops_core import _ptr, _stream                            # noqa: E402

B, N, DIM, Q, Z_BINS, RADIUS = 4, 120_000, 4, 100, 64, 10
RANGE, VS = [-40.0, -40.0, -3.0, 40.0, 40.0, 1.0], 0.15625
GRID = [512, 512, 1]
VOXEL = [VS, VS, 4.0]
dev = torch.device('cuda:0')
lib = _lib.load()


def scene(seed):
    """Seeded scans: 85 % road returns at z = -1.7 +- 0.05 with range-like density (more near the sensor), 15 % object returns
    over 40 car-sized boxes per scan; the instance map: those boxes grown by 3 cells."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((B, N, DIM), dtype=np.float32)
    imap = np.full((B, GRID[1], GRID[0]), -1, dtype=np.int32)
    for b in range(B):
        n_obj = N * 15 // 100
        r, phi = 42.0 * rng.uniform(0, 1, N - n_obj) ** 1.5, rng.uniform(0, 2 * np.pi, N - n_obj)
        pts[b, n_obj:, 0], pts[b, n_obj:, 1] = r * np.cos(phi), r * np.sin(phi)
        pts[b, n_obj:, 2] = rng.uniform(-1.75, -1.65, N - n_obj)
        centres = rng.uniform(-35, 35, (40, 2))
        which = rng.integers(0, 40, n_obj)
        half = np.where(rng.uniform(0, 1, (40, 1)) < 0.5, [[2.2, 0.9]], [[0.9, 2.2]])
        pts[b, :n_obj, :2] = centres[which] + rng.uniform(-1, 1, (n_obj, 2)) * half[which]
        pts[b, :n_obj, 2] = rng.uniform(-1.3, -0.2, n_obj)
        pts[b, :, 3] = rng.uniform(0, 1, N)
        for k in range(40):
            lo = np.floor((centres[k] - half[k] - RANGE[0:2]) / VS).astype(int) - 3
            hi = np.ceil((centres[k] + half[k] - RANGE[0:2]) / VS).astype(int) + 3
            imap[b, max(lo[1], 0):hi[1], max(lo[0], 0):hi[0]] = k
        pts[b] = pts[b][rng.permutation(N)]
    return pts.reshape(B * N, DIM), imap


def timed(fn):
    ms = []
    for w in range(args.windows + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if w:                                                             # window 0 is the warm-up
            ms.append(e0.elapsed_time(e1) / args.calls)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), calls=args.calls, windows=args.windows)


points_np, imap_np = scene(35)
points = torch.from_numpy(points_np).to(dev)
imap = torch.from_numpy(imap_np).to(dev)
offsets = torch.arange(0, B + 1, dtype=torch.int32, device=dev) * N
total = B * N
cells = B * GRID[0] * GRID[1]
point_query = torch.empty((total,), dtype=torch.int32, device=dev)
counts = torch.empty((B, Q), dtype=torch.int32, device=dev)
z_extent = torch.empty((B, Q, 4), dtype=torch.float32, device=dev)
ws_lift = torch.empty((lib.mbv_lift_instances_workspace_bytes(B, Q, Z_BINS),), dtype=torch.uint8, device=dev)
geometry = (*RANGE, *VOXEL, *GRID, 1)
stream = _stream()


def k31():
    rc = lib.mbv_lift_instances(_ptr(points), DIM, total, _ptr(offsets), B, *geometry, _ptr(imap), Q, Z_BINS, 0.0, 1.0,
                                _ptr(point_query), _ptr(counts), _ptr(z_extent), _ptr(ws_lift), ws_lift.numel(), stream)
    assert rc == 0, rc


result = dict(root=os.path.abspath(args.root), device=torch.cuda.get_device_name(0), batch=B, points_per_scan=N, grid=GRID[:2],
              queries=Q, radius=RADIUS, k31_lift=timed(k31))
k31()
labelled_plain = int((point_query >= 0).sum())
pt_bytes, pq_bytes, hist_bytes = total * DIM * 4, total * 4, B * Q * Z_BINS * 4
result['k31_lift']['bytes'] = dict(init=pq_bytes + hist_bytes, points=pt_bytes + pq_bytes + total * 4, finalize=hist_bytes)

if hasattr(lib, 'mbv_ground_map'):
    cell_min = torch.empty((B, GRID[1], GRID[0]), dtype=torch.float32, device=dev)
    ground = torch.empty_like(cell_min)
    z_ground = torch.empty((B, Q), dtype=torch.float32, device=dev)
    ws_ground = torch.empty((lib.mbv_ground_map_workspace_bytes(B, GRID[0], GRID[1]),), dtype=torch.uint8, device=dev)
    ws_gl = torch.empty((lib.mbv_lift_instances_ground_workspace_bytes(B, Q, Z_BINS),), dtype=torch.uint8, device=dev)

    def k35a():
        rc = lib.mbv_ground_map(_ptr(points), DIM, total, _ptr(offsets), B, *geometry, RADIUS, float('-inf'), _ptr(cell_min),
                                _ptr(ground), _ptr(ws_ground), ws_ground.numel(), stream)
        assert rc == 0, rc

    def k35b():
        rc = lib.mbv_lift_instances_ground(_ptr(points), DIM, total, _ptr(offsets), B, *geometry, _ptr(imap), Q, Z_BINS, 0.0, 1.0,
                                           _ptr(ground), 0.3, float('inf'), _ptr(point_query), _ptr(counts), _ptr(z_extent),
                                           _ptr(z_ground), _ptr(ws_gl), ws_gl.numel(), stream)
        assert rc == 0, rc

    def both():
        k35a()
        k35b()

    result['k35a_ground_map'] = timed(k35a)
    result['k35b_ground_lift'] = timed(k35b)
    result['k35a_then_k35b'] = timed(both)
    result['k31_lift_again'] = timed(k31)                                 # the spread of the baseline inside this process
    both()
    plane = cells * 4
    result['k35a_ground_map']['bytes'] = dict(init=plane, points=pt_bytes + total * 4, rows=plane + 2 * plane, cols=2 * plane)
    result['k35b_ground_lift']['bytes'] = dict(init=pq_bytes + hist_bytes, points=pt_bytes + pq_bytes + 2 * total * 4,
                                               finalize=hist_bytes)
    result['occupied_cells'] = int(torch.isfinite(cell_min).sum())
    result['cells'] = cells
    result['labelled_plain'], result['labelled_ground'] = labelled_plain, int((point_query >= 0).sum())

line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
