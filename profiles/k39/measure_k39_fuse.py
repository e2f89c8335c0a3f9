"""K39 (footprint fusion) next to K33a's tracker step, device events, one process: python profiles/k39/measure_k39_fuse.py
[--out FILE]  (--trace-grid N: a few calls only, to run under a kernel trace).  Per grid (500 x 500 and 1024 x 1024, Q = 100,
8 frames per call, a driving and turning ego over world-fixed rectangles, a third of the cells unseen): `ops.track_frames`
(K33a), `ops.fuse_frames` (K39a, with visibility; with and without the query map) and `ops.masks_from_map` (K39b), each in 7
windows of 10 calls after 3 warm-up calls, the four paths in turn; then the same again in the reverse order: 14 windows per
path.  Microseconds per frame, median (min - max) over the 14."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mask_bev_amd import ops                                           # noqa: E402

F, Q, WINDOWS, CALLS, WARMUP = 8, 100, 7, 10, 3


def pose(x, y, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, x], [s, c, y], [0.0, 0.0, 1.0]])


def scene(g, voxel, rng):
    """(maps (F, g, g) int32, prev_from_cur, world_from_cur, cur_from_world (F, 2, 3) f64, visibility (F, g, g) uint8)"""
    half = g * voxel / 2
    rects = [(rng.uniform(-half, half - 5), rng.uniform(-half, half - 3)) for _ in range(Q)]
    ix, iy = np.meshgrid(np.arange(g), np.arange(g))
    x, y = -half + (ix + 0.5) * voxel, -half + (iy + 0.5) * voxel
    maps, ms, wm, wn, prev = [], [], [], [], None
    for k in range(F):
        p = pose(1.0 * k, 0.2 * k, 0.03 * k)
        wx, wy = p[0, 0] * x + p[0, 1] * y + p[0, 2], p[1, 0] * x + p[1, 1] * y + p[1, 2]
        im = np.full((g, g), -1, np.int32)
        for q, (x0, y0) in enumerate(rects):
            im[(wx >= x0) & (wx < x0 + 4.5) & (wy >= y0) & (wy < y0 + 2.0)] = q
        maps.append(im)
        ms.append(np.eye(3)[:2] if prev is None else (np.linalg.inv(prev) @ p)[:2])
        wm.append(p[:2])
        wn.append(np.linalg.inv(p)[:2])
        prev = p
    vis = (rng.random((F, g, g)) > 0.33).astype(np.uint8)
    return np.stack(maps), np.stack(ms), np.stack(wm), np.stack(wn), vis


def windows(fn, reset):
    out = []
    for _ in range(WINDOWS):
        reset()
        for _ in range(WARMUP):
            fn()
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / (CALLS * F))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace-grid', type=int, default=0, help='only 3 calls each of K33a, K39a and K39b at this grid, for a kernel trace')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    if args.trace_grid:
        g, voxel = args.trace_grid, 0.16
        maps, ms, wm, wn, vis = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in scene(g, voxel, np.random.default_rng(g)))
        lo = -g * voxel / 2
        track, fuse = ops.TrackState.fresh(g, g, 256, dev), ops.FusionState.fresh(g, g, dev)
        for _ in range(3):
            qt = ops.track_frames(maps, ms, track, lo, lo, voxel, Q).query_track
            fused = ops.fuse_frames(maps, qt, wm, wn, fuse, lo, lo, voxel, visibility=vis)
            ops.masks_from_map(fused.queries, Q)
        torch.cuda.synchronize()
        return 0
    result = dict(device=torch.cuda.get_device_name(0), frames_per_call=F, queries=Q, windows_per_round=WINDOWS, rounds=2,
                  windows_per_path=2 * WINDOWS, calls_per_window=CALLS, grids={})
    for g, voxel in ((500, 0.16), (1024, 0.16)):
        rng = np.random.default_rng(g)
        maps, ms, wm, wn, vis = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in scene(g, voxel, rng))
        lo = -g * voxel / 2
        track = {'state': None}
        fuse = {'state': None}

        def reset_track():
            track['state'] = ops.TrackState.fresh(g, g, 256, dev)

        def reset_fuse():
            fuse['state'] = ops.FusionState.fresh(g, g, dev)

        reset_track()
        qt = ops.track_frames(maps, ms, track['state'], lo, lo, voxel, Q).query_track
        reset_fuse()
        fused = ops.fuse_frames(maps, qt, wm, wn, fuse['state'], lo, lo, voxel, visibility=vis)
        torch.cuda.synchronize()
        rows = {}
        order = [('k33a_track_frames', lambda: ops.track_frames(maps, ms, track['state'], lo, lo, voxel, Q), reset_track),
                 ('k39a_fuse_frames', lambda: ops.fuse_frames(maps, qt, wm, wn, fuse['state'], lo, lo, voxel, visibility=vis), reset_fuse),
                 ('k39a_fuse_frames_ids_only', lambda: ops.fuse_frames(maps, qt, wm, wn, fuse['state'], lo, lo, voxel, visibility=vis,
                                                                       queries=False), reset_fuse),
                 ('k39b_masks_from_map', lambda: ops.masks_from_map(fused.queries, Q), lambda: None)]
        for name, fn, reset in order + order[::-1]:                     # every path twice, the second round in reverse order
            rows.setdefault(name, []).extend(windows(fn, reset))
        s = int(fuse['state'].owner.shape[0])
        result['grids'][f'{g}x{g}'] = dict(
            store_side=s, store_bytes_moved_per_frame_model=16 * s * s, owned_cells_last_frame=int((fused.ids[-1] >= 0).sum()),
            detected_cells_last_frame=int((maps[-1] >= 0).sum()),
            us_per_frame={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in rows.items()})
        for k, v in rows.items():
            print(f'{g}x{g} {k}: {np.median(v):.2f} us/frame ({np.min(v):.2f} - {np.max(v):.2f})', flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
