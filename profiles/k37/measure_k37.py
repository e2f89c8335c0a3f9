"""K37 measurement: the tracker step with the motion model (ops.track_frames(motion=...)) against the step without it
(motion=None, K33a's path) per frame at the 512 x 512 / 100-query and the 1024 x 1024 / 300-query shape of
profiles/k33/measure_k33.py, a third of the boxes moving.  Both are timed in the same process in alternating windows: device
events around 20 calls of 8 frames, 5 warm-up calls, 7 windows each.  Prints one JSON line and writes it to the path given as
the first argument (default: k37_measure.json beside this file).

``--off-only --package-root DIR`` times only the step without the motion model, on the same maps with the same loop, with the
package of another checkout (the parent commit's, built there): the baseline the motion-off numbers are held against."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
OFF_ONLY = '--off-only' in sys.argv
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if '--package-root' in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index('--package-root') + 1])
    ARGS.remove(sys.argv[sys.argv.index('--package-root') + 1])
sys.path.insert(0, ROOT)

from mask_bev_amd import ops, synthetic                                   # noqa: E402
if not OFF_ONLY:
    from tests import track_motion_ref as M                               # noqa: E402

dev = torch.device('cuda:0')
FRAMES, ITERS, WINDOWS, WARM = 8, 20, 7, 5


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stats(ms, **extra):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), spread_pct=100.0 * (max(ms) - min(ms)) / statistics.median(ms),
                **extra)


def moved_left(x, cells):
    """x moved by `cells` columns towards -x; what leaves the grid is gone (no wrap-around: a box split between two edges
    would have its centroid in the middle of the grid)."""
    out = torch.full_like(x, -1)
    out[:, :x.shape[1] - cells] = x[:, cells:]
    return out


def shape(workload, p):
    """A sequence of FRAMES maps: car-sized boxes, the ego moving two cells per frame along x; every third box drives three
    more cells per frame along x, every fifth box is missed in every other frame, the query indices are permuted per frame."""
    w = synthetic.WORKLOADS[workload]
    vs, q = w['voxel_size'], w['num_queries']
    n = int((w['x_range'][1] - w['x_range'][0]) / vs)
    gen = torch.Generator(device=dev).manual_seed(33)
    _, masks = synthetic.gt_masks(1, q, n, n, gen, dev, k_range=(min(40, q), min(40, q)), cell=vs)
    ids = torch.arange(1, q + 1, device=dev, dtype=torch.float32).view(1, q, 1, 1)
    world = (masks * ids).amax(1)[0].to(torch.int64) - 1                  # (n, n), -1 = none
    moving = (world >= 0) & (world % 3 == 0)
    still, mover = torch.where(moving, torch.full_like(world, -1), world), torch.where(moving, world, torch.full_like(world, -1))
    maps = []
    for k in range(FRAMES):
        a, b = moved_left(still, 2 * k), moved_left(mover, 5 * k)
        m = torch.where(b >= 0, b, a)
        if k % 2:
            m = torch.where(m % 5 == 4, torch.full_like(m, -1), m)
        perm = torch.randperm(q, generator=gen, device=dev)
        maps.append(torch.where(m >= 0, perm[m.clamp(min=0)], m).to(torch.int32))
    maps = torch.stack(maps).contiguous()
    tf = torch.tensor([[1.0, 0.0, 2 * vs], [0.0, 1.0, 0.0]], dtype=torch.float64, device=dev).repeat(FRAMES, 1, 1).contiguous()
    x_lo, y_lo = float(w['x_range'][0]), float(w['y_range'][0])
    off_state = ops.TrackState.fresh(n, n, p, dev)
    if OFF_ONLY:
        run = lambda: ops.track_frames(maps, tf, off_state, x_lo, y_lo, vs, q, track_map=True)
        for _ in range(1 + 2 * WARM):
            run()
        torch.cuda.synchronize()
        ms = [window(run, ITERS) / FRAMES for _ in range(2 * WINDOWS)][::2]      # the windows the full run gives this path
        return dict(grid=[n, n], queries=q, max_tracks=p, frames=FRAMES, frame_ms_motion_off=stats(ms, iters=ITERS, windows=WINDOWS))
    inv = ops.invert_transforms(tf)
    settings = ops.MotionSettings()
    on_state = ops.TrackState.fresh(n, n, p, dev)
    on_state.motion = ops.TrackMotion.fresh(p, dev)

    def run_off():
        return ops.track_frames(maps, tf, off_state, x_lo, y_lo, vs, q, track_map=True)

    def run_on():
        return ops.track_frames(maps, tf, on_state, x_lo, y_lo, vs, q, track_map=True, motion=settings, cur_from_prev=inv)

    first_off, first_on = run_off(), run_on()
    torch.cuda.synchronize()
    ids_off, ids_on = off_state.counters.cpu().tolist(), on_state.counters.cpu().tolist()
    gated = on_state.motion.motion_counters.cpu().tolist()[0]
    # the restatement on the same arrays
    host, equal = M.fresh_state(n, n, p), True
    hm, ht, hn = maps.cpu().numpy(), tf.cpu().numpy(), inv.cpu().numpy()
    for k in range(FRAMES):
        qt, _, qv = M.step(host, hm[k], ht[k], hn[k], x_lo, y_lo, vs, q, 0.3, 2, 4, settings.gain, settings.gate_m,
                           settings.max_shift(vs))
        equal = equal and np.array_equal(qt, first_on.query_track[k].cpu().numpy())
        equal = equal and qv.tobytes() == first_on.query_velocity[k].cpu().numpy().tobytes()
    equal = equal and np.array_equal(host['state_map'], on_state.state_map.cpu().numpy())
    equal = equal and host['vel'].tobytes() == on_state.motion.vel.cpu().numpy().tobytes()
    for _ in range(WARM):
        run_off()
        run_on()
    torch.cuda.synchronize()
    off_ms, on_ms = [], []
    for _ in range(WINDOWS):                                              # alternating windows in one process
        off_ms.append(window(run_off, ITERS) / FRAMES)
        on_ms.append(window(run_on, ITERS) / FRAMES)
    return dict(grid=[n, n], queries=q, max_tracks=p, frames=FRAMES, cells_in_instances=float((maps >= 0).float().mean()),
                moving_boxes=int(torch.unique(mover[mover >= 0]).numel()), boxes=int(torch.unique(world[world >= 0]).numel()),
                counters_after_first_pass_motion_off=ids_off, counters_after_first_pass_motion_on=ids_on, gated_in_first_pass=gated,
                equals_restatement=bool(equal),
                frame_ms_motion_off=stats(off_ms, iters=ITERS, windows=WINDOWS),
                frame_ms_motion_on=stats(on_ms, iters=ITERS, windows=WINDOWS),
                ratio_of_medians=statistics.median(on_ms) / statistics.median(off_ms))


res = dict(shapes={'semantic_kitti_512': shape('semantic_kitti_512', 256), 'waymo_1024': shape('waymo_1024', 1024)})
target = ARGS[0] if ARGS else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'k37_measure.json')
with open(target, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
