"""K33 measurement: the tracker step (ops.track_frames) and ops.tube_accumulate per frame at the 512 x 512 / 100-query and the
1024 x 1024 / 300-query shape, the numpy restatement on the same arrays, and predict + lift for scale.  Prints one JSON line and
writes it to the path given as the first argument (default: k33_measure.json beside this file)."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mask_bev_amd import ops, synthetic                                   # noqa: E402
from mask_bev_amd.mask_bev_module import MaskBevModule                    # noqa: E402
from tests import track_ref as R                                          # noqa: E402

dev = torch.device('cuda:0')
FRAMES = 8


def timed(fn, iters, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return ms


def stats(ms, **extra):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), **extra)


def shape(workload, p):
    """A sequence of FRAMES maps: car-sized boxes fixed in the world, the ego moving two cells per frame along x, every fifth
    box missed in every other frame, the query indices permuted per frame."""
    w = synthetic.WORKLOADS[workload]
    vs, q = w['voxel_size'], w['num_queries']
    n = int((w['x_range'][1] - w['x_range'][0]) / vs)
    gen = torch.Generator(device=dev).manual_seed(33)
    _, masks = synthetic.gt_masks(1, q, n, n, gen, dev, k_range=(min(40, q), min(40, q)), cell=vs)
    ids = torch.arange(1, q + 1, device=dev, dtype=torch.float32).view(1, q, 1, 1)
    world = (masks * ids).amax(1)[0].to(torch.int64) - 1                  # (n, n), -1 = none
    maps, gts = [], []
    for k in range(FRAMES):
        m = torch.roll(world, -2 * k, 1)
        gts.append(m.clone())
        if k % 2:
            m = torch.where(m % 5 == 4, torch.full_like(m, -1), m)
        perm = torch.randperm(q, generator=gen, device=dev)
        maps.append(torch.where(m >= 0, perm[m.clamp(min=0)], m).to(torch.int32))
    maps = torch.stack(maps).contiguous()
    # the current cell centre lies two cells further along x in the previous frame
    tf = torch.tensor([[1.0, 0.0, 2 * vs], [0.0, 1.0, 0.0]], dtype=torch.float64, device=dev).repeat(FRAMES, 1, 1).contiguous()
    x_lo, y_lo = float(w['x_range'][0]), float(w['y_range'][0])
    state = ops.TrackState.fresh(n, n, p, dev)

    def run_all():
        return ops.track_frames(maps, tf, state, x_lo, y_lo, vs, q, track_map=True)

    def run_one():
        return ops.track_frames(maps[:1], tf[:1], state, x_lo, y_lo, vs, q)

    first = run_all()
    torch.cuda.synchronize()
    host_state = R.fresh_state(n, n, p)
    t_np, equal = [], True
    hm, ht = maps.cpu().numpy(), tf.cpu().numpy()
    for k in range(FRAMES):
        t0 = time.perf_counter()
        qt, _ = R.step(host_state, hm[k], ht[k], x_lo, y_lo, vs, q, 0.3, 2, 4)
        t_np.append((time.perf_counter() - t0) * 1e3)
        equal = equal and np.array_equal(qt, first.query_track[k].cpu().numpy())
    equal = equal and np.array_equal(host_state['state_map'], state.state_map.cpu().numpy())
    counters = state.counters.cpu().tolist()
    all_ms = [v / FRAMES for v in timed(run_all, 20, 7, 5)]
    one_ms = timed(run_one, 100, 7, 10)
    # tube association with the cells of one frame as the elements
    track = first.track_map[FRAMES - 1].reshape(-1).contiguous()
    gt = gts[FRAMES - 1].reshape(-1)
    words = torch.where(gt >= 0, ((gt + 1) << 16) | 10, torch.full_like(gt, 40)).to(torch.int32).contiguous()
    lut = torch.zeros(64, dtype=torch.int32, device=dev)
    lut[10] = 1
    tables = ops.TubeTables.zeros(2, 1024, 4096, dev)
    tube_ms = timed(lambda: ops.tube_accumulate(track, words, lut, tables), 100, 7, 10)
    score_ms = timed(lambda: ops.tube_scores(tables), 50, 5, 5)
    ref_tables = R.fresh_tables(2, 1024, 4096)
    hp, hw_, hl = track.cpu().numpy(), words.cpu().numpy(), lut.cpu().numpy()
    t_tube = []
    for _ in range(3):
        t0 = time.perf_counter()
        R.tube_accumulate(ref_tables, hp, hw_, hl, 2, 1024, 4096)
        t_tube.append((time.perf_counter() - t0) * 1e3)
    return dict(grid=[n, n], queries=q, max_tracks=p, frames=FRAMES, counters_after_first_pass=counters,
                cells_in_instances=float((maps >= 0).float().mean()), equals_restatement=bool(equal),
                track_frame_ms_in_one_call_of_8=stats(all_ms, iters=20, reps=7),
                track_frame_ms_one_call_per_frame=stats(one_ms, iters=100, reps=7),
                tube_accumulate_ms=stats(tube_ms, iters=100, reps=7, elements=int(track.numel())),
                tube_scores_ms=stats(score_ms, iters=50, reps=5, rows=1024, tracks=4096),
                numpy_step_ms=stats(t_np, reps=FRAMES), numpy_tube_accumulate_ms=stats(t_tube, reps=3))


res = dict(shapes={'semantic_kitti_512': shape('semantic_kitti_512', 256), 'waymo_1024': shape('waymo_1024', 1024)})

B = 4
kw = synthetic.module_kwargs('semantic_kitti_512', B, 'bf16')
torch.manual_seed(0)
model = MaskBevModule(**kw).to(dev)
model.log_scalars = False
gen = torch.Generator(device=dev).manual_seed(32)
scans = [synthetic.lidar_scan(120000, 4, gen, dev) for _ in range(B)]


def predict_lift():
    p = model.predict(scans)
    return p.lift(scans, model)


res['predict_plus_lift_ms_per_batch_of_4'] = stats(timed(predict_lift, 10, 5, 3), iters=10, reps=5)
target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'k33_measure.json')
with open(target, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
