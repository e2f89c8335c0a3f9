"""K32 measurement: ops.panoptic_frames on 4 scans of ~120 000 points with 45 queries, the numpy restatement on the same data,
and predict + lift for scale.  Prints one JSON line and writes it to the path given as the first argument (default: k32_measure.json beside this file)."""
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
from mask_bev_amd.metrics import semantic_kitti_class_lut                 # noqa: E402
from tests import panoptic_ref as R                                       # noqa: E402

dev = torch.device('cuda:0')
B, Q, POINTS = 4, 45, 120000
w = synthetic.WORKLOADS['semantic_kitti_512']
vs = w['voxel_size']
nx = int((w['x_range'][1] - w['x_range'][0]) / vs)
ny = int((w['y_range'][1] - w['y_range'][0]) / vs)
gen = torch.Generator(device=dev).manual_seed(32)
scans = [synthetic.lidar_scan(POINTS, 4, gen, dev) for _ in range(B)]
_, masks = synthetic.gt_masks(B, Q, ny, nx, gen, dev, cell=vs)
ids = torch.arange(1, Q + 1, device=dev, dtype=torch.float32).view(1, Q, 1, 1)
gt_map = (masks * ids).amax(1).to(torch.int32)                            # (B, ny, nx), 0 = background
pred_map = torch.roll(gt_map, (1, 2), (1, 2)) - 1                         # shifted by a cell and two; -1 = none
pred_map[pred_map % 10 == 9] = -1                                         # every tenth instance is missed
geom = ops.VoxelGeometry.from_ranges([w['x_range'][0], w['y_range'][0], w['z_range'][0], w['x_range'][1], w['y_range'][1],
                                      w['z_range'][1]], [vs, vs, w['z_range'][1] - w['z_range'][0]])
pred_l = ops.lift_instances(scans, pred_map.contiguous(), geom, Q)
gt_l = ops.lift_instances(scans, (gt_map - 1).contiguous(), geom, Q)
gq = gt_l.point_query.long()
n = gq.numel()
words = torch.where(gq >= 0, ((gq + 1) << 16) | 10, torch.full_like(gq, 40))
words = torch.where(torch.rand(n, generator=gen, device=dev) < 0.03, torch.zeros_like(words), words).to(torch.int32)
query_class = torch.ones((B, Q), dtype=torch.int32, device=dev)
lut_host = semantic_kitti_class_lut()
lut = torch.from_numpy(lut_host).to(dev)
lengths = list(pred_l.lengths)


def run():
    return ops.panoptic_frames(pred_l.point_query, words, pred_l.scan_offsets, query_class, lut, 2, max_gt=256, min_points=50)


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


out = run()
torch.cuda.synchronize()
host = dict(pq=pred_l.point_query.cpu().numpy(), gw=words.cpu().numpy(), qc=query_class.cpu().numpy())
t_np = []
for _ in range(3):
    t0 = time.perf_counter()
    ref = R.frames(host['pq'], host['gw'], lengths, host['qc'], lut_host, 2, 256, 50)
    t_np.append((time.perf_counter() - t0) * 1e3)
equal = all(np.array_equal(a.cpu().numpy(), ref[k]) for a, k in ((out.frame_stats, 'stats'), (out.confusion, 'confusion'),
                                                                  (out.n_gt, 'n_gt'), (out.gt_key, 'gt_key'),
                                                                  (out.gt_area, 'gt_area'), (out.pred_area, 'pred_area')))
iou_err = float(np.max(np.abs(out.frame_iou.cpu().numpy() - ref['iou']) / np.maximum(np.abs(ref['iou']), 1e-300)))
k32 = timed(run, 200, 7, 20)

kw = synthetic.module_kwargs('semantic_kitti_512', B, 'bf16', num_queries=Q)
torch.manual_seed(0)
model = MaskBevModule(**kw).to(dev)
model.log_scalars = False


def predict_lift():
    p = model.predict(scans)
    return p.lift(scans, model)


pl = timed(predict_lift, 10, 5, 3)
res = dict(scans=B, points=lengths, queries=Q, classes=2, max_gt=256, min_points=50,
           share_pred_in_instance=float((pred_l.point_query >= 0).float().mean()),
           share_gt_in_instance=float((gq >= 0).float().mean()), share_ignored=float((words == 0).float().mean()),
           share_in_pair=ref['in_pair'] / n, n_gt=ref['n_gt'].tolist(), stats_tp_fp_fn=ref['stats'][:, 1].sum(0).tolist(),
           equals_restatement=bool(equal), iou_sum_max_rel_err=iou_err,
           panoptic_frames_ms=dict(median=statistics.median(k32), min=min(k32), max=max(k32), iters=200, reps=7),
           numpy_restatement_ms=dict(median=statistics.median(t_np), min=min(t_np), max=max(t_np), reps=3),
           predict_plus_lift_ms=dict(median=statistics.median(pl), min=min(pl), max=max(pl), iters=10, reps=5))
target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'k32_measure.json')
with open(target, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
