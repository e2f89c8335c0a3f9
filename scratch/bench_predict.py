"""Inference timing: eager ``MaskBevModule.predict`` vs ``GraphedPredictStep`` (ms per batch, scans/s), K21's device time
(HIP events around select + extract on the last decoder output) against its byte floor, and the dense torch route it
replaces (interpolate → threshold → argmax map) with its peak memory.  One JSON line per configuration.

    python scratch/bench_predict.py WORKLOAD BATCH DTYPE [--iters N]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mask_bev_amd import synthetic                       # noqa: E402
from mask_bev_amd.mask_bev_module import MaskBevModule  # noqa: E402
from mask_bev_amd.predict import GraphedPredictStep, extract_instances, grid_hw  # noqa: E402


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def event_us(fn, iters):
    best = 1e30
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3)
    return best


def dense_route(cls, mk, grid):
    p = torch.softmax(cls.float(), -1)
    score, label = p.max(-1)
    keep = label > 0
    v = F.interpolate(mk, grid, mode='bilinear', align_corners=False)
    bits = v > 0
    prod = torch.where(bits & keep[..., None, None], score[..., None, None] * torch.sigmoid(v), torch.full_like(v, -1.0))
    best, idx = prod.max(1)
    return bits, torch.where(best >= 0, idx, torch.full_like(idx, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('workload')
    ap.add_argument('batch', type=int)
    ap.add_argument('dtype')
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(420)
    m = MaskBevModule(**synthetic.module_kwargs(a.workload, a.batch, compute_dtype=a.dtype)).to(dev).train()
    m.flatten_parameters()
    batches = [synthetic.make_batch(a.workload, a.batch, 0, s, dev)[0] for s in range(2)]
    out = dict(workload=a.workload, batch=a.batch, dtype=a.dtype)

    g = GraphedPredictStep(m, batches[0])
    for s in batches:                                    # warm both paths
        m.predict(s)
        g.step(s)
    k = [0]

    def eager():
        m.predict(batches[k[0] % 2])
        k[0] += 1

    def graphed():
        g.step(batches[k[0] % 2])
        k[0] += 1

    out['eager_ms'] = round(wall_ms(eager, a.iters), 3)
    out['graphed_ms'] = round(wall_ms(graphed, a.iters), 3)
    out['eager_scans_per_s'] = round(a.batch * 1e3 / out['eager_ms'], 2)
    out['graphed_scans_per_s'] = round(a.batch * 1e3 / out['graphed_ms'], 2)
    g.close()

    m.eval()
    with torch.no_grad():
        cls, mk, _ = m(batches[0])
    cls, mk = cls[-1], mk[-1].contiguous()
    grid = grid_hw(m)
    b, q, h, w = mk.shape
    H, W = grid
    out['shape'] = dict(B=b, Q=q, h=h, w=w, H=H, W=W, classes=int(cls.shape[-1]))
    out['k21_us'] = round(event_us(lambda: extract_instances(cls, mk, grid), 20), 2)
    out['k21_map_only_us'] = round(event_us(lambda: extract_instances(cls, mk, grid, masks=False), 20), 2)
    nbytes = b * q * h * w * 4 + b * q * ((H * W + 63) // 64) * 8 + b * H * W * 4
    out['k21_bytes_floor_us'] = round(nbytes / 8e12 * 1e6, 2)
    out['k21_interpolations'] = b * q * H * W
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    extract_instances(cls, mk, grid)
    torch.cuda.synchronize()
    out['k21_peak_extra_MB'] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    dense = b * q * H * W * 4
    out['dense_f32_MB'] = round(dense / 2 ** 20, 1)
    free = torch.cuda.mem_get_info()[0]
    if dense * 4 < free:
        with torch.no_grad():
            out['dense_torch_us'] = round(event_us(lambda: dense_route(cls, mk, grid), 5), 1)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            dense_route(cls, mk, grid)
            torch.cuda.synchronize()
            out['dense_torch_peak_extra_MB'] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
