"""K42 measurement: mask NMS and the overlap filter at the two inference shapes, one process, interleaved.

    python scratch/k42_resolve_bench.py [--rounds 20] [--out FILE.json] [--no-graph]

Synthetic decoder outputs: every query's logit map is -4 but for one random rectangle of +4 (4 .. 24 quarter-resolution cells a
side; every third query repeats its predecessor's rectangle shifted by one cell), scores uniform, one label; `keep` is a random
30 % of the queries, or all of them.  Shapes: 512 x 512 with Q = 100 and 1024 x 1024 with Q = 300, B = 4, logits a quarter of
the grid.

Part (a) — every call of the resolved path through its Python wrapper (device events on the launch stream, medians of
--rounds, all calls of a shape in a shuffled order per round): K21b as the parent commit runs it (masks + map), its two
passes here (masks only; map only, over the survivors), K42a, K42b, K42c and K39b (`exclusive`).
Part (b) — K42a against `ops.pairwise_mask_overlap(masks, masks, B)` (K29a), the only way the parent commit can get these
numbers, on the same masks in the same rounds; the two tables are compared where both queries are kept.
Part (c) — a GraphedPredictStep replay of the bench module with and without `resolve` (both graphs alive, replayed in turn);
without `resolve` the captured launches are the parent commit's.  The module is untrained; the bias of its "empty" class is
lowered by 20, so that (nearly) every query is kept and the resolved path has work to do — the masks are those of random weights.

Next to each time: the bytes and operations the call needs, from the shapes and the kept count."""
import argparse
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {'512': (512, 512, 100, 4), '1024': (1024, 1024, 300, 4)}


def _summary(t):
    return dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))


def synthetic_outputs(h, w, q, b, dev, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((b, q, h, w), -4.0)
    for f in range(b):
        box = None
        for i in range(q):
            if i % 3 == 1 and box is not None:
                y0, x0, y1, x1 = box
                box = (min(y0 + 1, h - 2), x0, min(y1 + 1, h), x1)
            else:
                sy, sx = (int(v) for v in torch.randint(4, 25, (2,), generator=g))
                y0, x0 = int(torch.randint(0, h - sy, (1,), generator=g)), int(torch.randint(0, w - sx, (1,), generator=g))
                box = (y0, x0, y0 + sy, x0 + sx)
            logits[f, i, box[0]:box[2], box[1]:box[3]] = 4.0
    scores = torch.rand((b, q), generator=g) * 0.9 + 0.05
    keep30 = torch.rand((b, q), generator=g) < 0.3
    return logits.to(dev), scores.to(dev), keep30.to(dev)


def time_calls(calls, rounds, warmup=3):
    """calls: name -> (setup or None, fn).  Every round runs all of them in an order of its own; setup is outside the bracket."""
    times = {k: [] for k in calls}
    pending = []
    for it in range(warmup + rounds):
        order = list(calls.items())
        random.Random(it).shuffle(order)
        for name, (setup, fn) in order:
            if setup is not None:
                setup()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            if it >= warmup:
                pending.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in pending:
        times[name].append(e0.elapsed_time(e1))
    return {k: _summary(v) for k, v in times.items()}


def model(name, H, W, q, b, h, w, k):
    """Bytes and operations per call from the shapes; k = kept queries per frame (mean)."""
    nwords = H * W // 32
    pairs = k * (k + 1) / 2
    return {
        'k42a_self_overlap': dict(and_popc_words=b * pairs * nwords, bytes_read_min=b * k * nwords * 4, bytes_written=b * q * q * 4,
                                  note='tiles of 32 kept rows: a row is re-read once per tile pair it is in'),
        'k29a_pairwise_overlap': dict(and_popc_words=b * q * q * nwords, bytes_read_min=2 * b * q * nwords * 4,
                                      bytes_written=b * q * q * 4),
        'k42b_nms': dict(bytes_read=b * (k * k + 4 * q) * 4, serial_rounds_max=k),
        'k42c_overlap_filter': dict(bytes_read=2 * b * H * W * 4, bytes_written_max=b * H * W * 4),
        'k21b_map_only_survivors': dict(logit_bytes_read=b * k * h * w * 4, bytes_written=b * H * W * 4),
        'k21b_masks_only': dict(logit_bytes_read=b * q * h * w * 4, bytes_written=b * q * nwords * 4),
        'k21b_parent_masks_and_map': dict(logit_bytes_read=b * q * h * w * 4, bytes_written=b * q * nwords * 4 + b * H * W * 4),
        'k39b_masks_from_map': dict(bytes_read=b * H * W * 4, bytes_written=b * q * nwords * 4),
    }[name]


def kernels(args, dev):
    from mask_bev_amd import ops
    out = {}
    for tag, (H, W, q, b) in SHAPES.items():
        h, w = H // 4, W // 4
        logits, scores, keep30 = synthetic_outputs(h, w, q, b, dev, seed=q)
        labels = torch.ones((b, q), dtype=torch.int32, device=dev)
        for kept_name, keep in (('kept30', keep30), ('all', torch.ones_like(keep30))):
            first = ops.extract_masks(logits, scores, keep, (H, W), masks=True, instance_map=False)
            pm, areas = first['masks'], first['areas']
            inter = ops.mask_self_overlap(pm, keep)
            keep1, by = ops.mask_nms(inter, scores, labels, keep)
            imap0 = ops.extract_masks(logits, scores, keep1, (H, W), masks=False, instance_map=True)['instance_map']
            imap = imap0.clone()
            keep2, owned = ops.overlap_filter(imap, areas, keep1)
            old, _, _ = ops.pairwise_mask_overlap(pm, pm, b)
            both = (keep.unsqueeze(2) & keep.unsqueeze(1))
            assert torch.equal(inter, torch.where(both, old, torch.zeros_like(old))), 'K42a and K29a disagree'
            calls = {
                'k21b_parent_masks_and_map': (None, lambda: ops.extract_masks(logits, scores, keep, (H, W))),
                'k21b_masks_only': (None, lambda: ops.extract_masks(logits, scores, keep, (H, W), masks=True, instance_map=False)),
                'k42a_self_overlap': (None, lambda: ops.mask_self_overlap(pm, keep)),
                'k29a_pairwise_overlap': (None, lambda: ops.pairwise_mask_overlap(pm, pm, b)),
                'k42b_nms': (None, lambda: ops.mask_nms(inter, scores, labels, keep)),
                'k21b_map_only_survivors': (None, lambda: ops.extract_masks(logits, scores, keep1, (H, W), masks=False)),
                'k42c_overlap_filter': (lambda: imap.copy_(imap0), lambda: ops.overlap_filter(imap, areas, keep1)),
                'k39b_masks_from_map': (None, lambda: ops.masks_from_map(imap, q)),
            }
            res = time_calls(calls, args.rounds)
            k = float(keep.sum()) / b
            for name in res:
                res[name]['model'] = model(name, H, W, q, b, h, w, k)
            a, o = res['k42a_self_overlap']['median_ms'], res['k29a_pairwise_overlap']['median_ms']
            out[f'{tag}_{kept_name}'] = dict(shape=dict(H=H, W=W, Q=q, B=b, h=h, w=w), kept_per_frame=k,
                                             survivors_per_frame=float(keep1.sum()) / b, final_per_frame=float(keep2.sum()) / b,
                                             k42a_over_k29a=a / o, calls=res)
            print(tag, kept_name, {n: round(v['median_ms'], 4) for n, v in res.items()}, flush=True)
        del logits
    return out


def graphed(args, dev):
    from mask_bev_amd import synthetic
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.predict import GraphedPredictStep, ResolveSettings
    out = {}
    for workload, batch in (('semantic_kitti_512', 4), ('waymo_1024', 4)):
        torch.manual_seed(420)
        m = MaskBevModule(**synthetic.module_kwargs(workload, batch, compute_dtype='bf16')).to(dev).train()
        with torch.no_grad():                           # an untrained head calls almost every query "empty": take that class away
            for mod in m.modules():
                if hasattr(mod, 'cls_embed'):
                    mod.cls_embed.bias[0] -= 20.0
        m.flatten_parameters()
        scans = synthetic.make_batch(workload, batch, 0, 0, dev)[0]
        plain = GraphedPredictStep(m, scans)
        resolved = GraphedPredictStep(m, scans, resolve=ResolveSettings())
        exclusive = GraphedPredictStep(m, scans, resolve=ResolveSettings(exclusive=True))
        plain.step(scans), resolved.step(scans), exclusive.step(scans)
        torch.cuda.synchronize()
        res = time_calls({'replay_plain': (None, plain.graph.replay), 'replay_resolve': (None, resolved.graph.replay),
                          'replay_resolve_exclusive': (None, exclusive.graph.replay)}, args.rounds)
        base = res['replay_plain']['median_ms']
        out[workload] = dict(batch=batch, queries=int(plain.out.labels.shape[1]), kept=int(plain.out.keep.sum()),
                             kept_after_resolve=int(resolved.out.keep.sum()), replays=res,
                             resolve_extra_ms=res['replay_resolve']['median_ms'] - base,
                             resolve_extra_percent=100.0 * (res['replay_resolve']['median_ms'] - base) / base,
                             exclusive_extra_ms=res['replay_resolve_exclusive']['median_ms'] - base)
        print(workload, {n: round(v['median_ms'], 4) for n, v in res.items()}, flush=True)
        for g in (plain, resolved, exclusive):
            g.close()
        del m
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-graph', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('k42_resolve_bench: no GPU; nothing is measured on a CPU')
    dev = torch.device('cuda')
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, kernels=kernels(args, dev))
    if not args.no_graph:
        result['graphed'] = graphed(args, dev)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
