"""K43 measurement: the weight-averaging passes at the bench arena, one process, interleaved.

    python scratch/k43_average_bench.py [--workload semantic_kitti_512] [--rounds 20] [--out FILE.json] [--no-graph]

Part 1 — per call (device events on the launch stream, medians of --rounds; every round runs all of them in a shuffled order of
its own): mbv_sgd_step, the yardstick (26 B/elem), against mbv_weight_average_update with a weight between 0 and 1 (tick + blend,
12 B/elem), mbv_weight_average_swap (18 B/elem with the bf16 shadow; called twice per round, so the arena ends every round as it
began), and mbv_weight_average_update with every = 4, whose calls are split into the three that do nothing and the one that
blends.  Model bytes (workmodel.MODELS) / time.
Part 2 — a GraphedTrainStep over the bench module without an average, with `weight_average: ema` and with
`weight_average_every: 4` (one captured step alive at a time, built and timed in that order, twice).  The arm without an average
runs the code the parent commit runs.

The module is the one bench.py builds (bf16 compute, flattened); the gradient is filled once with N(0, 1e-3) and re-filled in
front of every SGD step, outside the timed brackets."""
import argparse
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _summary(t):
    return dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))


def launches(args, dev):
    from mask_bev_amd import synthetic
    from mask_bev_amd.arena import FlatSGD, WeightAverage
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(420)
    model = MaskBevModule(**synthetic.module_kwargs(args.workload, 4, compute_dtype='bf16')).to(dev).train()
    arena = model.flatten_parameters()
    n = arena.numel
    sgd = FlatSGD(arena, lr=1e-4, momentum=0.9, weight_decay=1e-2)
    on = WeightAverage(arena, mode='ema', decay=0.9999, warmup=False)
    every4 = WeightAverage(arena, mode='ema', decay=0.9999, warmup=False, every=4)
    grad = torch.randn(n, device=dev) * 1e-3
    for p, o in arena.layout:                          # padding stays zero, as the arena keeps it
        grad[o + p.numel():o + (p.numel() + 63) // 64 * 64] = 0.0
    events = {k: [] for k in ('mbv_sgd_step', 'update', 'swap', 'update_every4_off', 'update_every4_on')}
    calls4 = 0

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        events[name].append((e0, e1))

    def both_swaps():
        timed('swap', on.swap)
        timed('swap', on.swap)

    for it in range(args.warmup + args.rounds):
        if it == args.warmup:
            torch.cuda.synchronize()
            for v in events.values():
                v.clear()
        order = ['sgd', 'update', 'swap', 'every4']
        random.Random(it).shuffle(order)
        for what in order:
            if what == 'sgd':
                arena.grad.copy_(grad)
                timed('mbv_sgd_step', sgd.step)
            elif what == 'update':
                timed('update', on.update)
            elif what == 'swap':
                both_swaps()
            else:
                calls4 += 1
                timed('update_every4_on' if calls4 % 4 == 0 else 'update_every4_off', every4.update)
    torch.cuda.synchronize()
    assert int(every4.num_updates) == calls4 // 4 and int(on.num_updates) == args.warmup + args.rounds
    per_elem = {'mbv_sgd_step': 26.0, 'update': 12.0, 'swap': 18.0, 'update_every4_on': 12.0, 'update_every4_off': 0.0}
    out = dict(workload=args.workload, arena_elements=n, parameters=len(arena.layout), rounds=args.rounds,
               last_weight=float(on.last_weight), calls={})
    times = {k: [a.elapsed_time(b) for a, b in v] for k, v in events.items()}
    base = n * 26.0 / (statistics.median(times['mbv_sgd_step']) * 1e-3) / 1e12
    for name, t in times.items():
        rate = n * per_elem[name] / (statistics.median(t) * 1e-3) / 1e12
        out['calls'][name] = dict(samples=len(t), model_bytes=n * per_elem[name], tb_per_s=rate, ratio_to_k_sgd=rate / base,
                                  **_summary(t))
    return out


def graphed_steps(args, dev):
    from mask_bev_amd import synthetic
    from mask_bev_amd.graph import GraphedTrainStep
    from mask_bev_amd.mask_bev_module import MaskBevModule
    pool = [synthetic.make_batch(args.workload, 4, 0, s, dev) for s in range(2)]
    arms = (('none', {}), ('ema', dict(weight_average='ema')), ('ema_every4', dict(weight_average='ema', weight_average_every=4)))
    out = {tag: dict(t=[]) for tag, _ in arms}
    for rep in range(2):
        for tag, extra in arms:
            torch.manual_seed(420)
            m = MaskBevModule(**synthetic.module_kwargs(args.workload, 4, compute_dtype='bf16', **extra)).to(dev).train()
            m.log_scalars = False
            m.flatten_parameters()
            opt = m.configure_optimizers()['optimizer']
            av = m.make_weight_average()
            g = GraphedTrainStep(m, opt, pool[0], average=av)
            out[tag].update(k3_fused=bool(g._k3_fused), matrices_fused=len(g._mx_fused))
            for it in range(args.warmup + args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                g.step(pool[it % len(pool)])
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    out[tag]['t'].append(e0.elapsed_time(e1))
            if av is not None:
                out[tag]['updates'] = int(av.num_updates)
            g.close()
            del g, opt, m, av
            torch.cuda.empty_cache()
    for tag, _ in arms:
        t = out[tag].pop('t')
        out[tag].update(samples=len(t), first_pass_median_ms=statistics.median(t[:args.rounds]),
                        second_pass_median_ms=statistics.median(t[args.rounds:]), **_summary(t))
    out['cost_ms'] = out['ema']['median_ms'] - out['none']['median_ms']
    out['cost_every4_ms'] = out['ema_every4']['median_ms'] - out['none']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='semantic_kitti_512')
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-graph', action='store_true', help='skip part 2')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a CPU run measures nothing'
    dev = torch.device('cuda:0')
    out = launches(args, dev)
    torch.cuda.empty_cache()
    if not args.no_graph:
        out['graphed_step_ms'] = graphed_steps(args, dev)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
