"""K41 measurement: the two gradient-clipping launches at the bench arena, one process, interleaved.

    python scratch/k41_clip_bench.py [--workload semantic_kitti_512] [--rounds 20] [--out FILE.json] [--no-graph]

Part 1 — per C-ABI launch (device events on the launch stream, medians of --rounds): mbv_grad_norm_partials and
mbv_grad_clip_coef against mbv_lamb_moments, the yardstick measured in the same run; model bytes (workmodel.MODELS) / time.
Part 2 — a whole FlatAdam.step() with max_grad_norm None, inf and 0.01 (three optimizers over one arena, each with its own
state, stepping in turn; every round has a shuffled order of its own, so that no optimizer always follows the same one).
Part 3 — what losing the two fused arms costs the graphed step: a GraphedTrainStep over the bench module with
max_grad_norm=inf against one with None (one captured step alive at a time, built and timed in the order none, inf, none, inf;
inf measures and never clips, so both train alike).

The module is the one bench.py builds (bf16 compute, flattened); the gradient is filled once with N(0, 1e-3) and re-filled in
front of every step, outside the timed brackets."""
import argparse
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K41 = ('mbv_grad_norm_partials', 'mbv_grad_clip_coef')


def _summary(t):
    return dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))


def launches_and_steps(args, dev):
    from mask_bev_amd import _lib, synthetic, workmodel
    from mask_bev_amd.arena import FlatAdam, FlatLamb
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(420)
    model = MaskBevModule(**synthetic.module_kwargs(args.workload, 4, compute_dtype='bf16')).to(dev).train()
    arena = model.flatten_parameters()
    groups = [dict(segment=s) for s in ('encoder', 'backbone', 'head')]
    adam = lambda clip: FlatAdam(arena, groups, lr=1e-4, weight_decay=1e-2, decoupled=True, max_grad_norm=clip)
    opts = {'adamw': adam(None), 'adamw_clip_inf': adam(float('inf')), 'adamw_clip_0.01': adam(0.01),
            'lamb': FlatLamb(arena, groups, lr=1e-4, weight_decay=1e-2)}
    grad = torch.randn(arena.numel, device=dev) * 1e-3
    pad = torch.ones(arena.numel, dtype=torch.bool, device=dev)
    for p, o in arena.layout:
        pad[o:o + p.numel()] = False
    grad[pad] = 0.0                                    # padding stays zero, as the arena keeps it
    del pad
    lib = _lib.load()
    records, steps = [], {k: [] for k in opts}

    def hook(name, fn, a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*a)
        e1.record()
        records.append((name, workmodel.MODELS[name](a)[2] if name in workmodel.MODELS else 0.0, e0, e1))
        return rc

    # pass A: whole steps, no per-launch events inside them; pass B: per-launch events
    for timed_launches in (False, True):
        for it in range(args.warmup + args.rounds):
            if it == args.warmup:
                torch.cuda.synchronize()
                records.clear()
                lib.hook = hook if timed_launches else None
            order = list(opts.items())
            random.Random(1000 * timed_launches + it).shuffle(order)
            for name, opt in order:                    # interleaved: every round runs all four, in an order of its own
                arena.grad.copy_(grad)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                opt.step()
                e1.record()
                if it >= args.warmup and not timed_launches:
                    steps[name].append((e0, e1))
        torch.cuda.synchronize()
        lib.hook = None
    times, nbytes = {}, {}
    for name, by, e0, e1 in records:
        times.setdefault(name, []).append(e0.elapsed_time(e1))
        nbytes[name] = by
    clipped = opts['adamw_clip_0.01']
    out = dict(workload=args.workload, arena_elements=arena.numel, parameters=len(arena.layout), rounds=args.rounds,
               norm_chunks=sum((b - a + 4095) // 4096 for a, b in arena.segments.values()), grad_norm=float(clipped.grad_norm),
               clip_coef=float(clipped.clip_coef), launches={}, step_ms={})
    base = nbytes['mbv_lamb_moments'] / (statistics.median(times['mbv_lamb_moments']) * 1e-3) / 1e12
    for name in ('mbv_lamb_moments',) + K41:
        t = times[name]
        rate = nbytes[name] / (statistics.median(t) * 1e-3) / 1e12
        out['launches'][name] = dict(samples=len(t), model_bytes=nbytes[name], tb_per_s=rate,
                                     ratio_to_k_lamb_moments=rate / base, **_summary(t))
    for name in ('adamw', 'adamw_clip_inf', 'adamw_clip_0.01'):
        out['step_ms'][name] = _summary([a.elapsed_time(b) for a, b in steps[name]])
    return out


def graphed_steps(args, dev):
    from mask_bev_amd import synthetic
    from mask_bev_amd.graph import GraphedTrainStep
    from mask_bev_amd.mask_bev_module import MaskBevModule
    pool = [synthetic.make_batch(args.workload, 4, 0, s, dev) for s in range(2)]
    out = {'none': dict(t=[]), 'inf': dict(t=[])}
    # one captured step alive at a time (a capture retires the records of the one before it): none, inf, none, inf
    for rep in range(2):
        for tag, clip in (('none', None), ('inf', float('inf'))):
            torch.manual_seed(420)
            m = MaskBevModule(**synthetic.module_kwargs(args.workload, 4, compute_dtype='bf16', gradient_clip_val=clip))
            m = m.to(dev).train()
            m.log_scalars = False
            m.flatten_parameters()
            opt = m.configure_optimizers()['optimizer']
            g = GraphedTrainStep(m, opt, pool[0])
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
            if clip is not None:
                out[tag]['grad_norm'] = float(opt.grad_norm)
            g.close()
            del g, opt, m
            torch.cuda.empty_cache()
    for tag in ('none', 'inf'):
        t = out[tag].pop('t')
        out[tag].update(samples=len(t), first_pass_median_ms=statistics.median(t[:args.rounds]),
                        second_pass_median_ms=statistics.median(t[args.rounds:]), **_summary(t))
    out['cost_ms'] = out['inf']['median_ms'] - out['none']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='semantic_kitti_512')
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-graph', action='store_true', help='skip part 3')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a CPU run measures nothing'
    dev = torch.device('cuda:0')
    out = launches_and_steps(args, dev)
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
