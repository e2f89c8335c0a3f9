"""K40 measurement: FlatAdam.step (k_adamw, the yardstick), FlatLamb.step and FlatSGD.step at the bench arena, one process,
interleaved.  Per C-ABI launch: device-event time, model bytes (workmodel.MODELS) / time, and the ratio to k_adamw's bytes/s.

    python scratch/k40_optim_bench.py [--workload semantic_kitti_512] [--rounds 20] [--out FILE.json]

The module is the one bench.py builds (bf16 compute, flattened); the gradient is filled once with N(0, 1e-3) and re-filled in
front of every step (LAMB's apply pass and the others' zero_grad clear it), outside the timed brackets."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='semantic_kitti_512')
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from mask_bev_amd import _lib, synthetic, workmodel
    from mask_bev_amd.arena import FlatAdam, FlatLamb, FlatSGD
    from mask_bev_amd.mask_bev_module import MaskBevModule
    assert torch.cuda.is_available(), 'needs the GPU: a CPU run measures nothing'
    dev = torch.device('cuda:0')
    torch.manual_seed(420)
    model = MaskBevModule(**synthetic.module_kwargs(args.workload, 4, compute_dtype='bf16')).to(dev).train()
    arena = model.flatten_parameters()
    groups = [dict(segment=s) for s in ('encoder', 'backbone', 'head')]
    opts = {'adamw': FlatAdam(arena, groups, lr=1e-4, weight_decay=1e-2, decoupled=True),
            'lamb': FlatLamb(arena, groups, lr=1e-4, weight_decay=1e-2),
            'sgd': FlatSGD(arena, lr=1e-4, weight_decay=1e-2)}
    grad = torch.randn(arena.numel, device=dev) * 1e-3
    pad = torch.ones(arena.numel, dtype=torch.bool, device=dev)
    for p, o in arena.layout:
        pad[o:o + p.numel()] = False
    grad[pad] = 0.0                                    # padding stays zero, as the arena keeps it
    del pad
    lib = _lib.load()
    records = []

    def hook(name, fn, a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*a)
        e1.record()
        records.append((name, workmodel.MODELS[name](a)[2] if name in workmodel.MODELS else 0.0, e0, e1))
        return rc

    for it in range(args.warmup + args.rounds):
        if it == args.warmup:
            torch.cuda.synchronize()
            records.clear()
            lib.hook = hook
        for name, opt in opts.items():                 # interleaved: every round runs all three
            arena.grad.copy_(grad)
            opt.step()
    torch.cuda.synchronize()
    lib.hook = None
    times, nbytes = {}, {}
    for name, by, e0, e1 in records:
        times.setdefault(name, []).append(e0.elapsed_time(e1))
        nbytes[name] = by
    # the 34 B / element of k_adamw (bench.py's model of it): it has no workmodel entry of its own
    nbytes['mbv_adamw_step'] = arena.numel * 34.0
    out = dict(workload=args.workload, arena_elements=arena.numel, parameters=len(arena.layout), rounds=args.rounds,
               lamb_chunks=opts['lamb'].n_chunks, launches={})
    base = None
    for name in ('mbv_adamw_step', 'mbv_lamb_moments', 'mbv_lamb_trust', 'mbv_lamb_apply', 'mbv_sgd_step'):
        t = times[name]
        per_round = len(t) // args.rounds
        med = statistics.median(t)
        rate = nbytes[name] / (med * 1e-3) / 1e12
        if name == 'mbv_adamw_step':
            base = rate
        out['launches'][name] = dict(launches_per_step=per_round, median_ms=med, min_ms=min(t), max_ms=max(t),
                                     model_bytes=nbytes[name], tb_per_s=rate, ratio_to_k_adamw=rate / base)
    out['step_ms'] = dict(adamw=out['launches']['mbv_adamw_step']['median_ms'],
                          lamb=sum(out['launches'][n]['median_ms'] * out['launches'][n]['launches_per_step']
                                   for n in ('mbv_lamb_moments', 'mbv_lamb_trust', 'mbv_lamb_apply')),
                          sgd=out['launches']['mbv_sgd_step']['median_ms'])
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
