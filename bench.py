#!/usr/bin/env python3
"""Benchmark of the MaskBEV scan -> BEV -> mask forward+backward path on MI355X.

Contract: ``python bench.py --gpus N --steps K --warmup W`` (for N > 1 launched through
``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...``, one rank per GPU over RCCL).
A *step* is one full training step of ``MaskBevModule`` on one batch of synthetic SemanticKITTI-shaped
scans already resident in HBM: voxelise → PFN → scatter+LN → Swin → pixel decoder → masked-attention decoder
→ Hungarian-matched loss → backward (gradient all-reduce overlapped for N > 1) → AdamW step.
Rank 0 prints ONE JSON line (metric of BASELINE.json: LiDAR scans/s fwd+bwd, whole job).

A plain run sets up, warms up, times the K steps and prints the line: `metric`, `value`, `unit`, `n_gpus`, `steps`,
`warmup`, `ms_per_step`, `higher_is_better`, `scaling`, `vs_baseline`, `dtype`, `data` and `config`.  Everything else
the benchmark measures or checks (below) runs only with ``--full``; ``--detail-out`` and ``--aten-detail`` imply it.
``--dump-outputs DIR`` writes what the timed step computed in its last step, right after the timed region
(`dump_outputs`): the inputs and the initial parameters are seeded, so two builds can be compared output for output.

Extra objects on the line of a ``--full`` run:
  roofline      roofline of the kernel of this repository that costs the most time per step (launches x average
                duration): algorithmic bytes (HBM-bound) or flops (MFMA-bound) of one launch over its average launch
                duration, measured live with HIP events on the stream the kernel is launched on.  K3's kernels and
                the optimizer kernel run eagerly inside the timed region and are timed there; the kernels inside the
                replayed HIP graphs cannot carry events, so every C-ABI call of two eager steps run right AFTER the
                timed region is bracketed by events instead (mask_bev_amd/workmodel.py holds the work of each call).
                `traffic` is the measured HBM bytes per launch from the PMC passes kept in `roofline_traffic_source`
                (null when not measured).  The printed line stays under 4 KB (`compact_line`): it carries `roofline`,
                `roofline_top` (the five families that cost the most time) and `roofline_worst`; the table of EVERY
                instrumented family of both dtypes (`roofline_all`) goes to `--detail-out` (gpurun_out/bench_detail.json).
  cpu_baseline  the oracle (CPU restatement, kind "port") timed on this box's host cores on a bounded sample:
                1 warm-up + 3 iterations, forward and forward+backward, at 6 threads (the reference's setting).
  fp32          the same step in fp32 — the precision the reference trains in — timed the same way (50 steps).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)       # a timed region of more than 5 s at ≈ 27 ms per step
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--workload', default='semantic_kitti_512')
    ap.add_argument('--batch', type=int, default=4, help='scans per GPU per step (YAML batch_size)')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32', 'fp16'])
    ap.add_argument('--distribution', default='lidar', choices=['lidar', 'uniform'],
                    help="synthetic point distribution: 64-beam LiDAR-shaped scans (headline) or uniform x/y "
                         "(worst case for the pillar count)")
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-fp32', action='store_true', help='skip the secondary fp32 (reference precision) timing')
    ap.add_argument('--cpu-baseline-budget-s', type=float, default=75.0)
    ap.add_argument('--cpu-baseline-worker', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--cpu-threads', type=int, default=6, help=argparse.SUPPRESS)
    ap.add_argument('--no-kernel-profile', action='store_true', help='skip the instrumented eager step behind roofline_all')
    ap.add_argument('--pool', type=int, default=2, help='distinct synthetic batches kept resident in HBM')
    ap.add_argument('--no-arena', action='store_true', help='per-tensor parameters and torch.optim.AdamW')
    ap.add_argument('--no-graph', action='store_true', help='launch every kernel eagerly instead of replaying the HIP graph')
    ap.add_argument('--dry-run-collectives', action='store_true',
                    help='N > 1: log, per step, the bytes and host launch time of every gradient all-reduce piece relative '
                         'to the graph replays / the encoder backward it is meant to hide under (any backend; with '
                         'MBV_DIST_BACKEND=gloo it runs where no RCCL fabric is available)')
    ap.add_argument('--aten-detail', default=None, metavar='FILE',
                    help='write the per-operator times of the ATen calls of the instrumented step (name, shapes, call site)')
    ap.add_argument('--force-reducer', action='store_true',
                    help='N = 1: run the data-parallel step anyway — `init_process_group("nccl", world_size=1)`, the arena '
                         'reducer and its four-piece exchange around the two graph replays — so that RCCL executes the '
                         'graph step\'s collectives on the one GPU there is (implies --dry-run-collectives)')
    ap.add_argument('--grad-wire', default='f32', choices=['f32', 'bf16'],
                    help='N > 1: type the gradient all-reduce travels in (bf16 = half the xGMI bytes, sums formed in bf16; '
                         'default f32 = the exact in-place exchange)')
    ap.add_argument('--gemm-table', default=None, metavar='CSV',
                    help='a TunableOp selection table other than the committed one (A/B of a re-tuned table)')
    ap.add_argument('--detail-out', default=None, metavar='FILE',
                    help='where the full record (roofline_all of both dtypes, every cpu_baseline row) is written; '
                         'default gpurun_out/bench_detail.json — the printed line carries the summary only')
    ap.add_argument('--switch', action='append', default=[], metavar='NAME=VALUE',
                    help='A/B runs: set a path selector of mask_bev_amd/switches.py (recorded in config.switches)')
    ap.add_argument('--full', action='store_true',
                    help='also measure and check what the headline figure does not need: the per-family roofline table '
                         '(instrumented eager steps), the fp32 step, the CPU baseline, the data-parallel replica check '
                         'and the full record behind --detail-out')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='after the timed steps, write what the last one computed as DIR/<name>.npy (see dump_outputs)')
    args = ap.parse_args()
    if args.detail_out or args.aten_detail:
        args.full = True            # both files are records of the full run
    return args


def free_port() -> int:
    """A TCP port the kernel just handed out (bound to port 0 and released): not derived from the pid, which collides on
    a shared box."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def cpu_baseline_worker(state_file: str, workload: str, threads: int, budget_s: float):
    """One thread setting of the CPU baseline, in a process of its own (so that a pathological setting can be cut off):
    1 warm-up + up to 3 timed iterations of forward+loss+backward and of forward+loss of the oracle on 1 scan."""
    from oracle import maskbev_oracle as O
    from mask_bev_amd import synthetic
    torch.set_num_threads(threads)
    kw = synthetic.module_kwargs(workload, 1)
    cfg = O.make_cfg(**kw)
    sd = torch.load(state_file)
    scans, (labels, masks) = synthetic.make_batch(workload, 1, 0, 10_000, torch.device('cpu'))

    def one(backward: bool) -> float:
        sd_g = {k: (v.clone().requires_grad_(backward) if v.is_floating_point() and 'running_' not in k else v.clone())
                for k, v in sd.items()}
        t0 = time.perf_counter()
        with torch.set_grad_enabled(backward):
            cls, mk, _ = O.model_forward(cfg, sd_g, scans, training=True)
            loss = O.total_loss(O.loss_dict(cfg, cls, mk, labels, masks, O.PointSource(0)))
        if backward:
            loss.backward()
        return time.perf_counter() - t0

    t_warm = one(True)                                        # warm-up (allocator, thread pools)
    print(json.dumps(dict(stage='warmup', s=t_warm)), flush=True)
    iters = 3 if t_warm * 5.5 <= budget_s else (1 if t_warm * 2.5 <= budget_s else 0)
    fb = [one(True) for _ in range(iters)]
    fw = [one(False) for _ in range(iters)]
    print(json.dumps(dict(stage='done', iterations=iters, warmup_s=t_warm, fwd_bwd_s=fb, fwd_s=fw)), flush=True)


def cpu_baseline(workload: str, module, budget_s: float):
    """The oracle (CPU restatement of the reference's dense algorithm, kind "port") on the host cores of this box, on
    a bounded sample: 1 scan of the same workload per iteration, fp32.  ORACLE USE: checker / baseline only — never
    on the measured GPU path.  Protocol of SURVEY.md §8d / BASELINE.md §3: 1 warm-up + 3 timed iterations, forward(+loss)
    and forward+backward timed separately, at 6 threads (the reference pins ``OMP_NUM_THREADS=6``,
    /root/reference: train_mask_bev.py:14) and at ``os.cpu_count()`` threads.  Each thread setting runs in a child
    process with a share of the time budget: a many-core host oversubscribed with the oracle's tiny torch ops can be
    an order of magnitude slower, and the default bench run must still end within minutes — a setting that exceeds its
    share is cut off and says so.  ``value`` is the best forward+backward rate; every row is kept."""
    import subprocess
    import tempfile
    sd = {k: v.detach().float().cpu() for k, v in module.state_dict().items()}
    # 6 threads = the reference's own setting; the second row is every core of a small host, capped at 32 on the GPU
    # box's 256-core host: oversubscribed with the oracle's tiny torch ops that row never finished its warm-up
    # iteration inside the budget (round 2: 121 s of a 167 s run for nothing)
    # Round 4: the second (32-thread) row is gone — it never beat 6 threads on the GPU box's host and took half of the
    # budget, which cut the 6-thread row to ONE timed iteration; the whole budget now buys the protocol's 1 + 3.
    ncpu = os.cpu_count() or 1
    settings = [min(6, ncpu)]
    share = budget_s / len(settings)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        state_file = os.path.join(tmp, 'state.pt')
        torch.save(sd, state_file)
        for threads in settings:
            cmd = [sys.executable, os.path.abspath(__file__), '--cpu-baseline-worker', state_file, '--workload', workload,
                   '--cpu-threads', str(threads), '--cpu-baseline-budget-s', str(share)]
            env = dict(os.environ, OMP_NUM_THREADS=str(threads), HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
            t0, out, timed_out = time.perf_counter(), '', False
            try:
                out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=share * 1.5 + 30).stdout
            except subprocess.TimeoutExpired as e:
                out, timed_out = (e.stdout or b'').decode() if isinstance(e.stdout, bytes) else (e.stdout or ''), True
            recs = [json.loads(l) for l in out.splitlines() if l.startswith('{')]
            done = next((r for r in recs if r.get('stage') == 'done'), None)
            warm = next((r for r in recs if r.get('stage') == 'warmup'), None)
            row = dict(threads=threads, wall_s=round(time.perf_counter() - t0, 1))
            if done and done['iterations'] > 0:
                fb, fw = done['fwd_bwd_s'], done['fwd_s']
                row.update(iterations=done['iterations'], warmup_s=round(done['warmup_s'], 2),
                           fwd_bwd_s=[round(t, 2) for t in fb], fwd_s=[round(t, 2) for t in fw],
                           fwd_bwd_scans_per_s=len(fb) / sum(fb), fwd_scans_per_s=len(fw) / sum(fw),
                           note=None if done['iterations'] == 3 else 'iteration count cut to fit the time budget')
            elif warm or done:
                t = (done or warm).get('warmup_s', (warm or {}).get('s'))
                row.update(iterations=0, warmup_s=round(t, 2), fwd_bwd_s=[round(t, 2)], fwd_s=[],
                           fwd_bwd_scans_per_s=1.0 / t, fwd_scans_per_s=None,
                           note='too slow for the time budget: the warm-up iteration is the only sample'
                                + (' (cut off)' if timed_out else ''))
            else:
                row.update(iterations=0, fwd_bwd_scans_per_s=None, fwd_scans_per_s=None,
                           note='cut off before the warm-up iteration finished' if timed_out else 'failed')
            rows.append(row)
    ok = [r for r in rows if r.get('fwd_bwd_scans_per_s')]
    if not ok:
        return dict(value=None, unit='scans/s', cores=None, kind='port', sample='no thread setting finished', rows=rows)
    best = max(ok, key=lambda r: r['fwd_bwd_scans_per_s'])
    return dict(value=best['fwd_bwd_scans_per_s'], unit='scans/s', cores=best['threads'], kind='port',
                sample=f'n = 1 scan of {workload} per iteration (the GPU line steps 4), fp32, oracle forward+loss+backward; '
                       f'1 warm-up + {best["iterations"]} timed iterations at {best["threads"]} threads '
                       f'(host has {os.cpu_count()} logical cores; the reference pins OMP_NUM_THREADS=6)',
                rows=rows)


def kernel_profile(model, opt, batch, steps: int = 2, detail_file=None):
    """HIP-event duration of every C-ABI call of `steps` eager training steps (after one untimed eager step), on the
    stream the kernels are launched on, with the algorithmic work of each call (mask_bev_amd/workmodel.py).
    Runs AFTER the timed region: the timed steps replay HIP graphs, which cannot carry per-kernel events.
    Returns {kernel: dict(launches_per_step, avg_ms, total_ms_per_step, bytes, flops, bound)}."""
    from mask_bev_amd import _lib, workmodel
    lib = _lib.load()
    records = []

    state = dict(spin=None)

    def hook(name, fn, args):
        if name == 'mbv_pfn_decorate' and state['spin'] is not None:
            # the step's one host read (K1's pillar count) is behind us: from here on the host only issues work
            state['spin']()
        model_fn = workmodel.MODELS.get(name)
        if model_fn is None:
            return fn(*args)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*args)
        b.record()
        records.append((model_fn(args), a, b))
        return rc

    def one(i):
        loss = model.training_step(batch, i)
        model.scale_loss(loss).backward()
        opt.step()
        if not getattr(opt, 'zero_grad_in_step', False):
            opt.zero_grad(set_to_none=False)

    t_host = time.perf_counter()
    one(0)
    torch.cuda.synchronize()
    t_host = time.perf_counter() - t_host
    # An eager step is launch-bound (the host needs longer to issue it than the GPU to run it), and a bracket around a
    # call whose host path is long (a hipBLASLt GEMM: descriptor + heuristic look-up) then also counts the stream's wait
    # for the launch — the library GEMMs read 30 % above the rocprof trace (scratch/gemm_bracket.py: 23 us for a 3 us GEMM,
    # 7.6 us behind a spin).  A spin kernel issued right after the step's only host read (K1's pillar count) keeps the
    # stream BEHIND the host for the rest of the step: every bracket then sees back-to-back execution.
    def spin_ms(ms: float) -> None:
        torch.cuda._sleep(int(spin_ms.cycles_per_ms * ms))
    a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a0.record()
    torch.cuda._sleep(10_000_000)
    b0.record()
    torch.cuda.synchronize()
    spin_ms.cycles_per_ms = 10_000_000 / max(a0.elapsed_time(b0), 1e-3)
    # cost of an empty event bracket on this stream (two records back to back): what every bracket adds to the kernel
    # it surrounds.  Subtracted below — 70 brackets x 3 us around a 20 us kernel family was enough to swap the two
    # leading families against the rocprof trace.
    cal = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(256)]
    for a, b in cal:
        a.record()
        b.record()
    torch.cuda.synchronize()
    gaps = sorted(a.elapsed_time(b) for a, b in cal)
    empty_ms = gaps[len(gaps) // 2]
    lib.hook = hook
    try:
        # every ATen operator of the step (hipBLASLt GEMMs, MIOpen convolutions, element-wise / reduction kernels) is
        # bracketed the same way through a dispatch mode, so that the table prices the whole step
        detail = [] if detail_file else None
        with workmodel.aten_timer(records, detail):
            state['spin'] = lambda: spin_ms(min(1.3 * t_host * 1e3, 400.0))
            for i in range(steps):
                one(1 + i)
                torch.cuda.synchronize()
    finally:
        lib.hook = None
    if detail_file:
        per = {}
        for name, shapes, where, a, b in detail:
            e = per.setdefault((name, str(shapes), where), [0, 0.0])
            e[0] += 1
            e[1] += max(a.elapsed_time(b) - empty_ms, 0.0)
        rows = sorted(([k[0], k[1], k[2], v[0] / steps, v[1] / steps * 1e3] for k, v in per.items()), key=lambda r: -r[4])
        with open(detail_file, 'w') as fh:
            json.dump(rows, fh, indent=0)
    agg = {}
    for (kernel, bound, nbytes, flops), a, b in records:
        e = agg.setdefault(kernel, dict(kernel=kernel, bound=bound, launches=0, ms=0.0, bytes=0.0, flops=0.0))
        e['launches'] += 1
        raw = a.elapsed_time(b)
        e['ms'] += max(raw - empty_ms, 0.5 * raw)
        e['raw_ms'] = e.get('raw_ms', 0.0) + raw
        e['bytes'] += nbytes
        e['flops'] += flops
    out = {}
    for k, e in agg.items():
        n = e['launches']
        bound = e['bound']
        if bound.startswith('mfma'):
            # a GEMM family spans shapes on both sides of the ridge (the 65 536-token weight gradients stream 100 MB
            # for 14 GFLOP): the family is priced against the roofline that bounds MORE of its launches' ideal time
            t_hbm = e['bytes'] / (workmodel.HBM_PEAK_GBS * 1e9)
            t_mfma = e['flops'] / (workmodel.peak_of(bound)[0] * 1e12)
            bound = bound if t_mfma >= t_hbm else 'hbm'
        out[k] = dict(kernel=k, bound=bound, launches_per_step=n / steps, avg_ms=e['ms'] / n,
                      total_ms_per_step=e['ms'] / steps, algorithmic_bytes=e['bytes'] / n,
                      algorithmic_flops=e['flops'] / n, avg_ms_bracket=e['raw_ms'] / n, empty_bracket_ms=empty_ms)
    return out


def time_other_dtype(args, dtype, device, pool, steps, warmup, exact_f32_steps=0):
    """The same step in another compute dtype, timed the same way (graph replay, inputs resident), as a secondary
    object of the JSON line: fp32 is the precision the reference trains in (/root/reference: train_mask_bev.py:96
    `precision=32`), so the reference-precision rate is measured by the same driver run as the headline one."""
    from mask_bev_amd import synthetic
    from mask_bev_amd.graph import GraphedTrainStep
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(420)
    model = MaskBevModule(**synthetic.module_kwargs(args.workload, args.batch, compute_dtype=dtype)).to(device).train()
    model.log_scalars = False
    model.flatten_parameters()
    opt = model.configure_optimizers()['optimizer']
    g = GraphedTrainStep(model, opt, pool[0])
    for i in range(warmup):
        g.step(pool[i % len(pool)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = g.step(pool[(warmup + i) % len(pool)])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = dict(value=args.batch * steps / dt, unit='scans/s', ms_per_step=dt / steps * 1e3, steps=steps, warmup=warmup,
               dtype=dtype, final_loss=float(loss.detach()))
    g.close()
    if dtype == 'fp32':
        from mask_bev_amd import switches
        split = bool(switches.get('gemm32s'))
        # which arithmetic this figure is: f32 tensors everywhere; with K20 on, the >= 1024-token
        # products, every weight gradient, the 3 x 3 convolution, K4 and K6 multiply IEEE-half PAIRS on the 16-bit matrix pipe
        out['arithmetic'] = ('f32 storage; products from f16 hi/lo pairs (22-bit significand, lo.lo dropped), f32 accumulate '
                             '(K20 / K4 / K6 split modes)' if split else 'IEEE f32 products (library GEMMs, exact-f32 MFMA)')
        if split and exact_f32_steps > 0:
            # the same step with every product in exact f32 (library f32 GEMMs, v_mfma_f32_32x32x2_f32 in K4 / K6), fresh model
            try:
                with switches.override(gemm32s=False, k4_split=False, k6_split=False, ffn32=False, conv3x3_k20=False,
                                       tn32_group=False, msda_packed_f32=False):
                    torch.manual_seed(420)
                    m2 = MaskBevModule(**synthetic.module_kwargs(args.workload, args.batch, compute_dtype=dtype)).to(device).train()
                    m2.log_scalars = False
                    m2.flatten_parameters()
                    o2 = m2.configure_optimizers()['optimizer']
                    g2 = GraphedTrainStep(m2, o2, pool[0])
                    for i in range(min(warmup, 3)):
                        g2.step(pool[i % len(pool)])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(exact_f32_steps):
                        g2.step(pool[i % len(pool)])
                    torch.cuda.synchronize()
                    dt2 = time.perf_counter() - t0
                    g2.close()
                    del g2, m2, o2
                out['exact_f32'] = dict(value=args.batch * exact_f32_steps / dt2, ms_per_step=dt2 / exact_f32_steps * 1e3,
                                        steps=exact_f32_steps)
            except Exception as e:
                out['exact_f32'] = dict(error=f'{type(e).__name__}: {e}'[:200])
    if not args.no_kernel_profile:
        # the same per-family table for this dtype (one instrumented eager step): `roofline` = the family that costs the
        # most time per step (K3's two kernels and the optimizer pass are not bracketed here: ≈ 1.7 ms of the step)
        try:
            prof = kernel_profile(model, opt, pool[0], steps=1)
            # measured HBM bytes per launch of this dtype's families, from the committed PMC passes of the same workload
            traffic = {}
            if args.workload == 'semantic_kitti_512' and args.batch == 4 and args.distribution == 'lidar':
                for rnd in ('r06', 'r05'):
                    tf = os.path.join(ROOT, 'profiles', rnd, f'{dtype}_pmc_hbm_traffic.json')
                    if os.path.exists(tf):
                        with open(tf) as fh:
                            raw = json.load(fh)
                        traffic = {k: v for k, v in raw.items() if not k.startswith('_')}
                        for k in raw.get('_per_step', []):
                            if k in traffic and k in prof and prof[k]['launches_per_step'] > 0:
                                traffic[k] = traffic[k] / prof[k]['launches_per_step']
                        out['roofline_traffic_source'] = os.path.join('profiles', rnd, f'{dtype}_pmc_hbm_traffic.json')
                        break
            ranked = rank_profile(prof, traffic)
            out['roofline'] = ranked[0] if ranked else None
            out['roofline_all'] = [dict(kernel=r['kernel'], bound=r['bound'], frac=r['frac'],
                                        total_ms_per_step=r['total_ms_per_step'], launches_per_step=r['launches_per_step'])
                                   for r in ranked]
            out['roofline_coverage'] = sum(r['total_ms_per_step'] for r in ranked) / out['ms_per_step']
        except Exception as e:      # never take the headline number down
            out['roofline'] = dict(error=f'{type(e).__name__}: {e}')
    return out


def rank_profile(profile, traffic, skip=()):
    """`kernel_profile` output -> roofline entries ranked by time per step."""
    roof = []
    for name, e in profile.items():
        if name in skip:
            continue
        r = roofline_entry(name, e['bound'], e['avg_ms'], e['launches_per_step'], e['algorithmic_bytes'],
                           e['algorithmic_flops'], traffic.get(name),
                           'HIP events around the call (C ABI hook / ATen dispatch mode), eager step after the timed '
                           f'region, minus the empty-bracket cost ({e["empty_bracket_ms"] * 1e3:.1f} us)')
        r['avg_ms_bracket'] = e['avg_ms_bracket']
        roof.append(r)
    return sorted(roof, key=lambda r: -r['total_ms_per_step'])


def roofline_entry(kernel, bound, avg_ms, launches_per_step, nbytes, flops, traffic, source):
    """One `roofline` object: achieved = algorithmic bytes (HBM-bound kernels) or flops (MFMA-bound) of one launch
    over its average duration, against the chip peak of MI355X_MICROARCH.md."""
    from mask_bev_amd import workmodel
    peak, unit = workmodel.peak_of(bound)
    work = flops if bound.startswith('mfma') else nbytes
    achieved = work / (avg_ms * 1e-3) / (1e12 if bound.startswith('mfma') else 1e9)
    return dict(bound='mfma' if bound.startswith('mfma') else 'hbm', achieved=achieved, peak=peak, unit=unit,
                frac=achieved / peak, traffic=traffic, kernel=kernel, avg_ms=avg_ms,
                launches_per_step=launches_per_step, total_ms_per_step=avg_ms * launches_per_step,
                algorithmic_bytes=nbytes, algorithmic_flops=flops, timing=source)


LINE_LIMIT = 4096      # the driver keeps the tail of stdout: the ONE JSON line must fit it whole (a 35.8 KB
                       # line with `roofline_all` x 2 dtypes came back `parsed: null`)


def _short(x, digits=6):
    """Floats to `digits` significant digits (the line is read by people and parsers, not re-used as input)."""
    if isinstance(x, float):
        return float(f'{x:.{digits}g}')
    if isinstance(x, dict):
        return {k: _short(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_short(v, digits) for v in x]
    return x


def _roofline_object(r):
    """The contract's `roofline` object + the few fields that say which kernel it is and what it costs per step."""
    if not isinstance(r, dict) or 'frac' not in r:
        return r
    keep = ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'kernel', 'avg_ms', 'launches_per_step',
            'total_ms_per_step', 'algorithmic_bytes', 'algorithmic_flops')
    return {k: r.get(k) for k in keep}


def compact_line(full: dict, detail_path=None) -> dict:
    """The ONE line rank 0 prints last: every key of the bench contract, `roofline` (dominant family), `roofline_coverage`,
    `step_roofline`, the reference-precision `fp32` figure with its own `roofline`, `cpu_baseline` (one row), and — instead
    of the per-family tables, which go to `detail_path` — the five families that cost the most time and the one that sits
    furthest below its roofline.  Always shorter than LINE_LIMIT bytes: optional pieces are dropped in a fixed order
    until it is."""
    top = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
           'vs_baseline', 'dtype', 'data')
    line = {k: full.get(k) for k in top}
    cfg = dict(full.get('config') or {})
    line['config'] = cfg
    line['roofline'] = _roofline_object(full.get('roofline'))
    ranked = full.get('roofline_all') or []
    if ranked:
        line['roofline_top'] = [dict(kernel=r['kernel'], bound=r['bound'], frac=r['frac'],
                                     ms_per_step=r['total_ms_per_step']) for r in ranked[:5]]
        priced = [r for r in ranked if r.get('frac') and r['total_ms_per_step'] >= 0.05]
        if priced:
            w = min(priced, key=lambda r: r['frac'])
            line['roofline_worst'] = dict(kernel=w['kernel'], bound=w['bound'], frac=w['frac'],
                                          ms_per_step=w['total_ms_per_step'])
    line['roofline_coverage'] = full.get('roofline_coverage')
    line['roofline_traffic_source'] = full.get('roofline_traffic_source')
    line['roofline_traffic_measured_in_run'] = False       # `traffic` = the committed PMC passes of the same workload, not this run
    line['roofline_detail'] = detail_path
    sr = full.get('step_roofline')
    if sr:
        line['step_roofline'] = {k: sr[k] for k in ('flops_per_scan', 'bytes_per_scan', 'achieved_tflops', 'frac_mfma',
                                                    'achieved_gbs', 'frac_hbm') if k in sr}
    f32 = full.get('fp32')
    if f32:
        line['fp32'] = {k: (_roofline_object(v) if k == 'roofline' else v) for k, v in f32.items()
                        if k in ('value', 'unit', 'ms_per_step', 'steps', 'warmup', 'dtype', 'roofline',
                                 'roofline_coverage', 'error', 'arithmetic', 'exact_f32', 'roofline_traffic_source')}
    if full.get('collectives'):
        line['collectives'] = full['collectives']
    cb = full.get('cpu_baseline')
    if cb:
        cb = dict(cb)
        rows = cb.pop('rows', None) or []
        if rows:
            r = rows[0]
            cb['row'] = {k: r.get(k) for k in ('threads', 'iterations', 'fwd_bwd_s', 'fwd_s', 'fwd_scans_per_s', 'note')}
        line['cpu_baseline'] = cb
    line = _short(line)
    # unbounded strings (an exception text in fp32.error / roofline.error / cpu_baseline.sample) are cut, never fatal
    def _clip(node):
        for k, v in list(node.items()):
            if isinstance(v, dict):
                _clip(v)
            elif isinstance(v, str) and len(v) > 300:
                node[k] = v[:297] + '...'
    _clip(line)
    for drop in (('collectives', 'schedule'), ('roofline_top',), ('cpu_baseline', 'row'), ('fp32', 'roofline'),
                 ('roofline_worst',), ('config', 'switches'), ('step_roofline',)):
        if len(json.dumps(line)) < LINE_LIMIT:
            break
        node = line
        for k in drop[:-1]:
            node = node.get(k) or {}
        node.pop(drop[-1], None)
    if len(json.dumps(line)) >= LINE_LIMIT:      # last resort: the contract keys alone (the full record is in the detail file)
        line = {k: line.get(k) for k in top + ('config', 'roofline', 'cpu_baseline', 'roofline_detail')}
        line['config'] = {'workload': (line.get('config') or {}).get('workload')}
        line['truncated'] = True
    return line


def write_detail(full: dict, path=None):
    """The whole record (every family of both dtypes, every CPU-baseline row) as a JSON file beside the run; returns
    the path written, relative to the repository, or None when it cannot be written (never fatal)."""
    path = path or os.path.join('gpurun_out', 'bench_detail.json')
    try:
        target = path if os.path.isabs(path) else os.path.join(ROOT, path)
        os.makedirs(os.path.dirname(target), exist_ok=True)
        with open(target, 'w') as fh:
            json.dump(full, fh)
        return path
    except OSError:
        return None


def collectives_schedule(last, world: int) -> dict:
    """Host-side launch schedule of the last step: (mark, ms after the first graph replay was issued, MB reduced)."""
    t0m = last[0][1]
    total = sum(nb for _, _, nb in last)
    return dict(
        backend=os.environ.get('MBV_DIST_BACKEND', 'nccl'), world_size=world, bytes_per_step=total,
        schedule=[dict(mark=name, ms=round((t - t0m) * 1e3, 3), mb=round(nb / 1e6, 2)) for name, t, nb in last],
        note='host launch times: a piece is launched as soon as the host has issued the work that completes its '
             'gradients; on the device it waits for that work through stream order (the comm stream waits for '
             'the compute stream at launch)')


def _flush_c_stdio(needed: bool) -> None:
    """RCCL prints its version banner through C stdio, which is fully buffered on a pipe: push it out before the JSON
    line, so that the line stays the LAST line of stdout."""
    if not needed:
        return
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


DUMP_SAMPLE = 1 << 22      # model-state values kept by `dump_outputs`: 16 MB of float32


def dump_outputs(out_dir: str, model, loss) -> None:
    """What a caller of the timed step holds after its last step — the loss the step returns and the model state its
    AdamW update leaves — as float32 / float64 ``.npy`` files in `out_dir` (< 20 MB in all):

      loss.npy          float32 (1,)   the loss of the last timed step
      state_sums.npy    float64 (T, 2) sum and sum of |x| of every floating tensor of ``model.state_dict()``, in its order
      state_sample.npy  float32 (S,)   the values at DUMP_SAMPLE fixed positions (seed 0, ascending) of those tensors
                                       flattened and concatenated in the same order (all of them if there are fewer)

    The inputs and the initial state are the same in every run with the same arguments, but the step is not bit-exact
    from process to process (some gradients meet through f32 atomics): two runs of one build agree to a tolerance
    (bench workload, 25 steps: the loss within ≈ 0.5 %), not bit for bit."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    state = [t.detach() for t in model.state_dict().values() if t.is_floating_point()]
    np.save(os.path.join(out_dir, 'loss.npy'), np.asarray([float(loss.detach())], dtype=np.float32))
    sums = torch.stack([torch.stack([t.double().sum(), t.double().abs().sum()]) for t in state])
    np.save(os.path.join(out_dir, 'state_sums.npy'), sums.cpu().numpy().astype(np.float64))
    flat = torch.cat([t.reshape(-1).float() for t in state])
    if flat.numel() > DUMP_SAMPLE:
        idx = torch.randint(0, flat.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
        flat = flat[idx.to(flat.device)]
    np.save(os.path.join(out_dir, 'state_sample.npy'), flat.cpu().numpy().astype(np.float32))


def main():
    args = parse()
    from mask_bev_amd import switches
    for item in args.switch:
        name, _, value = item.partition('=')
        switches.set_value(name.strip().lower(), value.strip())
    if args.cpu_baseline_worker:
        cpu_baseline_worker(args.cpu_baseline_worker, args.workload, args.cpu_threads, args.cpu_baseline_budget_s)
        return
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world != args.gpus and world == 1 and args.gpus > 1:
        # launched without torchrun: spawn it as a child and exit with its code
        import subprocess
        port = free_port()
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}',
               '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X (no CPU fallback for the product path)')
    ndev = torch.cuda.device_count()
    dev_index = local_rank % max(1, ndev)      # one rank per GPU; wraps only in the single-GPU smoke test of the N > 1 path
    torch.cuda.set_device(dev_index)
    device = torch.device('cuda', dev_index)
    import torch.distributed as dist
    force = args.force_reducer and world == 1
    if force:
        args.dry_run_collectives = True
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(free_port()))
        os.environ.update(RANK='0', WORLD_SIZE='1')
    if world > 1 or force:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        backend = os.environ.get('MBV_DIST_BACKEND', 'nccl')      # 'nccl' is RCCL on ROCm; gloo only for smoke tests
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=device)
        else:
            dist.init_process_group(backend)

    from mask_bev_amd import ops, synthetic, tuning
    from mask_bev_amd.mask_bev_module import MaskBevModule

    torch.manual_seed(420)
    kw = synthetic.module_kwargs(args.workload, args.batch, compute_dtype=args.dtype)
    tuned = tuning.use_tuned_gemms(args.gemm_table)     # hipBLASLt solution table for this step's GEMM shapes (look-up only)
    model = MaskBevModule(**kw).to(device)
    model.train()
    model.log_scalars = False           # scalar logging is host-side bookkeeping, not the path
    if not args.no_arena:
        model.flatten_parameters()      # flat param / grad / bf16-shadow arena + single-launch AdamW (K11)
    opt = model.configure_optimizers()['optimizer']
    reducer = None
    if world > 1 or force:
        from mask_bev_amd.ddp import GradientAllReducer
        reducer = GradientAllReducer(model, bucket_mb=64.0,
                                     grad_dtype=torch.bfloat16 if args.grad_wire == 'bf16' else None)
        if getattr(model, '_arena', None) is not None:
            model._arena.refresh_shadow()       # the construction-time parameter broadcast wrote the f32 arena
            # arena gradients are accumulated in place, once per USE of a parameter (a packed in_proj weight is used
            # by three projections): the per-parameter ready-hooks of the bucketed reducer do not apply — the arena
            # is reduced in contiguous ranges after (graph step: during) the backward
            reducer.no_sync(True)

    pool = [synthetic.make_batch(args.workload, args.batch, rank, s, device, args.distribution)
            for s in range(args.pool)]
    torch.cuda.synchronize()

    graphed = None
    if not args.no_graph:
        from mask_bev_amd.graph import GraphedTrainStep
        if reducer is not None:
            reducer.no_sync(True)          # gradients are averaged after the replay, not from hooks inside it
        graphed = GraphedTrainStep(model, opt, pool[0], reducer=reducer)

    def step(i: int):
        scans, gt = pool[i % len(pool)]
        if graphed is not None:
            return graphed.step((scans, gt))
        if reducer is not None:
            reducer.sync_buffers()
        loss = model.training_step((scans, gt), i)
        model.scale_loss(loss).backward()
        if reducer is not None:
            if getattr(model, '_arena', None) is not None:
                reducer.reduce_arena(model._arena, opt)
            else:
                reducer.finish()
        opt.step()
        opt.zero_grad(set_to_none=args.no_arena)
        return loss

    for i in range(args.warmup):
        step(i)
    if args.dry_run_collectives and graphed is not None:
        graphed.trace = []
    ops.TIMER.reset()
    ops.TIMER.enabled = args.full           # the in-region events of the roofline table
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(args.warmup + i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ops.TIMER.enabled = False
    if world > 1:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    final_loss = float(loss.detach())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, loss)      # before anything else runs a step on the model
    w = synthetic.WORKLOADS[args.workload]
    nx = int((w['x_range'][1] - w['x_range'][0]) / w['voxel_size'])
    ny = int((w['y_range'][1] - w['y_range'][0]) / w['voxel_size'])
    k3_fused = bool(graphed is not None and getattr(graphed, '_k3_fused', False))
    line = dict(
        # BASELINE.json's metric on its own workload; the other BASELINE configs name their shape in the same form
        metric=('LiDAR scans/sec fwd+bwd, 120k-pt 512x512 BEV 100q' if args.workload == 'semantic_kitti_512' else
                f'LiDAR scans/sec fwd+bwd, {w["points"] // 1000}k-pt {ny}x{nx} BEV {w["num_queries"]}q'),
        value=args.batch * world * args.steps / dt,
        unit='scans/s', n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=dt / args.steps * 1e3,
        higher_is_better=True, scaling='weak', vs_baseline=None, dtype=args.dtype, data='synthetic' if args.distribution == 'lidar' else 'synthetic (uniform x/y points)',
        config=dict(workload=f'{args.workload}: {w["points"]} pts/scan, {ny}x{nx} BEV, {w["num_queries"]} queries',
                    scans_per_gpu=args.batch, global_batch=args.batch * world, parallelism=f'dp{world}',
                    step='fwd + Hungarian loss + bwd + AdamW; inputs device-resident', launch='eager' if args.no_graph else 'hip-graph', tuned_gemm_table=tuned, grad_wire=(args.grad_wire if (world > 1 or force) else None),
                    forced_reducer=True if force else None, replica_param_checksum_spread=None,
                    final_loss=final_loss, k3_adam_fused=k3_fused or None,
                    switches={k: v for k, v in switches._values.items() if v != switches.defaults()[k]}))
    if not args.full:
        if rank == 0:
            if args.dry_run_collectives and graphed is not None and graphed.trace:
                line['collectives'] = collectives_schedule(graphed.trace[-1], world)
            _flush_c_stdio(world > 1 or force)
            print(json.dumps(_short(line)), flush=True)
        if world > 1 or force:
            dist.destroy_process_group()
        return
    profile = {}
    if world == 1 and not args.no_kernel_profile:
        profile = kernel_profile(model, opt, pool[0], detail_file=args.aten_detail)
    fp32_line = None
    if world == 1 and args.dtype != 'fp32' and not args.no_fp32 and not args.no_graph and not args.no_arena:
        try:
            fp32_line = time_other_dtype(args, 'fp32', device, pool, min(args.steps, 50), min(args.warmup, 5),
                                         exact_f32_steps=min(args.steps, 20))
        except Exception as e:      # the secondary figure must never take the headline number down with it
            fp32_line = dict(value=None, error=f'{type(e).__name__}: {e}')
    replica_spread = None
    if world > 1:
        # data-parallel sanity, outside the timed region: every rank must hold the same parameters after the run
        cs = torch.stack([p.detach().double().sum() for p in model.parameters()]).sum().reshape(1)
        lo, hi = cs.clone(), cs.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        replica_spread = float((hi - lo).item())

    if rank == 0:
        c = kw['encoder_feat_channels'][-1]
        times = ops.TIMER.summary_ms()
        # algorithmic HBM bytes per launch: fwd reads weight+bias once per batch and writes the
        # output; bwd reads grad_out and weight, writes grad_weight+grad_bias.  V*C*4 pillar rows are < 2 % and
        # left out (stated in DESIGN.md), as is the 4 B/cell map.
        cells = nx * ny
        acc = 0 if args.no_arena else 2 * c * cells          # arena: d(weight), d(bias) are read and accumulated into
        n_params = sum(p.numel() for p in model.parameters())
        # bf16 compute: the map leaves K3 (and its gradient comes back) as the backbone's bf16 patch rows
        io = 2.0 if model._patch_handoff() else 4.0
        # round 6, one GPU: the AdamW update of the two (C, ny, nx) affine parameters runs inside K3's backward — per
        # parameter it reads param + 2 moments and writes them + the 16-bit shadow (26 B) instead of the gradient round
        # trip; the optimizer pass proper covers the other parameters, in however many launches it took (the family's
        # bytes PER LAUNCH = the pass's bytes / launches per step)
        adam_launches = max(1.0, len(times.get('k_adamw') or []) / max(1, args.steps))
        adam_params = n_params - (2 * c * cells if k3_fused else 0)
        algo = {'k_ln_apply': 2 * c * cells * 4.0 + args.batch * c * cells * io,
                'k_ln_bwd_dense': (args.batch * c * cells * io + 2 * c * cells * 26.0) if k3_fused else
                                  (args.batch * c * cells * io + (c * cells + 2 * c * cells + acc) * 4.0),
                # K11: read param, grad, exp_avg, exp_avg_sq; write param, exp_avg, exp_avg_sq, zeroed grad, bf16 shadow
                'k_adamw': adam_params * (16.0 + 16.0 + 2.0) / adam_launches}
        # HBM bytes per launch measured with the PMC counters (separate FETCH_SIZE / WRITE_SIZE passes, FETCH_SIZE
        # doubled: the gfx950 correction of MI355X_MICROARCH.md), same workload: profiles/rNN/pmc_hbm_traffic.json
        traffic, traffic_file = {}, None
        for rnd in ('r06', 'r05', 'r04', 'r03'):                      # the latest round that holds a PMC pass of this workload
            traffic_file = os.path.join('profiles', rnd, 'pmc_hbm_traffic.json')
            if os.path.exists(os.path.join(ROOT, traffic_file)):
                break
        if (args.workload == 'semantic_kitti_512' and args.batch == 4 and not args.no_arena and io == 2.0
                and args.distribution == 'lidar' and os.path.exists(os.path.join(ROOT, traffic_file))):
            with open(os.path.join(ROOT, traffic_file)) as fh:
                raw = json.load(fh)
            traffic = {k: v for k, v in raw.items() if not k.startswith('_')}
            for k in raw.get('_per_step', []):      # group launches at the end of a backward: recorded per step
                if k in traffic and k in profile and profile[k]['launches_per_step'] > 0:
                    traffic[k] = traffic[k] / profile[k]['launches_per_step']
        roof = {}
        for name, ms in times.items():          # in-library / in-stream events recorded inside the timed region
            if not ms or name not in algo:
                continue
            avg = sum(ms) / len(ms)
            roof[name] = roofline_entry(name, 'hbm', avg, len(ms) / args.steps, algo[name], 0.0, traffic.get(name),
                                        'HIP events inside the timed region')
        for r in rank_profile(profile, traffic, skip=set(roof)):      # the instrumented eager step after the timed region
            roof[r['kernel']] = r
        ranked = sorted(roof.values(), key=lambda r: -r['total_ms_per_step'])
        dominant = ranked[0] if ranked else None      # the kernel that costs the most time per step
        # whole-step figure: algorithmic work per scan of the S2 configuration — 0.97 TFLOP and 4.5 GB
        # forward + backward, plus the optimizer pass shared by the scans of a step — against the chip peaks
        step_roof = None
        if args.workload == 'semantic_kitti_512':
            sps = args.batch * args.steps / dt                        # scans per second on this GPU
            bytes_scan = 4.5e9 + algo['k_adamw'] / args.batch
            step_roof = dict(flops_per_scan=0.97e12, achieved_tflops=0.97 * sps, mfma_peak_tflops=2500.0,
                             frac_mfma=0.97 * sps / 2500.0, bytes_per_scan=bytes_scan,
                             achieved_gbs=bytes_scan * sps / 1e9, hbm_peak_gbs=8000.0,
                             frac_hbm=bytes_scan * sps / 1e9 / 8000.0)
        line['config']['replica_param_checksum_spread'] = replica_spread
        line.update(
            roofline=dominant, roofline_all=ranked, roofline_traffic_source=traffic_file if traffic else None,
            # share of the step the table prices: sum of the families' time per step over the measured step time
            roofline_coverage=sum(r['total_ms_per_step'] for r in ranked) / (dt / args.steps * 1e3) if ranked else None,
            step_roofline=step_roof)
        if fp32_line is not None:
            line['fp32'] = fp32_line
        if args.dry_run_collectives and graphed is not None and graphed.trace:
            line['collectives'] = collectives_schedule(graphed.trace[-1], world)
        if not args.no_cpu_baseline and world == 1:
            try:
                line['cpu_baseline'] = cpu_baseline(args.workload, model, args.cpu_baseline_budget_s)
            except Exception as e:  # the baseline must never take the GPU number down with it
                line['cpu_baseline'] = dict(value=None, unit='scans/s', cores=os.cpu_count(), kind='port',
                                            sample=f'failed: {type(e).__name__}: {e}')
        detail_path = write_detail(line, args.detail_out)
        _flush_c_stdio(world > 1 or force)
        print(json.dumps(compact_line(line, detail_path)), flush=True)
    if world > 1 or force:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
