"""K34 measurement: ``SemanticKittiRasterizer.rasterize_bank`` (one native call per batch on a scene bank that stays on the
device) against the route the package had before it for the same scenes — lists of per-scan device tensors through
``SemanticKittiRasterizer.rasterize_batch``, which concatenates them with ``torch.cat`` and makes one ``mbv_rasterize`` call per
sample — at B = 4 on the SemanticKITTI grid (500 x 500 cells of 0.16 m, k = 9), a synthetic bank of 4 000 scans x 8 000 points,
300 and 60 selected scans per sample.  The two routes are timed alternately in one process and their maps compared.  Also: the
two phases of the call alone (binning = the streaming stage, morphology + paint), the bytes the streaming stage needs over its
time against the 8 TB/s of the project's rooflines, and the wall time of ``--build-mask-cache`` per scan on a synthetic tree.
No real SemanticKITTI scan is read anywhere.  Prints one JSON line and writes it to the path given as the first argument
(default: k34_measure.json beside this file).  ``--dry`` builds a tiny bank and its tables on the CPU and stops (no timing); ``--trace`` makes ten calls of each route at the
300-scan shape and stops, for a kernel trace taken in a run of its own."""
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mask_bev_amd import datasets, ops                                    # noqa: E402
from mask_bev_amd.rasterize import SemanticKittiRasterizer                # noqa: E402
from mask_bev_amd.scene_bank import SceneBank                             # noqa: E402
from tests import scene_bank_util as U                                    # noqa: E402

DRY = '--dry' in sys.argv
TRACE = '--trace' in sys.argv
args = [a for a in sys.argv[1:] if a not in ('--dry', '--trace')]
dev = torch.device('cpu' if DRY else 'cuda:0')
RANGES, VS, K, B = ((-40.0, 40.0), (-40.0, 40.0), (-3.0, 1.0)), 0.16, 9, 4
N_SCANS, PER_SCAN = (40, 500) if DRY else (4000, 8000)
STEP = 0.1                                                                # metres the vehicle moves per scan


def pose(s):
    return U.pose_2d(STEP * s, 0.0, 0.3 * np.sin(s / 300.0))


def make_bank():
    """Cars of 4 m x 1.8 m every 2 m along the road, up to 35 m to either side; every scan sees PER_SCAN points of the cars within
    38 m of it along the road, stored in the scan's own frame."""
    gen = torch.Generator(device=dev).manual_seed(34)
    n_cars = int(N_SCANS * STEP / 2) + 40
    car_xy = torch.stack([2.0 * torch.arange(n_cars, device=dev, dtype=torch.float64) - 40.0,
                          (torch.rand(n_cars, generator=gen, device=dev, dtype=torch.float64) * 2 - 1) * 35.0], 1)
    pts, ids = [], []
    for s0 in range(0, N_SCANS, 250):
        s = torch.arange(s0, min(s0 + 250, N_SCANS), device=dev).repeat_interleave(PER_SCAN)
        n = s.numel()
        ego_x = STEP * s.to(torch.float64)
        yaw = 0.3 * torch.sin(s.to(torch.float64) / 300.0)
        along = ego_x + (torch.rand(n, generator=gen, device=dev, dtype=torch.float64) * 2 - 1) * 38.0
        car = ((along + 40.0) / 2.0).floor().long().clamp(0, n_cars - 1)
        box = (torch.rand((n, 2), generator=gen, device=dev, dtype=torch.float64) - 0.5) * torch.tensor([4.0, 1.8], device=dev,
                                                                                                    dtype=torch.float64)
        w = car_xy[car] + box
        dx, dy = w[:, 0] - ego_x, w[:, 1]
        c, si = torch.cos(yaw), torch.sin(yaw)
        local = torch.stack([c * dx + si * dy, -si * dx + c * dy, torch.full_like(dx, -1.0)], 1)
        pts.append(local.to(torch.float32))
        ids.append((car + 1).to(torch.int32))
    return SceneBank(torch.cat(pts), torch.cat(ids), np.arange(N_SCANS + 1, dtype=np.int64) * PER_SCAN, device=dev)


def scenes_of(n_selected):
    """B scenes of ``n_selected`` scans, every other scan around the centre: not a contiguous range of the bank."""
    out = []
    for b in range(B):
        centre = (b + 1) * N_SCANS // (B + 1)
        scans = np.arange(centre - n_selected, centre + n_selected, 2)
        scans = scans[(scans >= 0) & (scans < N_SCANS)]
        tf = np.stack([np.linalg.inv(pose(centre)) @ pose(int(s)) for s in scans])
        out.append((scans, tf, centre))
    return out


def timed_alternating(fns, iters, reps, warm):
    """Every function ``iters`` times between two events, the functions taking turns, ``reps`` rounds → {name: [ms per call]}."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    return ms


def stats(ms, **extra):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), **extra)


bank = make_bank()
r = SemanticKittiRasterizer(*RANGES, VS, morph_kernel_size=K)
if DRY:
    tables = r.bank_tables(bank, scenes_of(6))
    print('dry run:', bank.points.shape, [np.asarray(t).shape for t in tables], ops.bank_chunks(tables[1], tables[2]).shape)
    sys.exit(0)

if TRACE:
    scenes = scenes_of(300)
    lists = [([bank.scan(s)[0] for s in sc], [bank.scan(s)[1] for s in sc], tf) for sc, tf, _ in scenes]
    for _ in range(10):
        r.rasterize_bank(bank, scenes)
        r.rasterize_batch(lists)
    torch.cuda.synchronize()
    sys.exit(0)

res = dict(grid=[r.nx, r.ny], voxel_size=VS, morph_kernel_size=K, batch=B, bank_scans=N_SCANS, bank_points=int(bank.points.shape[0]),
           bank_bytes=bank.nbytes, real_semantic_kitti_used=False, shapes={})
for n_selected in (300, 60):
    scenes = scenes_of(n_selected)
    lists = [([bank.scan(s)[0] for s in sc], [bank.scan(s)[1] for s in sc], tf) for sc, tf, _ in scenes]
    points = int(sum(len(bank.scan(s)[1]) for sc, _, _ in scenes for s in sc))
    tables = r.bank_tables(bank, scenes)
    ws = ops.rasterize_bank(bank.points, bank.inst, *tables, *RANGES, VS, r.nx, r.ny, K)[2]
    got, want = r.rasterize_bank(bank, scenes), r.rasterize_batch(lists)
    torch.cuda.synchronize()
    fns = {'rasterize_bank': lambda: r.rasterize_bank(bank, scenes),
           'rasterize_batch_of_lists': lambda: r.rasterize_batch(lists),
           'bank_binning_phase': lambda: ops.rasterize_bank(bank.points, bank.inst, *tables, *RANGES, VS, r.nx, r.ny, K, phases=1,
                                                            workspace=ws),
           'bank_paint_phase': lambda: ops.rasterize_bank(bank.points, bank.inst, *tables, *RANGES, VS, r.nx, r.ny, K, phases=2,
                                                          workspace=ws)}
    ms = timed_alternating(fns, 20, 7, 3)
    wall = {}
    for name in ('rasterize_bank', 'rasterize_batch_of_lists'):          # host clock around calls that end in a synchronise
        t = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[name]()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        wall[name] = stats(t, reps=7)
    needed = 2 * 16 * points                  # both passes of the binning read 12 bytes of coordinates and 4 of id per point
    binning = statistics.median(ms['bank_binning_phase'])
    res['shapes'][f'{n_selected}_scans_per_sample'] = dict(
        selected_points=points, segments=int(sum(len(sc) for sc, _, _ in scenes)),
        chunks=int(len(ops.bank_chunks(tables[1], tables[2]))), instances_per_map=[int(len(torch.unique(m)) - 1) for m in got],
        maps_equal=bool(torch.equal(got, want)),
        ms_per_call_by_events={k: stats(v, iters=20, reps=7) for k, v in ms.items()},
        ms_per_call_wall_with_sync=wall,
        speedup_median=statistics.median(ms['rasterize_batch_of_lists']) / statistics.median(ms['rasterize_bank']),
        binning_needed_bytes=needed, binning_bytes_per_second=needed / (binning * 1e-3),
        binning_share_of_8TBs=needed / (binning * 1e-3) / 8e12)

# --build-mask-cache on a synthetic tree: 200 scans of 10 000 points (8 000 of them on 40 cars), every scan in every scene
with tempfile.TemporaryDirectory() as tmp:
    root = pathlib.Path(tmp)
    rng = np.random.default_rng(34)
    cars = [(float(x), float(y)) for x, y in zip(rng.uniform(-30, 90, 40), rng.uniform(-35, 35, 40))]
    poses, scans, words = U.drive(rng, 200, cars, 3.0, (40.0, 40.0), n_car=200, n_other=2000)
    U.write_sequence(root / 'sequences' / '00', poses, scans, words)
    cfg = dict(x_range=RANGES[0], y_range=RANGES[1], z_range=RANGES[2], voxel_size=VS)
    t0 = time.perf_counter()
    datasets.build_scene_banks(cfg, root, [0])
    t1 = time.perf_counter()
    written = datasets.build_mask_cache(cfg, dev, root, [0])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    first = np.load(written[0])
    res['build_mask_cache_synthetic_tree'] = dict(scans=len(written), points_per_scan=10000, kept_points_per_scan=8000,
                                                  scans_per_scene=200, build_scene_bank_ms_per_scan=(t1 - t0) * 1e3 / len(written),
                                                  build_mask_cache_ms_per_scan=(t2 - t1) * 1e3 / len(written),
                                                  instances_in_first_map=int(len(np.unique(first)) - 1), dtype=str(first.dtype))

target = args[0] if args else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'k34_measure.json')
with open(target, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
