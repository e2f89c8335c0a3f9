"""K38 measurement.  Prints one JSON line and writes it to the path given as the first argument (default: k38_measure.json
beside this file).

K38a: ``ops.visibility_map`` on LiDAR-shaped synthetic scans (``synthetic.lidar_scan``, 64 beams, the sensor 1.73 m over flat
ground, walls at random ranges) at the SemanticKITTI (512 x 512, the sensor in the middle) and the KITTI (496 x 432 as
(ny, nx), the sensor on the x = 0 edge) grids of the shipped configurations, batch 1 and 4: the targets, the mean ray length,
the share of PASSED / HIT / unknown cells, equality with the numpy restatement at batch 1, and the time of a call from device
events.  ``--k38a-only --shape=N`` runs only the calls of shape N (20 after 5 warm-up calls): the run a kernel trace is taken of.

K38b: the tracker step per frame on the 512 x 512 / 100-query maps of profiles/k37/measure_k37.py (8 frames per call,
``track_map=True``) with a visibility map whose columns are unknown in stripes, in alternating windows of one process:
``mbv_track_frames_occluded`` with the maps (on), the same entry with visibility NULL (off), this tree's
``mbv_track_frames_motion``, and — with ``--parent-lib PATH``, the parent commit's library built elsewhere —
the parent's ``mbv_track_frames_motion`` on the same tensors.  All four are called through ctypes with the same per-call
allocations."""
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
PARENT = None
if '--parent-lib' in sys.argv:
    PARENT = os.path.abspath(sys.argv[sys.argv.index('--parent-lib') + 1])
    ARGS.remove(sys.argv[sys.argv.index('--parent-lib') + 1])
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mask_bev_amd import _lib, ops, synthetic                             # noqa: E402
from mask_bev_amd.ops_core import _ptr, _stream, _workspace               # noqa: E402
from mask_bev_amd.ops_encoder import VoxelGeometry                        # noqa: E402

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


def geometry(workload):
    w = synthetic.WORKLOADS[workload]
    r = [w['x_range'][0], w['y_range'][0], w['z_range'][0], w['x_range'][1], w['y_range'][1], w['z_range'][1]]
    return VoxelGeometry.from_ranges(r, [w['voxel_size'], w['voxel_size'], w['z_range'][1] - w['z_range'][0]]), w


def k38a(workload, batch, timed=True, check=False):
    geom, w = geometry(workload)
    gen = torch.Generator(device=dev).manual_seed(38)
    scans = [synthetic.lidar_scan(w['points'], w['pc_point_dim'], gen, dev) for _ in range(batch)]
    run = lambda: ops.visibility_map(scans, geom)
    vis = run()
    torch.cuda.synchronize()
    out = dict(grid_ny_nx=[int(geom.grid[1]), int(geom.grid[0])], batch=batch, points_per_scan=int(scans[0].shape[0]))
    if not timed:
        for _ in range(WARM - 1):
            run()
        torch.cuda.synchronize()
        for _ in range(ITERS):
            run()
        torch.cuda.synchronize()
        return out
    ocx, ocy = ops.origin_cell(geom, (0.0, 0.0, 0.0))
    hit = (vis & ops.VIS_HIT) != 0
    ty, tx = torch.nonzero(hit[0], as_tuple=True)
    n = torch.maximum((tx - ocx).abs(), (ty - ocy).abs())
    cells = vis[0].numel()
    out.update(origin_cell=[ocx, ocy], targets_scan0=int(hit[0].sum()), mean_ray_cells_scan0=float(n.float().mean()),
               max_ray_cells_scan0=int(n.max()), samples_scan0=int(n.sum()),
               passed_share=float(((vis[0] & ops.VIS_PASSED) != 0).sum()) / cells, hit_share=float(hit[0].sum()) / cells,
               unknown_share=float((vis[0] == 0).sum()) / cells)
    if check:
        from tests import visibility_ref as V
        ref = V.visibility_map([scans[0].cpu().numpy()], geom.pc_range, geom.voxel_size, geom.grid, ocx, ocy, 0.0, -0.2)
        out['equals_restatement'] = bool(ref.tobytes() == vis[:1].cpu().numpy().tobytes())
    for _ in range(WARM):
        run()
    torch.cuda.synchronize()
    out['call_ms'] = stats([window(run, ITERS) for _ in range(WINDOWS)], iters=ITERS, windows=WINDOWS)
    return out


def moved_left(x, cells):
    out = torch.full_like(x, -1)
    out[:, :x.shape[1] - cells] = x[:, cells:]
    return out


def k38b(workload='semantic_kitti_512', p=256):
    """The maps of profiles/k37/measure_k37.py; visibility: unknown in stripes of 32 of every 96 columns, PASSED elsewhere."""
    w = synthetic.WORKLOADS[workload]
    vs, q = w['voxel_size'], w['num_queries']
    n = int((w['x_range'][1] - w['x_range'][0]) / vs)
    gen = torch.Generator(device=dev).manual_seed(33)
    _, masks = synthetic.gt_masks(1, q, n, n, gen, dev, k_range=(min(40, q), min(40, q)), cell=vs)
    ids = torch.arange(1, q + 1, device=dev, dtype=torch.float32).view(1, q, 1, 1)
    world = (masks * ids).amax(1)[0].to(torch.int64) - 1
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
    inv = ops.invert_transforms(tf)
    vis = torch.ones((FRAMES, n, n), dtype=torch.uint8, device=dev)
    vis[:, :, (torch.arange(n, device=dev) % 96) < 32] = 0
    x_lo, y_lo = float(w['x_range'][0]), float(w['y_range'][0])
    motion, occlusion = ops.MotionSettings(), ops.OcclusionSettings()

    def fresh(with_occlusion):
        s = ops.TrackState.fresh(n, n, p, dev)
        s.motion = ops.TrackMotion.fresh(p, dev)
        if with_occlusion:
            s.occlusion = ops.TrackOcclusion.fresh(p, dev)
        return s

    s_on, s_off, s_motion, s_parent = fresh(True), fresh(True), fresh(False), fresh(False)
    here = _lib.load()
    shift = motion.max_shift(vs)
    num, den = occlusion.hidden_fraction

    # Every path is the C entry itself with the same per-call allocations (what ops.track_frames allocates), so the windows
    # compare the launches and not the Python in front of them.
    def outputs():
        return (torch.empty((FRAMES, q), dtype=torch.int32, device=dev), torch.empty((FRAMES, n, n), dtype=torch.int32, device=dev),
                torch.empty((FRAMES, q, 2), dtype=torch.float64, device=dev))

    def motion_call(lib, s):
        ws = _workspace(lib.mbv_track_frames_motion_workspace_bytes(n, n, q, p), dev)

        def run():
            qt, tm, qv = outputs()
            rc = lib.mbv_track_frames_motion(_ptr(maps), _ptr(tf), _ptr(inv), FRAMES, n, n, x_lo, y_lo, vs, q, p, 0.3, 2, 4, motion.gain,
                                             motion.gate_m, shift, _ptr(s.state_map), _ptr(s.live_id), _ptr(s.live_seen),
                                             _ptr(s.counters), _ptr(s.motion.pos), _ptr(s.motion.vel), _ptr(s.motion.motion_counters),
                                             _ptr(qt), _ptr(tm), _ptr(qv), _ptr(ws), ws.numel(), _stream())
            assert rc == 0
            return qt
        return run

    def occluded_call(s, visibility):
        ws = _workspace(here.mbv_track_frames_occluded_workspace_bytes(n, n, q, p), dev)

        def run():
            qt, tm, qv = outputs()
            rc = here.mbv_track_frames_occluded(_ptr(maps), _ptr(tf), _ptr(inv), _ptr(visibility), FRAMES, n, n, x_lo, y_lo, vs, q, p,
                                                0.3, 2, 4, motion.gain, motion.gate_m, shift, num, den, occlusion.max_hold,
                                                _ptr(s.state_map), _ptr(s.live_id), _ptr(s.live_seen), _ptr(s.occlusion.live_held),
                                                _ptr(s.counters), _ptr(s.motion.pos), _ptr(s.motion.vel),
                                                _ptr(s.motion.motion_counters), _ptr(s.occlusion.occlusion_counters), _ptr(qt),
                                                _ptr(tm), _ptr(qv), _ptr(ws), ws.numel(), _stream())
            assert rc == 0
            return qt
        return run

    runs = dict(occluded_on=occluded_call(s_on, vis), occluded_off=occluded_call(s_off, None),
                motion_this_tree=motion_call(here, s_motion))
    if PARENT:
        parent = ctypes.CDLL(PARENT)
        for name in ('mbv_track_frames_motion', 'mbv_track_frames_motion_workspace_bytes'):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        runs['motion_parent_commit'] = motion_call(parent, s_parent)
    first = {k: fn() for k, fn in runs.items()}
    torch.cuda.synchronize()
    out = dict(grid=[n, n], queries=q, max_tracks=p, frames=FRAMES,
               counters_after_first_pass={k: s.counters.cpu().tolist() for k, s in (('occluded_on', s_on), ('occluded_off', s_off),
                                                                                    ('motion_this_tree', s_motion))},
               held_in_first_pass=int(s_on.occlusion.occlusion_counters.cpu()[0]),
               off_equals_motion_first_pass=bool(torch.equal(first['occluded_off'], first['motion_this_tree'])
                                                 and torch.equal(s_off.state_map, s_motion.state_map)))
    if PARENT:
        out['parent_equals_motion_first_pass'] = bool(torch.equal(first['motion_parent_commit'], first['motion_this_tree'])
                                                      and torch.equal(s_parent.state_map, s_motion.state_map))
    for _ in range(WARM):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(WINDOWS):                                              # alternating windows in one process
        for k, fn in runs.items():
            ms[k].append(window(fn, ITERS) / FRAMES)
    out['frame_ms'] = {k: stats(v, iters=ITERS, windows=WINDOWS) for k, v in ms.items()}
    base = statistics.median(ms['motion_parent_commit' if PARENT else 'motion_this_tree'])
    out['ratio_to_' + ('parent_motion' if PARENT else 'this_tree_motion')] = {k: statistics.median(v) / base for k, v in ms.items()}
    return out


SHAPES = (('semantic_kitti_512', 1), ('semantic_kitti_512', 4), ('kitti_496x432', 1), ('kitti_496x432', 4))
if '--k38a-only' in sys.argv:
    picked = [SHAPES[int(a.split('=')[1])] for a in sys.argv if a.startswith('--shape=')] or SHAPES
    res = dict(k38a_trace_run=[dict(workload=wl, **k38a(wl, b, timed=False)) for wl, b in picked])
else:
    res = dict(k38a=[dict(workload=wl, **k38a(wl, b, check=(b == 1))) for wl, b in SHAPES], k38b=k38b())
target = ARGS[0] if ARGS else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'k38_measure.json')
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
with open(target, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
