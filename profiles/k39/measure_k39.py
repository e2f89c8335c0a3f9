"""K39 measurement: the three tracker entries of this tree against the parent commit's, after the fold of track.hip's two host
drivers into one.  Prints one JSON line and writes it to the path given as the first argument (default: k39_measure.json beside
this file).  ``--parent-lib PATH`` names the parent commit's ``libmaskbev_hip.so``, built in another directory; it is required.

The sequence is profiles/k38/measure_k38.py's ``k38b()``: 512 x 512 cells, 100 queries, ``max_tracks`` 256, 8 frames per call,
``track_map`` on, a visibility map whose columns are unknown in stripes.  Every path is the C entry itself through ctypes with
the per-call allocations ``ops.track_frames`` makes, so the windows compare the launches and not the Python in front of them.

First pass, asserted: for each entry ``query_track``, ``track_map``, ``query_velocity`` and every state and record tensor are
byte-equal between the two libraries.  Then six paths (three entries x two libraries) in alternating windows of one process,
every second round of windows in the reverse order.  With ``--parent-lib`` naming a copy of this tree's own library the script
is its own control: both sides run the same code, and what differs is what the allocations and the order make of it."""
import ctypes
import json
import os
import statistics
import sys

import torch

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
assert '--parent-lib' in sys.argv, 'measure_k39.py --parent-lib PATH [out.json]'
PARENT = os.path.abspath(sys.argv[sys.argv.index('--parent-lib') + 1])
ARGS.remove(sys.argv[sys.argv.index('--parent-lib') + 1])
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mask_bev_amd import _lib, ops, synthetic                             # noqa: E402
from mask_bev_amd.ops_core import _ptr, _stream, _workspace               # noqa: E402

dev = torch.device('cuda:0')
FRAMES, ITERS, WINDOWS, WARM = 8, 20, 7, 5
ENTRIES = dict(plain='mbv_track_frames', motion='mbv_track_frames_motion', occluded='mbv_track_frames_occluded')


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / iters                         # µs


def stats(us):
    return dict(median=statistics.median(us), min=min(us), max=max(us), spread_pct=100.0 * (max(us) - min(us)) / statistics.median(us),
                iters=ITERS, windows=WINDOWS)


def moved_left(x, cells):
    out = torch.full_like(x, -1)
    out[:, :x.shape[1] - cells] = x[:, cells:]
    return out


def state_tensors(s):
    out = dict(state_map=s.state_map, live_id=s.live_id, live_seen=s.live_seen, counters=s.counters)
    if s.motion is not None:
        out.update(pos=s.motion.pos, vel=s.motion.vel, motion_counters=s.motion.motion_counters)
    if s.occlusion is not None:
        out.update(live_held=s.occlusion.live_held, occlusion_counters=s.occlusion.occlusion_counters)
    return out


def main(workload='semantic_kitti_512', p=256):
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
    step = (FRAMES, n, n, x_lo, y_lo, vs, q, p, 0.3, 2, 4)
    model = (motion.gain, motion.gate_m, motion.max_shift(vs))
    hold = occlusion.hidden_fraction + (occlusion.max_hold,)

    parent = ctypes.CDLL(PARENT)
    for name in ENTRIES.values():
        for sym in (name, name + '_workspace_bytes'):
            getattr(parent, sym).restype, getattr(parent, sym).argtypes = _lib.SIGNATURES[sym]
    libs = dict(parent=parent, this_tree=_lib.load())

    def path(lib, entry):
        """→ (the call, its state, the outputs of the last call)"""
        s = ops.TrackState.fresh(n, n, p, dev, motion=entry != 'plain', occlusion=entry == 'occluded')
        ws = _workspace(getattr(lib, ENTRIES[entry] + '_workspace_bytes')(n, n, q, p), dev)
        last = {}

        def run():
            qt = torch.empty((FRAMES, q), dtype=torch.int32, device=dev)
            tm = torch.empty((FRAMES, n, n), dtype=torch.int32, device=dev)
            lists = (_ptr(s.state_map), _ptr(s.live_id), _ptr(s.live_seen))
            if entry == 'plain':
                args = (_ptr(maps), _ptr(tf)) + step + lists + (_ptr(s.counters), _ptr(qt), _ptr(tm))
                last.update(query_track=qt, track_map=tm)
            else:
                qv = torch.empty((FRAMES, q, 2), dtype=torch.float64, device=dev)
                rec = (_ptr(s.counters), _ptr(s.motion.pos), _ptr(s.motion.vel), _ptr(s.motion.motion_counters))
                if entry == 'motion':
                    args = (_ptr(maps), _ptr(tf), _ptr(inv)) + step + model + lists + rec + (_ptr(qt), _ptr(tm), _ptr(qv))
                else:
                    args = (_ptr(maps), _ptr(tf), _ptr(inv), _ptr(vis)) + step + model + hold + lists + \
                        (_ptr(s.occlusion.live_held),) + rec + (_ptr(s.occlusion.occlusion_counters), _ptr(qt), _ptr(tm), _ptr(qv))
                last.update(query_track=qt, track_map=tm, query_velocity=qv)
            rc = getattr(lib, ENTRIES[entry])(*args, _ptr(ws), ws.numel(), _stream())
            assert rc == 0, (entry, rc)
        return run, s, last

    paths = {(entry, which): path(lib, entry) for entry in ENTRIES for which, lib in libs.items()}
    for run, _, _ in paths.values():
        run()
    torch.cuda.synchronize()
    out = dict(grid=[n, n], queries=q, max_tracks=p, frames=FRAMES, first_pass_byte_equal={}, counters_after_first_pass={})
    for entry in ENTRIES:
        (_, sa, la), (_, sb, lb) = paths[(entry, 'parent')], paths[(entry, 'this_tree')]
        both = [(k, la[k], lb[k]) for k in la] + [(k, v, state_tensors(sb)[k]) for k, v in state_tensors(sa).items()]
        for k, x, y in both:
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (entry, k)
        out['first_pass_byte_equal'][entry] = [k for k, _, _ in both]
        out['counters_after_first_pass'][entry] = sb.counters.cpu().tolist()
    out['held_in_first_pass'] = int(paths[('occluded', 'this_tree')][1].occlusion.occlusion_counters.cpu()[0])
    for _ in range(WARM - 1):                                             # the first pass was the first warm-up call
        for run, _, _ in paths.values():
            run()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for wnd in range(WINDOWS):                                            # alternating windows in one process
        for k, (run, _, _) in (reversed(paths.items()) if wnd % 2 else paths.items()):   # and no path always after the same one
            us[k].append(window(run, ITERS) / FRAMES)
    out['frame_us'] = {f'{entry}_{which}': stats(v) for (entry, which), v in us.items()}
    out['verdict'] = {}
    for entry in ENTRIES:
        base, here = out['frame_us'][f'{entry}_parent'], out['frame_us'][f'{entry}_this_tree']
        out['verdict'][entry] = dict(ratio_of_medians=here['median'] / base['median'],
                                     this_tree_median_inside_parent_min_max=bool(base['min'] <= here['median'] <= base['max']),
                                     this_tree_median_not_above_parent_max=bool(here['median'] <= base['max']))
    return out


res = main()
target = ARGS[0] if ARGS else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'k39_measure.json')
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
with open(target, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
