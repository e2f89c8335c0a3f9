"""What the tracker's GPU tests share (tests/test_k33_track_gpu.py, test_k37_track_motion_gpu.py,
test_k38_track_occlusion_gpu.py): one caller of the three C entries into poisoned memory, the comparison of two host states
and the walk of a scene through the kernels and the restatement side by side.  `entry` is 'plain' (mbv_track_frames), 'motion'
(mbv_track_frames_motion) or 'occluded' (mbv_track_frames_occluded)."""
import numpy as np
import torch

from tests import track_motion_ref as M
from tests import track_occlusion_ref as O
from tests import track_ref as R

POISON = 0x5a5a5a5a
ENTRIES = dict(plain='mbv_track_frames', motion='mbv_track_frames_motion', occluded='mbv_track_frames_occluded')
PLAIN_KEYS = ('state_map', 'live_id', 'live_seen', 'counters')
MOTION_KEYS = PLAIN_KEYS + ('pos', 'vel', 'motion_counters')
STATE_KEYS = dict(plain=PLAIN_KEYS, motion=MOTION_KEYS, occluded=MOTION_KEYS + ('live_held', 'occlusion_counters'))
FRESH = dict(plain=R.fresh_state, motion=M.fresh_state, occluded=O.fresh_state)


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def call(lib, device, state, maps, ms, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells, gain=None, gate=None, max_shift=None,
         hold_num=None, hold_den=None, max_hold=None, *, entry, ns=None, vis=None, track_map=True):
    """The entry named on F frames into poisoned outputs and workspace; `state` (host dict) is stepped.  The tails of the
    state's own tables (past n_live) and the reserved counters go in as garbage too.  `ns` (F, 2, 3) with 'motion' and
    'occluded'; `vis` (F, H, W) uint8 or None with 'occluded'.
    → (rc, query_track (F, Q), track_map (F, H, W)), and query_velocity (F, Q, 2) unless the entry is 'plain'"""
    from mask_bev_amd.ops_core import _ptr, _stream
    motion, occluded = entry != 'plain', entry == 'occluded'
    maps, ms = np.ascontiguousarray(maps, np.int32), np.ascontiguousarray(ms, np.float64)
    f, h, w = maps.shape
    p = state['live_id'].shape[0]
    n_live = int(min(max(int(state['counters'][0]), 0), p))
    host = {k: state[k].copy() for k in STATE_KEYS[entry]}
    host['live_id'][n_live:], host['live_seen'][n_live:] = POISON, POISON
    if motion:
        host['pos'][n_live:], host['vel'][n_live:] = 1.25e7, -3.5e-3
        host['motion_counters'][1] = POISON
    if occluded:
        host['live_held'][n_live:] = POISON
        host['occlusion_counters'][1] = POISON
    on_device = {k: dev(v, device) for k, v in host.items()}
    d = {k: _ptr(t) for k, t in on_device.items()}
    d_maps, d_ms = dev(maps, device), dev(ms, device)
    d_ns = dev(np.ascontiguousarray(ns, np.float64), device) if motion else None
    d_vis = dev(np.ascontiguousarray(vis, np.uint8), device) if occluded and vis is not None else None
    qt = torch.full((f, max(q_num, 1)), POISON, dtype=torch.int32, device=device)
    tm = torch.full((f, h, w), POISON, dtype=torch.int32, device=device)
    qv = torch.full((f, max(q_num, 1), 2), 7.5e11, dtype=torch.float64, device=device) if motion else None
    nbytes = getattr(lib, ENTRIES[entry] + '_workspace_bytes')(h, w, q_num, p)
    ws = torch.full((max(nbytes, 256),), 0x5a, dtype=torch.uint8, device=device)
    step = (f, h, w, x_lo, y_lo, voxel, q_num, p, min_iou, max_age, min_cells)
    lists = (d['state_map'], d['live_id'], d['live_seen'])
    outs = (_ptr(qt), _ptr(tm) if track_map else None)
    if entry == 'plain':
        args = (_ptr(d_maps), _ptr(d_ms)) + step + lists + (d['counters'],) + outs
    elif entry == 'motion':
        args = (_ptr(d_maps), _ptr(d_ms), _ptr(d_ns)) + step + (gain, gate, max_shift) + lists + \
            (d['counters'], d['pos'], d['vel'], d['motion_counters']) + outs + (_ptr(qv),)
    else:
        args = (_ptr(d_maps), _ptr(d_ms), _ptr(d_ns), _ptr(d_vis)) + step + (gain, gate, max_shift, hold_num, hold_den, max_hold) + \
            lists + (d['live_held'], d['counters'], d['pos'], d['vel'], d['motion_counters'], d['occlusion_counters']) + outs + \
            (_ptr(qv),)
    rc = getattr(lib, ENTRIES[entry])(*args, _ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    if rc == 0:
        for k, t in on_device.items():
            state[k] = t.cpu().numpy()
    out = (rc, qt.cpu().numpy()[:, :q_num].reshape(f, q_num), tm.cpu().numpy())
    return out + (qv.cpu().numpy()[:, :q_num].reshape(f, q_num, 2),) if motion else out


def same_state(a, b):
    assert set(a) == set(b)
    for k in b:
        if k in ('pos', 'vel'):
            assert a[k].dtype == np.float64 and a[k].tobytes() == b[k].tobytes(), (k, a[k], b[k])
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (k, a[k], b[k])


def walk(lib, device, frames, h, w, x_lo, y_lo, voxel, q_num, p, min_iou, max_age, min_cells, gain=None, gate=None, max_shift=None,
         hold_num=None, hold_den=None, max_hold=None, *, entry, start=None):
    """Every frame — (instance_map, m), with 'motion' also n, with 'occluded' also the visibility map or None — through the
    kernels (F = 1) and through the restatement; everything equal after every frame.  → (the final state, the (Q) query_track
    of every frame)."""
    got = FRESH[entry](h, w, p) if start is None else R.copy_state(start)
    ref = R.copy_state(got)
    step = (x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells)
    tracks = []
    for im, m, *more in frames:
        n = np.asarray(more[0])[None] if entry != 'plain' else None
        vis = more[1] if entry == 'occluded' else None
        rc, qt, tm, *qv = call(lib, device, got, im[None], np.asarray(m)[None], *step, gain, gate, max_shift, hold_num, hold_den,
                               max_hold, entry=entry, ns=n, vis=None if vis is None else vis[None])
        assert rc == 0
        rqt, rtm, *rqv = R.step(ref, im, m, *step, motion=None if entry == 'plain' else (more[0], gain, gate, max_shift),
                                occlusion=(vis, hold_num, hold_den, max_hold) if entry == 'occluded' else None)
        assert qt.dtype == rqt.dtype and np.array_equal(qt[0], rqt), (qt, rqt)
        assert np.array_equal(tm[0], rtm)
        assert len(qv) == len(rqv)
        for v, rv in zip(qv, rqv):
            assert v.dtype == np.float64 and v[0].tobytes() == rv.tobytes(), (v[0], rv)
        same_state(got, ref)
        tracks.append(qt[0].copy())
    return got, tracks
