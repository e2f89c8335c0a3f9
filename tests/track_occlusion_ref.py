"""K38b restated: K37's tracker step with occlusion-aware ageing, from the words of include/maskbev_hip.h — the yardstick of
tests/test_k38_track_occlusion_gpu.py.  `step` is the numpy version (steps 0 – 3b are K37's, shared with
tests/track_motion_ref.py piece by piece); `plain_hidden` and `plain_hold` restate the two additions independently in plain
loops (the fraction test with exact fractions).  tests/test_track_occlusion_cpu.py holds them against each other.  Nothing
here imports the package."""
import functools
from fractions import Fraction

import numpy as np

from tests import track_motion_ref as M
from tests import track_ref as R
from tests.track_ref import _before, warp

F64 = np.float64


def fresh_state(h, w, p):
    s = M.fresh_state(h, w, p)
    s.update(live_held=np.zeros((p,), np.int32), occlusion_counters=np.zeros((2,), np.int32))
    return s


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def step(state, instance_map, m, n, visibility, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells, gain, gate, max_shift,
         hold_num, hold_den, max_hold, log=None):
    """One frame of K38b on `state` (changed in place); `visibility` (H, W) uint8 or None.  → (query_track (Q) int32,
    track_map (H, W) int32, query_velocity (Q, 2) f64).  `log`, a dict, receives the frame's intermediate tables."""
    sm, live_id, live_seen, counters = state['state_map'], state['live_id'], state['live_seen'], state['counters']
    pos, vel, live_held = state['pos'], state['vel'], state['live_held']
    h, w = sm.shape
    p = live_id.shape[0]
    n_live = int(min(max(int(counters[0]), 0), p))
    next_id, frame, dropped = int(counters[1]), int(counters[2]), int(counters[3])
    n = np.asarray(n, F64).reshape(2, 3)
    gain, gate, voxel = F64(gain), F64(gate), F64(voxel)
    # 0. advect; 1. warp
    moved = M.advect(sm, n_live, vel, voxel, max_shift)
    warped = warp(moved, n_live, m, x_lo, y_lo, voxel)
    # 2. count, and the hidden cells of every warped footprint
    im = instance_map.astype(np.int64)
    im = np.where((im >= 0) & (im < q_num), im, -1)
    area_q = np.bincount(im[im >= 0], minlength=q_num).astype(np.int64)
    area_t = np.bincount(warped[warped >= 0], minlength=p).astype(np.int64)
    both = (im >= 0) & (warped >= 0)
    inter = np.bincount(im[both] * p + warped[both], minlength=q_num * p).reshape(q_num, p).astype(np.int64)
    hidden = np.zeros((p,), np.int64)
    if visibility is not None:
        unseen = (warped >= 0) & (np.asarray(visibility) == 0)
        hidden = np.bincount(warped[unseen], minlength=p).astype(np.int64)
    present = area_q >= min_cells
    c_q = M.centroids(im, area_q, x_lo, y_lo, voxel)
    # 3. match
    cands = []
    for q, t in zip(*np.nonzero(inter)):
        if not present[q]:
            continue
        k = int(inter[q, t])
        u = int(area_q[q] + area_t[t] - k)
        if F64(k) / F64(u) >= F64(min_iou):
            cands.append((k, u, int(q), int(t)))
    cands.sort(key=functools.cmp_to_key(_before))
    q_match, t_taken = {}, set()
    for k, u, q, t in cands:
        if q in q_match or t in t_taken:
            continue
        q_match[q] = t
        t_taken.add(t)
    # 3b. gate
    with np.errstate(all='ignore'):
        a = pos[:n_live] + vel[:n_live]
        pred = np.stack([(n[0, 0] * a[:, 0] + n[0, 1] * a[:, 1]) + n[0, 2],
                         (n[1, 0] * a[:, 0] + n[1, 1] * a[:, 1]) + n[1, 2]], axis=1).reshape(n_live, 2)
        velr = np.stack([n[0, 0] * vel[:n_live, 0] + n[0, 1] * vel[:n_live, 1],
                         n[1, 0] * vel[:n_live, 0] + n[1, 1] * vel[:n_live, 1]], axis=1).reshape(n_live, 2)
    gated = 0
    if gate > 0 and n_live > 0:
        open_q = [q for q in range(q_num) if present[q] and q not in q_match]
        open_t = [t for t in range(n_live) if t not in t_taken]
        pairs = []
        with np.errstate(all='ignore'):
            g2 = gate * gate
            for q in open_q:
                dx, dy = c_q[q, 0] - pred[open_t, 0], c_q[q, 1] - pred[open_t, 1]
                d2 = dx * dx + dy * dy
                pairs += [(float(d2[k]), q, t) for k, t in enumerate(open_t) if d2[k] <= g2]
        pairs.sort()
        for _, q, t in pairs:
            if q in q_match or t in t_taken:
                continue
            q_match[q] = t
            t_taken.add(t)
            gated += 1
    # 4. update
    new_id, new_seen, new_held = np.full((p,), -1, np.int32), np.full((p,), -1, np.int32), np.zeros((p,), np.int32)
    new_pos, new_vel = np.zeros((p, 2), F64), np.zeros((p, 2), F64)
    q_new, t_new = np.full((q_num,), -1, np.int64), np.full((p,), -1, np.int64)
    query_track = np.full((q_num,), -1, np.int32)
    query_velocity = np.zeros((q_num, 2), F64)
    n_new = 0
    for q in range(q_num):
        if not present[q]:
            continue
        if q in q_match:
            t = q_match[q]
            gid = int(live_id[t])
            with np.errstate(all='ignore'):
                v = M.finite_or_zero(velr[t] + gain * (c_q[q] - pred[t]))
        else:
            gid = next_id
            next_id += 1
            v = np.zeros((2,), F64)
        new_id[n_new], new_seen[n_new] = gid, frame
        new_pos[n_new], new_vel[n_new] = c_q[q], v
        query_velocity[q] = v
        q_new[q] = n_new
        query_track[q] = gid
        n_new += 1
    held_now, occluded = 0, []
    for t in range(n_live):
        if t in t_taken:
            continue
        seen, held = int(live_seen[t]), int(live_held[t])
        if (visibility is not None and area_t[t] > 0 and int(hidden[t]) * int(hold_den) >= int(area_t[t]) * int(hold_num)
                and held < max_hold):
            seen, held = seen + 1, held + 1
            held_now += 1
            occluded.append(t)
        if frame - seen <= max_age:
            if n_new < p:
                new_id[n_new], new_seen[n_new], new_held[n_new] = live_id[t], seen, held
                new_pos[n_new], new_vel[n_new] = pred[t], M.finite_or_zero(velr[t])
                t_new[t] = n_new
                n_new += 1
            else:
                dropped += 1
    if log is not None:
        log.update(warped=warped, area_t=area_t, hidden=hidden, t_taken=sorted(t_taken), occluded=occluded, t_new=t_new.copy(),
                   frame=frame)
    present, q_new, of_query = np.append(present, False), np.append(q_new, -1), np.append(query_track, -1)   # Q = 0 indexes too
    pres_cell = (im >= 0) & present[np.maximum(im, 0)]
    from_q = q_new[np.maximum(im, 0)]
    from_t = np.where(warped >= 0, t_new[np.maximum(warped, 0)], -1)
    sm[...] = np.where(pres_cell, from_q, from_t).astype(np.int32)
    track_map = np.where(pres_cell, of_query[np.maximum(im, 0)], -1).astype(np.int32)
    live_id[...] = new_id
    live_seen[...] = new_seen
    live_held[...] = new_held
    pos[...] = new_pos
    vel[...] = new_vel
    counters[...] = np.array([n_new, next_id, frame + 1, dropped], np.int64).astype(np.int32)
    state['motion_counters'][...] = np.array([int(state['motion_counters'][0]) + gated, 0], np.int64).astype(np.int32)
    state['occlusion_counters'][...] = np.array([int(state['occlusion_counters'][0]) + held_now, 0], np.int64).astype(np.int32)
    return query_track, track_map, query_velocity


# ---- the two additions once more, in plain loops ------------------------------------------------------------------------------

def plain_hidden(warped, visibility, p):
    """→ (area_t, hidden), two lists of P ints, cell by cell."""
    area, hidden = [0] * p, [0] * p
    h, w = warped.shape
    for iy in range(h):
        for ix in range(w):
            t = int(warped[iy, ix])
            if t < 0:
                continue
            area[t] += 1
            if visibility is not None and int(visibility[iy, ix]) == 0:
                hidden[t] += 1
    return area, hidden


def plain_hold(n_live, taken, live_seen, live_held, area, hidden, have_visibility, frame, max_age, room, hold_num, hold_den,
               max_hold):
    """Step 4's walk over the unmatched old tracks in ascending t with `room` free slots → (occluded tracks, [(t, seen',
    held')] of the appended ones in order, dropped).  The fraction test in exact fractions."""
    occluded, appended, dropped = [], [], 0
    for t in range(n_live):
        if t in taken:
            continue
        seen, held = int(live_seen[t]), int(live_held[t])
        if have_visibility and area[t] > 0 and Fraction(hidden[t], area[t]) >= Fraction(hold_num, hold_den) and held < max_hold:
            occluded.append(t)
            seen, held = seen + 1, held + 1
        if frame - seen > max_age:
            continue
        if len(appended) < room:
            appended.append((t, seen, held))
        else:
            dropped += 1
    return occluded, appended, dropped


# ---- scenes -------------------------------------------------------------------------------------------------------------------

OCC_PARAMS = dict(q_num=8, p=16, min_iou=0.3, max_age=2, min_cells=4, gain=0.5, gate=3.0, max_shift=6, hold_num=1, hold_den=2,
                  max_hold=10)


def random_walk(seed, h=48, w=40, q_num=8, frames=12, voxel=0.5):
    """A random moving scene of tests/track_motion_ref.py with random visibility bytes (a third of them 0, in blocks and as
    noise) → (list of (instance_map, m, n, visibility), x_lo, y_lo)."""
    scene, x_lo, y_lo = M.random_moving_scene(seed, h, w, q_num, frames=frames, voxel=voxel, rects=q_num + 3)
    rng = np.random.default_rng(seed + 1000)
    out = []
    for im, m, n in scene:
        vis = rng.integers(0, 4, (h, w)).astype(np.uint8)
        vis[rng.random((h, w)) < 0.2] = 0
        for _ in range(3):                                         # blocks out of sight
            y0, x0 = int(rng.integers(0, h - 8)), int(rng.integers(0, w - 8))
            vis[y0:y0 + int(rng.integers(4, 16)), x0:x0 + int(rng.integers(4, 16))] = 0
        out.append((im, m, n, vis))
    return out, x_lo, y_lo


H2, W2 = 16, 20
FOOT = (slice(4, 8), slice(6, 11))                                 # 4 x 5 = 20 cells


def gap_scene(seen_while_absent, frames=9, first_gap=3, last_gap=7):
    """A standing sensor, voxel 1: one object of 20 cells (query 2) in frames 0 – 2 and again from frame 8 on (as query 5),
    absent in between; a second object (query 0) all the time.  The visibility over the first object's footprint while it is
    absent is 0 (`seen_while_absent` False) or PASSED; everything else is PASSED.  → list of (instance_map, m, n, visibility)"""
    out = []
    for k in range(frames):
        im = np.full((H2, W2), -1, np.int32)
        im[11:14, 2:6] = 0
        gap = first_gap <= k <= last_gap
        if not gap:
            im[FOOT] = 2 if k < first_gap else 5
        vis = np.ones((H2, W2), np.uint8)
        if gap and not seen_while_absent:
            vis[FOOT] = 0
        out.append((im, R.IDENTITY.copy(), R.IDENTITY.copy(), vis))
    return out
