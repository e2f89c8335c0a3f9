"""K33 restated: the tracker step (K33a) and tube association (K33b) from the words of include/maskbev_hip.h — the yardstick of
tests/test_k33_track_gpu.py.  Two versions of each: a numpy one (vectorised warp and counts, the match with i64
cross-multiplication), and an independent plain-loop one (`plain_*`) that orders the candidates and sums S_assoc with
`fractions.Fraction`.  tests/test_track_cpu.py holds them against each other.  `step` is the ONLY restatement of the frame:
its optional `motion` and `occlusion` parts make it K37's and K38b's step, the yardstick of tests/test_k37_track_motion_gpu.py
and tests/test_k38_track_occlusion_gpu.py too (tests/track_motion_ref.py and tests/track_occlusion_ref.py hold the pieces, the
plain-loop second opinions and the scenes).  Nothing here imports the package."""
import functools
import math
from fractions import Fraction

import numpy as np


def fresh_state(h, w, p):
    return dict(state_map=np.full((h, w), -1, np.int32), live_id=np.full((p,), -1, np.int32),
                live_seen=np.full((p,), -1, np.int32), counters=np.zeros((4,), np.int32))


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float64)


def warp(state_map, n_live, m, x_lo, y_lo, voxel):
    """Step 1: the old track index under every current cell, -1 for none."""
    h, w = state_map.shape
    m = np.asarray(m, np.float64).reshape(2, 3)
    x = (np.float64(x_lo) + (np.arange(w, dtype=np.float64) + 0.5) * np.float64(voxel))[None, :]
    y = (np.float64(y_lo) + (np.arange(h, dtype=np.float64) + 0.5) * np.float64(voxel))[:, None]
    with np.errstate(all='ignore'):
        xp = (m[0, 0] * x + m[0, 1] * y) + m[0, 2]
        yp = (m[1, 0] * x + m[1, 1] * y) + m[1, 2]
        fx = np.floor((xp - np.float64(x_lo)) / np.float64(voxel))
        fy = np.floor((yp - np.float64(y_lo)) / np.float64(voxel))
        ok = (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
    jx = np.where(ok, fx, 0).astype(np.int64)
    jy = np.where(ok, fy, 0).astype(np.int64)
    t = np.where(ok, state_map[jy, jx], -1).astype(np.int64)
    t[(t < 0) | (t >= n_live)] = -1
    return t


def _before(a, b):
    """candidates (inter, union, q, t): negative when a comes first"""
    lhs, rhs = a[0] * b[1], b[0] * a[1]
    if lhs != rhs:
        return -1 if lhs > rhs else 1
    return -1 if (a[2], a[3]) < (b[2], b[3]) else 1


def step(state, instance_map, m, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells, log=None, motion=None, occlusion=None,
         tables=None):
    """One frame of the tracker on `state` (changed in place): the only restatement of the frame.  With neither option it is
    K33a's step and returns (query_track (Q) int32, track_map (H, W) int32).  `motion` = (n, gain, gate, max_shift) adds K37's
    steps 0 and 3b and the update of `pos` / `vel` / `motion_counters`, and a third return value, query_velocity (Q, 2) f64;
    its pieces are tests/track_motion_ref.py's.  `occlusion` = (visibility (H, W) uint8 or None, hold_num, hold_den, max_hold),
    with `motion` only, adds K38b's hidden count and the hold of step 4, on `live_held` / `occlusion_counters`.  `log`, a list,
    receives the events of the frame as tuples; `tables`, a dict, the frame's intermediate tables."""
    sm, live_id, live_seen, counters = state['state_map'], state['live_id'], state['live_seen'], state['counters']
    h, w = sm.shape
    p = live_id.shape[0]
    n_live = int(min(max(int(counters[0]), 0), p))
    next_id, frame, dropped = int(counters[1]), int(counters[2]), int(counters[3])
    assert occlusion is None or motion is not None, 'K38b runs on K37\'s step'
    # 0. advect (K37); 1. warp
    source = sm
    if motion is not None:
        from tests import track_motion_ref as M                    # it imports this module: not at the top
        n, gain, gate, max_shift = motion
        n, gain, gate = np.asarray(n, np.float64).reshape(2, 3), np.float64(gain), np.float64(gate)
        pos, vel = state['pos'], state['vel']
        source = moved = M.advect(sm, n_live, vel, np.float64(voxel), max_shift)
    warped = warp(source, n_live, m, x_lo, y_lo, voxel)
    # 2. count; K38b: the hidden cells of every warped footprint
    im = instance_map.astype(np.int64)
    im = np.where((im >= 0) & (im < q_num), im, -1)
    area_q = np.bincount(im[im >= 0], minlength=q_num).astype(np.int64)
    area_t = np.bincount(warped[warped >= 0], minlength=p).astype(np.int64)
    both = (im >= 0) & (warped >= 0)
    inter = np.bincount(im[both] * p + warped[both], minlength=q_num * p).reshape(q_num, p).astype(np.int64)
    present = area_q >= min_cells
    if occlusion is not None:
        visibility, hold_num, hold_den, max_hold = occlusion
        live_held = state['live_held']
        hidden = np.zeros((p,), np.int64)
        if visibility is not None:
            unseen = (warped >= 0) & (np.asarray(visibility) == 0)
            hidden = np.bincount(warped[unseen], minlength=p).astype(np.int64)
    # 3. match
    cands = []
    for q, t in zip(*np.nonzero(inter)):
        if not present[q]:
            continue
        k = int(inter[q, t])
        u = int(area_q[q] + area_t[t] - k)
        if np.float64(k) / np.float64(u) >= np.float64(min_iou):
            cands.append((k, u, int(q), int(t)))
    cands.sort(key=functools.cmp_to_key(_before))
    q_match, t_taken = {}, set()
    for i, (k, u, q, t) in enumerate(cands):
        if q in q_match or t in t_taken:
            continue
        q_match[q] = t
        t_taken.add(t)
        if log is not None:
            tied = [c for c in cands if c is not cands[i] and c[0] * u == k * c[1] and (c[2] == q or c[3] == t)]
            log.append(('match', frame, q, t, int(live_id[t]), k, u, int(live_seen[t]), len(tied)))
    # 3b. gate (K37)
    if motion is not None:
        c_q = M.centroids(im, area_q, x_lo, y_lo, np.float64(voxel))
        with np.errstate(all='ignore'):
            a = pos[:n_live] + vel[:n_live]
            pred = np.stack([(n[0, 0] * a[:, 0] + n[0, 1] * a[:, 1]) + n[0, 2],
                             (n[1, 0] * a[:, 0] + n[1, 1] * a[:, 1]) + n[1, 2]], axis=1).reshape(n_live, 2)
            velr = np.stack([n[0, 0] * vel[:n_live, 0] + n[0, 1] * vel[:n_live, 1],
                             n[1, 0] * vel[:n_live, 0] + n[1, 1] * vel[:n_live, 1]], axis=1).reshape(n_live, 2)
        open_q, open_t, gate_taken = [], [], []
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
                gate_taken.append((q, t))
        new_pos, new_vel = np.zeros((p, 2), np.float64), np.zeros((p, 2), np.float64)
        query_velocity = np.zeros((q_num, 2), np.float64)
    # 4. update
    new_id, new_seen, new_held = np.full((p,), -1, np.int32), np.full((p,), -1, np.int32), np.zeros((p,), np.int32)
    q_new, t_new = np.full((q_num,), -1, np.int64), np.full((p,), -1, np.int64)
    query_track = np.full((q_num,), -1, np.int32)
    n_new = 0
    for q in range(q_num):
        if not present[q]:
            if log is not None and area_q[q] > 0:
                log.append(('small', frame, q, int(area_q[q])))
            continue
        if q in q_match:
            gid = int(live_id[q_match[q]])
        else:
            gid = next_id
            next_id += 1
            if log is not None:
                log.append(('birth', frame, q, gid))
        if motion is not None:
            v = np.zeros((2,), np.float64)
            if q in q_match:
                with np.errstate(all='ignore'):
                    v = M.finite_or_zero(velr[q_match[q]] + gain * (c_q[q] - pred[q_match[q]]))
            new_pos[n_new], new_vel[n_new], query_velocity[q] = c_q[q], v, v
        new_id[n_new], new_seen[n_new] = gid, frame
        q_new[q] = n_new
        query_track[q] = gid
        n_new += 1
    occluded = []
    for t in range(n_live):
        if t in t_taken:
            continue
        seen, held = int(live_seen[t]), 0
        if occlusion is not None:
            held = int(live_held[t])
            if (visibility is not None and area_t[t] > 0 and int(hidden[t]) * int(hold_den) >= int(area_t[t]) * int(hold_num)
                    and held < max_hold):
                seen, held = seen + 1, held + 1
                occluded.append(t)
        if frame - seen <= max_age:
            if n_new < p:
                new_id[n_new], new_seen[n_new], new_held[n_new] = live_id[t], seen, held
                if motion is not None:
                    new_pos[n_new], new_vel[n_new] = pred[t], M.finite_or_zero(velr[t])
                t_new[t] = n_new
                n_new += 1
                if log is not None:
                    log.append(('coast', frame, t, int(live_id[t])))
            else:
                dropped += 1
                if log is not None:
                    log.append(('drop', frame, t, int(live_id[t])))
        elif log is not None:
            log.append(('death', frame, t, int(live_id[t])))
    if tables is not None:
        tables.update(warped=warped, area_q=area_q, area_t=area_t, t_taken=sorted(t_taken), t_new=t_new.copy(), frame=frame)
        if motion is not None:
            tables.update(moved=moved, c_q=c_q, pred=pred, velr=velr, open_q=open_q, open_t=open_t, gate_taken=gate_taken,
                          gated=len(gate_taken))
        if occlusion is not None:
            tables.update(hidden=hidden, occluded=occluded)
    present, q_new, of_query = np.append(present, False), np.append(q_new, -1), np.append(query_track, -1)   # Q = 0 indexes too
    pres_cell = (im >= 0) & present[np.maximum(im, 0)]
    from_q = q_new[np.maximum(im, 0)]
    from_t = np.where(warped >= 0, t_new[np.maximum(warped, 0)], -1)
    if log is not None:
        fell = int(((im >= 0) & ~pres_cell & (from_t >= 0)).sum())
        if fell:
            log.append(('fall_through', frame, fell))
    sm[...] = np.where(pres_cell, from_q, from_t).astype(np.int32)
    track_map = np.where(pres_cell, of_query[np.maximum(im, 0)], -1).astype(np.int32)
    live_id[...] = new_id
    live_seen[...] = new_seen
    counters[...] = np.array([n_new, next_id, frame + 1, dropped], np.int64).astype(np.int32)
    if motion is None:
        return query_track, track_map
    pos[...] = new_pos
    vel[...] = new_vel
    state['motion_counters'][...] = np.array([int(state['motion_counters'][0]) + len(gate_taken), 0], np.int64).astype(np.int32)
    if occlusion is not None:
        live_held[...] = new_held
        state['occlusion_counters'][...] = np.array([int(state['occlusion_counters'][0]) + len(occluded), 0],
                                                    np.int64).astype(np.int32)
    return query_track, track_map, query_velocity


def plain_step(state, instance_map, m, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells):
    """The same frame in plain loops, with exact fractions for the order of the candidates."""
    sm, live_id, live_seen, counters = state['state_map'], state['live_id'], state['live_seen'], state['counters']
    h, w = sm.shape
    p = len(live_id)
    n_live = min(max(int(counters[0]), 0), p)
    next_id, frame, dropped = int(counters[1]), int(counters[2]), int(counters[3])
    m = [float(v) for v in np.asarray(m, np.float64).reshape(-1)]
    x_lo, y_lo, voxel = float(x_lo), float(y_lo), float(voxel)
    warped = [[-1] * w for _ in range(h)]
    area_q, area_t, inter = [0] * q_num, [0] * p, {}
    for iy in range(h):
        for ix in range(w):
            x = x_lo + (ix + 0.5) * voxel
            y = y_lo + (iy + 0.5) * voxel
            xp = (m[0] * x + m[1] * y) + m[2]
            yp = (m[3] * x + m[4] * y) + m[5]
            t = -1
            if math.isfinite(xp) and math.isfinite(yp):
                a, b = (xp - x_lo) / voxel, (yp - y_lo) / voxel
                if math.isfinite(a) and math.isfinite(b):
                    jx, jy = math.floor(a), math.floor(b)
                    if 0 <= jx < w and 0 <= jy < h:
                        t = int(sm[jy, jx])
                        if not 0 <= t < n_live:
                            t = -1
            warped[iy][ix] = t
            q = int(instance_map[iy, ix])
            if not 0 <= q < q_num:
                q = -1
            if q >= 0:
                area_q[q] += 1
            if t >= 0:
                area_t[t] += 1
            if q >= 0 and t >= 0:
                inter[(q, t)] = inter.get((q, t), 0) + 1
    cands = []
    for (q, t), n in inter.items():
        u = area_q[q] + area_t[t] - n
        if area_q[q] >= min_cells and float(n) / float(u) >= float(min_iou):
            cands.append((-Fraction(n, u), q, t))
    cands.sort()
    q_match, t_taken = {}, set()
    for _, q, t in cands:
        if q not in q_match and t not in t_taken:
            q_match[q] = t
            t_taken.add(t)
    new = []                                     # (id, seen)
    q_new, t_new, query_track = {}, {}, [-1] * q_num
    for q in range(q_num):
        if area_q[q] < min_cells:
            continue
        if q in q_match:
            gid = int(live_id[q_match[q]])
        else:
            gid, next_id = next_id, next_id + 1
        q_new[q] = len(new)
        query_track[q] = gid
        new.append((gid, frame))
    for t in range(n_live):
        if t in t_taken or frame - int(live_seen[t]) > max_age:
            continue
        if len(new) < p:
            t_new[t] = len(new)
            new.append((int(live_id[t]), int(live_seen[t])))
        else:
            dropped += 1
    track_map = np.full((h, w), -1, np.int32)
    for iy in range(h):
        for ix in range(w):
            q = int(instance_map[iy, ix])
            if 0 <= q < q_num and q in q_new:
                sm[iy, ix] = q_new[q]
                track_map[iy, ix] = query_track[q]
            else:
                sm[iy, ix] = t_new.get(warped[iy][ix], -1)
    for k in range(p):
        live_id[k], live_seen[k] = new[k] if k < len(new) else (-1, -1)
    counters[...] = np.array([len(new), next_id, frame + 1, dropped], np.int64).astype(np.int32)
    return np.array(query_track, np.int32), track_map


# ---- K33b -----------------------------------------------------------------------------------------------------------------

def fresh_tables(c, i, t):
    rows = (c - 1) * i
    return dict(gt_size=np.zeros((rows,), np.int64), pred_size=np.zeros((t,), np.int64), pair=np.zeros((rows, t), np.int32),
                overflow=np.zeros((2,), np.int64))


def classes_of(words, lut, c):
    sem = (words & 0xffff).astype(np.int64)
    lut = np.asarray(lut, np.int64)
    cls = np.full(sem.shape, -1, np.int64)
    ok = sem < len(lut)
    cls[ok] = lut[sem[ok]]
    return np.where((cls < 0) | (cls >= c), -1, cls)


def tube_accumulate(tables, pred_track, gt_words, lut, c, i, t):
    words = np.asarray(gt_words).astype(np.int64) & 0xffffffff
    p = np.asarray(pred_track).astype(np.int64)
    cls = classes_of(words, lut, c)
    inst = words >> 16
    live = cls >= 0
    thing = live & (cls >= 1)
    tables['overflow'][0] += int((thing & (inst >= i)).sum())
    tables['overflow'][1] += int((live & (p >= t)).sum())
    tube = thing & (inst >= 1) & (inst < i)
    row = (cls - 1) * i + inst
    np.add.at(tables['gt_size'], row[tube], 1)
    has_p = live & (p >= 0) & (p < t)
    np.add.at(tables['pred_size'], p[has_p], 1)
    np.add.at(tables['pair'], (row[tube & has_p], p[tube & has_p]), 1)
    return tables


def tube_scores(tables, c, i):
    """(assoc (rows) f64, class_assoc (C) f64, class_tubes (C) int32): f64, the sums in ascending order."""
    gt, ps, pair = tables['gt_size'], tables['pred_size'], tables['pair']
    rows = gt.shape[0]
    assoc = np.zeros((rows,), np.float64)
    for r in np.nonzero(gt > 0)[0]:
        g, s = int(gt[r]), np.float64(0.0)
        for p in np.nonzero(pair[r] > 0)[0]:
            tpa = np.float64(int(pair[r, p]))
            s = s + tpa * (tpa / np.float64(g + int(ps[p]) - int(pair[r, p])))
        assoc[r] = s / np.float64(g)
    class_assoc, class_tubes = np.zeros((c,), np.float64), np.zeros((c,), np.int32)
    for k in range(1, c):
        s = np.float64(0.0)
        for r in range((k - 1) * i, k * i):
            if gt[r] > 0:
                s = s + assoc[r]
                class_tubes[k] += 1
        class_assoc[k] = s
    return assoc, class_assoc, class_tubes


def plain_tube(pred_track, gt_words, lut, c, i, t):
    """The whole of K33b from the elements in plain loops: ({row: Fraction assoc}, overflow list)."""
    gt, ps, pair, over = {}, {}, {}, [0, 0]
    for p, word in zip((int(v) for v in pred_track), (int(v) & 0xffffffff for v in gt_words)):
        sem = word & 0xffff
        cls = int(lut[sem]) if sem < len(lut) else -1
        if not 0 <= cls < c:
            continue
        inst, r = word >> 16, None
        if cls >= 1:
            if inst >= i:
                over[0] += 1
            elif inst >= 1:
                r = (cls - 1) * i + inst
                gt[r] = gt.get(r, 0) + 1
        if p >= t:
            over[1] += 1
        elif p >= 0:
            ps[p] = ps.get(p, 0) + 1
            if r is not None:
                pair[(r, p)] = pair.get((r, p), 0) + 1
    assoc = {r: Fraction(0) for r in gt}
    for (r, p), n in pair.items():
        assoc[r] += Fraction(n) * Fraction(n, gt[r] + ps[p] - n)
    return {r: v / gt[r] for r, v in assoc.items()}, over


# ---- scenes ---------------------------------------------------------------------------------------------------------------

def pose_2d(x, y, yaw):
    """A 4 x 4 sensor pose: a turn about z and a shift in the plane."""
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)


def prev_from_cur(pose_prev, pose_cur):
    m = np.linalg.inv(pose_prev) @ pose_cur
    return np.ascontiguousarray(m[:2][:, [0, 1, 3]])


def render(rects, pose, h, w, x_lo, y_lo, voxel):
    """World-fixed rectangles (query, x0, x1, y0, y1) seen from `pose`: the instance map (H, W) of the cell centres inside."""
    ix, iy = np.meshgrid(np.arange(w), np.arange(h))
    x, y = x_lo + (ix + 0.5) * voxel, y_lo + (iy + 0.5) * voxel
    wx = pose[0, 0] * x + pose[0, 1] * y + pose[0, 3]
    wy = pose[1, 0] * x + pose[1, 1] * y + pose[1, 3]
    out = np.full((h, w), -1, np.int32)
    for q, x0, x1, y0, y1 in rects:
        out[(wx >= x0) & (wx < x1) & (wy >= y0) & (wy < y1)] = q
    return out


H0, W0, VOXEL0, X_LO0, Y_LO0 = 40, 48, 0.5, -12.0, -10.0
SCRIPT_PARAMS = dict(q_num=4, p=4, min_iou=0.3, max_age=1, min_cells=4)


def scripted_scene():
    """Six frames on a 40 x 48 grid, voxel 0.5: rectangles fixed in the world, the ego moving 1 m and turning 0.05 rad per
    frame; Q = P = 4, max_age = 1.  Returns a list of (instance_map, prev_from_cur).  Which rectangles the detector "sees"
    changes per frame: A always (a match under rotation + translation), B misses frame 2 (it coasts one frame and is
    re-identified in frame 3), C is seen in frame 0 only (coasts in frame 1, dies by age in frame 2), D and E are born in
    frame 3 and missed in frame 4, where F and G are born: the list is full and D and E are dropped by capacity."""
    rects = dict(A=(-3.0, 0.0, -5.0, -3.0), B=(2.0, 5.0, 3.0, 5.0), C=(-4.0, -2.0, 3.0, 5.0), D=(5.0, 7.0, -6.0, -4.0),
                 E=(-1.0, 1.0, 5.5, 7.0), F=(1.0, 3.0, -8.0, -6.0), G=(6.0, 8.0, 1.0, 3.0))
    seen = ['ABC', 'AB', 'A', 'ABDE', 'ABFG', 'AB']
    frames, prev = [], None
    for k, names in enumerate(seen):
        pose = pose_2d(1.0 * k, 0.0, 0.05 * k)
        m = IDENTITY.copy() if prev is None else prev_from_cur(prev, pose)
        # the query index of a rectangle changes from frame to frame, as a detector's would
        shown = [((j + k) % 4,) + rects[n] for j, n in enumerate(names)]
        frames.append((render(shown, pose, H0, W0, X_LO0, Y_LO0, VOXEL0), m))
        prev = pose
    return frames


def constructed_cases():
    """Three two-frame cases on a 6 x 8 grid (x_lo = y_lo = 0, voxel = 1, identity transforms), name -> (frames, params):
    'fall_through' — a query below min_cells is left out and its cells fall through to the warped track, which coasts;
    'tie' — query 0 overlaps tracks 0 and 1 with IoU 1/4 each (the smaller t wins), queries 1 and 2 overlap track 2 with IoU
    2/4 each (the smaller q wins); 'half' — inter = 1, union = 2 at min_iou = 0.5 is accepted."""
    def grid(cells):
        im = np.full((6, 8), -1, np.int32)
        for q, where in cells.items():
            for iy, ix in where:
                im[iy, ix] = q
        return im

    block = [(iy, ix) for iy in range(1, 5) for ix in range(2, 6)]
    cases = {}
    cases['fall_through'] = ([(grid({0: block}), IDENTITY), (grid({1: [(2, 3), (2, 4)]}), IDENTITY)],
                             dict(q_num=4, p=4, min_iou=0.3, max_age=2, min_cells=4))
    first = grid({0: [(0, 0), (0, 1)], 1: [(0, 3), (0, 4)], 2: [(2, 0), (2, 1), (2, 2), (2, 3)]})
    second = grid({0: [(0, 1), (0, 2), (0, 3)], 1: [(2, 0), (2, 1)], 2: [(2, 2), (2, 3)]})
    cases['tie'] = ([(first, IDENTITY), (second, IDENTITY)], dict(q_num=4, p=6, min_iou=0.2, max_age=2, min_cells=1))
    cases['half'] = ([(grid({0: [(0, 0), (0, 1)]}), IDENTITY), (grid({3: [(0, 1)]}), IDENTITY)],
                     dict(q_num=4, p=4, min_iou=0.5, max_age=2, min_cells=1))
    return cases


def random_scene(seed, h, w, q_num, frames=4, voxel=0.5):
    """Random world-fixed rectangles, some missing per frame, under a random ego path; ids permuted per frame."""
    rng = np.random.default_rng(seed)
    x_lo, y_lo = -w * voxel / 2, -h * voxel / 2
    rects = []
    for _ in range(q_num):
        cx, cy = rng.uniform(x_lo * 0.8, -x_lo * 0.8), rng.uniform(y_lo * 0.8, -y_lo * 0.8)
        sx, sy = rng.uniform(0.4, 3.0), rng.uniform(0.4, 3.0)
        rects.append((cx - sx, cx + sx, cy - sy, cy + sy))
    out, prev = [], None
    for k in range(frames):
        pose = pose_2d(rng.uniform(0.5, 1.5) * k, rng.uniform(-0.3, 0.3) * k, rng.uniform(-0.08, 0.08) * k)
        m = IDENTITY.copy() if prev is None else prev_from_cur(prev, pose)
        perm = rng.permutation(q_num)
        shown = [(int(perm[j]),) + r for j, r in enumerate(rects) if rng.random() < 0.75]
        out.append((render(shown, pose, h, w, x_lo, y_lo, voxel), m))
        prev = pose
    return out, x_lo, y_lo


def random_elements(seed, n, c, i, t, lut_len=12):
    """Random tube elements: (pred_track int32, gt_words uint32, lut int32), with ignored ids, instance 0, and a few ids past
    the two limits."""
    rng = np.random.default_rng(seed)
    lut = rng.integers(-1, c, lut_len).astype(np.int32)
    lut[1] = 1                                    # at least one thing class
    sem = rng.integers(0, lut_len + 2, n)
    inst = rng.integers(0, min(i, 6), n)
    inst[rng.random(n) < 0.02] = i + rng.integers(0, 3)
    pred = rng.integers(-1, min(t, 7), n)
    pred[rng.random(n) < 0.02] = t + rng.integers(0, 3)
    # correlate the prediction with the instance so that pairs carry weight
    same = rng.random(n) < 0.6
    pred = np.where(same & (inst < min(t, 7)), inst, pred)
    words = ((inst.astype(np.int64) << 16) | sem).astype(np.uint32)
    return pred.astype(np.int32), words, lut
