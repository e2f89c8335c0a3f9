"""K38b restated: K37's tracker step with occlusion-aware ageing, from the words of include/maskbev_hip.h — the yardstick of
tests/test_k38_track_occlusion_gpu.py.  The frame itself is tests/track_ref.py's `step` with its motion and occlusion parts;
`plain_hidden` and `plain_hold` restate the two additions independently in plain loops (the fraction test with exact
fractions).  tests/test_track_occlusion_cpu.py holds them against each other.  Nothing here imports the package."""
from fractions import Fraction

import numpy as np

from tests import track_motion_ref as M
from tests import track_ref as R


def fresh_state(h, w, p):
    s = M.fresh_state(h, w, p)
    s.update(live_held=np.zeros((p,), np.int32), occlusion_counters=np.zeros((2,), np.int32))
    return s


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def step(state, instance_map, m, n, visibility, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells, gain, gate, max_shift,
         hold_num, hold_den, max_hold, log=None):
    """One frame of K38b on `state` (changed in place): tests/track_ref.py's step with the motion and the occlusion part;
    `visibility` (H, W) uint8 or None.  → (query_track (Q) int32, track_map (H, W) int32, query_velocity (Q, 2) f64).  `log`,
    a dict, receives the frame's intermediate tables."""
    return R.step(state, instance_map, m, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells,
                  motion=(n, gain, gate, max_shift), occlusion=(visibility, hold_num, hold_den, max_hold), tables=log)


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
