"""K37 restated: the tracker step with the constant-velocity motion model and the gated second stage, from the words of
include/maskbev_hip.h — the yardstick of tests/test_k37_track_motion_gpu.py.  The frame itself is tests/track_ref.py's `step`
with its motion part, which takes `advect`, `centroids` and `finite_or_zero` from here; `plain_advect`, `plain_centroids` and
`plain_gate` restate the three new pieces independently in plain loops (the gate order with exact fractions).
tests/test_track_motion_cpu.py holds them against each other.  Nothing here imports the package."""
import math
from fractions import Fraction

import numpy as np

from tests.track_ref import IDENTITY, pose_2d, prev_from_cur, render
from tests import track_ref as R

F64 = np.float64


def fresh_state(h, w, p):
    s = R.fresh_state(h, w, p)
    s.update(pos=np.zeros((p, 2), F64), vel=np.zeros((p, 2), F64), motion_counters=np.zeros((2,), np.int32))
    return s


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def invert(m):
    """cur_from_prev of a (2, 3) prev_from_cur: the inverse of the completed 3 x 3."""
    full = np.vstack([np.asarray(m, F64).reshape(2, 3), [0.0, 0.0, 1.0]])
    return np.ascontiguousarray(np.linalg.inv(full)[:2])


def shifts(vel, n_live, voxel, max_shift):
    """Step 0: the integer cell shift (sx, sy) of every live track, (n_live, 2) int64."""
    with np.errstate(all='ignore'):
        s = np.rint(vel[:n_live] / F64(voxel))
        ok = (np.abs(s[:, 0]) <= max_shift) & (np.abs(s[:, 1]) <= max_shift)
    return np.where(ok[:, None], s, 0.0).astype(np.int64)


def advect(state_map, n_live, vel, voxel, max_shift):
    h, w = state_map.shape
    moved = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    sh = shifts(vel, n_live, voxel, max_shift)
    iy, ix = np.nonzero((state_map >= 0) & (state_map < n_live))
    t = state_map[iy, ix].astype(np.int64)
    ty, tx = iy + sh[t, 1], ix + sh[t, 0]
    ok = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
    np.minimum.at(moved, (ty[ok], tx[ok]), t[ok])
    return np.where(moved == np.iinfo(np.int64).max, -1, moved).astype(np.int32)


def centroids(im, area_q, x_lo, y_lo, voxel):
    """(Q, 2) f64: the centre of a query's cells; rows of an empty query are 0 and mean nothing."""
    q_num = area_q.shape[0]
    iy, ix = np.nonzero(im >= 0)
    sum_ix = np.zeros((q_num,), np.int64)
    sum_iy = np.zeros((q_num,), np.int64)
    np.add.at(sum_ix, im[iy, ix], ix)
    np.add.at(sum_iy, im[iy, ix], iy)
    c = np.zeros((q_num, 2), F64)
    some = area_q > 0
    c[some, 0] = F64(x_lo) + (sum_ix[some].astype(F64) / area_q[some].astype(F64) + 0.5) * F64(voxel)
    c[some, 1] = F64(y_lo) + (sum_iy[some].astype(F64) / area_q[some].astype(F64) + 0.5) * F64(voxel)
    return c


def finite_or_zero(v):
    v = np.asarray(v, F64).copy()
    v[~np.isfinite(v)] = 0.0
    return v


def step(state, instance_map, m, n, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells, gain, gate, max_shift,
         log=None):
    """One frame of K37 on `state` (changed in place): tests/track_ref.py's step with the motion part.  → (query_track (Q)
    int32, track_map (H, W) int32, query_velocity (Q, 2) f64).  `log`, a dict, receives the frame's intermediate tables."""
    return R.step(state, instance_map, m, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells,
                  motion=(n, gain, gate, max_shift), tables=log)


# ---- the new pieces once more, in plain loops -------------------------------------------------------------------------------

def plain_advect(state_map, n_live, vel, voxel, max_shift):
    h, w = state_map.shape
    shift = []
    for t in range(n_live):
        s = []
        for c in range(2):
            v = float(vel[t, c]) / float(voxel)
            s.append(float(round(v)) if math.isfinite(v) else v)      # Python rounds halves to even, as rint does
        ok = all(math.isfinite(v) and abs(v) <= max_shift for v in s)
        shift.append((int(s[0]), int(s[1])) if ok else (0, 0))
    moved = [[-1] * w for _ in range(h)]
    for iy in range(h):
        for ix in range(w):
            t = int(state_map[iy, ix])
            if not 0 <= t < n_live:
                continue
            ty, tx = iy + shift[t][1], ix + shift[t][0]
            if 0 <= ty < h and 0 <= tx < w and (moved[ty][tx] < 0 or t < moved[ty][tx]):
                moved[ty][tx] = t
    return np.array(moved, np.int32).reshape(h, w)


def plain_centroids(instance_map, q_num, x_lo, y_lo, voxel):
    """{q: (x, y)} of every query with a cell, the mean as an exact fraction rounded once."""
    h, w = instance_map.shape
    sums = {}
    for iy in range(h):
        for ix in range(w):
            q = int(instance_map[iy, ix])
            if 0 <= q < q_num:
                s = sums.setdefault(q, [0, 0, 0])
                s[0], s[1], s[2] = s[0] + ix, s[1] + iy, s[2] + 1
    return {q: (float(x_lo) + (float(sx) / float(k) + 0.5) * float(voxel), float(y_lo) + (float(sy) / float(k) + 0.5) * float(voxel))
            for q, (sx, sy, k) in sums.items()}


def plain_gate(c_q, pred, open_q, open_t, gate):
    """The pairs stage 2 takes, in the order it takes them.  d2 is the f64 value the rules name; there is no sort: the
    minimum (d2, q, t) among the pairs whose query and track are still free is taken until none is left."""
    g2 = float(gate) * float(gate)
    pairs = {}
    for q in open_q:
        for t in open_t:
            dx, dy = float(c_q[q][0]) - float(pred[t][0]), float(c_q[q][1]) - float(pred[t][1])
            d2 = dx * dx + dy * dy
            if d2 <= g2:
                pairs[(q, t)] = Fraction(d2)
    taken = []
    while pairs:
        q, t = min(pairs, key=lambda qt: (pairs[qt], qt[0], qt[1]))
        taken.append((q, t))
        pairs = {k: v for k, v in pairs.items() if k[0] != q and k[1] != t}
    return taken


# ---- scenes -------------------------------------------------------------------------------------------------------------------

H1, W1, VOXEL1, X_LO1, Y_LO1 = 48, 96, 0.5, -24.0, -12.0
MOTION_PARAMS = dict(q_num=4, p=8, min_iou=0.3, max_age=2, min_cells=4, gain=0.5, gate=4.0, max_shift=16)


def moving_scene(ego=True, frames=8):
    """Eight frames on a 48 x 96 grid, voxel 0.5: a parked car, an oncoming car at 3 m per frame that the detector misses in
    frame 4, and a crossing car at 1.5 m per frame; the ego moves 0.8 m and turns 0.03 rad per frame (`ego=False`: it
    stands).  The query index of a rectangle changes from frame to frame.  → a list of (instance_map, prev_from_cur,
    cur_from_prev)."""
    out, prev = [], None
    for k in range(frames):
        pose = pose_2d(0.8 * k, 0.0, 0.03 * k) if ego else pose_2d(0.0, 0.0, 0.0)
        rects = [(4.0, 8.5, 4.0, 6.0)]
        if k != 4:
            rects.append((20.0 - 3.0 * k - 4.5, 20.0 - 3.0 * k, -5.0, -3.0))
        else:
            rects.append(None)
        rects.append((-10.0, -5.5, -8.0 + 1.5 * k, -8.0 + 1.5 * k + 2.0))
        shown = [((j + k) % 4,) + r for j, r in enumerate(rects) if r is not None]
        m = IDENTITY.copy() if prev is None else prev_from_cur(prev, pose)
        out.append((render(shown, pose, H1, W1, X_LO1, Y_LO1, VOXEL1), m, invert(m)))
        prev = pose
    return out


def random_moving_scene(seed, h, w, q_num, frames=4, voxel=0.5, moving=0.5, rects=None):
    """Random rectangles, a share of them moving at a constant velocity in the world, some missing per frame, under a random
    ego path; query indices permuted per frame.  → (list of (instance_map, m, n), x_lo, y_lo)"""
    rng = np.random.default_rng(seed)
    x_lo, y_lo = -w * voxel / 2, -h * voxel / 2
    boxes = []
    for _ in range(q_num if rects is None else rects):
        cx, cy = rng.uniform(x_lo * 0.8, -x_lo * 0.8), rng.uniform(y_lo * 0.8, -y_lo * 0.8)
        sx, sy = rng.uniform(0.6, 2.5), rng.uniform(0.6, 2.5)
        v = rng.uniform(-2.0, 2.0, 2) if rng.random() < moving else np.zeros(2)
        boxes.append((cx, cy, sx, sy, v))
    out, prev = [], None
    for k in range(frames):
        pose = pose_2d(rng.uniform(0.3, 1.0) * k, rng.uniform(-0.2, 0.2) * k, rng.uniform(-0.05, 0.05) * k)
        m = IDENTITY.copy() if prev is None else prev_from_cur(prev, pose)
        perm = rng.permutation(q_num)
        shown = [(int(perm[j % q_num]), cx + v[0] * k - sx, cx + v[0] * k + sx, cy + v[1] * k - sy, cy + v[1] * k + sy)
                 for j, (cx, cy, sx, sy, v) in enumerate(boxes) if rng.random() < 0.8]
        out.append((render(shown, pose, h, w, x_lo, y_lo, voxel), m, invert(m)))
        prev = pose
    return out, x_lo, y_lo
