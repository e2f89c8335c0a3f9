"""K39 restated from the words of include/maskbev_hip.h: the rolling world grid of tracked footprints (K39a) and the query map
turned back into bit-packed masks (K39b) — the yardstick of tests/test_k39_fuse_gpu.py and tests/test_fuse_cpu.py.  `step` /
`masks_from_map` are numpy, with the f64 expressions in the header's order ((a * x + b * y) + c, (p - lo) / v, one rounding per
operation); `plain_step` / `plain_masks_from_map` say the same in plain Python loops with integer `%` and `math.floor`.  The
scene builders reuse tests/track_ref.py's `render` and `pose_2d`."""
import math

import numpy as np

from tests import track_ref as R

TWO40 = float(2 ** 40)


def store_size(h, w):
    """The smallest store side: even, (S - 4)^2 >= h^2 + w^2."""
    s = 4
    while (s - 4) ** 2 < h * h + w * w:
        s += 1
    return s + (s & 1)


def fresh_state(h, w, s=None):
    s = store_size(h, w) if s is None else s
    return dict(owner=np.full((s, s), -1, np.int32), count=np.zeros((s, s), np.int32), window=np.zeros(4, np.int64))


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def new_corner(m, n, h, w, s, x_lo, y_lo, v):
    """Step 1's (wx0', wy0') as Python ints, or None for an invalid frame."""
    m, n = np.asarray(m, np.float64).reshape(6), np.asarray(n, np.float64).reshape(6)
    if not (np.all(np.isfinite(m)) and np.all(np.isfinite(n))):
        return None
    with np.errstate(all='ignore'):
        x_lo, y_lo, v = np.float64(x_lo), np.float64(y_lo), np.float64(v)
        cx, cy = x_lo + (np.float64(w) * 0.5) * v, y_lo + (np.float64(h) * 0.5) * v
        qx = ((m[0] * cx + m[1] * cy) + m[2]) / v
        qy = ((m[3] * cx + m[4] * cy) + m[5]) / v
    if not (abs(qx) < TWO40 and abs(qy) < TWO40):
        return None
    return int(math.floor(qx)) - s // 2, int(math.floor(qy)) - s // 2


def moving_queries(vel, q_num, static_speed):
    """(Q) bool: vx * vx + vy * vy > static_speed * static_speed; all False without velocities; a NaN is not moving."""
    if vel is None:
        return np.zeros(q_num, bool)
    vel = np.asarray(vel, np.float64).reshape(q_num, 2)
    with np.errstate(all='ignore'):
        return vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1] > np.float64(static_speed) * np.float64(static_speed)


def step(state, imap, qt, m, n, x_lo, y_lo, v, cap, hit, miss, min_count, vis=None, vel=None, static_speed=0.0):
    """One frame of K39a on `state` (changed in place) → (fused_ids, fused_queries), both (H, W) int32."""
    imap, qt = np.asarray(imap, np.int32), np.asarray(qt, np.int32)
    m, n = np.asarray(m, np.float64).reshape(6), np.asarray(n, np.float64).reshape(6)
    h, w = imap.shape
    s, q_num = state['owner'].shape[0], qt.shape[0]
    none = np.full((h, w), -1, np.int32)
    corner = new_corner(m, n, h, w, s, x_lo, y_lo, v)
    if corner is None:
        return none, none.copy()
    wx0, wy0 = corner
    mov = moving_queries(vel, q_num, static_speed)
    qt_pad = np.concatenate([qt, np.array([-1], np.int32)])            # slot Q: "no query"
    mov_pad = np.concatenate([mov, [False]])
    # 1. the window
    idx = np.arange(s, dtype=np.int64)
    gx, gy = wx0 + np.mod(idx - wx0, s), wy0 + np.mod(idx - wy0, s)
    owner, count = state['owner'].copy(), state['count'].astype(np.int64)
    if int(state['window'][2]) == 0:
        clear = np.ones((s, s), bool)
    else:
        ox0, oy0 = int(state['window'][0]), int(state['window'][1])
        clear = (gy != oy0 + np.mod(idx - oy0, s))[:, None] | (gx != ox0 + np.mod(idx - ox0, s))[None, :]
    owner[clear], count[clear] = -1, 0
    # 2. the update: one gather per store cell
    with np.errstate(all='ignore'):
        x, y = ((gx.astype(np.float64) + 0.5) * v)[None, :], ((gy.astype(np.float64) + 0.5) * v)[:, None]
        xs, ys = (n[0] * x + n[1] * y) + n[2], (n[3] * x + n[4] * y) + n[5]
        fx, fy = np.floor((xs - x_lo) / v), np.floor((ys - y_lo) / v)
        inside = (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
    jx, jy = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
    q = imap[jy, jx]
    qc = np.where(inside & (q >= 0) & (q < q_num), q, q_num)
    act = inside & ~mov_pad[qc]
    g = qt_pad[qc]
    same, other = act & (g >= 0) & (owner == g), act & (g >= 0) & (owner != g)
    seen = np.ones((s, s), bool) if vis is None else np.asarray(vis)[jy, jx] != 0
    nod = act & (g < 0) & seen
    take, drop = other & (count - hit <= 0), nod & (count - miss <= 0)
    count = np.where(same, np.minimum(count + hit, cap),
                     np.where(other, np.where(take, hit, count - hit), np.where(nod, np.where(drop, 0, count - miss), count)))
    owner = np.where(take, g, np.where(drop, -1, owner)).astype(np.int32)
    state['owner'], state['count'] = owner, count.astype(np.int32)
    # 3. the read-out: one gather per sensor cell
    ix, iy = np.meshgrid(np.arange(w), np.arange(h))
    with np.errstate(all='ignore'):
        x, y = x_lo + (ix + 0.5) * v, y_lo + (iy + 0.5) * v
        wgx, wgy = np.floor(((m[0] * x + m[1] * y) + m[2]) / v), np.floor(((m[3] * x + m[4] * y) + m[5]) / v)
        inwin = (wgx >= float(wx0)) & (wgx < float(wx0) + float(s)) & (wgy >= float(wy0)) & (wgy < float(wy0) + float(s))
    sx, sy = np.mod(np.where(inwin, wgx, 0).astype(np.int64), s), np.mod(np.where(inwin, wgy, 0).astype(np.int64), s)
    own, cnt = state['owner'][sy, sx], state['count'][sy, sx]
    ok = inwin & (own >= 0) & (cnt >= min_count)
    query = np.full((h, w), -1, np.int32)
    for k in reversed(range(q_num)):                                   # the smallest q wins: written last
        if not mov[k]:
            query[ok & (own == qt[k])] = k
    q0 = np.where((imap >= 0) & (imap < q_num), imap, q_num)
    through = mov_pad[q0] & (qt_pad[q0] >= 0)
    ids = np.where(through, qt_pad[q0], np.where(ok, own, -1)).astype(np.int32)
    queries = np.where(through, imap, np.where(ok, query, -1)).astype(np.int32)
    state['window'] = np.array([wx0, wy0, int(state['window'][2]) + 1, 0], np.int64)
    return ids, queries


def plain_step(state, imap, qt, m, n, x_lo, y_lo, v, cap, hit, miss, min_count, vis=None, vel=None, static_speed=0.0):
    """The same frame cell by cell in plain Python: integer `%`, `math.floor`, Python floats."""
    h, w = len(imap), len(imap[0])
    s, q_num = state['owner'].shape[0], len(qt)
    m, n = [float(a) for a in np.asarray(m).reshape(6)], [float(a) for a in np.asarray(n).reshape(6)]
    x_lo, y_lo, v = float(x_lo), float(y_lo), float(v)
    none = np.full((h, w), -1, np.int32)
    if not all(math.isfinite(a) for a in m + n):
        return none, none.copy()
    cx, cy = x_lo + (w * 0.5) * v, y_lo + (h * 0.5) * v
    qx, qy = ((m[0] * cx + m[1] * cy) + m[2]) / v, ((m[3] * cx + m[4] * cy) + m[5]) / v
    if not (abs(qx) < TWO40 and abs(qy) < TWO40):
        return none, none.copy()
    wx0, wy0 = math.floor(qx) - s // 2, math.floor(qy) - s // 2
    ox0, oy0, frames = (int(a) for a in state['window'][:3])

    def moving(q):
        if vel is None:
            return False
        vx, vy = float(vel[q][0]), float(vel[q][1])
        return vx * vx + vy * vy > float(static_speed) * float(static_speed)

    def finite_floor(a):
        return math.floor(a) if math.isfinite(a) else None

    owner, count = state['owner'], state['count']
    for sy in range(s):
        for sx in range(s):
            gx, gy = wx0 + (sx - wx0) % s, wy0 + (sy - wy0) % s
            own, cnt = int(owner[sy, sx]), int(count[sy, sx])
            if frames == 0 or gx != ox0 + (sx - ox0) % s or gy != oy0 + (sy - oy0) % s:
                own, cnt = -1, 0
            x, y = (float(gx) + 0.5) * v, (float(gy) + 0.5) * v
            fx = finite_floor(((n[0] * x + n[1] * y) + n[2] - x_lo) / v)
            fy = finite_floor(((n[3] * x + n[4] * y) + n[5] - y_lo) / v)
            if fx is not None and fy is not None and 0 <= fx < w and 0 <= fy < h:
                q = int(imap[fy][fx])
                is_query = 0 <= q < q_num
                if not (is_query and moving(q)):
                    g = int(qt[q]) if is_query else -1
                    if g >= 0 and own == g:
                        cnt = min(cnt + hit, cap)
                    elif g >= 0:
                        cnt -= hit
                        if cnt <= 0:
                            own, cnt = g, hit
                    elif vis is None or int(vis[fy][fx]) != 0:
                        cnt -= miss
                        if cnt <= 0:
                            own, cnt = -1, 0
            owner[sy, sx], count[sy, sx] = own, cnt
    ids, queries = none, none.copy()
    for iy in range(h):
        for ix in range(w):
            q = int(imap[iy][ix])
            if 0 <= q < q_num and moving(q) and int(qt[q]) >= 0:
                ids[iy, ix], queries[iy, ix] = int(qt[q]), q
                continue
            x, y = x_lo + (ix + 0.5) * v, y_lo + (iy + 0.5) * v
            gx, gy = finite_floor(((m[0] * x + m[1] * y) + m[2]) / v), finite_floor(((m[3] * x + m[4] * y) + m[5]) / v)
            if gx is None or gy is None or not (wx0 <= gx < wx0 + s and wy0 <= gy < wy0 + s):
                continue
            own, cnt = int(owner[gy % s, gx % s]), int(count[gy % s, gx % s])
            if own >= 0 and cnt >= min_count:
                ids[iy, ix] = own
                for k in range(q_num):
                    if int(qt[k]) == own and not moving(k):
                        queries[iy, ix] = k
                        break
    state['window'] = np.array([wx0, wy0, frames + 1, 0], np.int64)
    return ids, queries


def run(state, frames, x_lo, y_lo, v, cap, hit, miss, min_count, static_speed=0.0, fn=step):
    """`frames`: dicts with imap, qt, m, n and optionally vis, vel → [(ids, queries)] after stepping `state` through them."""
    return [fn(state, fr['imap'], fr['qt'], fr['m'], fr['n'], x_lo, y_lo, v, cap, hit, miss, min_count, fr.get('vis'), fr.get('vel'),
               static_speed) for fr in frames]


# ---- K39b -----------------------------------------------------------------------------------------------------------------

def packed_words(h, w):
    return (h * w + 63) // 64 * 2


def masks_from_map(maps, q_num):
    """(F, H, W) int32 → (words (F * Q, packed_words) uint32, areas (F, Q) int32)."""
    maps = np.asarray(maps, np.int32)
    f, h, w = maps.shape
    dense = maps.reshape(f, 1, h * w) == np.arange(q_num, dtype=np.int32).reshape(1, q_num, 1)
    bits = np.zeros((f * q_num, packed_words(h, w) * 32), np.uint64)
    bits[:, :h * w] = dense.reshape(f * q_num, h * w)
    words = (bits.reshape(f * q_num, -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return words, dense.sum(axis=2).astype(np.int32)


def plain_masks_from_map(maps, q_num):
    f, h, w = len(maps), len(maps[0]), len(maps[0][0])
    words = [[0] * packed_words(h, w) for _ in range(f * q_num)]
    areas = [[0] * q_num for _ in range(f)]
    for k in range(f):
        for y in range(h):
            for x in range(w):
                q = int(maps[k][y][x])
                if 0 <= q < q_num:
                    p = y * w + x
                    words[k * q_num + q][p // 32] |= 1 << (p % 32)
                    areas[k][q] += 1
    return np.array(words, np.uint32).reshape(f * q_num, packed_words(h, w)), np.array(areas, np.int32).reshape(f, q_num)


# ---- scenes ---------------------------------------------------------------------------------------------------------------

def transforms(pose0, pose):
    """(world_from_cur, cur_from_world), both (2, 3) f64, the world being the frame of `pose0`."""
    m = R.prev_from_cur(pose0, pose)
    return m, np.ascontiguousarray(np.linalg.inv(np.vstack([m, [0.0, 0.0, 1.0]]))[:2])


IDENTITY_PAIR = (R.IDENTITY.copy(), R.IDENTITY.copy())

WALK = dict(h=40, w=48, q_num=8, voxel=0.5, x_lo=-20.0, y_lo=-4.0, frames=12, static_speed=0.4)


def random_walk(seed=0):
    """12 frames on a 40 x 48 grid (S = 68), Q = 8, voxel 0.5, the grid off-centre (its centre is (-8, 6), so world cells
    are negative from the start); the ego turns 0.3 rad a frame (3.3 rad > pi in all) and drives 0.9 m a frame along its
    heading.  World-fixed rectangles with global ids from 10 up, the queries permuted per frame; some queries get -1 as their
    id, a few cells hold values outside [0, Q); random visibility bytes (a third 0); velocities around the static speed of 0.4,
    one of them NaN.  → a list of frame dicts (imap, qt, m, n, vis, vel)."""
    c = WALK
    rng = np.random.default_rng(seed)
    rects = []
    for _ in range(7):
        x0, y0 = rng.uniform(-24.0, 4.0), rng.uniform(-8.0, 18.0)
        rects.append((x0, x0 + rng.uniform(1.5, 5.0), y0, y0 + rng.uniform(1.0, 4.0)))
    pose0, frames = None, []
    x = y = yaw = 0.0
    for k in range(c['frames']):
        pose = R.pose_2d(x, y, yaw)
        pose0 = pose if pose0 is None else pose0
        m, n = transforms(pose0, pose)
        perm = rng.permutation(c['q_num'])
        shown = [(int(perm[j]),) + r for j, r in enumerate(rects) if rng.random() < 0.8]
        imap = R.render(shown, pose, c['h'], c['w'], c['x_lo'], c['y_lo'], c['voxel'])
        stray = rng.random(imap.shape) < 0.01
        imap[stray] = rng.choice(np.array([c['q_num'], 100, -5, 2 ** 31 - 1], np.int32), size=int(stray.sum()))
        qt = np.full(c['q_num'], -1, np.int32)
        for j in range(len(rects)):
            qt[perm[j]] = 10 + j
        qt[rng.random(c['q_num']) < 0.2] = -1
        vis = np.where(rng.random(imap.shape) < 0.33, 0, rng.integers(1, 4, imap.shape)).astype(np.uint8)
        vel = rng.normal(0.0, 0.4, (c['q_num'], 2))
        if k == 5:
            vel[3, 0] = np.nan
        frames.append(dict(imap=imap, qt=qt, m=m, n=n, vis=vis, vel=vel))
        yaw += 0.3
        x, y = x + 0.9 * math.cos(yaw), y + 0.9 * math.sin(yaw)
    return frames


def rect_map(h, w, rects):
    """(query, y0, y1, x0, x1) in cells → the (H, W) instance map."""
    out = np.full((h, w), -1, np.int32)
    for q, y0, y1, x0, x1 in rects:
        out[y0:y1, x0:x1] = q
    return out


def still_frame(imap, qt, vis=None, vel=None):
    """A frame of a standing sensor."""
    return dict(imap=np.asarray(imap, np.int32), qt=np.asarray(qt, np.int32), m=IDENTITY_PAIR[0], n=IDENTITY_PAIR[1], vis=vis,
                vel=vel)


def bridging_scene(h=16, w=20, passed=False):
    """An object (query 1, id 7) on rows 4 .. 9, columns 5 .. 12 in frames 0 - 3 and 6, absent in frames 4 - 5, where its
    footprint has visibility 0 (or, with `passed`, 1: seen empty); everything else is seen.  Q = 3."""
    foot = (slice(4, 10), slice(5, 13))
    frames = []
    for k in range(7):
        there = k not in (4, 5)
        vis = np.ones((h, w), np.uint8)
        if not there and not passed:
            vis[foot] = 0
        frames.append(still_frame(rect_map(h, w, [(1, 4, 10, 5, 13)] if there else []), [-1, 7 if there else -1, -1], vis))
    return frames, foot


def completion_scene(h=16, w=24):
    """A 4 x 12-cell object (id 5): its left half (columns 4 .. 9) is seen in frames 0 - 2 as query 0, then its right half
    (columns 10 .. 15) in frames 3 - 5 as query 2 with the left half unknown (visibility 0).  Q = 3."""
    frames = []
    for k in range(6):
        vis = np.ones((h, w), np.uint8)
        if k < 3:
            imap, qt = rect_map(h, w, [(0, 6, 10, 4, 10)]), [5, -1, -1]
        else:
            imap, qt = rect_map(h, w, [(2, 6, 10, 10, 16)]), [-1, -1, 5]
            vis[6:10, 4:10] = 0
        frames.append(still_frame(imap, qt, vis))
    return frames


def straight_drive(h=8, w=8, steps=24, cells_per_step=1, voxel=1.0):
    """The ego drives along +x in whole-cell steps over more than S cells (S = 16 for 8 x 8); an object (query 0, id 3) is seen
    in frame 0 only, every later frame is empty with everything seen... except that nothing of the old place is in view."""
    frames = []
    pose0 = R.pose_2d(0.0, 0.0, 0.0)
    for k in range(steps):
        m, n = transforms(pose0, R.pose_2d(k * cells_per_step * voxel, 0.0, 0.0))
        imap = rect_map(h, w, [(0, 2, 6, 0, 2)]) if k == 0 else np.full((h, w), -1, np.int32)
        frames.append(dict(imap=imap, qt=np.array([3 if k == 0 else -1], np.int32), m=m, n=n, vis=None, vel=None))
    return frames


# ---- scenarios: `runner(frames, h, w, x_lo, y_lo, v, cap, hit, miss, min_count, static_speed)` → ([(ids, queries)] per frame,
# [the state after every frame]); tests/test_fuse_cpu.py runs them on `step`, tests/test_k39_fuse_gpu.py on the kernels --------

def ref_runner(frames, h, w, x_lo, y_lo, v, cap, hit, miss, min_count, static_speed=0.0):
    state, outs, states = fresh_state(h, w), [], []
    for fr in frames:
        outs += run(state, [fr], x_lo, y_lo, v, cap, hit, miss, min_count, static_speed)
        states.append(copy_state(state))
    return outs, states


def scenario_scroll_and_wrap(runner):
    """8 x 8 cells of 1 m (S = 16), 24 whole-cell steps along +x, miss = 0 so that nothing decays: what frame 0 wrote into the
    store columns of world cells -4 and -3 must not come back when those columns are reused for world cells 12 and 13."""
    frames = straight_drive()
    outs, states = runner(frames, 8, 8, -4.0, -4.0, 1.0, 4, 4, 0, 1, 0.0)
    assert states[0]['owner'].shape == (16, 16) and int((states[0]['owner'] == 3).sum()) == 8
    assert np.array_equal(np.argwhere(outs[0][0] == 3), [[y, x] for y in range(2, 6) for x in range(2)])
    assert np.array_equal(np.argwhere(outs[1][0] == 3), [[y, 0] for y in range(2, 6)])          # world cell -3, remembered
    for k in range(2, len(frames)):
        assert (outs[k][0] == -1).all() and (outs[k][1] == -1).all(), k
    assert [int((s['owner'] == 3).sum()) for s in states[:6]] == [8, 8, 8, 8, 8, 4]              # cell -4 leaves at step 5
    assert all((s['owner'] == -1).all() and not s['count'].any() for s in states[6:])
    assert [tuple(int(a) for a in s['window']) for s in states[:3]] == [(-8, -8, 1, 0), (-7, -8, 2, 0), (-6, -8, 3, 0)]


def scenario_pose_jump(runner):
    """A jump of S cells or more clears everything, and jumping back finds nothing."""
    base = straight_drive(steps=1)[0]
    pose0 = R.pose_2d(0.0, 0.0, 0.0)
    far, back = dict(base), dict(base)
    far['m'], far['n'] = transforms(pose0, R.pose_2d(16.0, 0.0, 0.0))
    far['imap'] = back['imap'] = np.full((8, 8), -1, np.int32)
    outs, states = runner([base, far, back], 8, 8, -4.0, -4.0, 1.0, 4, 4, 0, 1, 0.0)
    assert int((states[0]['owner'] == 3).sum()) == 8
    for k in (1, 2):
        assert (states[k]['owner'] == -1).all() and not states[k]['count'].any() and (outs[k][0] == -1).all()
    assert tuple(int(a) for a in states[2]['window']) == (-8, -8, 3, 0)


def scenario_bridging(runner, passed):
    cap, hit, miss, min_count = 8, 1, 2, 2
    frames, foot = bridging_scene(passed=passed)
    outs, states = runner(frames, 16, 20, 0.0, 0.0, 1.0, cap, hit, miss, min_count, 0.0)
    c, shown = 0, []
    for k in range(7):
        if k not in (4, 5):
            c = min(c + hit, cap) if c > 0 else hit
        elif passed:
            c = max(c - miss, 0)
        want_ids = np.full((16, 20), -1, np.int32)
        want_q = want_ids.copy()
        if c >= min_count:
            want_ids[foot] = 7
            want_q[foot] = 1 if k not in (4, 5) else -1
        assert np.array_equal(outs[k][0], want_ids) and np.array_equal(outs[k][1], want_q), k
        shown.append(c >= min_count)
    assert shown == ([False, True, True, True, True, False, False] if passed else [False] + [True] * 6)


def scenario_completion(runner):
    frames = completion_scene()
    outs, states = runner(frames, 16, 24, 0.0, 0.0, 1.0, 8, 1, 1, 2, 0.0)
    whole = np.full((16, 24), -1, np.int32)
    whole[6:10, 4:16] = 5
    left = np.full((16, 24), -1, np.int32)
    left[6:10, 4:10] = 5
    assert np.array_equal(outs[2][0], left) and np.array_equal(outs[3][0], left)                 # the right half has count 1
    for k in (4, 5):
        assert np.array_equal(outs[k][0], whole) and np.array_equal(outs[k][1], np.where(whole >= 0, 2, -1)), k
    return frames, outs


def scenario_moving(runner):
    """A static object A (query 0, id 1; rows 4 .. 7, columns 4 .. 11) in every frame; in frame 2 a moving query (query 1, id
    2) covers columns 8 .. 15 of the same rows.  It is written through in frame 2, leaves nothing in the store, and the cells
    of A under it keep their count."""
    h, w = 12, 20
    a = rect_map(h, w, [(0, 4, 8, 4, 12)])
    both = rect_map(h, w, [(0, 4, 8, 4, 12), (1, 4, 8, 8, 16)])
    still, fast = np.zeros((2, 2)), np.array([[0.0, 0.0], [1.0, 0.0]])
    frames = [still_frame(a, [1, -1], vel=still), still_frame(a, [1, -1], vel=still), still_frame(both, [1, 2], vel=fast),
              still_frame(a, [1, -1], vel=still)]
    outs, states = runner(frames, h, w, 0.0, 0.0, 1.0, 8, 1, 1, 2, 0.5)
    want = np.where(both == 1, 2, np.where(a == 0, 1, -1))
    assert np.array_equal(outs[2][0], want) and np.array_equal(outs[2][1], np.where(both == 1, 1, np.where(a == 0, 0, -1)))
    assert all(not (s['owner'] == 2).any() for s in states)
    cnt = states[2]['count'][:h, :w]                                  # identity pose, x_lo = y_lo = 0: store cell = sensor cell
    assert (cnt[4:8, 4:8] == 3).all() and (cnt[4:8, 8:12] == 2).all() and not cnt[4:8, 12:16].any()
    assert (states[2]['owner'][4:8, 4:12] == 1).all() and (states[2]['owner'][4:8, 12:16] == -1).all()
    assert np.array_equal(outs[3][0], np.where(a == 0, 1, -1)) and (states[3]['count'][4:8, 8:12] == 3).all()


def scenario_invalid_pose(runner):
    h, w = 12, 20
    a = rect_map(h, w, [(0, 4, 8, 4, 12)])
    good = still_frame(a, [1])
    nan, huge = dict(good), dict(good)
    nan['m'] = np.array([[1.0, 0.0, np.nan], [0.0, 1.0, 0.0]])
    huge['n'] = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, np.inf]])
    far = dict(good)
    far['m'] = np.array([[1.0, 0.0, 1e300], [0.0, 1.0, 0.0]])
    outs, states = runner([good, good, nan, huge, far, good], h, w, 0.0, 0.0, 1.0, 8, 1, 1, 2, 0.0)
    for k in (2, 3, 4):
        assert (outs[k][0] == -1).all() and (outs[k][1] == -1).all()
        for key in states[1]:
            assert states[k][key].tobytes() == states[1][key].tobytes(), (k, key)
    assert np.array_equal(outs[5][0], np.where(a == 0, 1, -1)) and int(states[5]['window'][2]) == 3
    assert (states[5]['count'][4:8, 4:12] == 3).all()


def turning_footprint(frames=12, yaw_step=0.05, drive=0.5):
    """The nearest-cell loss, for the documents: a world-fixed 4 m x 2 m rectangle (32 cells of 0.5 m in frame 0) on the
    40 x 48 grid of tests/track_ref.py, the ego turning `yaw_step` rad and driving `drive` m a frame, default settings (cap 8,
    hit 1, miss 1, min_count 2), everything seen.  → per frame (detected cells, fused cells, cells that are both)."""
    state, out, pose0 = fresh_state(R.H0, R.W0), [], R.pose_2d(0.0, 0.0, 0.0)
    for k in range(frames):
        pose = R.pose_2d(drive * k, 0.0, yaw_step * k)
        m, n = transforms(pose0, pose)
        imap = R.render([(0, -3.0, 1.0, 2.0, 4.0)], pose, R.H0, R.W0, R.X_LO0, R.Y_LO0, R.VOXEL0)
        ids, _ = step(state, imap, np.array([4], np.int32), m, n, R.X_LO0, R.Y_LO0, R.VOXEL0, 8, 1, 1, 2)
        out.append((int((imap == 0).sum()), int((ids == 4).sum()), int(((ids == 4) & (imap == 0)).sum())))
    return out
