"""numpy f64 restatement of the KITTI object augmentations (mask_bev_amd/object_augment.py on the host, K28 in
csrc/object_augment.hip), written from the rules in include/maskbev_hip.h (K28) and the docstrings of the two transforms, not
from their code: the collision rule and the sequential noise search with plain loops over boxes, tries and edges; the
``object_sample`` count and acceptance rule; membership, move, removal and append order of the points, vectorised over the
points of one scan only.  Draws come from a ``np.random.Generator`` in the documented order, so a seeded product run can be
replayed here."""
import numpy as np

REMOVE, MOVE = 1, 2


# ------------------------------------------------------------------------------------------------ footprints, collision
def corners(box):
    """[cx, cy, cz, l, w, h, theta] → (4, 2): l along the yaw direction, w across it, counter-clockwise."""
    cx, cy, _, l, w, _, th = [float(v) for v in box]
    ux, uy = np.cos(th), np.sin(th)            # along
    vx, vy = -uy, ux                           # across
    hl, hw = l / 2, w / 2
    return np.array([[cx + hl * ux + hw * vx, cy + hl * uy + hw * vy], [cx - hl * ux + hw * vx, cy - hl * uy + hw * vy],
                     [cx - hl * ux - hw * vx, cy - hl * uy - hw * vy], [cx + hl * ux - hw * vx, cy + hl * uy - hw * vy]])


def _turns(p, q, r):
    return (r[1] - p[1]) * (q[0] - p[0]) > (q[1] - p[1]) * (r[0] - p[0])


def _strictly_inside(quad, pt):
    signs = []
    for k in range(4):
        a, b = quad[k], quad[(k + 1) % 4]
        signs.append((b[0] - a[0]) * (pt[1] - a[1]) - (b[1] - a[1]) * (pt[0] - a[0]))
    return all(s > 0 for s in signs) or all(s < 0 for s in signs)


def collide(p, q):
    """Two (4, 2) quadrilaterals: hulls overlap with positive width and height, and two edges cross by the strict
    orientation comparisons or one holds every corner of the other strictly."""
    if not (min(p[:, 0].max(), q[:, 0].max()) - max(p[:, 0].min(), q[:, 0].min()) > 0):
        return False
    if not (min(p[:, 1].max(), q[:, 1].max()) - max(p[:, 1].min(), q[:, 1].min()) > 0):
        return False
    for k in range(4):
        a, b = p[k], p[(k + 1) % 4]
        for m in range(4):
            c, d = q[m], q[(m + 1) % 4]
            if _turns(a, c, d) != _turns(b, c, d) and _turns(a, b, c) != _turns(a, b, d):
                return True
    return all(_strictly_inside(p, pt) for pt in q) or all(_strictly_inside(q, pt) for pt in p)


# ------------------------------------------------------------------------------------------------ the two transforms
def object_noise(rng, boxes, translation_std=(0.25, 0.25, 0.25), rot_range=(-0.15707963267, 0.15707963267), num_try=100):
    """→ (rot (n), loc (n, 3), selected (n) bool).  A frame without boxes draws nothing."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    n = len(boxes)
    rot, loc, selected = np.zeros(n), np.zeros((n, 3)), np.zeros(n, dtype=bool)
    if n == 0:
        return rot, loc, selected
    loc_noises = rng.normal(scale=np.asarray(translation_std, dtype=np.float64), size=(n, num_try, 3))
    rot_noises = rng.uniform(rot_range[0], rot_range[1], size=(n, num_try))
    current = [corners(b) for b in boxes]
    for i in range(n):
        for j in range(num_try):
            c, s = np.cos(rot_noises[i, j]), np.sin(rot_noises[i, j])
            rel = current[i] - boxes[i, :2]
            cand = np.stack([c * rel[:, 0] - s * rel[:, 1], s * rel[:, 0] + c * rel[:, 1]], -1) + (boxes[i, :2] + loc_noises[i, j, :2])
            if not any(collide(cand, current[k]) for k in range(n) if k != i):
                current[i] = cand
                rot[i], loc[i], selected[i] = rot_noises[i, j], loc_noises[i, j], True
                break
    return rot, loc, selected


def object_sample(rng, boxes, bank_boxes, num_sample):
    """→ the accepted bank indices in paste order."""
    count = (int(rng.integers(0, num_sample)) + int(rng.integers(0, num_sample)) + int(rng.integers(0, num_sample))) % num_sample
    avoid = [corners(b) for b in np.asarray(boxes, dtype=np.float64).reshape(-1, 7)]
    accepted = []
    for _ in range(count):
        k = int(rng.integers(0, len(bank_boxes)))
        fp = corners(bank_boxes[k])
        if not any(collide(fp, a) for a in avoid):
            accepted.append(k)
            avoid.append(fp)
    return accepted


def frame(rng, boxes, bank_boxes=None, num_sample=None, noise=None):
    """One frame through ``object_sample`` (when ``num_sample`` is given) then ``object_noise`` (when ``noise`` is a dict of its
    keywords) → (boxes before the noise (labels + pasted), pasted indices, rot, loc, flags)."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    n_labels = len(boxes)
    pasted = [] if num_sample is None else object_sample(rng, boxes, bank_boxes, num_sample)
    if pasted:
        boxes = np.concatenate([boxes, np.asarray(bank_boxes, dtype=np.float64)[pasted]])
    n = len(boxes)
    flags = np.zeros(n, dtype=np.int64)
    flags[n_labels:] |= REMOVE
    rot, loc = np.zeros(n), np.zeros((n, 3))
    if noise is not None:
        rot, loc, _ = object_noise(rng, boxes, **noise)
        flags |= MOVE
    return boxes, pasted, rot, loc, flags


def moved_boxes(boxes, rot, loc):
    out = np.array(boxes, dtype=np.float64).reshape(-1, 7)
    out[:, :3] += loc
    out[:, 6] += rot
    return out


# ------------------------------------------------------------------------------------------------ the points (K28)
def inside(points, box):
    """(n, >= 3) f32 points against one box [cx, cy, cz, l, w, h, theta]: strict on every face; cz is the bottom."""
    x, y, z = (points[:, k].astype(np.float64) for k in range(3))
    c, s = np.cos(box[6]), np.sin(box[6])
    dx, dy = x - box[0], y - box[1]
    lx = c * dx + s * dy
    ly = c * dy - s * dx
    dz = z - box[2]
    return (np.abs(lx) < box[3] / 2) & (np.abs(ly) < box[4] / 2) & (dz > 0) & (dz < box[5])


def first_box(points, boxes, mask=None):
    """Index of the first box (of those with ``mask``) that holds each point, or -1."""
    first = np.full(len(points), -1, dtype=np.int32)
    for j in range(len(boxes) - 1, -1, -1):
        if mask is None or mask[j]:
            first[inside(points, boxes[j])] = j
    return first


def move(points, boxes, rot, loc, flags):
    """Every point moved by the first box with the move bit that holds it (boxes: before the noise) → f32 copy."""
    out = np.array(points, dtype=np.float32, copy=True)
    first = first_box(points, boxes, (np.asarray(flags) & MOVE) != 0)
    for j in np.unique(first[first >= 0]):
        sel = first == j
        x, y, z = (points[sel, k].astype(np.float64) for k in range(3))
        dx, dy = x - boxes[j, 0], y - boxes[j, 1]
        c, s = np.cos(rot[j]), np.sin(rot[j])
        out[sel, 0] = (((c * dx - s * dy) + boxes[j, 0]) + loc[j, 0]).astype(np.float32)
        out[sel, 1] = (((s * dx + c * dy) + boxes[j, 1]) + loc[j, 1]).astype(np.float32)
        out[sel, 2] = (z + loc[j, 2]).astype(np.float32)
    return out


def scan(points, boxes, rot, loc, flags, pasted_points=()):
    """One scan (n, dim) f32 → the kept scene points in input order, moved, then every pasted sample's points (each (m, 4)
    f32; a dim = 3 scan takes their first three columns) in paste order, moved and never removed."""
    points = np.asarray(points, dtype=np.float32)
    dim = points.shape[1]
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    flags = np.asarray(flags, dtype=np.int64).reshape(-1)
    gone = np.zeros(len(points), dtype=bool)
    for j in range(len(boxes)):
        if flags[j] & REMOVE:
            gone |= inside(points, boxes[j])
    parts = [move(points, boxes, rot, loc, flags)[~gone]]
    for p in pasted_points:
        parts.append(move(np.asarray(p, dtype=np.float32)[:, :dim], boxes, rot, loc, flags))
    return np.concatenate(parts) if parts else points
