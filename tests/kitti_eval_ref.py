"""Plain numpy restatement of the KITTI BEV evaluation chain, the yardstick of K25 / K26 / K27 and ``mask_bev_amd.kitti_eval``:

* the moment-axis box of a binary mask, from the words of include/maskbev_hip.h (K25), in float64;
* rectangle intersection by half-plane clipping in world coordinates, in float64 or — every operation — float32;
* the KITTI object protocol for the BEV metric, written from the published procedure: per-box codes, the greedy assignment,
  the 41 recall sample points, the interpolated precision and the 11-point AP.

tests/golden/kitti_eval.npz pins the protocol part against the reference's own functions (make_golden_kitti_eval.py).
"""
import numpy as np

KITTI_TYPES = ('Car', 'Van', 'Truck', 'Pedestrian', 'Person_sitting', 'Cyclist', 'Tram', 'Misc', 'DontCare')
CLASS_NAMES = ('car', 'pedestrian', 'cyclist', 'van', 'person_sitting')
MIN_HEIGHT, MAX_OCCLUSION, MAX_TRUNCATION = (40, 25, 25), (0, 1, 2), (0.15, 0.3, 0.5)
N_SAMPLE_PTS = 41


# ------------------------------------------------------------------------------------------------ K25
def fit_box(mask):
    """mask (H, W) bool → (n, [Σx, Σy, Σx², Σy², Σxy] as Python ints, box (5,) f64 = cx, cy, dx, dy, theta) in cell units."""
    ys, xs = np.nonzero(np.asarray(mask, dtype=bool))
    n = int(xs.size)
    xi, yi = [int(v) for v in xs], [int(v) for v in ys]
    mom = [sum(xi), sum(yi), sum(v * v for v in xi), sum(v * v for v in yi), sum(a * b for a, b in zip(xi, yi))]
    if n == 0:
        return 0, mom, np.zeros(5)
    m20, m02, m11 = n * mom[2] - mom[0] ** 2, n * mom[3] - mom[1] ** 2, n * mom[4] - mom[0] * mom[1]
    d = m20 - m02
    theta = 0.0 if (m11 == 0 and d == 0) else 0.5 * np.arctan2(2.0 * float(m11), float(d))
    c, s = np.cos(theta), np.sin(theta)
    x, y = xs.astype(np.float64), ys.astype(np.float64)
    u, v = x * c + y * s, y * c - x * s
    cell = abs(c) + abs(s)
    return n, mom, np.array([mom[0] / n, mom[1] / n, (u.max() - u.min()) + cell, (v.max() - v.min()) + cell, theta])


# ------------------------------------------------------------------------------------------------ K26
def corners(box, dtype=np.float64):
    """(x, y, dx, dy, angle) → (4, 2) corners in the order and with the expressions of ``rasterize.box_vertices``."""
    x, y, dx, dy, a = [dtype(v) for v in box]
    half = dtype(0.5)
    dl, dw = abs(dx) * half, abs(dy) * half
    c, s = np.cos(a), np.sin(a)
    d, d_bar = (c, s), (-s, c)
    sl, sw = (1, -1, -1, 1), (1, 1, -1, -1)
    return [(x + dtype(sl[k]) * dl * d[0] + dtype(sw[k]) * dw * d_bar[0], y + dtype(sl[k]) * dl * d[1] + dtype(sw[k]) * dw * d_bar[1])
            for k in range(4)]


def intersection_area(a, b, dtype=np.float64):
    """Area of the intersection of two rectangles: ``a`` clipped against the four edges of ``b`` (both counter-clockwise),
    then the shoelace sum.  Exactly 0 when fewer than three vertices survive."""
    poly, clip = corners(a, dtype), corners(b, dtype)
    zero = dtype(0)
    for k in range(4):
        (ex0, ey0), (ex1, ey1) = clip[k], clip[(k + 1) % 4]
        side = [(ex1 - ex0) * (py - ey0) - (ey1 - ey0) * (px - ex0) for px, py in poly]       # >= 0: inside (left of the edge)
        out = []
        for i in range(len(poly)):
            p, q, sp, sq = poly[i - 1], poly[i], side[i - 1], side[i]
            if (sp >= zero) != (sq >= zero):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
            if sq >= zero:
                out.append(q)
        poly = out
        if len(poly) < 3:
            return zero
    twice = zero
    x0, y0 = poly[0]
    for i in range(1, len(poly) - 1):
        twice = twice + ((poly[i][0] - x0) * (poly[i + 1][1] - y0) - (poly[i + 1][0] - x0) * (poly[i][1] - y0))
    return abs(twice) * dtype(0.5)


def rotate_iou(boxes, qboxes, criterion=-1, dtype=np.float64):
    """(N, 5), (K, 5) → (N, K) in ``dtype``: -1 IoU, 0 intersection / area of the box, 1 / area of the query box, 2 the
    intersection; 0 where the intersection is 0."""
    boxes, qboxes = np.asarray(boxes, dtype=dtype).reshape(-1, 5), np.asarray(qboxes, dtype=dtype).reshape(-1, 5)
    inter = np.zeros((boxes.shape[0], qboxes.shape[0]), dtype=dtype)
    for i, a in enumerate(boxes):
        for j, b in enumerate(qboxes):
            inter[i, j] = intersection_area(a, b, dtype)
    return overlap_from_intersection(inter, boxes, qboxes, criterion)


def overlap_from_intersection(inter, boxes, qboxes, criterion):
    """The four criteria from the (N, K) intersection areas, in their dtype."""
    dtype = inter.dtype.type
    boxes, qboxes = np.asarray(boxes, dtype=dtype).reshape(-1, 5), np.asarray(qboxes, dtype=dtype).reshape(-1, 5)
    area_a, area_b = np.abs(boxes[:, 2] * boxes[:, 3])[:, None], np.abs(qboxes[:, 2] * qboxes[:, 3])[None, :]
    den = {-1: area_a + area_b - inter, 0: area_a + 0 * inter, 1: area_b + 0 * inter, 2: np.ones_like(inter)}[criterion]
    out = np.zeros_like(inter)
    np.divide(inter, den, out=out, where=inter > 0)
    return out


def rotate_iou_frames(boxes, qboxes, box_offsets, qbox_offsets, criterion=-1, dtype=np.float64):
    """The per-frame matrices, flattened and concatenated: K26's output."""
    parts = [rotate_iou(boxes[box_offsets[f]:box_offsets[f + 1]], qboxes[qbox_offsets[f]:qbox_offsets[f + 1]], criterion,
                        dtype).reshape(-1) for f in range(len(box_offsets) - 1)]
    return np.concatenate(parts) if parts else np.zeros((0,), dtype=dtype)


# ------------------------------------------------------------------------------------------------ the protocol
def clean_data(gt, dt, current_class=0, difficulty=0):
    """gt: ``type`` (n) codes into KITTI_TYPES, ``bbox`` (n, 4), ``occluded`` (n), ``truncated`` (n); dt: ``type`` (k) and
    optionally ``bbox`` (k, 4) (absent: 100 pixels high) → (number of counted ground truths, gt codes, dt codes)."""
    want = CLASS_NAMES[current_class]
    neighbour = {'pedestrian': 'person_sitting', 'car': 'van'}.get(want)
    gt_codes, n_valid = [], 0
    for i, t in enumerate(gt['type']):
        name = KITTI_TYPES[int(t)].lower()
        height = gt['bbox'][i][3] - gt['bbox'][i][1]
        hard = (gt['occluded'][i] > MAX_OCCLUSION[difficulty] or gt['truncated'][i] > MAX_TRUNCATION[difficulty]
                or height <= MIN_HEIGHT[difficulty])
        if name == want and not hard:
            gt_codes.append(0)
            n_valid += 1
        elif name == neighbour or (name == want and hard):
            gt_codes.append(1)
        else:
            gt_codes.append(-1)
    dt_codes = []
    for i, t in enumerate(dt['type']):
        height = abs(dt['bbox'][i][3] - dt['bbox'][i][1]) if 'bbox' in dt else 100.0
        if height < MIN_HEIGHT[difficulty]:
            dt_codes.append(1)
        else:
            dt_codes.append(0 if KITTI_TYPES[int(t)].lower() == want else -1)
    return n_valid, np.array(gt_codes, dtype=np.int64), np.array(dt_codes, dtype=np.int64)


def compute_statistics(overlaps, gt_codes, dt_codes, scores, min_overlap, thresh=0.0, compute_fp=False):
    """One frame: overlaps (n_dt, n_gt) → (tp, fp, fn, scores of the detections matched as true positives)."""
    n_dt, n_gt = len(dt_codes), len(gt_codes)
    assigned = [False] * n_dt
    usable = [dt_codes[j] != -1 and not (compute_fp and scores[j] < thresh) for j in range(n_dt)]
    tp = fp = fn = 0
    matched = []
    for i in range(n_gt):
        if gt_codes[i] == -1:
            continue
        det, best_score, best_overlap, took_ignored = -1, 0.0, 0.0, False
        for j in range(n_dt):
            if not usable[j] or assigned[j] or not overlaps[j, i] > min_overlap:
                continue
            if not compute_fp:
                if det < 0 or scores[j] > best_score:
                    det, best_score = j, scores[j]
            elif dt_codes[j] == 0 and (overlaps[j, i] > best_overlap or took_ignored):
                det, best_overlap, took_ignored = j, overlaps[j, i], False
            elif dt_codes[j] == 1 and det < 0:
                det, took_ignored = j, True
        if det < 0:
            fn += int(gt_codes[i] == 0)
            continue
        assigned[det] = True
        if gt_codes[i] == 0 and dt_codes[det] == 0:
            tp += 1
            matched.append(scores[det])
    if compute_fp:
        fp = sum(1 for j in range(n_dt) if usable[j] and dt_codes[j] == 0 and not assigned[j])
    return tp, fp, fn, matched


def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """The scores at which the recall crosses the sample points 0, 1 / 40, ... (the matched scores in descending order)."""
    scores = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    out, current = [], 0.0
    for i, s in enumerate(scores):
        left = (i + 1) / num_gt
        right = (i + 2) / num_gt if i < len(scores) - 1 else left
        if i < len(scores) - 1 and (right - current) < (current - left):
            continue
        out.append(s)
        current += 1 / (num_sample_pts - 1.0)
    return np.array(out, dtype=np.float64)


def eval_class(frames, overlaps, current_class=0, difficulties=(0, 1, 2), min_overlaps=(0.7, 0.5)):
    """frames: list of (gt dict, dt dict with ``score``); overlaps: per frame (n_dt, n_gt) →
    dict(precision (D, K, 41), thresholds (D, K, 41), num_thresholds (D, K), stats: {(d, k): (T, 3) int64},
    num_valid_gt (D))."""
    nd, nk = len(difficulties), len(min_overlaps)
    precision, thresholds = np.zeros((nd, nk, N_SAMPLE_PTS)), np.zeros((nd, nk, N_SAMPLE_PTS))
    counts, stats, valid = np.zeros((nd, nk), dtype=np.int64), {}, np.zeros((nd,), dtype=np.int64)
    for d, difficulty in enumerate(difficulties):
        codes = [clean_data(gt, dt, current_class, difficulty) for gt, dt in frames]
        valid[d] = sum(c[0] for c in codes)
        for k, mo in enumerate(min_overlaps):
            matched = []
            for (gt, dt), ov, (_, gc, dc) in zip(frames, overlaps, codes):
                matched += compute_statistics(ov, gc, dc, dt['score'], mo)[3]
            th = get_thresholds(matched, valid[d]) if valid[d] > 0 else np.zeros((0,))
            pr = np.zeros((len(th), 3), dtype=np.int64)
            for t, thresh in enumerate(th):
                for (gt, dt), ov, (_, gc, dc) in zip(frames, overlaps, codes):
                    pr[t] += compute_statistics(ov, gc, dc, dt['score'], mo, thresh, True)[:3]
            p = np.zeros((N_SAMPLE_PTS,))
            p[:len(th)] = pr[:, 0] / np.maximum(pr[:, 0] + pr[:, 1], 1)
            for t in range(len(th)):
                p[t] = p[t:].max()
            precision[d, k], counts[d, k], stats[(d, k)] = p, len(th), pr
            thresholds[d, k, :len(th)] = th
    return dict(precision=precision, thresholds=thresholds, num_thresholds=counts, stats=stats, num_valid_gt=valid)


def get_map(precision):
    """11-point AP in percent: every 4th of the 41 sample points."""
    return precision[..., ::4].sum(-1) / 11 * 100
