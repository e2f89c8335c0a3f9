"""K32's protocol in numpy, in the formulation of semantic-kitti-api's ``PanopticEval.addBatchPanoptic`` (eval_np.py):
ignored points removed first, instance ids + 1, then per class ``np.unique`` over the ids and over the offset-combined
(prediction, ground truth) ids.  :func:`plain_frame` says the same with dicts of sets and ``Fraction``, written independently;
:func:`planted_case` builds the frames the GPU test feeds to the kernel."""
from fractions import Fraction

import numpy as np

OFFSET = 2 ** 32


def element_classes(pred_query, gt_word, query_class, class_lut, C):
    """Per element: (gt class, -1 = ignored; gt instance id; query, -1 = none; prediction class, 0 = none)."""
    pred_query = np.asarray(pred_query, dtype=np.int64).reshape(-1)
    gt_word = np.asarray(gt_word).astype(np.int64).reshape(-1) & 0xffffffff
    query_class = np.asarray(query_class, dtype=np.int64).reshape(-1)
    lut = np.asarray(class_lut, dtype=np.int64).reshape(-1)
    P = query_class.shape[0]
    sem, inst = gt_word & 0xffff, gt_word >> 16
    y_sem = np.full(sem.shape, -1, dtype=np.int64)
    in_table = sem < lut.shape[0]
    y_sem[in_table] = lut[sem[in_table]]
    y_sem[(y_sem < 0) | (y_sem >= C)] = -1
    q = np.where((pred_query >= 0) & (pred_query < P), pred_query, -1)
    x_sem = np.zeros(q.shape, dtype=np.int64)
    x_sem[q >= 0] = query_class[q[q >= 0]]
    no_thing = (x_sem < 1) | (x_sem >= C)
    x_sem[no_thing] = 0
    q = np.where(no_thing, -1, q)
    return y_sem, inst, q, x_sem


def frame(pred_query, gt_word, query_class, class_lut, C, max_gt, min_points):
    """One frame → dict(stats (C, 3) i32 = tp fp fn, iou (C) f64, confusion (C, C) i64, n_gt, gt_key (max_gt) i32, gt_area
    (max_gt) i32, pred_area (P) i32, ignored, in_pair)."""
    P = np.asarray(query_class).reshape(-1).shape[0]
    y_sem, y_inst, q, x_sem = element_classes(pred_query, gt_word, query_class, class_lut, C)
    keep = y_sem >= 0                                             # only points outside the ignored classes
    x_sem_row, y_sem_row = x_sem[keep], y_sem[keep]
    x_inst_row, y_inst_row = q[keep] + 1, y_inst[keep] + 1        # instances are not zeros
    confusion = np.zeros((C, C), dtype=np.int64)
    np.add.at(confusion, (y_sem_row, x_sem_row), 1)
    stats, iou = np.zeros((C, 3), dtype=np.int32), np.zeros((C,), dtype=np.float64)
    in_pair = 0
    for cl in range(1, C):
        x_inst_in_cl = x_inst_row * (x_sem_row == cl).astype(np.int64)
        y_inst_in_cl = y_inst_row * (y_sem_row == cl).astype(np.int64)
        unique_pred, counts_pred = np.unique(x_inst_in_cl[x_inst_in_cl > 0], return_counts=True)
        id2idx_pred = {i: k for k, i in enumerate(unique_pred)}
        matched_pred = np.zeros(unique_pred.shape[0], dtype=bool)
        unique_gt, counts_gt = np.unique(y_inst_in_cl[y_inst_in_cl > 0], return_counts=True)
        id2idx_gt = {i: k for k, i in enumerate(unique_gt)}
        matched_gt = np.zeros(unique_gt.shape[0], dtype=bool)
        valid_combos = (x_inst_in_cl > 0) & (y_inst_in_cl > 0)
        in_pair += int(valid_combos.sum())
        offset_combo = x_inst_in_cl[valid_combos] + OFFSET * y_inst_in_cl[valid_combos]
        unique_combo, counts_combo = np.unique(offset_combo, return_counts=True)
        gt_labels, pred_labels = unique_combo // OFFSET, unique_combo % OFFSET
        gt_areas = np.array([counts_gt[id2idx_gt[i]] for i in gt_labels], dtype=np.int64)
        pred_areas = np.array([counts_pred[id2idx_pred[i]] for i in pred_labels], dtype=np.int64)
        intersections = counts_combo.astype(np.int64)
        unions = gt_areas + pred_areas - intersections
        ious = intersections.astype(np.float64) / unions.astype(np.float64)
        tp_indexes = ious > 0.5
        stats[cl, 0] = tp_indexes.sum()
        iou[cl] = np.sum(ious[tp_indexes])
        matched_gt[[id2idx_gt[i] for i in gt_labels[tp_indexes]]] = True
        matched_pred[[id2idx_pred[i] for i in pred_labels[tp_indexes]]] = True
        stats[cl, 2] = np.sum((counts_gt >= min_points) & ~matched_gt)
        stats[cl, 1] = np.sum((counts_pred >= min_points) & ~matched_pred)
    thing = y_sem_row >= 1
    keys, areas = np.unique((y_sem_row[thing] << 16) | (y_inst_row[thing] - 1), return_counts=True)
    n_gt = keys.shape[0]
    gt_key, gt_area = np.full((max_gt,), -1, dtype=np.int32), np.zeros((max_gt,), dtype=np.int32)
    gt_key[:min(n_gt, max_gt)], gt_area[:min(n_gt, max_gt)] = keys[:max_gt], areas[:max_gt]
    pred_area = np.bincount(x_inst_row[x_inst_row > 0] - 1, minlength=P).astype(np.int32)
    if n_gt > max_gt:                                             # the frame overflows the tables: no numbers
        stats[:], iou[:] = 0, 0.0
    return dict(stats=stats, iou=iou, confusion=confusion, n_gt=np.int32(n_gt), gt_key=gt_key, gt_area=gt_area,
                pred_area=pred_area, ignored=int((~keep).sum()), in_pair=in_pair)


def frames(pred_query, gt_word, lengths, query_class, class_lut, C, max_gt, min_points, one=frame):
    """All frames: the dict of :func:`frame` with a leading frame axis (``ignored`` and ``in_pair`` summed)."""
    query_class = np.asarray(query_class)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    per = [one(pred_query[offs[f]:offs[f + 1]], gt_word[offs[f]:offs[f + 1]], query_class[f], class_lut, C, max_gt, min_points)
           for f in range(len(lengths))]
    out = {k: np.stack([p[k] for p in per]) for k in ('stats', 'iou', 'confusion', 'n_gt', 'gt_key', 'gt_area', 'pred_area')}
    out['ignored'], out['in_pair'] = sum(p['ignored'] for p in per), sum(p['in_pair'] for p in per)
    return out


def plain_frame(pred_query, gt_word, query_class, class_lut, C, max_gt, min_points):
    """:func:`frame` as plain loops: segments are sets of element indices in dicts, the 0.5 comparison is a ``Fraction``."""
    query_class = [int(v) for v in np.asarray(query_class).reshape(-1)]
    lut = [int(v) for v in np.asarray(class_lut).reshape(-1)]
    P = len(query_class)
    gt_seg, pred_seg, pred_cls = {}, {}, {}
    confusion = [[0] * C for _ in range(C)]
    ignored = 0
    for i, (q, w) in enumerate(zip([int(v) for v in pred_query], [int(v) & 0xffffffff for v in gt_word])):
        sem, inst = w & 0xffff, w >> 16
        gc = lut[sem] if sem < len(lut) else -1
        if not 0 <= gc < C:
            ignored += 1
            continue
        pc = query_class[q] if 0 <= q < P else 0
        if not 1 <= pc < C:
            pc, q = 0, -1
        confusion[gc][pc] += 1
        if gc >= 1:
            gt_seg.setdefault((gc, inst), set()).add(i)
        if q >= 0:
            pred_seg.setdefault(q, set()).add(i)
            pred_cls[q] = pc
    stats, iou = [[0, 0, 0] for _ in range(C)], [0.0] * C
    matched_gt, matched_pred, in_pair = set(), set(), 0
    for (gc, inst) in sorted(gt_seg):
        for q in sorted(pred_seg):
            if pred_cls[q] != gc:
                continue
            inter = len(gt_seg[(gc, inst)] & pred_seg[q])
            in_pair += inter
            union = len(gt_seg[(gc, inst)]) + len(pred_seg[q]) - inter
            if inter > 0 and Fraction(inter, union) > Fraction(1, 2):
                stats[gc][0] += 1
                iou[gc] += inter / union
                matched_gt.add((gc, inst))
                matched_pred.add(q)
    for key, members in gt_seg.items():
        if key not in matched_gt and len(members) >= min_points:
            stats[key[0]][2] += 1
    for q, members in pred_seg.items():
        if q not in matched_pred and len(members) >= min_points:
            stats[pred_cls[q]][1] += 1
    keys = sorted(gt_seg)
    gt_key, gt_area = [-1] * max_gt, [0] * max_gt
    for k, key in enumerate(keys[:max_gt]):
        gt_key[k], gt_area[k] = (key[0] << 16) | key[1], len(gt_seg[key])
    if len(keys) > max_gt:
        stats, iou = [[0, 0, 0] for _ in range(C)], [0.0] * C
    return dict(stats=np.array(stats, dtype=np.int32), iou=np.array(iou, dtype=np.float64),
                confusion=np.array(confusion, dtype=np.int64), n_gt=np.int32(len(keys)),
                gt_key=np.array(gt_key, dtype=np.int32), gt_area=np.array(gt_area, dtype=np.int32),
                pred_area=np.array([len(pred_seg.get(q, ())) for q in range(P)], dtype=np.int32), ignored=ignored,
                in_pair=in_pair)


def word(sem, inst):
    return (np.asarray(inst, dtype=np.int64) << 16) | np.asarray(sem, dtype=np.int64)


def as_i32(words):
    """u32 bit patterns (held in int64) as the int32 array a device tensor carries."""
    return (np.asarray(words, dtype=np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)


def random_case(rng, lengths, P, C, lut_len=12):
    """Random frames with few distinct instances and queries, so that segments overlap: (pred_query i32, gt_word i32 bits,
    query_class (F, P) i32, class_lut i32)."""
    n = int(sum(lengths))
    lut = rng.integers(-1, C, lut_len).astype(np.int32)
    lut[1], lut[2] = 0, 1
    runs = n // 8 + 1                                               # runs of eight share semantics, instance and query, mostly
    run = np.repeat(rng.integers(0, 4, runs), 8)[:n]
    run_sem = np.repeat(np.where(rng.random(runs) < 0.7, 2, 1), 8)[:n]
    sem = np.where(rng.random(n) < 0.85, run_sem, rng.integers(0, lut_len + 2, n))
    inst = np.where(rng.random(n) < 0.9, run, rng.integers(0, 4, n))
    pq = np.where(rng.random(n) < 0.9, np.where(run_sem == 2, run % max(P, 1), -1), rng.integers(-2, P + 2, n))
    query_class = rng.integers(-1, C + 1, (len(lengths), P)).astype(np.int32)
    query_class[:, :min(P, 3)] = 1
    return pq.astype(np.int32), as_i32(word(sem, inst)), query_class, lut


# ---------------------------------------------------------------------------------------------- the GPU test's frames
SIZES = (0, 1, 257, 1000)               # an empty frame, and both sides of the 256-thread block
MIN_POINTS = 5
LUT = np.array([-1, 0, 1, 2, -7, 0, 1, 0] + [0] * 12, dtype=np.int32)   # [3], [5] and [7] are set per C in planted_case
LUT_LEN = LUT.shape[0]                  # 20: semantic ids 25 and 65535 lie outside the table


def planted_case(P, C, seed=0):
    """Four frames of SIZES elements for ``P`` queries and ``C`` classes, MIN_POINTS = 5: (pred_query, gt_word, lengths,
    query_class (4, P), class_lut).  Planted (see the comments): a segment fed by two blocks of a frame, the inter = 2,
    union = 4 tie, areas of MIN_POINTS and MIN_POINTS - 1 on both sides, instance ids 0 and 65535, a semantic id >= the
    table's length, table values -1, -7 and C, queries P, 2^30 and -5, query classes 0, C and -3, a query with no element,
    and in the last frame more than 8 (and fewer than 64) ground-truth segments."""
    rng = np.random.default_rng(seed)
    lut = LUT.copy()
    lut[3] = C - 1                      # semantic 3: the last thing class (class 1 again when C == 2)
    lut[5] = C                          # a table value past the classes: ignored
    lut[7] = C - 1
    hostile = np.array([-1, -1, P, 2 ** 30, -5], dtype=np.int64)
    # roles -> queries; with fewer than 7 queries the missing roles get values past P (they count as -1)
    role = {r: (k if k < P else P + k) for k, r in enumerate(('match', 'tie', 'fp5', 'cls0', 'clsC', 'clsneg', 'fpb'))}
    qc = rng.integers(-3, C + 1, (4, P)).astype(np.int32)
    for f in range(4):
        for r, c in (('match', 1), ('tie', 1), ('fp5', 1), ('cls0', 0), ('clsC', C), ('clsneg', -3), ('fpb', 1)):
            if role[r] < P:
                qc[f, role[r]] = c
    if P >= 7:
        qc[3, role['clsC']] = C - 1     # in the last frame that query is a thing of the last class
    free = np.arange(7, P) if P > 7 else np.array([], dtype=np.int64)
    if free.size:
        qc[:, free[-1]] = 1             # a valid query that owns no element (never drawn below)
        free = free[:-1]

    def background(n, thing_insts):
        """n elements: ignored and class-0 semantics, some small things, hostile and free queries."""
        sem = rng.choice([0, 1, 4, 5, 25, 65535, 1, 1], n)
        inst = rng.integers(0, 3, n)
        if len(thing_insts):
            t = rng.random(n) < 0.25
            sem = np.where(t, rng.choice([2, 3], n), sem)
            inst = np.where(t, rng.choice(thing_insts, n), inst)
        pq = rng.choice(hostile, n)
        if free.size:
            pq = np.where(rng.random(n) < 0.5, rng.choice(free, n), pq)
        return word(sem, inst), pq

    def plant(words, pq, at, sems, insts, queries):
        k = len(queries)
        words[at:at + k], pq[at:at + k] = word(np.broadcast_to(sems, (k,)), np.broadcast_to(insts, (k,))), queries

    out_w, out_q = [], []
    # frame 0: empty.  frame 1: one element, a thing of one point under the matching query
    out_w.append(word([2], [1]))
    out_q.append(np.array([role['match']]))
    # frame 2, 257 elements, 5 ground-truth segments
    w, q = background(257, [])
    w[:140], q[:140] = word(1, 0), -1
    every = dict(role)
    if P < 7:                                                               # too few queries for every role: here the first
        role = dict(role, match=P + 7, fpb=0)                               # one is the unmatched prediction
    plant(w, q, 0, 2, 0, [role['match']] * 50 + [-1] * 10)                  # instance 0: 61 points with the last element,
    plant(w, q, 256, 2, 0, [-1])                                            # which the second block feeds; IoU 50 / 61
    plant(w, q, 60, 0, 0, [role['match']] * 2)                              # ignored under the prediction: not its area
    plant(w, q, 62, [6, 6, 6, 1], [65535, 65535, 65535, 0], [-1, role['tie'], role['tie'], role['tie']])   # 2 / 4: no match
    plant(w, q, 70, 2, 7, [-1] * 5)                                         # unmatched, MIN_POINTS points: fn
    plant(w, q, 80, 2, 8, [2 ** 30] * 4)                                    # unmatched, MIN_POINTS - 1: not counted
    plant(w, q, 90, 1, 0, [role['fp5']] * 4)                                # a prediction of MIN_POINTS - 1: not counted
    plant(w, q, 100, 1, 0, [role['fpb']] * 5)                               # a prediction of MIN_POINTS: fp
    plant(w, q, 110, 2, 5, [role['cls0']] * 10)                             # under a query of class 0: unmatched, fn
    plant(w, q, 120, 1, 0, [role['clsC']] * 10 + [role['clsneg']] * 10)     # queries of classes C and -3: no segment
    role = every
    out_w.append(w)
    out_q.append(q)
    # frame 3, 1000 elements, between 9 and 63 segments
    w, q = background(1000, np.arange(100, 110))
    w[200:440], q[200:440] = word(1, 0), -1
    plant(w, q, 200, 2, 0, [role['match']] * 120 + [-1] * 10)   # crosses the block border at 256; 120 / 130
    plant(w, q, 330, 0, 0, [role['match']] * 5)
    plant(w, q, 340, [6, 6, 6, 1], [65535, 65535, 65535, 0], [-1, role['tie'], role['tie'], role['tie']])
    plant(w, q, 350, 2, 7, [-5] * 5)
    plant(w, q, 360, 2, 8, [P] * 4)
    plant(w, q, 370, 1, 0, [role['fp5']] * 5)                               # a prediction of MIN_POINTS: fp
    plant(w, q, 390, 7, 3, [role['clsC']] * 10)                             # the last class: a perfect match
    plant(w, q, 400, 2, 9, [role['fpb']] * 6 + [-1] * 4)                    # 6 / 10
    plant(w, q, 410, 25, 4, [role['fpb']] * 10)                             # semantic id past the table: ignored
    plant(w, q, 420, [4, 5] * 10, 2, [role['fp5']] * 20)                    # table values -7 and C: ignored
    out_w.append(w)
    out_q.append(q)
    return (np.concatenate(out_q).astype(np.int64).astype(np.int32), as_i32(np.concatenate(out_w)), list(SIZES), qc, lut)
