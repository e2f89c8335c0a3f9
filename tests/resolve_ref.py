"""K42 restated in plain Python loops over dense boolean masks with Python ints (include/maskbev_hip.h states the rule): the
pairwise overlap of the kept masks, greedy mask NMS, Mask2Former's overlap filter and their composition for ONE frame.  Nothing
here is vectorised: the kernels of csrc/resolve.hip are held against these loops bit for bit."""


def self_overlap(masks, keep):
    """masks: Q dense maps (rows of rows of truth values), keep: Q flags → Q x Q ints: the cells set in both maps where both are
    kept (the diagonal: a kept mask's area), 0 wherever either is not."""
    q_num = len(keep)
    cells = []
    for q in range(q_num):
        cells.append({(y, x) for y, row in enumerate(masks[q]) for x, v in enumerate(row) if v} if keep[q] else None)
    inter = [[0] * q_num for _ in range(q_num)]
    for i in range(q_num):
        for j in range(i, q_num):                      # an intersection does not depend on the order of its two sets
            if cells[i] is not None and cells[j] is not None:
                inter[i][j] = inter[j][i] = len(cells[i] & cells[j])
    return inter


def nms(inter, scores, labels, keep, iou=(1, 2), same_label=True):
    """Stage N → (keep1, suppressed_by).  ``scores`` are compared as given (the callers pass f32 values)."""
    num, den = int(iou[0]), int(iou[1])
    q_num = len(keep)
    order = [q for q in range(q_num) if keep[q]]
    order.sort(key=lambda q: (-float(scores[q]), q))          # descending score, ties to the smaller q
    suppressed_by = [-1] * q_num
    for pos, i in enumerate(order):
        if suppressed_by[i] >= 0:
            continue
        for j in order[pos + 1:]:
            if suppressed_by[j] >= 0:
                continue
            if same_label and int(labels[i]) != int(labels[j]):
                continue
            both = int(inter[i][j])
            union = int(inter[i][i]) + int(inter[j][j]) - both
            if union > 0 and both * den >= num * union:
                suppressed_by[j] = i
    keep1 = [bool(keep[q]) and suppressed_by[q] < 0 for q in range(q_num)]
    return keep1, suppressed_by


def overlap_filter(instance_map, areas, keep, min_overlap=(4, 5), min_cells=1):
    """Stage F on one frame's map (rows of ints) → (keep2, owned, the new map).  ``min_overlap=None``: only ``min_cells``."""
    q_num = len(keep)
    owned = [0] * q_num
    for row in instance_map:
        for v in row:
            v = int(v)
            if 0 <= v < q_num and keep[v]:
                owned[v] += 1
    keep2 = []
    for q in range(q_num):
        ok = bool(keep[q]) and owned[q] >= int(min_cells)
        if ok and min_overlap is not None:
            ok = owned[q] * int(min_overlap[1]) >= int(min_overlap[0]) * int(areas[q])
        keep2.append(ok)
    new_map = [[-1 if (0 <= int(v) < q_num and not keep2[int(v)]) else int(v) for v in row] for row in instance_map]
    return keep2, owned, new_map


def resolve(masks, scores, labels, keep, rebuilt_map, nms_iou=(1, 2), min_overlap=(4, 5), min_cells=1, same_label=True):
    """The composition for one frame.  ``rebuilt_map``: the instance map of the queries that survive stage N (stage M is K21b's,
    pinned elsewhere) — the map itself, or a function of keep1 that returns it.  Returns a dict: ``keep``, ``suppressed_by``,
    ``owned``, ``instance_map`` and ``keep1``."""
    q_num = len(keep)
    if nms_iou is None:
        keep1, suppressed_by = [bool(k) for k in keep], [-1] * q_num
    else:
        keep1, suppressed_by = nms(self_overlap(masks, keep), scores, labels, keep, nms_iou, same_label)
    imap = rebuilt_map(keep1) if callable(rebuilt_map) else rebuilt_map
    areas = [sum(1 for row in masks[q] for v in row if v) for q in range(q_num)]
    keep2, owned, new_map = overlap_filter(imap, areas, keep1, min_overlap, min_cells)
    return dict(keep=keep2, suppressed_by=suppressed_by, owned=owned, instance_map=new_map, keep1=keep1)


def strip(*spans, width=12):
    """Dense 1 x ``width`` masks from half-open column spans: ``strip((0, 8), (2, 10))``; ``None``: an empty mask."""
    return [[[s is not None and s[0] <= x < s[1] for x in range(width)]] for s in spans]
