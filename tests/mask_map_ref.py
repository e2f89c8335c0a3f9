"""Shared by the mask-mAP tests: the state ``DeviceMaskMeanAveragePrecision`` keeps per image (rank, matched / ignored
flag words, counted ground truths), built from the oracle's ``coco_evaluate_image``, and the integer tables K29b is
tested on."""
import numpy as np

from oracle import metrics_oracle as MO

AREAS = list(MO.COCO_AREAS.values())
T, A = len(MO.COCO_IOU_THRS), len(AREAS)
RANK_NONE = 1 << 30


def iou_from_tables(inter, pa, ga):
    """(Q, G) f64 IoU of integer tables, 0 where the union is empty (oracle.pairwise_mask_iou's rule)."""
    union = pa[:, None] + ga[None, :] - inter
    return np.where(union > 0, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0)


def oracle_state(im, num_labels, max_det=MO.COCO_MAX_DETS[-1]):
    """One image (a dict as ``coco_mask_map`` takes it) → rank (Q,), matched (Q,), ignored (Q,) int64 with bit a * T + t,
    npig (num_labels, A): ``coco_evaluate_image`` per (class, area range), scattered back to the detections."""
    pl, gl = np.asarray(im['pred_labels']), np.asarray(im['gt_labels'])
    sc = np.asarray(im['scores'], dtype=np.float64)
    q = len(sc)
    rank = np.full(q, RANK_NONE, np.int64)
    matched, ignored = np.zeros(q, np.int64), np.zeros(q, np.int64)
    npig = np.zeros((num_labels, A), np.int64)
    for c in range(num_labels):
        di, gi = np.nonzero(pl == c)[0], np.nonzero(gl == c)[0]
        for a, rng in enumerate(AREAS):
            iou = np.asarray(im['ious'])[di][:, gi] if len(di) and len(gi) else np.zeros((len(di), len(gi)))
            dtind, dtm, dtig, gig = MO.coco_evaluate_image(iou, sc[di], np.asarray(im['pred_areas'])[di],
                                                           np.asarray(im['gt_areas'])[gi], rng, max_det)
            npig[c, a] = int((~gig).sum())
            for r, j in enumerate(dtind):
                d = di[j]
                rank[d] = r
                for t in range(T):
                    matched[d] |= int(dtm[t, r]) << (a * T + t)
                    ignored[d] |= int(dtig[t, r]) << (a * T + t)
    return rank, matched, ignored, npig


def integer_tables(rng, q, g, labels_below=3, no_object=False):
    """Integer tables of one image with everything the protocol can trip on: scores in steps of 0.05 (ties), IoUs that are
    exact fractions from {0, .5, .55, .6, .75, .9, 1} (ties at thresholds), areas on the 32^2 / 96^2 borders, two zero-area
    padding slots of class 0 at the end.  → inter (q, g), pred_area (q,), gt_area (g,) int64, scores (q,) f32,
    pred_labels (q,), gt_labels (g,) int64."""
    ga = np.concatenate([rng.choice([0, 900, 1024, 1025, 5000, 9216, 9217, 11000], g - 2), [0, 0]]).astype(np.int64)
    pa = rng.choice([0, 800, 1024, 3000, 9216, 9300, 12000], q).astype(np.int64)
    frac = rng.choice([0, 0, 0, .5, .55, .6, .75, .9, 1.0], (q, g))
    inter = np.floor(frac * np.minimum(pa[:, None], ga[None, :])).astype(np.int64)
    sc = (rng.integers(0, 20, q) / 20).astype(np.float32)
    pl = rng.integers(0, labels_below, q)
    gl = np.concatenate([rng.integers(1, 3, g - 2), [0, 0]])
    if no_object:
        gl[:], ga[:], inter[:] = 0, 0, 0
    return inter, pa, ga, sc, pl, gl


def image_dict(inter, pa, ga, sc, pl, gl):
    return dict(ious=iou_from_tables(inter, pa, ga), scores=sc.astype(np.float64), pred_labels=pl,
                pred_areas=pa.astype(np.float64), gt_labels=gl, gt_areas=ga.astype(np.float64))
