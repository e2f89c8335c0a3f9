"""The Mask2Former loss of all decoder outputs in ONE dtype (float32 or float64), with its two discrete decisions — the
Hungarian assignment and the importance-sampled points — either taken by the restatement itself (free mode) or handed in
(teacher-forced mode).

A dense restatement of oracle/maskbev_oracle.py A13 (match_cost, get_targets_single, loss_single, loss_dict; the reference's
mask2former_head.py:154-232, 326-426 with mmdet 3.0.0's costs and losses): the same operations in the same order, the same
draws in the same order from a ``PointSource``, and no ``.float()`` casts, so the whole evaluation runs in the dtype of its
inputs.  Every ground-truth column is a plain column (no padding convention).  The coordinates are the float32 draws, taken
as exact values of the evaluation dtype; the constant eps of the averaging factors is float32's, a constant of the model.

Free mode: assignment by scipy's linear_sum_assignment on its own cost, selection by its own ``topk``.
Teacher-forced: ``assignment`` (D, B, Q) holds the ground-truth column of every query or -1, ``points`` (D * g, P, 2) the
loss points of the matched (output, image, query) rows in ascending order — the order of the reference's
``mask_preds[mask_weights > 0]``.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

EPS32 = torch.finfo(torch.float32).eps
LOSS_W = dict(cls=2.0, mask=5.0, dice=5.0)               # loss weights (mask2former_head.py:96-110)
COST_W = dict(cls=2.0, mask=5.0, dice=5.0)               # matcher weights (ClassificationCost / CrossEntropyLossCost / DiceCost)


def spec(num_points, num_classes=1, class_weight=None, oversample_ratio=3.0, importance_sample_ratio=0.75):
    cw = list(class_weight) if class_weight is not None else [1.0] * num_classes + [0.1]
    return SimpleNamespace(num_points=int(num_points), num_classes=int(num_classes), class_weight=cw,
                           oversample_ratio=oversample_ratio, importance_sample_ratio=importance_sample_ratio)


def counts(cfg):
    """(candidates 3P, selected int(0.75 P), uniform tail) per row."""
    n_samp = int(cfg.num_points * cfg.oversample_ratio)
    n_unc = int(cfg.importance_sample_ratio * cfg.num_points)
    return n_samp, n_unc, cfg.num_points - n_unc


def draw_points(cfg, pts, outputs, batch, g):
    """Every uniform draw of one loss evaluation in the reference's order — per decoder output: B x rand(1, P, 2) for the
    matcher, then rand(g, 3P, 2) and rand(g, P - int(0.75 P), 2) for the importance sampling; g = matched rows per output
    = B * min(Q, G).  float32: (D, B, P, 2), (D * g, 3P, 2), (D * g, n_rand, 2)."""
    n_samp, _, n_rand = counts(cfg)
    mc, oc, rc = [], [], []
    for _ in range(outputs):
        mc.append(torch.cat([pts.rand(1, cfg.num_points, 2) for _ in range(batch)], 0))
        oc.append(pts.rand(g, n_samp, 2))
        rc.append(pts.rand(g, n_rand, 2) if n_rand > 0 else torch.zeros(g, 0, 2))
    return torch.stack(mc, 0), torch.cat(oc, 0), torch.cat(rc, 0)


def sample(maps, points):
    """mmcv point_sample: maps (N, H, W), points (N, P, 2) as (x, y) in [0, 1] -> (N, P); grid_sample at 2p - 1,
    align_corners=False, zero padding, in the dtype of ``maps``."""
    grid = 2.0 * points.to(maps.dtype).unsqueeze(2) - 1.0
    return F.grid_sample(maps.unsqueeze(1), grid, align_corners=False).squeeze(3).squeeze(1)


def match_cost(cls_score, mask_pts, gt_labels, gt_pts):
    """(Q, G) matching cost: 2 * (-softmax(cls)[label]) + 5 * BCE / P + 5 * dice (eps 1) on the sampled points."""
    cls_cost = -cls_score.softmax(-1)[:, gt_labels] * COST_W['cls']
    p, g = mask_pts, gt_pts
    n = p.shape[1]
    pos = F.binary_cross_entropy_with_logits(p, torch.ones_like(p), reduction='none')
    neg = F.binary_cross_entropy_with_logits(p, torch.zeros_like(p), reduction='none')
    bce = (torch.einsum('nc,mc->nm', pos, g) + torch.einsum('nc,mc->nm', neg, 1 - g)) / n * COST_W['mask']
    ps = p.sigmoid()
    numerator = 2 * torch.einsum('nc,mc->nm', ps, g)
    denominator = ps.sum(-1)[:, None] + g.sum(-1)[None, :]
    dice = (1 - (numerator + 1.0) / (denominator + 1.0)) * COST_W['dice']
    return cls_cost + bce + dice


def solve(cost):
    """(Q, G) cost -> (Q,) long: the column of every row in scipy's optimum, -1 for rows left out."""
    from scipy.optimize import linear_sum_assignment
    rows, cols = linear_sum_assignment(cost.detach().cpu().numpy())
    out = torch.full((cost.shape[0],), -1, dtype=torch.long)
    out[torch.from_numpy(rows)] = torch.from_numpy(cols)
    return out


def matched_rows(assignment):
    """Rows of the (D * B * Q) stacked maps that enter the mask losses: matched queries in ascending order per (output,
    image) — ``mask_preds[mask_weights > 0]`` — and their ground-truth rows b * G + column are the caller's to form."""
    return torch.nonzero(assignment.flatten() >= 0, as_tuple=False).squeeze(-1)


def _reduce(loss, avg_factor):
    return loss.sum() / (avg_factor + EPS32)                                # mmdet weight_reduce_loss


def _layer(cfg, cls, masks, labels_gt, gt, match_c, over_c, rand_c, assignment, points):
    """One decoder output: cls (B, Q, K + 1), masks (B, Q, H, W), gt (B, G, ny, nx) in the evaluation dtype."""
    b, q = cls.shape[:2]
    n_gt = labels_gt.shape[1]
    dt = masks.dtype
    n_samp, n_unc, n_rand = counts(cfg)
    costs, assign = [], []
    with torch.no_grad():
        for i in range(b):
            c = match_c[i:i + 1].to(dt)
            mp = sample(masks[i], c.repeat(q, 1, 1))
            gp = sample(gt[i], c.repeat(n_gt, 1, 1))
            costs.append(match_cost(cls[i], mp, labels_gt[i], gp))
            assign.append(solve(costs[-1]) if assignment is None else assignment[i].long().cpu())
    assign = torch.stack(assign, 0)                                          # (B, Q)
    pos = assign >= 0
    labels = torch.full((b, q), cfg.num_classes, dtype=torch.long)
    labels[pos] = torch.gather(labels_gt, 1, assign.clamp(min=0))[pos]
    labels = labels.flatten()
    class_weight = torch.tensor(cfg.class_weight, dtype=dt)
    ce = F.cross_entropy(cls.flatten(0, 1), labels, weight=class_weight, reduction='none')
    loss_cls = LOSS_W['cls'] * _reduce(ce, class_weight[labels].sum())
    num_total_masks = max(float(b * q), 1.0)                                 # MaskPseudoSampler: num_pos + num_neg = Q per image
    mp = masks[pos]                                                          # (g, H, W), ascending per image
    mask_targets = torch.cat([gt[i][assign[i][pos[i]]] for i in range(b)], 0)
    with torch.no_grad():
        logits = sample(mp, over_c.to(dt))                                   # (g, 3P)
        if points is None:
            idx = torch.topk(-logits.abs(), k=n_unc, dim=1)[1]
            coords = torch.gather(over_c, 1, idx.unsqueeze(-1).expand(-1, -1, 2))
            coords = torch.cat((coords, rand_c), dim=1) if n_rand > 0 else coords
        else:
            coords = points.float().cpu()
        tgt = sample(mask_targets, coords.to(dt))
    pred = sample(mp, coords.to(dt))
    ps = pred.sigmoid()
    a = torch.sum(ps * tgt, 1)
    dice = (2 * a + 1.0) / (torch.sum(ps, 1) + torch.sum(tgt, 1) + 1.0)
    loss_dice = LOSS_W['dice'] * _reduce(1 - dice, num_total_masks)
    bce = F.binary_cross_entropy_with_logits(pred.reshape(-1), tgt.reshape(-1), reduction='none')
    loss_mask = LOSS_W['mask'] * _reduce(bce, num_total_masks * cfg.num_points)
    return (loss_cls, loss_mask, loss_dice), torch.stack(costs, 0), assign, logits, coords


def loss_keys(outputs):
    """The entries of the loss dict that carry a value, in the reference's order (the height terms are the int 0)."""
    keys = ['loss_cls', 'loss_mask', 'loss_dice']
    for i in range(outputs - 1):
        keys += [f'd{i}.loss_cls', f'd{i}.loss_mask', f'd{i}.loss_dice']
    return keys


def loss_ref(cfg, cls, masks, labels_gt, gt, pts, dtype, assignment=None, points=None, weights=None):
    """cls (D, B, Q, K + 1), masks (D, B, Q, H, W), labels_gt (B, G) int64, gt (B, G, ny, nx); ``pts`` a PointSource (an
    object with ``rand(*shape)``).  ``weights``: {entry: upstream gradient} — the gradient of sum(w_k * loss[k]) with
    respect to cls and masks is then returned as well.  Result: loss (dict, the reference's keys and order), cost
    (D * B, Q, G), assignment (D, B, Q) long, candidates (D * g, 3P, 2) float32 with their sampled logits (D * g, 3P),
    tail (D * g, n_rand, 2), points (D * g, P, 2) float32, rows (D * g,) indices into the D * B * Q maps, d_cls, d_masks."""
    d, b, q = cls.shape[:3]
    n_gt = labels_gt.shape[1]
    g = b * min(q, n_gt)
    cls = cls.detach().to(dtype).clone().requires_grad_(weights is not None)
    masks = masks.detach().to(dtype).clone().requires_grad_(weights is not None)
    gt = gt.to(dtype)
    match_c, over_c, rand_c = draw_points(cfg, pts, d, b, g)
    res = []
    for i in range(d):
        res.append(_layer(cfg, cls[i], masks[i], labels_gt, gt, match_c[i], over_c[i * g:(i + 1) * g], rand_c[i * g:(i + 1) * g],
                          None if assignment is None else assignment[i],
                          None if points is None else points[i * g:(i + 1) * g]))
    terms = [r[0] for r in res]
    loss = dict(loss_cls=terms[-1][0], loss_mask=terms[-1][1], loss_dice=terms[-1][2], loss_height=0)
    for i, (lc, lm, ld) in enumerate(terms[:-1]):
        loss[f'd{i}.loss_cls'], loss[f'd{i}.loss_mask'], loss[f'd{i}.loss_dice'], loss[f'd{i}.loss_height'] = lc, lm, ld, 0
    out = SimpleNamespace(loss=loss, cost=torch.cat([r[1] for r in res], 0), assignment=torch.stack([r[2] for r in res], 0),
                          candidates=over_c, candidate_logits=torch.cat([r[3] for r in res], 0), tail=rand_c,
                          points=torch.cat([r[4] for r in res], 0), d_cls=None, d_masks=None)
    out.rows = matched_rows(out.assignment)
    if weights is not None:
        total = sum(float(weights[k]) * loss[k] for k in loss_keys(d))
        total.backward()
        out.d_cls, out.d_masks = cls.grad, masks.grad
    out.loss = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in loss.items()}
    return out
