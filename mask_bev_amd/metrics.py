"""Metrics path of the training / validation step, GPU-native.

Reference: ``MaskBevPanopticHead.update_mAP_metrics`` (mask_bev/models/head/mask_bev_panoptic_head.py:34-96), called
per decoder layer and step from ``MaskBevModule.training_step`` (mask_bev_module.py:273-275), with the metric objects
of mask_bev/evaluation/detection_metric.py.  There it re-runs the Hungarian matcher per sample, upsamples all Q masks
to ground-truth resolution, thresholds and hands dense tensors to torchmetrics.  Here:

* the assignment is the one the loss just computed (``Mask2FormerHead.last_assignment``, K9) — no second matching;
* the mask IoU of the matched pairs is computed by K15 straight from the low-resolution logits and the bit-packed
  ground truth (``matched_mask_iou``);
* ``MeanIoU`` / ``BinaryClassifScores`` mirror the reference's metric objects without torchmetrics (states are device
  tensors; ``compute`` is the only synchronisation).

* the ``map_metric`` slot (torchmetrics ``MeanAveragePrecision(iou_type='segm')`` in the reference, which hands the
  dense masks to pycocotools at ``compute``) is :class:`MaskMeanAveragePrecision`: the (Q, G) IoU matrix of every image
  is formed on the GPU at ``update`` (bilinear upsampling, threshold, two {0,1} GEMMs) and only that matrix, the
  scores, labels and areas are kept; ``compute`` runs the COCO protocol on them.
* :class:`DeviceMaskMeanAveragePrecision` fills the same slot without leaving the device: bit-packed predicted masks
  from K21, pairwise popcounts and the per-image COCO matching from K29 (csrc/mask_map.hip), no host synchronisation in
  ``update``; ``compute`` accumulates the whole dataset in vectorised torch and copies twelve numbers back.
* :class:`DevicePanopticQuality` has no counterpart in the reference: PQ / SQ / RQ / IoU of the lifted point labels (K31)
  or of the BEV instance map (K21) in the SemanticKITTI panoptic protocol, per-frame counts from K32 (csrc/panoptic.hip).
* :class:`DeviceTubeAssociation` and :func:`lstq`: the association term of LSTQ over a sequence from the tracked point ids
  (K33, csrc/track.hip), for the thing classes the model predicts.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import torch

from . import _lib, ops
from ._lib import MaskBevHipError, check

_EPS = 1e-12          # average_precision.py:7


@torch.no_grad()
def matched_mask_iou(pred_logits: torch.Tensor, assignment: torch.Tensor, gt: 'ops.PackedMasks') -> torch.Tensor:
    """``pred_logits`` (B, Q, h, w) mask logits of one decoder output, ``assignment`` (B, Q) int32 (query → ground-
    truth slot of its image, −1 = unmatched), ``gt``: the B*G bit-packed ground-truth masks at (ny, nx).
    → IoU (B, Q) f32 at ground-truth resolution: bilinear upsampling (align_corners=False), sigmoid > 0.5,
    ``inter / (union + 1e-12)`` (mask_bev_panoptic_head.py:74-85, average_precision.py:78-81)."""
    lib = _lib.load()
    if not pred_logits.is_cuda:
        raise MaskBevHipError('matched_mask_iou needs ROCm device tensors (no CPU fallback)')
    b, q, h, w = pred_logits.shape
    logits = pred_logits.float().contiguous()
    g = gt.words.shape[0] // b
    dev = logits.device
    assignment = assignment.to(torch.int32)
    img = torch.arange(b, device=dev, dtype=torch.int32).view(b, 1)
    gt_row = torch.where(assignment >= 0, img * g + assignment, torch.full_like(assignment, -1)).contiguous()
    pred_row = torch.arange(b * q, device=dev, dtype=torch.int32)
    inter = torch.empty(b * q, dtype=torch.int32, device=dev)
    union = torch.empty(b * q, dtype=torch.int32, device=dev)
    check(lib.mbv_matched_mask_iou(logits.data_ptr(), pred_row.data_ptr(), gt.words.data_ptr(), gt_row.data_ptr(),
                                   b * q, h, w, gt.h, gt.w, inter.data_ptr(), union.data_ptr(),
                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
          'mbv_matched_mask_iou')
    return (inter.float() / (union.float() + _EPS)).view(b, q)


class MeanIoU:
    """detection_metric.py:77-92 — mean of all IoUs seen since ``reset``."""

    def __init__(self):
        self.ious: List[torch.Tensor] = []

    def update(self, ious: torch.Tensor):
        self.ious.append(ious.detach().flatten())

    def compute(self):
        if not self.ious:
            return 0.0
        return torch.cat(self.ious).mean()

    def reset(self):
        self.ious = []


class BinaryClassifScores:
    """State of detection_metric.py:10-31 (scores of the evaluated class and the matched targets); the 11-threshold
    average precision of ``compute`` is the binned binary AP of torchmetrics ``binary_average_precision``."""

    def __init__(self, thresholds: int = 11):
        self.y_score: List[torch.Tensor] = []
        self.y_true: List[torch.Tensor] = []
        self.thresholds = thresholds

    def update(self, y_score: torch.Tensor, y_true: torch.Tensor):
        self.y_score.append(y_score.detach().flatten())
        self.y_true.append(y_true.detach().flatten())

    def compute(self):
        if not self.y_score:
            return 0.0
        s, t = torch.cat(self.y_score).float(), torch.cat(self.y_true) > 0
        th = torch.linspace(0, 1, self.thresholds, device=s.device)
        pred = s.view(1, -1) >= th.view(-1, 1)                                   # (T, N)
        tp = (pred & t.view(1, -1)).sum(1).float()
        fp = (pred & ~t.view(1, -1)).sum(1).float()
        fn = (~pred & t.view(1, -1)).sum(1).float()
        precision = torch.where(tp + fp > 0, tp / (tp + fp), torch.ones_like(tp))
        recall = torch.where(tp + fn > 0, tp / (tp + fn), torch.zeros_like(tp))
        precision = torch.cat([precision, precision.new_ones(1)])
        recall = torch.cat([recall, recall.new_zeros(1)])
        return -torch.sum((recall[1:] - recall[:-1]) * precision[:-1])

    def reset(self):
        self.y_score, self.y_true = [], []


class MaskMeanAveragePrecision:
    """COCO-protocol mask mAP with torchmetrics' defaults (IoU thresholds 0.50:0.05:0.95, 101 recall thresholds, max
    detections 1 / 10 / 100, area ranges all / small / medium / large, classes = labels present) — the object the
    reference puts in the ``map_metric`` slot (mask_bev_module.py:85-94) and feeds at mask_bev_panoptic_head.py:87-96
    with ``scores = softmax[:, 0]``, ``labels = argmax``, all Q upsampled binary masks and ALL ground-truth slots (the
    zero-mask padding included: class-0 ground truths of area 0).  ``compute()`` returns the twelve COCO numbers under
    torchmetrics' names (map, map_50, map_75, map_small/medium/large, mar_1/10/100, mar_small/medium/large).
    The greedy matching of COCOeval.evaluateImg is vectorised over the IoU thresholds; checked against the plain-loop
    restatement in oracle/metrics_oracle.py (parity with torchmetrics itself is unpinned: it is not installed)."""

    IOU_THRS = torch.linspace(0.5, 0.95, 10, dtype=torch.float64)
    REC_THRS = torch.linspace(0.0, 1.0, 101, dtype=torch.float64)
    MAX_DETS = (1, 10, 100)
    AREAS = (('all', 0.0, 1e10), ('small', 0.0, 32.0 ** 2), ('medium', 32.0 ** 2, 96.0 ** 2), ('large', 96.0 ** 2, 1e10))

    def __init__(self):
        self.images: List[dict] = []

    def reset(self):
        self.images = []

    @torch.no_grad()
    def update(self, pred_logits: torch.Tensor, scores: torch.Tensor, pred_labels: torch.Tensor,
               gt_masks: torch.Tensor, gt_labels: torch.Tensor):
        """One batch: ``pred_logits`` (B, Q, h, w) mask logits, ``scores`` / ``pred_labels`` (B, Q), ``gt_masks``
        (B, G, ny, nx) {0, 1}, ``gt_labels`` (B, G).  Pairwise IoU at ground-truth resolution on the device."""
        b, q = scores.shape
        gt = gt_masks.to(torch.bfloat16).flatten(2)                                         # {0,1}: exact in bf16
        for i in range(b):
            up = torch.nn.functional.interpolate(pred_logits[i].float().unsqueeze(1), gt_masks.shape[-2:],
                                                 mode='bilinear', align_corners=False).squeeze(1)
            pm = (up > 0).to(torch.bfloat16).flatten(1)                                     # sigmoid(x) > 0.5
            inter = torch.mm(pm, gt[i].t(), out_dtype=torch.float32) if pm.is_cuda else (pm.float() @ gt[i].float().t())
            pa, ga = pm.float().sum(1), gt[i].float().sum(1)
            union = pa.view(-1, 1) + ga.view(1, -1) - inter
            iou = torch.where(union > 0, inter / union.clamp(min=1), torch.zeros_like(inter))
            self.images.append(dict(ious=iou.double().cpu(), scores=scores[i].double().cpu(),
                                    pred_labels=pred_labels[i].long().cpu(), pred_areas=pa.double().cpu(),
                                    gt_labels=gt_labels[i].long().cpu(), gt_areas=ga.double().cpu()))

    @classmethod
    def _evaluate_image(cls, iou, sc, d_area, g_area, lo, hi, max_det):
        """COCOeval.evaluateImg for one (image, class, area range), all IoU thresholds at once."""
        g_ig = ~((g_area >= lo) & (g_area <= hi))
        gtind = torch.sort(g_ig.to(torch.int8), stable=True).indices
        dtind = torch.sort(-sc, stable=True).indices[:max_det]
        g_ig = g_ig[gtind]
        d, g, t = len(dtind), len(gtind), len(cls.IOU_THRS)
        iou = iou[dtind][:, gtind] if d and g else torch.zeros((d, g), dtype=torch.float64)
        taken = torch.zeros((t, g), dtype=torch.bool)
        dtm = torch.zeros((t, d), dtype=torch.bool)
        dt_ig = torch.zeros((t, d), dtype=torch.bool)
        thr = torch.clamp(cls.IOU_THRS, max=1 - 1e-10)
        rev = torch.arange(g - 1, -1, -1)
        for k in range(d):
            if g == 0:
                break
            ok = (~taken) & (iou[k].view(1, g) >= thr.view(t, 1))                          # (T, G) candidates
            best = torch.full((t,), -1, dtype=torch.long)
            for ig in (False, True):                      # a non-ignored ground truth wins over any ignored one
                cand = ok & (g_ig.view(1, g) == ig)
                val = torch.where(cand, iou[k].view(1, g).expand(t, g), torch.full((t, g), -1.0, dtype=torch.float64))
                # among equal IoUs the LAST ground truth in the sorted order wins (the loop's `>=` update)
                arg = rev[torch.argmax(val[:, rev], dim=1)]
                hit = (val.gather(1, arg.view(t, 1)).view(t) >= 0) & (best < 0)
                best = torch.where(hit, arg, best)
            m = best >= 0
            if m.any():
                rows = torch.nonzero(m).flatten()
                taken[rows, best[rows]] = True
                dtm[rows, k] = True
                dt_ig[rows, k] = g_ig[best[rows]]
        out_rng = ~((d_area[dtind] >= lo) & (d_area[dtind] <= hi))
        dt_ig = dt_ig | (~dtm & out_rng.view(1, d))
        return sc[dtind], dtm, dt_ig, g_ig

    def compute(self) -> dict:
        imgs = self.images
        classes = sorted({int(c) for im in imgs for c in im['pred_labels'].tolist() + im['gt_labels'].tolist()})
        t, r, k_n, a_n, m_n = len(self.IOU_THRS), len(self.REC_THRS), len(classes), len(self.AREAS), len(self.MAX_DETS)
        precision = -torch.ones((t, r, k_n, a_n, m_n), dtype=torch.float64)
        recall = -torch.ones((t, k_n, a_n, m_n), dtype=torch.float64)
        eps = torch.finfo(torch.float64).eps
        for k, c in enumerate(classes):
            for a, (_, lo, hi) in enumerate(self.AREAS):
                per_img = []
                for im in imgs:
                    di = torch.nonzero(im['pred_labels'] == c).flatten()
                    gi = torch.nonzero(im['gt_labels'] == c).flatten()
                    if len(di) == 0 and len(gi) == 0:
                        continue
                    iou = im['ious'][di][:, gi]
                    per_img.append(self._evaluate_image(iou, im['scores'][di], im['pred_areas'][di], im['gt_areas'][gi],
                                                        lo, hi, self.MAX_DETS[-1]))
                if not per_img:
                    continue
                for m, max_det in enumerate(self.MAX_DETS):
                    scores = torch.cat([e[0][:max_det] for e in per_img])
                    inds = torch.sort(-scores, stable=True).indices
                    dtm = torch.cat([e[1][:, :max_det] for e in per_img], 1)[:, inds]
                    dtig = torch.cat([e[2][:, :max_det] for e in per_img], 1)[:, inds]
                    npig = int(sum(int((~e[3]).sum()) for e in per_img))
                    if npig == 0:
                        continue
                    tp = torch.cumsum((dtm & ~dtig).double(), 1)
                    fp = torch.cumsum((~dtm & ~dtig).double(), 1)
                    nd = tp.shape[1]
                    rc = tp / npig
                    pr = tp / (fp + tp + eps)
                    recall[:, k, a, m] = rc[:, -1] if nd else 0.0
                    if nd:
                        pr = torch.flip(torch.cummax(torch.flip(pr, (1,)), 1).values, (1,))     # monotone envelope
                        idx = torch.searchsorted(rc.contiguous(), self.REC_THRS.view(1, r).expand(t, r).contiguous(),
                                                 right=False)
                        q = torch.where(idx < nd, pr.gather(1, idx.clamp(max=nd - 1)), torch.zeros((t, r), dtype=torch.float64))
                    else:
                        q = torch.zeros((t, r), dtype=torch.float64)
                    precision[:, :, k, a, m] = q

        def ap(thr=None, area=0):
            s = precision[:, :, :, area, m_n - 1]
            if thr is not None:
                s = s[torch.isclose(self.IOU_THRS, torch.tensor(thr, dtype=torch.float64))]
            s = s[s > -1]
            return float(s.mean()) if s.numel() else -1.0

        def ar(mi, area=0):
            s = recall[:, :, area, mi]
            s = s[s > -1]
            return float(s.mean()) if s.numel() else -1.0

        return dict(map=ap(), map_50=ap(0.5), map_75=ap(0.75), map_small=ap(area=1), map_medium=ap(area=2),
                    map_large=ap(area=3), mar_1=ar(0), mar_10=ar(1), mar_100=ar(2), mar_small=ar(2, 1),
                    mar_medium=ar(2, 2), mar_large=ar(2, 3))


class DeviceMaskMeanAveragePrecision:
    """The metric of :class:`MaskMeanAveragePrecision` — same ``update`` / ``compute`` / ``reset``, same twelve keys — with
    the per-image work on the device: ``update`` takes the predicted masks at ground-truth resolution bit-packed from K21
    (``ops.extract_masks``), the pairwise popcounts from K29a and COCOeval.evaluateImg of every (image, class, area range,
    IoU threshold) from K29b, and keeps per detection its score, label, rank in its class and two 64-bit flag words
    (matched / ignored, bit ``area * T + threshold``) plus the counted ground truths per (class, area range): no dense
    mask, no IoU matrix, no host synchronisation.  ``compute`` is plain torch on the device the state lives on (CPU
    tensors work): one stable sort by score over the whole dataset, per class and detection limit f64 cumulative sums, the
    monotone envelope and a ``searchsorted`` at the 101 recall thresholds, then ONE host copy of the twelve numbers.
    Classes ``0 .. num_labels - 1`` are all evaluated; one without counted ground truths drops out of the means exactly as
    a label that never occurs does in the other class.  With ``torch.distributed`` initialised, ``compute`` gathers the
    states of all ranks first (``all_gather``: every rank must hold equally many images), so every rank returns the same
    numbers.  The ground truth may be dense (B, G, ny, nx) or :class:`ops.PackedMasks`.
    Checked against the plain-loop restatement in oracle/metrics_oracle.py; parity with torchmetrics / pycocotools
    themselves stays unpinned: neither is installed."""

    IOU_THRS = torch.from_numpy(np.linspace(0.5, 0.95, 10))          # the oracle's own f64 values: comparisons are bit-equal
    REC_THRS = torch.from_numpy(np.linspace(0.0, 1.0, 101))
    MAX_DETS = MaskMeanAveragePrecision.MAX_DETS
    AREAS = MaskMeanAveragePrecision.AREAS
    STATE = ('scores', 'labels', 'rank', 'matched', 'ignored', 'npig')

    def __init__(self, num_labels: Optional[int] = None):
        self.num_labels = num_labels            # update_metrics sets it from the class logits when None
        self.state: List[tuple] = []
        self._const = {}

    def reset(self):
        self.state = []

    def append_state(self, scores: torch.Tensor, labels: torch.Tensor, rank: torch.Tensor, matched: torch.Tensor,
                     ignored: torch.Tensor, npig: torch.Tensor):
        """The state of some images as K29b leaves it: ``scores`` (.., Q) float, ``labels`` / ``rank`` (.., Q) integer,
        ``matched`` / ``ignored`` (.., Q) int64 flag words, ``npig`` (.., num_labels, A) integer.  Tensors of any one device."""
        a = len(self.AREAS)
        if npig.dim() < 2 or npig.shape[-1] != a:
            raise ValueError(f'append_state: npig must be (.., num_labels, {a}), got {tuple(npig.shape)}')
        if not (scores.shape == labels.shape == rank.shape == matched.shape == ignored.shape):
            raise ValueError('append_state: scores, labels, rank, matched and ignored must have one shape')
        if self.num_labels is None:
            self.num_labels = int(npig.shape[-2])
        if int(npig.shape[-2]) != self.num_labels:
            raise ValueError(f'append_state: npig of {npig.shape[-2]} classes, {self.num_labels} expected')
        self.state.append((scores.detach().flatten(), labels.detach().flatten(), rank.detach().flatten(),
                           matched.detach().flatten().to(torch.int64), ignored.detach().flatten().to(torch.int64),
                           npig.detach().reshape(-1, self.num_labels, a)))

    def _constants(self, dev):
        if dev not in self._const:
            areas = torch.tensor([[lo, hi] for _, lo, hi in self.AREAS], dtype=torch.float64)
            self._const[dev] = (self.IOU_THRS.to(dev), areas.to(dev))
        return self._const[dev]

    @torch.no_grad()
    def update(self, pred_logits: torch.Tensor, scores: torch.Tensor, pred_labels: torch.Tensor, gt_masks, gt_labels: torch.Tensor):
        """One batch: ``pred_logits`` (B, Q, h, w) mask logits, ``scores`` / ``pred_labels`` (B, Q), ``gt_masks`` (B, G, ny, nx)
        {0, 1} or the B * G maps as :class:`ops.PackedMasks`, ``gt_labels`` (B, G).  K21, K29a, K29b; nothing is copied back."""
        if self.num_labels is None:
            raise MaskBevHipError('DeviceMaskMeanAveragePrecision: num_labels is not set')
        if not pred_logits.is_cuda:
            raise MaskBevHipError('DeviceMaskMeanAveragePrecision.update needs ROCm device tensors (no CPU fallback)')
        b, q = scores.shape
        gt = gt_masks if isinstance(gt_masks, ops.PackedMasks) else ops.pack_binary_masks(gt_masks.float().flatten(0, 1))
        dev = pred_logits.device
        scores = scores.float().contiguous()
        keep = torch.ones((b, q), dtype=torch.bool, device=dev)
        pred = ops.extract_masks(pred_logits.float(), scores, keep, (gt.h, gt.w), masks=True, instance_map=False)['masks']
        inter, pred_area, gt_area = ops.pairwise_mask_overlap(pred, gt, b)
        thrs, areas = self._constants(dev)
        labels = pred_labels.to(torch.int32)
        rank, matched, ignored, npig = ops.coco_match(inter, pred_area, gt_area, scores, labels,
                                                      gt_labels.to(torch.int32), self.num_labels, thrs, areas,
                                                      self.MAX_DETS[-1])
        self.append_state(scores, labels, rank, matched, ignored, npig)

    def _gathered_state(self):
        state = [torch.cat([s[i] for s in self.state]) for i in range(len(self.STATE))]
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            out = []
            for x in state:
                parts = [torch.empty_like(x) for _ in range(dist.get_world_size())]
                dist.all_gather(parts, x.contiguous())
                out.append(torch.cat(parts))
            state = out
        return state

    @torch.no_grad()
    def compute(self) -> dict:
        keys = ('map', 'map_50', 'map_75', 'map_small', 'map_medium', 'map_large', 'mar_1', 'mar_10', 'mar_100',
                'mar_small', 'mar_medium', 'mar_large')
        if not self.state:
            return {k: -1.0 for k in keys}
        scores, labels, rank, matched, ignored, npig = self._gathered_state()
        dev = scores.device
        t_n, r_n, a_n, m_n, l_n = len(self.IOU_THRS), len(self.REC_THRS), len(self.AREAS), len(self.MAX_DETS), self.num_labels
        n_det = scores.numel()
        npig = npig.sum(0).double()                                                       # (L, A)
        precision = -torch.ones((t_n, r_n, l_n, a_n, m_n), dtype=torch.float64, device=dev)
        recall = -torch.ones((t_n, l_n, a_n, m_n), dtype=torch.float64, device=dev)
        if n_det > 0:
            # ONE stable sort by score for the whole dataset; a (class, detection limit) selection is a mask in that order: a
            # masked-out detection adds nothing to the cumulative sums, so it repeats the values of the selected one before it
            # (or the zeros in front of the first) and moves neither the envelope nor the first position that reaches a recall
            order = torch.sort(-scores.double(), stable=True).indices
            labels, rank = labels[order], rank[order]
            shifts = torch.arange(a_n * t_n, device=dev, dtype=torch.int64)
            dtm = ((matched[order].view(-1, 1) >> shifts) & 1).bool()                      # (D, A * T)
            counted = ((ignored[order].view(-1, 1) >> shifts) & 1) == 0
            tp_flag, fp_flag = dtm & counted, ~dtm & counted
            eps = torch.finfo(torch.float64).eps
            rec_thrs = self.REC_THRS.to(dev).view(1, r_n).expand(a_n * t_n, r_n).contiguous()
            for c in range(l_n):
                in_class = labels == c
                denom = npig[c].repeat_interleave(t_n).view(-1, 1)                         # (A * T, 1)
                valid = (denom > 0).view(a_n, t_n)
                for m, max_det in enumerate(self.MAX_DETS):
                    sel = (in_class & (rank < max_det)).view(-1, 1)
                    tp = torch.cumsum((tp_flag & sel).double(), 0).t().contiguous()          # (A * T, D)
                    fp = torch.cumsum((fp_flag & sel).double(), 0).t().contiguous()
                    rc = tp / denom
                    pr = tp / (fp + tp + eps)
                    pr = torch.flip(torch.cummax(torch.flip(pr, (1,)), 1).values, (1,))     # monotone envelope
                    idx = torch.searchsorted(rc, rec_thrs, right=False)
                    q = torch.where(idx < n_det, pr.gather(1, idx.clamp(max=n_det - 1)), torch.zeros_like(rec_thrs))
                    q = torch.where(valid.view(a_n, t_n, 1), q.view(a_n, t_n, r_n), -torch.ones_like(q).view(a_n, t_n, r_n))
                    precision[:, :, c, :, m] = q.permute(1, 2, 0)
                    recall[:, c, :, m] = torch.where(valid, rc[:, -1].view(a_n, t_n), -torch.ones_like(valid, dtype=torch.float64)).t()
        else:
            has = (npig > 0).view(1, l_n, a_n, 1)
            precision = torch.where(has.view(1, 1, l_n, a_n, 1), torch.zeros_like(precision), precision)
            recall = torch.where(has, torch.zeros_like(recall), recall)

        def mean(s):
            ok = s > -1
            cnt = ok.sum()
            return torch.where(cnt > 0, torch.where(ok, s, torch.zeros_like(s)).sum() / cnt.clamp(min=1), -torch.ones((), dtype=torch.float64, device=dev))

        t50 = int(np.nonzero(np.isclose(self.IOU_THRS.numpy(), 0.5))[0][0])
        t75 = int(np.nonzero(np.isclose(self.IOU_THRS.numpy(), 0.75))[0][0])
        last = m_n - 1
        out = torch.stack([mean(precision[:, :, :, 0, last]), mean(precision[t50, :, :, 0, last]),
                           mean(precision[t75, :, :, 0, last]), mean(precision[:, :, :, 1, last]),
                           mean(precision[:, :, :, 2, last]), mean(precision[:, :, :, 3, last]),
                           mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, 2]),
                           mean(recall[:, :, 1, last]), mean(recall[:, :, 2, last]), mean(recall[:, :, 3, last])]).cpu().tolist()
        return dict(zip(keys, out))


def semantic_kitti_class_lut(things=((10,),), ignore=(0, 1, 252), length: int = 260) -> np.ndarray:
    """The ``class_lut`` of :class:`DevicePanopticQuality` for raw SemanticKITTI semantic ids: an int32 table of ``length``
    entries in which the ids of the k-th tuple of ``things`` map to class k + 1, the ids of ``ignore`` to -1 and every other
    id to 0 ("everything else").  The default scores static cars: raw label 10 is class 1, as the reference trains on that
    label alone (semantic_kitti_mask_data_module.py:56); unlabelled (0), outlier (1) and MOVING cars (252) are ignored, so
    a moving car is neither rewarded nor penalised — its points take part in nothing, whatever was predicted on them."""
    lut = np.zeros((int(length),), dtype=np.int32)
    for k, ids in enumerate(things):
        for i in ids:
            if not 0 <= int(i) < length:
                raise ValueError(f'semantic_kitti_class_lut: semantic id {i} outside the table of {length}')
            lut[int(i)] = k + 1
    for i in ignore:
        if not 0 <= int(i) < length:
            raise ValueError(f'semantic_kitti_class_lut: semantic id {i} outside the table of {length}')
        lut[int(i)] = -1
    return lut


def panoptic_quality(tp, fp, fn, iou_sum, confusion) -> dict:
    """The numbers of ``PanopticEval.getPQ`` / ``getSemIoU`` (semantic-kitti-api, eval_np.py) from the sums of a dataset:
    ``tp``, ``fp``, ``fn``, ``iou_sum`` (C) per class (class 0 is not scored: zeros), ``confusion`` (C, C) [gt][prediction].
    Per class ``pq = iou_sum / max(tp + 0.5 fp + 0.5 fn, 1e-15)``, ``sq = iou_sum / max(tp, 1e-15)``, ``rq = tp / max(tp +
    0.5 fp + 0.5 fn, 1e-15)`` and ``iou = confusion[c][c] / max(row + column - confusion[c][c], 1e-15)`` →
    ``{'pq', 'sq', 'rq', 'iou'}`` the means over the thing classes 1 .. C-1, ``'per_class'`` the lists of all C classes under
    the same four names plus the raw ``tp``, ``fp``, ``fn``."""
    tp, fp, fn = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (tp, fp, fn))
    iou_sum, conf = np.asarray(iou_sum, dtype=np.float64).reshape(-1), np.asarray(confusion, dtype=np.float64)
    c = tp.shape[0]
    eps = 1e-15
    denom = np.maximum(tp + 0.5 * fp + 0.5 * fn, eps)
    pq, sq, rq = iou_sum / denom, iou_sum / np.maximum(tp, eps), tp / denom
    inter = np.diag(conf)
    iou = inter / np.maximum(conf.sum(1) + conf.sum(0) - inter, eps)
    things = slice(1, c)

    def mean(x):
        return float(x[things].mean()) if c > 1 else 0.0

    per_class = dict(pq=pq.tolist(), sq=sq.tolist(), rq=rq.tolist(), iou=iou.tolist(), tp=[int(v) for v in tp],
                     fp=[int(v) for v in fp], fn=[int(v) for v in fn])
    return dict(pq=mean(pq), sq=mean(sq), rq=mean(rq), iou=mean(iou), per_class=per_class)


class _ClassTable:
    """What the point metrics share: ``num_classes`` (2 .. 16) and ``class_lut``, the int32 table semantic id → class, given
    as a numpy array or a tensor, kept on the host and handed out per device."""

    def __init__(self, num_classes: int, class_lut):
        self.num_classes = int(num_classes)
        if not 2 <= self.num_classes <= 16:
            raise ValueError(f'{type(self).__name__}: 2 <= num_classes <= 16, got {num_classes}')
        lut = class_lut.detach().cpu().numpy() if torch.is_tensor(class_lut) else np.asarray(class_lut)
        self._lut_host = np.ascontiguousarray(lut.reshape(-1).astype(np.int32))
        self._lut = {}

    def class_lut(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device not in self._lut:
            self._lut[device] = torch.from_numpy(self._lut_host).to(device)
        return self._lut[device]


class DevicePanopticQuality(_ClassTable):
    """PQ / SQ / RQ and IoU of point or BEV instances in the SemanticKITTI panoptic protocol (``PanopticEval`` of
    semantic-kitti-api's eval_np.py, restated; parity with that package is unpinned: it is not installed), with the per-frame
    work on the device (K32, ``ops.panoptic_frames``).  ``class_lut``: semantic id → class, -1 = ignored
    (:func:`semantic_kitti_class_lut`), a numpy array or a tensor; classes 1 .. ``num_classes`` - 1 are the thing classes.
    ``update`` adds the frames' tp / fp / fn, IoU sums and confusion into running device tensors without a host copy;
    ``compute`` sums the ranks (``all_reduce`` when ``torch.distributed`` is initialised), makes ONE host copy and returns
    :func:`panoptic_quality` of the sums plus ``frames``.  It raises ``MaskBevHipError`` if any frame held more than ``max_gt``
    ground-truth segments: such a frame has no numbers."""

    def __init__(self, num_classes: int, class_lut, min_points: int = 50, max_gt: int = 256):
        super().__init__(num_classes, class_lut)
        self.min_points, self.max_gt = int(min_points), int(max_gt)
        self.reset()

    def reset(self):
        self.state = None
        self.frames = 0

    @torch.no_grad()
    def update(self, pred_query: torch.Tensor, query_class: torch.Tensor, gt_words: torch.Tensor, lengths) -> 'ops.PanopticFrames':
        """One batch of F frames: ``pred_query`` (N) int32, ``query_class`` (F, P) int32, ``gt_words`` (N) int32 / uint32,
        ``lengths`` the frames' element counts (host) or (F + 1) int32 device offsets — the arguments of
        ``ops.panoptic_frames``.  Returns the frames' record; nothing is copied back."""
        out = ops.panoptic_frames(pred_query, gt_words, lengths, query_class, self.class_lut(pred_query.device),
                                  self.num_classes, max_gt=self.max_gt, min_points=self.min_points)
        self.append_state(out.frame_stats, out.frame_iou, out.confusion, out.n_gt)
        return out

    @torch.no_grad()
    def append_state(self, frame_stats: torch.Tensor, frame_iou: torch.Tensor, confusion: torch.Tensor, n_gt: torch.Tensor):
        """The records of some frames as K32 leaves them (tensors of any one device)."""
        c = self.num_classes
        if tuple(frame_stats.shape[1:]) != (c, 3) or tuple(frame_iou.shape[1:]) != (c,) or tuple(confusion.shape[1:]) != (c, c):
            raise ValueError(f'append_state: records of {c} classes expected')
        part = (frame_stats.to(torch.int64).sum(0), frame_iou.to(torch.float64).sum(0), confusion.to(torch.int64).sum(0),
                (n_gt > self.max_gt).to(torch.int64).sum().view(1))
        self.state = part if self.state is None else tuple(a + b for a, b in zip(self.state, part))
        self.frames += int(frame_stats.shape[0])

    @torch.no_grad()
    def compute(self, reduce: bool = True) -> dict:
        """``reduce=False``: the numbers of this rank alone, without a collective (the other ranks need not call)."""
        c = self.num_classes
        import torch.distributed as dist
        gather = reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if self.state is None and not gather:
            return dict(panoptic_quality(np.zeros(c), np.zeros(c), np.zeros(c), np.zeros(c), np.zeros((c, c))), frames=0)
        if self.state is None:
            dev = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
            stats, iou, conf, over = (torch.zeros((c, 3), dtype=torch.int64, device=dev), torch.zeros((c,), dtype=torch.float64, device=dev),
                                      torch.zeros((c, c), dtype=torch.int64, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev))
        else:
            stats, iou, conf, over = self.state
        counts = torch.cat([stats.reshape(-1), conf.reshape(-1), over, torch.tensor([self.frames], dtype=torch.int64, device=over.device)])
        if gather:                                         # sums over the ranks; the f64 sums in rank order, on every rank alike
            dist.all_reduce(counts)
            parts = [torch.empty_like(iou) for _ in range(dist.get_world_size())]
            dist.all_gather(parts, iou.contiguous())
            iou = torch.stack(parts).sum(0)
        host = torch.cat([counts, iou.contiguous().view(torch.int64)]).cpu()          # the ONE host copy: f64 bits ride as int64
        stats = host[:3 * c].view(c, 3).numpy()
        conf = host[3 * c:3 * c + c * c].view(c, c).numpy()
        over, frames = int(host[3 * c + c * c]), int(host[3 * c + c * c + 1])
        iou_sum = host[3 * c + c * c + 2:].contiguous().view(torch.float64).numpy()
        if over > 0:
            raise MaskBevHipError(f'DevicePanopticQuality: {over} of {frames} frames hold more than max_gt = {self.max_gt} '
                                  'ground-truth segments and have no numbers; raise max_gt (<= 1024)')
        return dict(panoptic_quality(stats[:, 0], stats[:, 1], stats[:, 2], iou_sum, conf), frames=frames)


def lstq(s_assoc: float, s_cls: float) -> float:
    """LSTQ = sqrt(S_assoc * S_cls) (Aygün et al., 4D Panoptic LiDAR Segmentation)."""
    return float(np.sqrt(float(s_assoc) * float(s_cls)))


class DeviceTubeAssociation(_ClassTable):
    """S_assoc, the association term of LSTQ, over a whole sequence, with the tables on the device (K33b,
    ``ops.tube_accumulate`` / ``ops.tube_scores``).  A ground-truth tube is a (thing class, instance id) pair over all frames
    fed since :meth:`reset`, a predicted tube a global track id (``Predictions.point_tracks``); a tube's score is ``(1 / |gt|)
    * sum over the overlapping tracks of TPA * TPA / (|gt| + |track| - TPA)`` and S_assoc the mean over the tubes.
    ``class_lut`` as in :class:`DevicePanopticQuality`; instance ids must stay below ``id_limit`` and track ids below
    ``max_tracks`` — elements past either are counted and :meth:`compute` raises.  Feed ONE sequence, or give the tracks of
    different sequences different ids: SemanticKITTI's instance ids are unique per sequence only.

    This is LSTQ RESTRICTED TO THE THING CLASSES THE MODEL PREDICTS: with ``s_cls`` the ``iou`` of a
    :class:`DevicePanopticQuality` over the same frames, :func:`lstq` gives ``sqrt(S_assoc * S_cls)`` of those classes, not
    the benchmark's number over all 19.  Parity with semantic-kitti-api's 4D evaluator is not pinned (it is not installed).
    ``update`` synchronises nothing; ``compute`` makes one host copy.  Ranks are not summed: a sequence is tracked on one rank.
    Tables that live on the host (``tables=`` a record copied back) are scored by the same formula in numpy."""

    def __init__(self, num_classes: int, class_lut, id_limit: int = 1024, max_tracks: int = 4096, tables=None):
        super().__init__(num_classes, class_lut)
        self.id_limit, self.max_tracks, self.tables = int(id_limit), int(max_tracks), tables

    def reset(self):
        self.tables = None

    @torch.no_grad()
    def update(self, point_tracks: torch.Tensor, gt_words: torch.Tensor) -> None:
        """``point_tracks`` (N) int32 global track ids (-1 = none) and ``gt_words`` (N) int32 / uint32 ``.label`` words of the
        same elements, on the device.  Nothing is copied back."""
        if self.tables is None:
            self.tables = ops.TubeTables.zeros(self.num_classes, self.id_limit, self.max_tracks, point_tracks.device)
        ops.tube_accumulate(point_tracks, gt_words, self.class_lut(point_tracks.device), self.tables)

    @torch.no_grad()
    def compute(self) -> dict:
        """``{'s_assoc', 'tubes', 'per_class', 'overflow'}``: the mean over the ground-truth tubes of the thing classes, their
        number, per class ``{'s_assoc', 'tubes'}`` lists of all C classes, and the two overflow counters (zeros).  Raises
        ``MaskBevHipError`` when an overflow counter is not zero: the tables then miss elements."""
        c = self.num_classes
        if self.tables is None:
            class_assoc, class_tubes, over = np.zeros(c), np.zeros(c, dtype=np.int64), np.zeros(2, dtype=np.int64)
        elif self.tables.pair.is_cuda:
            s = ops.tube_scores(self.tables)
            host = torch.cat([s.class_assoc.view(torch.int64), s.class_tubes.to(torch.int64), self.tables.overflow]).cpu()
            class_assoc = host[:c].contiguous().view(torch.float64).numpy()
            class_tubes, over = host[c:2 * c].numpy(), host[2 * c:].numpy()
        else:
            gt, ps = self.tables.gt_size.numpy().astype(np.float64), self.tables.pred_size.numpy().astype(np.float64)
            pair = self.tables.pair.numpy().astype(np.float64)
            with np.errstate(all='ignore'):
                terms = np.where(pair > 0, pair * (pair / (gt[:, None] + ps[None, :] - pair)), 0.0)
                assoc = np.where(gt > 0, terms.sum(1) / np.maximum(gt, 1.0), 0.0).reshape(c - 1, self.id_limit)
            class_assoc = np.concatenate([[0.0], assoc.sum(1)])
            class_tubes = np.concatenate([[0], (gt > 0).reshape(c - 1, self.id_limit).sum(1)]).astype(np.int64)
            over = self.tables.overflow.numpy()
        if int(over[0]) or int(over[1]):
            raise MaskBevHipError(f'DeviceTubeAssociation: {int(over[0])} elements carry an instance id >= id_limit = '
                                  f'{self.id_limit} and {int(over[1])} a track id >= max_tracks = {self.max_tracks}; raise the limits')
        tubes = int(class_tubes[1:].sum())
        per_class = dict(s_assoc=[float(a) / max(int(n), 1) for a, n in zip(class_assoc, class_tubes)],
                         tubes=[int(n) for n in class_tubes])
        return dict(s_assoc=float(class_assoc[1:].sum()) / max(tubes, 1), tubes=tubes, per_class=per_class,
                    overflow=[int(over[0]), int(over[1])])


@torch.no_grad()
def update_metrics(head, layer_index: int, pred_cls, pred_masks, labels_gt: torch.Tensor, masks_gt,
                   cls_metric: Optional[BinaryClassifScores], miou_metric: Optional[MeanIoU],
                   map_metric=None):
    """``MaskBevPanopticHead.update_mAP_metrics`` for the classification and mIoU metrics, batched over the images and
    reusing the assignment of the loss that was just evaluated on the same predictions (``head`` is the
    ``Mask2FormerHead``; call after ``compute_loss``).  ``pred_cls`` / ``pred_masks``: the per-layer output lists."""
    if head.last_assignment is None:
        raise MaskBevHipError('update_metrics: evaluate the loss first (it provides the assignment)')
    assigned = head.last_assignment[layer_index]                                 # (B, Q)
    cls = pred_cls[layer_index]
    b, q = cls.shape[:2]
    safe = assigned.clamp(min=0).long()
    labels = torch.where(assigned >= 0, torch.gather(labels_gt, 1, safe), torch.full_like(safe, head.num_classes))
    if cls_metric is not None:
        cls_metric.update(cls.float().softmax(-1)[..., 0], labels)               # evaluated_class = 0 (:66-71)
    if miou_metric is not None:
        gt = head.last_gt_packed
        if gt is None:
            gt = masks_gt if isinstance(masks_gt, ops.PackedMasks) else ops.pack_binary_masks(
                masks_gt.float().flatten(0, 1))
        miou_metric.update(matched_mask_iou(pred_masks[layer_index], assigned, gt))
    if map_metric is not None:                            # mask_bev_panoptic_head.py:87-96
        sm = cls.float().softmax(-1)
        if isinstance(map_metric, DeviceMaskMeanAveragePrecision):
            if map_metric.num_labels is None:
                map_metric.num_labels = int(cls.shape[-1])
            gt = head.last_gt_packed if head.last_gt_packed is not None else masks_gt
        elif isinstance(masks_gt, ops.PackedMasks):
            raise MaskBevHipError('the mask-mAP metric needs the dense (B, G, ny, nx) ground-truth masks')
        else:
            gt = masks_gt
        map_metric.update(pred_masks[layer_index], sm[..., 0], cls.argmax(-1), gt, labels_gt)
