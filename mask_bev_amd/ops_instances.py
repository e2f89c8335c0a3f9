"""K21 — instance extraction at inference (csrc/instances.hip): query selection from the class logits and the BEV masks,
areas, mask scores and instance map of one decoder output, straight from the (h, w) logits with no (B, Q, H, W)
intermediate.  Class convention: index 0 = empty, > 0 = object; a pixel is set when its interpolated
logit is > 0 (sigmoid > 0.5)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import MaskBevHipError, check
from .ops_core import _dt_flag, _need_gpu, _ptr, _stream, _workspace
from .ops_loss import PackedMasks


@torch.no_grad()
def select_queries(cls: torch.Tensor, score_threshold: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """cls (B, Q, K+1) f32 / bf16 / fp16, K+1 <= 256 → labels (B, Q) int32 (first argmax), scores (B, Q) f32
    (softmax[label]), keep (B, Q) bool (label > 0 and score >= score_threshold).  One K21a launch."""
    lib = _lib.load()
    _need_gpu(cls)
    if cls.dim() != 3:
        raise MaskBevHipError(f'select_queries: cls must be (B, Q, K+1), got {tuple(cls.shape)}')
    b, q, k = cls.shape
    if not 0 < k <= 256:
        raise MaskBevHipError(f'select_queries: 1 <= K+1 <= 256 classes, got {k}')
    cls = cls.contiguous()
    dev = cls.device
    labels = torch.empty((b, q), dtype=torch.int32, device=dev)
    scores = torch.empty((b, q), dtype=torch.float32, device=dev)
    keep = torch.empty((b, q), dtype=torch.bool, device=dev)
    check(lib.mbv_select_queries(_ptr(cls), _dt_flag(cls.dtype), b * q, k, float(score_threshold), _ptr(labels),
                                 _ptr(scores), _ptr(keep), _stream()), 'mbv_select_queries')
    return labels, scores, keep


@torch.no_grad()
def extract_masks(logits: torch.Tensor, scores: torch.Tensor, keep: torch.Tensor, grid_hw, masks: bool = True,
                  instance_map: bool = True) -> Dict[str, Optional[object]]:
    """logits (B, Q, h, w) f32, scores (B, Q) f32 and keep (B, Q) bool of :func:`select_queries` → a dict with
    ``masks`` (:class:`PackedMasks` of the B*Q maps at grid_hw = (H, W)), ``areas`` (B, Q) int32, ``mask_scores`` (B, Q)
    f32 (mean sigmoid over the set pixels, 0 when empty) — all three None when ``masks`` is False — and ``instance_map``
    (B, H, W) int32 (best kept query by score * sigmoid, -1 for none; None when ``instance_map`` is False).  K21b + its
    fixed-order reduction; deterministic."""
    lib = _lib.load()
    _need_gpu(logits, scores, keep)
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise MaskBevHipError(f'extract_masks: logits must be (B, Q, h, w) f32, got {tuple(logits.shape)} {logits.dtype}')
    b, q, h, w = logits.shape
    H, W = int(grid_hw[0]), int(grid_hw[1])
    if H <= 0 or W <= 0 or H * W > 1024 * 1024:
        raise MaskBevHipError(f'extract_masks: BEV grid {H}x{W} outside 1 <= H*W <= 1024*1024')
    if (tuple(scores.shape) != (b, q) or scores.dtype != torch.float32 or tuple(keep.shape) != (b, q)
            or keep.dtype != torch.bool):
        raise MaskBevHipError('extract_masks: scores must be (B, Q) f32 and keep (B, Q) bool')
    if not (scores.device == keep.device == logits.device):
        raise MaskBevHipError('extract_masks: tensors on different devices')
    dev = logits.device
    logits, scores, keep = logits.contiguous(), scores.contiguous(), keep.contiguous()
    words = torch.empty((b * q, lib.mbv_packed_mask_words(H, W)), dtype=torch.int32, device=dev) if masks else None
    areas = torch.empty((b, q), dtype=torch.int32, device=dev) if masks else None
    mscores = torch.empty((b, q), dtype=torch.float32, device=dev) if masks else None
    imap = torch.empty((b, H, W), dtype=torch.int32, device=dev) if instance_map else None
    ws = None
    nbytes = 0
    if masks and b * q > 0:
        nbytes = lib.mbv_extract_masks_workspace_bytes(b, q, h, w, H, W)
        if nbytes == 0:
            raise MaskBevHipError(f'extract_masks: {h}x{w} logits on a {H}x{W} grid are not supported')
        ws = _workspace(nbytes, dev)
    check(lib.mbv_extract_masks(_ptr(logits), _ptr(scores), _ptr(keep), b, q, h, w, H, W, _ptr(words), _ptr(areas),
                                _ptr(mscores), _ptr(imap), _ptr(ws), nbytes if ws is not None else 0, _stream()),
          'mbv_extract_masks')
    return dict(masks=PackedMasks(words, H, W) if masks else None, areas=areas, mask_scores=mscores, instance_map=imap)


__all__ = ['select_queries', 'extract_masks']
