"""Torch-facing wrappers of the C-ABI kernels (``include/maskbev_hip.h``) — the ONE name the rest of the package uses.

PyTorch is plumbing here: it owns device memory, the stream and the autograd graph; every wrapper enqueues hand-written
gfx950 kernels on ``torch.cuda.current_stream()`` through ctypes.  There is no CPU fallback — tensors must live on a ROCm
device.  The wrappers live in one module per kernel family; this facade re-exports them (callers write ``ops.linear``,
tests patch ``ops.mask_logits`` / ``ops.hungarian`` here):

    ops_core       pointers, stream, dtype flags, the HIP-event timer, workspaces
    ops_records    fp32 mode: absmax records — pools, hints, static / weight / LayerNorm-bound registries, amax_verify
    ops_gemm_kernels, ops_pgrad, ops_gemm   K17 / K20 GEMM launches and who takes one; in-place arena parameter gradients
                   and their deferred / grouped queues; the autograd nodes on both: patch projection, 3 x 3 conv, Linear, FFN
    ops_encoder    K1 voxelise, K2 PillarFeatureNet, K3 scatter + LayerNorm
    ops_attention  K4 window attention, K6 decoder attention (+ shared K / V), K7 mask logits
    ops_msda       K5 / K16 multi-scale deformable attention
    ops_norm       K12 add + LayerNorm, bias + activation, K18 GroupNorm, patch merging
    ops_loss       K8 point sampling, K9 Hungarian, K10 importance sampling, K13 loss rows / costs
    ops_instances  K21 query selection + BEV mask / instance-map extraction at inference; K31 lift of the instance map to
                   the points (per-point labels, points and z-extent per query); K35 ground height per BEV cell and the
                   lift restricted to the returns above it; K38a BEV visibility map of a scan (PASSED / HIT / unknown);
                   K42 the kept queries reconciled with each other: self-overlap of the kept masks, greedy mask NMS, overlap filter
    ops_rasterize  K22 SemanticKITTI scene -> instance-id map (binning, close + open, paint)
    ops_augment    K23 training augmentations: per-point op program, compaction / sort, instance-map warp;
                   K28 KITTI object augmentations: box-table membership, move, removal and pasting of points
    ops_eval       K25 oriented box of a packed mask, K26 / K26b rotated-box overlap (BEV / 3-D) over ragged frames, K27 KITTI tp / fp / fn,
                   K29 pairwise overlap of packed masks + COCO per-image matching (mask mAP),
                   K30 largest 8-connected component + minimum-area rectangle of a packed mask,
                   K32 panoptic tp / fp / fn, IoU sums and confusion per frame from two id arrays (points or BEV cells)
    ops_track      K33 the tracker step over consecutive BEV instance maps (global instance ids) and tube association (S_assoc of LSTQ);
                   K37 the same step with a constant-velocity motion model and gated re-association;
                   K38b the same step with occlusion-aware ageing from K38a's maps;
                   K39 tracked footprints fused over time in a rolling world grid, and a query map back to packed masks
    ops_render     K36 returns per BEV cell and the composed BEV frame (density, instances / tracks, ground-truth contour, boxes)
"""
from .ops_core import *            # noqa: F401,F403
from .ops_records import *         # noqa: F401,F403
from .ops_gemm_kernels import *    # noqa: F401,F403
from .ops_pgrad import *           # noqa: F401,F403
from .ops_gemm import *            # noqa: F401,F403
from .ops_encoder import *         # noqa: F401,F403
from .ops_attention import *       # noqa: F401,F403
from .ops_msda import *            # noqa: F401,F403
from .ops_norm import *            # noqa: F401,F403
from .ops_loss import *            # noqa: F401,F403
from .ops_instances import *       # noqa: F401,F403
from .ops_rasterize import *       # noqa: F401,F403
from .ops_augment import *         # noqa: F401,F403
from .ops_eval import *            # noqa: F401,F403
from .ops_track import *           # noqa: F401,F403
from .ops_render import *          # noqa: F401,F403
