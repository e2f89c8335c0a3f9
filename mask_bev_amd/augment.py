"""Training augmentations of SemanticKITTI, KITTI and Waymo samples on the device (K23, csrc/augment.hip): the reference's
``mask_bev/augmentations/semantic_kitti_mask_augmentations.py``, ``kitti_mask_augmentations.py`` and
``waymo_mask_augmentations.py`` — same names, same keyword arguments, same magnitude rules — with the per-sample decisions (which transform fires, the angle, one 64-bit seed) drawn on the host from a seeded
generator and everything per point or per cell done by three kernels.

    aug = DeviceAugmentation(make_semantic_kitti_augmentation_list(config['augmentations']), seed=420,
                             x_range=..., y_range=..., voxel_size=...)
    aug.reseed(seed, rank, epoch, batch_index)
    out = aug.apply(scans, instance_maps=maps)            # cached maps: warped by K23c
    out = aug.apply(scans, scene_transforms=[tf, ...])    # scenes: diag(A, 1, 1) @ tf, rasterised afterwards (K22)
    out = aug.apply(scans, boxes=[(n, 7) f64, ...])       # box tables: moved on the host, rasterised afterwards (K24)

Boxes [cx, cy, cz, l, w, h, theta] follow the points: a linear op acts on the centre; theta changes as the reference changes
``rotation_y`` / ``heading`` — a rotation adds its angle, the KITTI y-flip negates it, the Waymo y-flip LEAVES the heading
as it is (waymo_mask_augmentations.py:54-59 mirrors ``center_y`` only; restated, not repaired); ``global_noise`` scales
centre and dimensions and shifts the centre.  ``object_sample`` (needs the dataset's ``samples.pkl``) and ``object_noise``
(mmdet3d's numba collision search) are not provided by the three list factories here and raise ``NotImplementedError``;
``object_augment.make_kitti_object_augmentation_list`` builds the KITTI list with both (K28): their object stage runs in
``apply`` before the point program, which then returns an ``ObjectAugmentedBatch``: its ``boxes`` hold the pasted and
perturbed boxes too.

Differences from the reference: a rotated map turns about the origin's cell, not about OpenCV's
(sx / 2, sy / 2) pixel; flips mirror about the origin also on an asymmetric range; a shuffle orders points by a 26-bit hash
with ties in input order; all drops of a list act before its decimates; ``cut_pc`` (a dead path there) is not implemented.
"""
from __future__ import annotations

import copy
import math
import numbers
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops_augment
from ._lib import MaskBevHipError

MAX_OPS = 8
OP_LINEAR, OP_JITTER, OP_DROP, OP_SHUFFLE, OP_DECIMATE, OP_GLOBAL_NOISE = 1, 2, 3, 4, 5, 6

# one scan's record as the kernels read it (include/maskbev_hip.h, K23): 656 bytes
OP_DTYPE = np.dtype([('code', '<i4'), ('arg', '<u4'), ('p', '<f8', (9,))])
RECORD_DTYPE = np.dtype([('seed_lo', '<u4'), ('seed_hi', '<u4'), ('n_ops', '<i4'), ('flags', '<i4'), ('ops', OP_DTYPE, (MAX_OPS,))])
assert RECORD_DTYPE.itemsize == ops_augment.AUGMENT_RECORD_BYTES


class Op(NamedTuple):
    code: int
    arg: int = 0
    p: Tuple[float, ...] = ()


class LinearOp(Op):
    """A linear ``Op`` — the same 3-tuple to records, comparisons and unpacking — that also says, on the host only, what it
    does to a box's theta: theta' = heading[0] * theta + heading[1] (a rotation: (1, angle); a mirror: (-1, 0) or (-1, pi);
    the Waymo y-flip: (1, 0)).  A plain linear ``Op`` turns theta with the mapped direction vector."""
    heading: Tuple[float, float] = (1., 0.)


def linear_op(p, heading) -> LinearOp:
    op = LinearOp(OP_LINEAR, 0, tuple(p))
    op.heading = (float(heading[0]), float(heading[1]))
    return op


def drop_threshold(p: float) -> int:
    """T of the drop rule ``kept iff (h >> 8) >= T``: ceil(p * 2^24), 0 for p <= 0 (all kept), 2^24 for p >= 1 (none)."""
    if not p > 0:
        return 0
    return min(int(math.ceil(p * (1 << 24))), 1 << 24)


# ---------------------------------------------------------------------------------------------------------
# the transforms: constructor = the reference's keywords; draw(rng, magnitude) = the ops of one sample
# ---------------------------------------------------------------------------------------------------------
class Flip:
    def __init__(self, prob_flip_x: float = 0.5, prob_flip_y: float = 0.5):
        self._prob_flip_x, self._prob_flip_y = prob_flip_x, prob_flip_y

    def draw(self, rng: np.random.Generator, magnitude: float = 1) -> List[Op]:
        ops = []
        if rng.uniform(0, 1) < self._prob_flip_x * magnitude:
            ops.append(linear_op((-1., 0., 0., 1.), (-1., math.pi)))
        if rng.uniform(0, 1) < self._prob_flip_y * magnitude:
            ops.append(linear_op((1., 0., 0., -1.), self._heading_flip_y))
        return ops

    _heading_flip_y = (-1., 0.)


class KittiFlip(Flip):
    """kitti_mask_augmentations.py:55-71: y only; ``rotation_y`` is negated.  One uniform is drawn."""

    def __init__(self, prob_flip_x: float = 0, prob_flip_y: float = 0.5):
        if prob_flip_x != 0:
            raise ValueError('Cannot flip in x')
        super().__init__(0, prob_flip_y)

    def draw(self, rng, magnitude: float = 1) -> List[Op]:
        if rng.uniform(0, 1) < self._prob_flip_y * magnitude:
            return [linear_op((1., 0., 0., -1.), self._heading_flip_y)]
        return []


class WaymoFlip(Flip):
    """waymo_mask_augmentations.py:38-59: y only, two uniforms drawn (the first decides nothing), ``center_y`` mirrored and
    the heading left as it is."""
    _heading_flip_y = (1., 0.)

    def __init__(self, prob_flip_x: float = 0, prob_flip_y: float = 0.5):
        if prob_flip_x != 0:
            raise ValueError('Cannot flip in x')
        super().__init__(0, prob_flip_y)


class ShufflePoints:
    def __init__(self, prob_shuffle: float = 0.5):
        self._prob_shuffle = prob_shuffle

    def draw(self, rng, magnitude: float = 1) -> List[Op]:
        return [Op(OP_SHUFFLE)] if rng.uniform(0, 1) < self._prob_shuffle * magnitude else []


class RandomRotate:
    def __init__(self, rotate_prob: float, rotation_range: Union[float, Tuple[float, float]]):
        self._rotate_prob = rotate_prob
        if isinstance(rotation_range, numbers.Number):
            rotation_range = (-rotation_range, rotation_range)
        self._rotation_range = tuple(rotation_range)

    def draw(self, rng, magnitude: float = 1) -> List[Op]:
        if not rng.uniform(0, 1) < self._rotate_prob:
            return []
        theta = rng.uniform(self._rotation_range[0] * magnitude, self._rotation_range[1] * magnitude)
        return [rotation_op(theta)]


def rotation_op(theta_deg: float) -> Op:
    c, s = float(np.cos(np.deg2rad(theta_deg))), float(np.sin(np.deg2rad(theta_deg)))
    return linear_op((c, -s, s, c), (1., float(np.deg2rad(theta_deg))))


class DecimatePoints:
    def __init__(self, prob_decimate: float, keep_every: int):
        self._prob_decimate, self._keep_every = prob_decimate, keep_every
        self._step(1)

    def _step(self, magnitude) -> int:
        k = int(self._keep_every * magnitude)
        if k < 1:
            raise ValueError(f'decimate: int(keep_every * magnitude) = {k}, must be at least 1')
        return k

    def draw(self, rng, magnitude: float = 1) -> List[Op]:
        k = self._step(magnitude)
        return [Op(OP_DECIMATE, k)] if rng.uniform(0, 1) < self._prob_decimate else []


class JitterPoints:
    def __init__(self, prob_jitter: float, jitter_std: Union[float, Tuple[float, float, float]],
                 max_delta: Optional[Union[float, Tuple[float, float, float]]] = None, intensity_std: float = 0.0,
                 intensity_max_delta: Optional[float] = None):
        self._prob_jitter = prob_jitter
        if isinstance(jitter_std, numbers.Number):
            jitter_std = (jitter_std, jitter_std, jitter_std)
        if isinstance(max_delta, numbers.Number):
            max_delta = (max_delta, max_delta, max_delta)
        self._jitter_std, self._max_delta = tuple(jitter_std), None if max_delta is None else tuple(max_delta)
        self._intensity_std, self._intensity_max_delta = intensity_std, intensity_max_delta

    def draw(self, rng, magnitude: float = 1) -> List[Op]:
        if not rng.uniform(0, 1) < self._prob_jitter:
            return []
        inf = float('inf')
        lim = (inf, inf, inf) if self._max_delta is None else self._max_delta
        ilim = inf if self._intensity_max_delta is None else self._intensity_max_delta
        return [Op(OP_JITTER, 0, (float(magnitude),) + tuple(float(v) for v in self._jitter_std) + (float(self._intensity_std),)
                   + tuple(float(v) for v in lim) + (float(ilim),))]


class RandomDropPoints:
    def __init__(self, prob_drop: float, per_point_drop_prob: float):
        self._prob_drop, self._per_point_drop_prob = prob_drop, per_point_drop_prob

    def draw(self, rng, magnitude: float = 1) -> List[Op]:
        if not rng.uniform(0, 1) < self._prob_drop:
            return []
        return [Op(OP_DROP, drop_threshold(self._per_point_drop_prob * magnitude))]


class GlobalNoise:
    """kitti_mask_augmentations.py:196-217: ALWAYS applied (``prob_aug`` is stored and never read there); one N(0,
    ``trans_std``) translation of x, y, z, then one scale in ``1 ± scale_delta``, drawn in that order."""

    def __init__(self, prob_aug: float, trans_std: float = 0.2, scale_delta: float = 0.05):
        self._prob_aug, self._trans_std, self._scale_delta = prob_aug, trans_std, scale_delta

    def draw(self, rng, magnitude: float = 1) -> List[Op]:
        noise = rng.standard_normal((3,)) * self._trans_std
        scale = rng.uniform(1 - self._scale_delta, 1 + self._scale_delta)
        return [Op(OP_GLOBAL_NOISE, 0, (float(scale),) + tuple(float(v) for v in noise))]


class RandAugment:
    """``num_augments`` of ``transforms`` drawn with replacement, each run at ``magnitude`` (rand_augment.py)."""

    def __init__(self, num_augments: int, transforms: Sequence, magnitude: float):
        self._num_augments, self._transforms, self._magnitude = num_augments, list(transforms), magnitude

    def draw(self, rng, magnitude: float = 1) -> List[Op]:
        ops = []
        for j in rng.integers(0, len(self._transforms), size=self._num_augments):
            ops += self._transforms[int(j)].draw(rng, self._magnitude)
        return ops


_CONSTRUCTORS = {'flip': Flip, 'shuffle': ShufflePoints, 'rotate': RandomRotate, 'decimate': DecimatePoints,
                 'jitter': JitterPoints, 'drop': RandomDropPoints}


_KITTI_CONSTRUCTORS = dict(_CONSTRUCTORS, flip=KittiFlip, global_noise=GlobalNoise)
_WAYMO_CONSTRUCTORS = dict(_CONSTRUCTORS, flip=WaymoFlip)
_NOT_PROVIDED = {
    'cut_pc': 'cut_pc is not implemented (in the reference it calls a tuple: a dead path)',
    'object_sample': 'object_sample is not implemented: it pastes objects from the dataset\'s samples.pkl, which this package '
                     'neither reads nor writes',
    'object_noise': 'object_noise is not implemented: it is mmdet3d\'s numba collision search (noise_per_object_v3_)',
}


def make_augmentation(args: Dict, constructors: Optional[Dict] = None, rand_augment: bool = True):
    constructors = _CONSTRUCTORS if constructors is None else constructors
    name = args.get('name')
    if name == 'rand_augment':
        if not rand_augment:
            raise NotImplementedError('rand augment')                 # waymo_mask_augmentations.py:25-26
        return RandAugment(args.get('num_augments'),
                           [make_augmentation(a, constructors) for a in args.get('transforms')], args.get('magnitude'))
    if name in _NOT_PROVIDED and name not in constructors:
        raise NotImplementedError(_NOT_PROVIDED[name])
    if name not in constructors:
        raise NotImplementedError(f'{name} is not implemented')
    kwargs = copy.copy(args)
    kwargs.pop('name')
    return constructors[name](**kwargs)


def make_semantic_kitti_augmentation_list(augmentations: List[Dict]) -> List:
    return [make_augmentation(aug) for aug in augmentations]


def make_kitti_augmentation_list(augmentations: List[Dict]) -> List:
    """kitti_mask_augmentations.py:19-52: the SemanticKITTI names with the y-only ``flip``, plus ``global_noise``."""
    return [make_augmentation(aug, _KITTI_CONSTRUCTORS) for aug in augmentations]


def make_waymo_augmentation_list(augmentations: List[Dict]) -> List:
    """waymo_mask_augmentations.py:11-35: the six point transforms with the y-only ``flip`` that keeps the heading; no
    ``rand_augment``, no magnitudes."""
    return [make_augmentation(aug, _WAYMO_CONSTRUCTORS, rand_augment=False) for aug in augmentations]


def transform_boxes(boxes, ops: Sequence[Op]) -> np.ndarray:
    """One sample's ``boxes`` (n, 7) f64 [cx, cy, cz, l, w, h, theta] under its ``ops``, in op order, as the reference moves
    its labels (kitti_mask_augmentations.py:67-71,118-123,209-214): a linear op maps the centre's x, y and sets theta by
    the op's ``heading`` rule (``LinearOp``); global noise scales centre and dimensions, then shifts the centre.  Other ops act on points
    only."""
    boxes = np.array(boxes, dtype=np.float64).reshape(-1, 7)
    for op in ops:
        if op.code == OP_LINEAR:
            a = np.array(op.p[:4], dtype=np.float64).reshape(2, 2)
            c, s = np.cos(boxes[:, 6]), np.sin(boxes[:, 6])
            x, y = boxes[:, 0].copy(), boxes[:, 1].copy()
            boxes[:, 0], boxes[:, 1] = a[0, 0] * x + a[0, 1] * y, a[1, 0] * x + a[1, 1] * y
            heading = getattr(op, 'heading', None)
            if heading is not None:
                boxes[:, 6] = heading[0] * boxes[:, 6] + heading[1]
            else:
                boxes[:, 6] = np.arctan2(a[1, 0] * c + a[1, 1] * s, a[0, 0] * c + a[0, 1] * s)
        elif op.code == OP_GLOBAL_NOISE:
            boxes[:, :6] *= op.p[0]
            boxes[:, :3] += np.array(op.p[1:4], dtype=np.float64)
    return boxes


# ---------------------------------------------------------------------------------------------------------
# one sample's draw, the records, the compose object
# ---------------------------------------------------------------------------------------------------------
class SampleDraw(NamedTuple):
    seed: int                      # 64 bits
    ops: Tuple[Op, ...]

    @property
    def matrix(self) -> np.ndarray:
        """The composed 2 x 2 matrix A (original → augmented) of the linear ops, in op order."""
        a = np.eye(2)
        for op in self.ops:
            if op.code == OP_LINEAR:
                a = np.array(op.p, dtype=np.float64).reshape(2, 2) @ a
        return a

    @property
    def permutes(self) -> bool:
        return any(op.code in (OP_SHUFFLE, OP_DECIMATE) for op in self.ops)

    @property
    def removes(self) -> bool:
        return any(op.code in (OP_DROP, OP_DECIMATE) for op in self.ops)


def batch_mode(draws: Sequence[SampleDraw]) -> int:
    """The smallest K23b mode that covers a batch: 2 with a shuffle or decimate, 1 with drops only, else 0."""
    if any(d.permutes for d in draws):
        return 2
    return 1 if any(d.removes for d in draws) else 0


def pack_records(draws: Sequence[SampleDraw]) -> np.ndarray:
    rec = np.zeros((len(draws),), dtype=RECORD_DTYPE)
    for b, d in enumerate(draws):
        if len(d.ops) > MAX_OPS:
            raise ValueError(f'{len(d.ops)} ops drawn for one sample; the device program holds {MAX_OPS}')
        rec[b]['seed_lo'], rec[b]['seed_hi'] = d.seed & 0xFFFFFFFF, (d.seed >> 32) & 0xFFFFFFFF
        rec[b]['n_ops'], rec[b]['flags'] = len(d.ops), int(d.permutes)
        for s, op in enumerate(d.ops):
            rec[b]['ops'][s]['code'], rec[b]['ops'][s]['arg'] = op.code, op.arg
            rec[b]['ops'][s]['p'][:len(op.p)] = op.p
    return rec


class AugmentedBatch(NamedTuple):
    scans: List[torch.Tensor]                       # views of one buffer
    instance_maps: Optional[torch.Tensor]
    scene_transforms: Optional[List[np.ndarray]]
    draws: List[SampleDraw]
    offsets: torch.Tensor                           # (B + 1) i32 on the device
    synced: bool
    boxes: Optional[List[np.ndarray]] = None        # per sample (n, 7) f64, moved with the points


class ObjectAugmentedBatch(AugmentedBatch):
    """The ``AugmentedBatch`` of a list with object transforms (K28) — the same fields to unpacking and comparisons — that
    also carries the object stage's decisions: one ``object_augment.ObjectFrame`` per sample.  ``boxes`` then holds the
    labels and the pasted boxes, after the noise and the point ops."""
    objects: Optional[List] = None


class DeviceAugmentation:
    """Compose of the transforms above.  ``x_range``, ``y_range``, ``voxel_size`` are needed only to warp instance maps."""

    def __init__(self, transforms: Sequence, seed: int = 0, x_range=None, y_range=None, voxel_size: Optional[float] = None):
        self.transforms = list(transforms)
        self.x_range, self.y_range, self.voxel_size = x_range, y_range, voxel_size
        self.reseed(seed)

    def reseed(self, *entropy: int) -> None:
        """Restart the host generator from integers, e.g. (seed, rank, epoch, batch index)."""
        self._rng = np.random.default_rng(np.random.SeedSequence([int(e) for e in entropy]))

    def draw(self, batch_size: int) -> List[SampleDraw]:
        draws = []
        for _ in range(batch_size):
            ops = []
            for t in self.transforms:
                ops += t.draw(self._rng)
            if len(ops) > MAX_OPS:
                raise ValueError(f'{len(ops)} ops drawn for one sample; the device program holds {MAX_OPS}')
            draws.append(SampleDraw(int(self._rng.integers(0, 1 << 64, dtype=np.uint64)), tuple(ops)))
        return draws

    @torch.no_grad()
    def apply(self, scans: Sequence[torch.Tensor], instance_maps: Optional[torch.Tensor] = None,
              scene_transforms: Optional[Sequence] = None, draws: Optional[Sequence[SampleDraw]] = None,
              boxes: Optional[Sequence] = None, object_frames: Optional[Sequence] = None,
              object_bank=None) -> AugmentedBatch:
        """``object_frames``: the object stage's decisions, made by the caller (one ``object_augment.ObjectFrame`` per scan)
        instead of drawn here; ``object_bank``: the bank their pasted entries index, when the list holds no ``ObjectSample``."""
        scans = list(scans)
        if len(scans) == 0:
            raise ValueError('empty batch')
        for s in scans:
            if not s.is_cuda:
                raise MaskBevHipError('DeviceAugmentation needs ROCm device tensors (no CPU fallback)')
            if s.dim() != 2 or s.shape[1] not in (3, 4) or s.shape[1] != scans[0].shape[1]:
                raise ValueError(f'scans must all be (n, 3) or all (n, 4), got {tuple(s.shape)}')
        if instance_maps is not None and not instance_maps.is_cuda:
            raise MaskBevHipError('DeviceAugmentation needs ROCm device tensors (no CPU fallback)')
        if boxes is not None and len(boxes) != len(scans):
            raise ValueError('one (n, 7) box table per scan expected')
        objects = self._object_frames(len(scans), instance_maps, scene_transforms, boxes, object_frames)   # drawn first
        draws = self.draw(len(scans)) if draws is None else list(draws)
        if len(draws) != len(scans):
            raise ValueError(f'{len(draws)} draws for {len(scans)} scans')
        if (instance_maps is not None or scene_transforms is not None) and \
                any(op.code == OP_GLOBAL_NOISE for d in draws for op in d.ops):
            raise ValueError('global_noise is not a linear map about the origin: it cannot be applied to instance maps or '
                             'scene transforms (use box tables)')
        dev = scans[0].device
        mode = batch_mode(draws)
        records = torch.from_numpy(pack_records(draws).view(np.uint8).reshape(-1)).to(dev, non_blocking=True)
        if objects is not None:
            # K28 first; "original index" below is the row in its output
            from . import object_augment
            points, offsets = object_augment.run_frames(
                scans, objects, object_augment.stage_bank(self.transforms) if object_bank is None else object_bank)
            offsets = np.asarray(offsets, dtype=np.int32)
            boxes = [f.moved_boxes for f in objects]
        else:
            counts = [int(s.shape[0]) for s in scans]
            offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            points = torch.cat([s.to(torch.float32) for s in scans]) if len(scans) > 1 else scans[0].to(torch.float32)
        out, out_offsets, out_counts = ops_augment.augment_points(
            points, torch.from_numpy(offsets).to(dev, non_blocking=True), records, mode)
        if mode:
            new_offsets = [int(v) for v in out_offsets.tolist()]             # the one sync: point removal sizes the views
        else:
            new_offsets = offsets.tolist()
        views = [out[new_offsets[b]:new_offsets[b + 1]] for b in range(len(scans))]
        maps = tfs = None
        mats = np.stack([d.matrix for d in draws])
        if instance_maps is not None:
            if self.voxel_size is None or self.x_range is None or self.y_range is None:
                raise ValueError('warping instance maps needs x_range, y_range and voxel_size')
            if instance_maps.dim() != 3 or instance_maps.shape[0] != len(scans):
                raise ValueError('instance_maps must be (B, nx, ny)')
            maps = instance_maps.to(torch.int32)
            if any(not np.array_equal(m, np.eye(2)) for m in mats):
                maps = ops_augment.warp_instance_maps(maps, torch.from_numpy(mats).to(dev, non_blocking=True),
                                                      -self.x_range[0] / self.voxel_size, -self.y_range[0] / self.voxel_size)
        if scene_transforms is not None:
            if len(scene_transforms) != len(scans):
                raise ValueError('one (S, 4, 4) transform stack per scan expected')
            tfs = []
            for m, tf in zip(mats, scene_transforms):
                tf = np.asarray(tf.detach().cpu().numpy() if isinstance(tf, torch.Tensor) else tf, dtype=np.float64)
                a4 = np.eye(4)
                a4[:2, :2] = m
                tfs.append(a4 @ tf.reshape(-1, 4, 4))                        # the last row stays 0 0 0 1
        moved = None if boxes is None else [transform_boxes(b, d.ops) for b, d in zip(boxes, draws)]
        if objects is None:
            return AugmentedBatch(views, maps, tfs, list(draws), out_offsets, bool(mode), moved)
        res = ObjectAugmentedBatch(views, maps, tfs, list(draws), out_offsets, True, moved)
        res.objects = objects
        return res

    def _object_frames(self, batch_size, instance_maps, scene_transforms, boxes, object_frames):
        """The object stage's host decisions (``object_augment``), or None when the list holds no object transform."""
        stage = [t for t in self.transforms if getattr(t, 'is_object_transform', False)]
        if not stage and object_frames is None:
            return None
        if instance_maps is not None or scene_transforms is not None:
            raise ValueError('object transforms move and paste boxes: they cannot be applied to instance maps or scene '
                             'transforms (use box tables)')
        if object_frames is not None:
            if len(object_frames) != batch_size:
                raise ValueError(f'{len(object_frames)} object frames for {batch_size} scans')
            return list(object_frames)
        if boxes is None:
            raise ValueError('object transforms need the box tables of the batch (boxes=)')
        if any(getattr(t, 'is_object_transform', False) for t in self.transforms[len(stage):]):
            raise ValueError('object transforms must come before every point transform of the list')
        from . import object_augment
        return object_augment.draw_frames(stage, self._rng, boxes)

    __call__ = apply


__all__ = ['make_augmentation', 'make_semantic_kitti_augmentation_list', 'make_kitti_augmentation_list',
           'make_waymo_augmentation_list', 'KittiFlip', 'WaymoFlip', 'GlobalNoise', 'LinearOp', 'linear_op', 'transform_boxes', 'OP_GLOBAL_NOISE',
           'DeviceAugmentation', 'AugmentedBatch', 'ObjectAugmentedBatch', 'SampleDraw',
           'Op', 'Flip', 'ShufflePoints', 'RandomRotate', 'DecimatePoints', 'JitterPoints', 'RandomDropPoints', 'RandAugment',
           'rotation_op', 'drop_threshold', 'pack_records', 'batch_mode', 'RECORD_DTYPE', 'MAX_OPS']
