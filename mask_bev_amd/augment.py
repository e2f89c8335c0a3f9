"""Training augmentations of SemanticKITTI samples on the device (K23, csrc/augment.hip): the reference's
``mask_bev/augmentations/semantic_kitti_mask_augmentations.py`` — same names, same keyword arguments, same magnitude rules
— with the per-sample decisions (which transform fires, the angle, one 64-bit seed) drawn on the host from a seeded
generator and everything per point or per cell done by three kernels.

    aug = DeviceAugmentation(make_semantic_kitti_augmentation_list(config['augmentations']), seed=420,
                             x_range=..., y_range=..., voxel_size=...)
    aug.reseed(seed, rank, epoch, batch_index)
    out = aug.apply(scans, instance_maps=maps)            # cached maps: warped by K23c
    out = aug.apply(scans, scene_transforms=[tf, ...])    # scenes: diag(A, 1, 1) @ tf, rasterised afterwards (K22)

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
OP_LINEAR, OP_JITTER, OP_DROP, OP_SHUFFLE, OP_DECIMATE = 1, 2, 3, 4, 5

# one scan's record as the kernels read it (include/maskbev_hip.h, K23): 656 bytes
OP_DTYPE = np.dtype([('code', '<i4'), ('arg', '<u4'), ('p', '<f8', (9,))])
RECORD_DTYPE = np.dtype([('seed_lo', '<u4'), ('seed_hi', '<u4'), ('n_ops', '<i4'), ('flags', '<i4'), ('ops', OP_DTYPE, (MAX_OPS,))])
assert RECORD_DTYPE.itemsize == ops_augment.AUGMENT_RECORD_BYTES


class Op(NamedTuple):
    code: int
    arg: int = 0
    p: Tuple[float, ...] = ()


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
            ops.append(Op(OP_LINEAR, 0, (-1., 0., 0., 1.)))
        if rng.uniform(0, 1) < self._prob_flip_y * magnitude:
            ops.append(Op(OP_LINEAR, 0, (1., 0., 0., -1.)))
        return ops


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
    return Op(OP_LINEAR, 0, (c, -s, s, c))


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


def make_augmentation(args: Dict):
    name = args.get('name')
    if name == 'rand_augment':
        return RandAugment(args.get('num_augments'), make_semantic_kitti_augmentation_list(args.get('transforms')),
                           args.get('magnitude'))
    if name == 'cut_pc':
        raise NotImplementedError('cut_pc is not implemented (in the reference it calls a tuple: a dead path)')
    if name not in _CONSTRUCTORS:
        raise NotImplementedError(f'{name} is not implemented')
    kwargs = copy.copy(args)
    kwargs.pop('name')
    return _CONSTRUCTORS[name](**kwargs)


def make_semantic_kitti_augmentation_list(augmentations: List[Dict]) -> List:
    return [make_augmentation(aug) for aug in augmentations]


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
              scene_transforms: Optional[Sequence] = None, draws: Optional[Sequence[SampleDraw]] = None) -> AugmentedBatch:
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
        draws = self.draw(len(scans)) if draws is None else list(draws)
        if len(draws) != len(scans):
            raise ValueError(f'{len(draws)} draws for {len(scans)} scans')
        dev = scans[0].device
        counts = [int(s.shape[0]) for s in scans]
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        mode = batch_mode(draws)
        records = torch.from_numpy(pack_records(draws).view(np.uint8).reshape(-1)).to(dev, non_blocking=True)
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
        return AugmentedBatch(views, maps, tfs, list(draws), out_offsets, bool(mode))

    __call__ = apply


__all__ = ['make_augmentation', 'make_semantic_kitti_augmentation_list', 'DeviceAugmentation', 'AugmentedBatch', 'SampleDraw',
           'Op', 'Flip', 'ShufflePoints', 'RandomRotate', 'DecimatePoints', 'JitterPoints', 'RandomDropPoints', 'RandAugment',
           'rotation_op', 'drop_threshold', 'pack_records', 'batch_mode', 'RECORD_DTYPE', 'MAX_OPS']
