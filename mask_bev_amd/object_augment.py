"""KITTI's two object augmentations on the device (K28, csrc/object_augment.hip): the reference's ``ObjectSample`` (ground-truth
pasting) and ``BoxNoise`` (``object_noise``: a perturbation per object) of
``mask_bev/augmentations/kitti_mask_augmentations.py:220-343``, the sampler of ``scripts/generate_kitti_object_sampler.py``
and the mmdet3d 1.1 functions they call (``noise_per_object_v3_``, ``noise_per_box``, ``box_collision_test``,
``points_in_rbbox``, ``points_transform_``, ``box3d_transform_``), restated.  The decisions of a frame — which bank entries are
pasted, which of ``num_try`` noises each box takes — are a few dozen boxes' worth of numpy f64 on the host, drawn from the
generator ``DeviceAugmentation`` owns; everything per point (every point of a scan against every box: moved, removed, joined
by pasted points) is K28's.

    bank = ObjectBank.build(frames)                     # (points, boxes) per training frame; cut on the device
    bank.save(ObjectBank.default_path('data/KITTI'))    # <dataset_root>/samples.npz
    aug = DeviceAugmentation(make_kitti_object_augmentation_list(config['augmentations']), seed=420)
    out = aug.apply(scans, boxes=[(n, 7) f64, ...])     # out.boxes: labels + pasted boxes, perturbed, then moved by K23's ops

Boxes are the package's (n, 7) f64 [cx, cy, cz, l, w, h, theta]: l along the yaw direction, w across it, counter-clockwise, as
``rasterize.box_vertices`` draws them; cz is the BOTTOM face (mmdet3d's origin (0.5, 0.5, 0)).

Parity with mmdet3d itself is not pinned by any test: mmdet3d, numba and a ``samples.pkl`` are not at hand, so the rules
written here and in include/maskbev_hip.h (K28) are the specification.  Restated, not repaired: a frame without boxes passes
``ObjectNoise`` untouched (the reference fails on ``np.stack([])``).  Not provided: reading ``samples.pkl`` (pickled instances
of the reference's own classes), a ``global_rot_range`` other than zero (no configuration uses it), ``cut_pc``.
"""
from __future__ import annotations

import os
import pathlib
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import augment, ops_augment
from ._lib import MaskBevHipError

FLAG_REMOVE, FLAG_MOVE = 1, 2
BUILD_COMMAND = 'python train_mask_bev_amd.py --config <config> --build-object-bank'


# ---------------------------------------------------------------------------------------------------------
# footprints and the collision rule (box_collision_test)
# ---------------------------------------------------------------------------------------------------------
def footprints(boxes) -> np.ndarray:
    """(n, 7) boxes → (n, 4, 2) f64 corners, counter-clockwise, in the corner order of ``rasterize.box_vertices``."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    c, s = np.cos(boxes[:, 6]), np.sin(boxes[:, 6])
    d = np.stack([c, s], -1)[:, None, :] * (boxes[:, 3] / 2)[:, None, None]
    e = np.stack([-s, c], -1)[:, None, :] * (boxes[:, 4] / 2)[:, None, None]
    sl = np.array([1., -1., -1., 1.])[None, :, None]
    sw = np.array([1., 1., -1., -1.])[None, :, None]
    return sl * d + sw * e + boxes[:, None, :2]


def _ccw(p, q, r):
    return (r[..., 1] - p[..., 1]) * (q[..., 0] - p[..., 0]) > (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0])


def _all_inside(outer, inner):
    """(n, m): every corner of inner[j] lies strictly inside outer[i] (either winding)."""
    a, b = outer[:, None, :, None, :], np.roll(outer, -1, axis=1)[:, None, :, None, :]     # (n, 1, 4 edges, 1, 2)
    p = inner[None, :, None, :, :]                                                         # (1, m, 1, 4 corners, 2)
    cross = (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])
    return ((cross > 0).all(2) | (cross < 0).all(2)).all(2)


def collides(a, b) -> np.ndarray:
    """a (n, 4, 2), b (m, 4, 2) → (n, m) bool.  Two quadrilaterals collide iff their axis-aligned hulls overlap with positive
    width and height AND (two edges cross by the four strict orientation comparisons ``acd != bcd and abc != abd``, or every
    corner of one lies strictly inside the other).  Touching is no collision."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 4, 2), np.asarray(b, dtype=np.float64).reshape(-1, 4, 2)
    lo_a, hi_a, lo_b, hi_b = a.min(1)[:, None], a.max(1)[:, None], b.min(1)[None], b.max(1)[None]
    hull = ((np.minimum(hi_a, hi_b) - np.maximum(lo_a, lo_b)) > 0).all(-1)
    A, B = a[:, None, :, None, :], np.roll(a, -1, axis=1)[:, None, :, None, :]             # (n, 1, 4, 1, 2)
    C, D = b[None, :, None, :, :], np.roll(b, -1, axis=1)[None, :, None, :, :]             # (1, m, 1, 4, 2)
    cross = ((_ccw(A, C, D) != _ccw(B, C, D)) & (_ccw(A, B, C) != _ccw(A, B, D))).any((2, 3))
    return hull & (cross | _all_inside(a, b) | _all_inside(b, a).T)


# ---------------------------------------------------------------------------------------------------------
# the bank of pasted objects
# ---------------------------------------------------------------------------------------------------------
def box_table(boxes, rot=None, loc=None, flags=None) -> np.ndarray:
    """K28's (n, 14) f64 rows of ``boxes`` (before the noise) with the noise (``rot`` (n), ``loc`` (n, 3)) and ``flags`` (n)."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    n = boxes.shape[0]
    rot = np.zeros(n) if rot is None else np.asarray(rot, dtype=np.float64).reshape(n)
    loc = np.zeros((n, 3)) if loc is None else np.asarray(loc, dtype=np.float64).reshape(n, 3)
    t = np.zeros((n, ops_augment.BOX_ROW), dtype=np.float64)
    t[:, 0:3] = boxes[:, 0:3]
    t[:, 3], t[:, 4], t[:, 5] = boxes[:, 3] / 2, boxes[:, 4] / 2, boxes[:, 5]
    t[:, 6], t[:, 7] = np.cos(boxes[:, 6]), np.sin(boxes[:, 6])
    t[:, 8], t[:, 9] = np.cos(rot), np.sin(rot)
    t[:, 10:13] = loc
    t[:, 13] = 0 if flags is None else np.asarray(flags, dtype=np.float64).reshape(n)
    return t


class ObjectBank:
    """The objects ``ObjectSample`` pastes: ``points`` (P, 4) f32, all samples concatenated; ``offsets`` (S + 1) i32;
    ``boxes`` (S, 7) f64, in the velodyne frame.  One ``.npz``, by default ``<dataset_root>/samples.npz``; the points are
    uploaded once per device and stay there."""

    def __init__(self, points, offsets, boxes):
        self.points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        self.boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 7)
        if self.offsets.size != len(self.boxes) + 1 or self.offsets[0] != 0 or self.offsets[-1] != len(self.points) or \
                (np.diff(self.offsets) < 0).any():
            raise ValueError('ObjectBank: offsets must ascend from 0 to the number of points, one more than boxes')
        self.footprints = footprints(self.boxes)
        self._device_points: Dict[torch.device, torch.Tensor] = {}

    def __len__(self) -> int:
        return len(self.boxes)

    def sample_points(self, k: int) -> np.ndarray:
        return self.points[self.offsets[k]:self.offsets[k + 1]]

    def device_points(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device not in self._device_points:
            self._device_points[device] = torch.from_numpy(self.points).to(device)
        return self._device_points[device]

    @staticmethod
    def default_path(dataset_root) -> pathlib.Path:
        return pathlib.Path(dataset_root).expanduser() / 'samples.npz'

    @classmethod
    def build(cls, frames: Iterable[Tuple], min_points: int = 5, device=None) -> 'ObjectBank':
        """``frames``: (points (N, 4) f32, boxes (n, 7) f64) in the velodyne frame.  Every box that holds at least
        ``min_points`` points by K28's membership rule (mbv_points_in_boxes, on ``device``; a point in two boxes counts for
        the first) becomes a sample: generate_kitti_object_sampler.py's rule."""
        device = torch.device('cuda' if device is None else device)
        if device.type != 'cuda':
            raise MaskBevHipError('ObjectBank.build cuts the samples on a ROCm device (no CPU fallback)')
        pts, counts, kept = [], [], []
        for points, boxes in frames:
            points = np.ascontiguousarray(points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points,
                                          dtype=np.float32)
            boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
            if points.ndim != 2 or points.shape[1] != 4:
                raise ValueError(f'ObjectBank.build: points must be (N, 4), got {points.shape}')
            if not len(boxes) or not len(points):
                continue
            index = ops_augment.points_in_boxes(torch.from_numpy(points).to(device),
                                                torch.from_numpy(box_table(boxes)).to(device)).cpu().numpy()
            for k in range(len(boxes)):
                inside = np.flatnonzero(index == k)
                if len(inside) >= min_points:
                    pts.append(points[inside])
                    counts.append(len(inside))
                    kept.append(boxes[k])
        return cls(np.concatenate(pts) if pts else np.zeros((0, 4), np.float32), np.concatenate([[0], np.cumsum(counts)]),
                   np.array(kept, dtype=np.float64).reshape(-1, 7))

    def save(self, path) -> None:
        path = pathlib.Path(path).expanduser()
        path.parent.mkdir(parents=True, exist_ok=True)
        with open(path, 'wb') as f:
            np.savez(f, points=self.points, offsets=self.offsets, boxes=self.boxes)

    @classmethod
    def load(cls, path) -> 'ObjectBank':
        path = pathlib.Path(path).expanduser()
        if not path.exists():
            pkl = path.with_name('samples.pkl')
            why = (f'{pkl} holds pickled instances of the reference\'s own classes and is not read; ' if pkl.exists() else '')
            raise FileNotFoundError(f'Cannot find the object bank at {path}: {why}build it with `{BUILD_COMMAND}`')
        with np.load(path) as z:
            return cls(z['points'], z['offsets'], z['boxes'])


# ---------------------------------------------------------------------------------------------------------
# the two transforms: host decisions of one frame
# ---------------------------------------------------------------------------------------------------------
class ObjectFrame:
    """One frame's object decisions.  ``boxes`` (n, 7): labels, then the accepted pasted boxes in paste order, all BEFORE the
    noise; ``pasted``: their bank indices; ``rot`` (n), ``loc`` (n, 3), ``selected`` (n): the noise each box takes (zeros and
    False where the search found no free place); ``noise``: whether an ``ObjectNoise`` ran."""

    def __init__(self, boxes):
        self.boxes = np.array(boxes, dtype=np.float64).reshape(-1, 7)
        self.n_labels = len(self.boxes)
        self.pasted: List[int] = []
        self.rot, self.loc = np.zeros(self.n_labels), np.zeros((self.n_labels, 3))
        self.selected = np.zeros(self.n_labels, dtype=bool)
        self.noise = False

    def paste(self, bank: ObjectBank, k: int) -> None:
        if self.noise:
            raise ValueError('object_sample must come before object_noise')
        self.boxes = np.concatenate([self.boxes, bank.boxes[k:k + 1]])
        self.pasted.append(int(k))
        self.rot, self.loc = np.append(self.rot, 0.), np.concatenate([self.loc, np.zeros((1, 3))])
        self.selected = np.append(self.selected, False)

    @property
    def table(self) -> np.ndarray:
        flags = np.zeros(len(self.boxes))
        flags[self.n_labels:] += FLAG_REMOVE
        if self.noise:
            flags += FLAG_MOVE             # an unmoved box keeps the bit with the identity noise: it still claims its points
        return box_table(self.boxes, self.rot, self.loc, flags)

    @property
    def moved_boxes(self) -> np.ndarray:
        """The boxes after the noise: centre += loc on all three components, theta += rot (box3d_transform_)."""
        out = self.boxes.copy()
        out[:, :3] += self.loc
        out[:, 6] += self.rot
        return out


class ObjectNoise:
    """``object_noise`` (BoxNoise, kitti_mask_augmentations.py:227-268; noise_per_object_v3_ / noise_per_box): per frame with n
    boxes, ``loc_noises`` (n, num_try, 3) normal with ``translation_std``, then ``rot_noises`` (n, num_try) uniform in
    ``rot_range``; for i = 0 .. n - 1 the first try j whose footprint — box i's, turned about its centre by rot_noises[i, j]
    and shifted by loc_noises[i, j, :2] — collides with no other box's CURRENT footprint (boxes before i already moved, boxes
    after it not yet) replaces box i's footprint.  Without a free try the box stays, with the identity noise."""
    is_object_transform = True

    def __init__(self, translation_std=None, global_rot_range=None, rot_range=None, num_try: int = 100):
        translation_std = [0.25, 0.25, 0.25] if translation_std is None else translation_std
        global_rot_range = [0.0, 0.0] if global_rot_range is None else global_rot_range
        rot_range = [-0.15707963267, 0.15707963267] if rot_range is None else rot_range
        if np.isscalar(translation_std):
            translation_std = [translation_std] * 3
        if np.isscalar(rot_range):
            rot_range = [-rot_range, rot_range]
        if np.isscalar(global_rot_range):
            global_rot_range = [-global_rot_range, global_rot_range]
        if abs(global_rot_range[1] - global_rot_range[0]) > 1e-3:
            raise NotImplementedError('object_noise: global_rot_range is not implemented (no configuration uses it)')
        self._translation_std = np.array(translation_std, dtype=np.float64).reshape(3)
        self._rot_range = (float(rot_range[0]), float(rot_range[1]))
        self._num_try = int(num_try)

    def draw(self, rng, magnitude: float = 1) -> List:
        return []                                                    # no point op: the object stage runs before K23

    def search(self, rng: np.random.Generator, boxes) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(n, 7) boxes → (rot (n), loc (n, 3), selected (n) bool)."""
        boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
        n, tries = len(boxes), self._num_try
        rot, loc, selected = np.zeros(n), np.zeros((n, 3)), np.zeros(n, dtype=bool)
        if n == 0:
            return rot, loc, selected
        loc_noises = rng.normal(scale=self._translation_std, size=(n, tries, 3))
        rot_noises = rng.uniform(self._rot_range[0], self._rot_range[1], size=(n, tries))
        if tries == 0:
            return rot, loc, selected
        corners = footprints(boxes)
        for i in range(n):
            rel = corners[i] - boxes[i, :2]                                                    # (4, 2)
            c, s = np.cos(rot_noises[i])[:, None], np.sin(rot_noises[i])[:, None]              # (tries, 1)
            cand = np.stack([c * rel[None, :, 0] - s * rel[None, :, 1], s * rel[None, :, 0] + c * rel[None, :, 1]], -1)
            cand = cand + (boxes[i, :2] + loc_noises[i, :, :2])[:, None, :]                    # (tries, 4, 2)
            others = np.delete(corners, i, axis=0)
            free = np.flatnonzero(~collides(cand, others).any(1)) if len(others) else np.arange(tries)
            if len(free):
                j = int(free[0])
                corners[i] = cand[j]
                rot[i], loc[i], selected[i] = rot_noises[i, j], loc_noises[i, j], True
        return rot, loc, selected

    def run(self, rng, frame: ObjectFrame) -> None:
        if frame.noise:
            raise ValueError('one object_noise per list')
        frame.rot, frame.loc, frame.selected = self.search(rng, frame.boxes)
        frame.noise = True


class ObjectSample:
    """``object_sample`` (kitti_mask_augmentations.py:278-343): count = (r1 + r2 + r3) % num_sample from three
    ``integers(0, num_sample)`` draws, then ``count`` attempts; each picks one bank entry uniformly, with replacement, and
    accepts it iff its footprint collides with none of the frame's boxes and none of the entries accepted before; a rejected
    attempt is not retried.  ``bank``: an ``ObjectBank``; ``None`` loads ``<dataset_root>/samples.npz``."""
    is_object_transform = True

    def __init__(self, dataset_root: str, num_sample: int, bank: Optional[ObjectBank] = None):
        self.bank = ObjectBank.load(ObjectBank.default_path(dataset_root)) if bank is None else bank
        if int(num_sample) < 1:
            raise ValueError('object_sample: num_sample must be at least 1')
        if len(self.bank) == 0:
            raise ValueError('object_sample: the object bank is empty')
        self._num_sample = int(num_sample)

    def draw(self, rng, magnitude: float = 1) -> List:
        return []

    def choose(self, rng: np.random.Generator, boxes) -> List[int]:
        """The accepted bank indices for a frame with ``boxes``, in paste order."""
        count = sum(int(rng.integers(0, self._num_sample)) for _ in range(3)) % self._num_sample
        avoid = footprints(boxes)
        accepted = []
        for _ in range(count):
            k = int(rng.integers(0, len(self.bank)))
            fp = self.bank.footprints[k:k + 1]
            if not collides(fp, avoid).any():
                accepted.append(k)
                avoid = np.concatenate([avoid, fp])
        return accepted

    def run(self, rng, frame: ObjectFrame) -> None:
        if frame.pasted or frame.noise:
            raise ValueError('one object_sample per list, before object_noise')
        for k in self.choose(rng, frame.boxes):
            frame.paste(self.bank, k)


_OBJECT_CONSTRUCTORS = {'object_sample': ObjectSample, 'object_noise': ObjectNoise}


def make_kitti_object_augmentation_list(augmentations: List[Dict], bank: Optional[ObjectBank] = None) -> List:
    """The KITTI list INCLUDING ``object_sample`` and ``object_noise`` (kitti_mask_augmentations.py:19-52); every other name
    goes to ``augment.make_augmentation`` unchanged.  The object transforms must stand before all point transforms, as in
    both shipped configurations, ``object_sample`` before ``object_noise``, and outside ``rand_augment``."""
    out, seen_point = [], False
    for args in augmentations:
        name = args.get('name')
        if name in _OBJECT_CONSTRUCTORS:
            if seen_point:
                raise ValueError(f'{name} must come before every point transform of the list')
            if any(isinstance(t, _OBJECT_CONSTRUCTORS[name]) for t in out) or \
                    (name == 'object_sample' and any(isinstance(t, ObjectNoise) for t in out)):
                raise ValueError(f'{name}: at most one per list, object_sample before object_noise')
            kwargs = {k: v for k, v in args.items() if k != 'name'}
            if name == 'object_sample':
                kwargs['bank'] = bank
            out.append(_OBJECT_CONSTRUCTORS[name](**kwargs))
            continue
        if name == 'rand_augment' and any(a.get('name') in _OBJECT_CONSTRUCTORS for a in args.get('transforms') or []):
            raise ValueError('object_sample / object_noise cannot run inside rand_augment')
        seen_point = True
        out.append(augment.make_augmentation(args, augment._KITTI_CONSTRUCTORS))
    return out


def object_transforms(transforms: Sequence) -> List:
    return [t for t in transforms if getattr(t, 'is_object_transform', False)]


def draw_frames(transforms: Sequence, rng: np.random.Generator, boxes: Sequence) -> List[ObjectFrame]:
    """Frame by frame, the object transforms in list order: all host draws of the object stage."""
    frames = []
    for b in boxes:
        frame = ObjectFrame(b)
        for t in transforms:
            t.run(rng, frame)
        frames.append(frame)
    return frames


@torch.no_grad()
def run_frames(scans: Sequence[torch.Tensor], frames: Sequence[ObjectFrame], bank: Optional[ObjectBank]):
    """K28 over a batch → (points (N', dim) f32: the output scans concatenated, offsets (B + 1) host list).  One host
    synchronisation reads the new scan offsets."""
    dev = scans[0].device
    counts = [int(s.shape[0]) for s in scans]
    points = torch.cat([s.to(torch.float32) for s in scans]) if len(scans) > 1 else scans[0].to(torch.float32)
    tables = [f.table for f in frames]
    segments, paste_offsets = [], [0]
    for f in frames:
        if f.pasted and bank is None:
            raise ValueError('pasted objects need the ObjectBank they come from')
        segments += [(int(bank.offsets[k]), int(bank.offsets[k + 1] - bank.offsets[k])) for k in f.pasted]
        paste_offsets.append(len(segments))
    out, out_offsets, _ = ops_augment.object_augment(
        points, np.concatenate([[0], np.cumsum(counts)]), torch.from_numpy(np.concatenate(tables)).to(dev, non_blocking=True),
        np.concatenate([[0], np.cumsum([len(t) for t in tables])]),
        None if bank is None or not segments else bank.device_points(dev), segments or None, paste_offsets)
    offsets = [int(v) for v in out_offsets.tolist()]                 # the one sync: removal and pasting size the views
    return out[:offsets[-1]], offsets


def stage_bank(transforms: Sequence) -> Optional[ObjectBank]:
    for t in transforms:
        if isinstance(t, ObjectSample):
            return t.bank
    return None


__all__ = ['ObjectNoise', 'ObjectSample', 'ObjectBank', 'ObjectFrame', 'make_kitti_object_augmentation_list', 'footprints',
           'collides', 'box_table', 'object_transforms', 'draw_frames', 'run_frames', 'stage_bank', 'FLAG_REMOVE', 'FLAG_MOVE',
           'BUILD_COMMAND']
