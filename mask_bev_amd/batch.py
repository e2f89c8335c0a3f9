"""Batch producer for the MaskBEV step: what the reference does on the host between the dataset
and ``training_step`` — reading a scan, and turning the cached instance-id map into padded (labels, masks) targets —
with the target construction moved to the GPU (K14, csrc/instance_masks.hip).

Reference: mask_bev/datasets/semantic_kitti/semantic_kitti_dataset.py (``.bin`` / ``.label`` readers),
semantic_kitti_mask_dataset.py:121-137 (``.npy`` mask cache), semantic_kitti_transforms.py:11-26,66-81,98-121
(FilterSmallMasks, MaskToLabelInstanceMasks, MaskListCollate[Height]); for the box datasets
mask_bev/datasets/kitti/kitti_dataset.py (``label_2`` / ``calib`` readers, camera → velodyne labels) and kitti_transforms.py
(difficulty and range filters, FrameMaskListCollate), with the box table rasterised on the GPU (K24) in front of K14.

What crosses PCIe per scan is the point cloud (1.9 MB) and the (nx, ny) int32 instance map (1 MB) instead of the
dense (Q, ny, nx) f32 masks (105 MB).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, ops
from ._lib import MaskBevHipError, check

CAR = 1           # SemanticKittiLearningLabel.CAR (semantic_kitti_dataset.py:175): the label of every real instance


# ---------------------------------------------------------------------------------------------------------
# host readers (plain numpy; the formats of the SemanticKITTI distribution)
# ---------------------------------------------------------------------------------------------------------
def read_velodyne_bin(path) -> np.ndarray:
    """``sequences/SS/velodyne/NNNNNN.bin`` → (N, 4) f32 x, y, z, remission."""
    pc = np.fromfile(str(path), dtype=np.float32)
    if pc.size % 4:
        raise ValueError(f'{path}: not a multiple of 4 floats')
    return pc.reshape(-1, 4)


def read_semantic_kitti_label(path) -> Tuple[np.ndarray, np.ndarray]:
    """``sequences/SS/labels/NNNNNN.label`` → (semantic (N,) u32 = lower 16 bits, instance (N,) u32 = upper 16 bits)."""
    raw = np.fromfile(str(path), dtype=np.uint32)
    return raw & 0xFFFF, raw >> 16


def apply_learning_map(sem: np.ndarray, inst: np.ndarray, learning_map_lut: np.ndarray, unlabeled: int = 0):
    """Class remap of semantic_kitti_dataset.py:369-372: ``sem`` through the learning-map look-up table, instance ids of
    points that become UNLABELED cleared."""
    sem = learning_map_lut[sem]
    inst = inst.copy()
    inst[sem == unlabeled] = 0
    return sem, inst


def read_poses(path) -> np.ndarray:
    """``sequences/SS/poses.txt`` → (N, 4, 4) f64 origin-to-scan transforms: each line holds the upper 3 x 4 block,
    the omitted last row is (0, 0, 0, 1) (semantic_kitti_dataset.py:336-349)."""
    reduced = np.loadtxt(str(path), ndmin=2)
    n = reduced.shape[0]
    full = np.zeros((n, 4, 4))
    full[:, :3, :] = reduced.reshape(n, 3, 4)
    full[:, 3, 3] = 1
    return full


def read_calib(path) -> dict:
    """``sequences/SS/calib.txt`` → ``{'p0': (3, 4), ..., 'velo_to_cam': (4, 4)}`` (``Tr`` completed with the row
    (0, 0, 0, 1); the other keys lower-cased — the fields of SemanticKittiCalib, semantic_kitti_dataset.py:374-385)."""
    calib = {}
    with open(str(path), 'r') as f:
        for line in f:
            if ':' not in line:
                continue
            k, v = line.split(':')
            mat = np.array(v.split(), dtype=np.float64).reshape(3, 4)
            if k == 'Tr':
                calib['velo_to_cam'] = np.vstack((mat, [0, 0, 0, 1]))
            else:
                calib[k.lower()] = mat
    return calib


def read_mask_cache(path) -> np.ndarray:
    """The reference's per-scan mask cache (``np.save`` of the (nx, ny) instance map,
    semantic_kitti_mask_dataset.py:121-137)."""
    with open(str(path), 'rb') as f:
        return np.load(f)


# ---------------------------------------------------------------------------------------------------------
# host readers of the KITTI object distribution (plain numpy; kitti_dataset.py)
# ---------------------------------------------------------------------------------------------------------
def read_kitti_label(path) -> dict:
    """``label_2/NNNNNN.txt`` → the camera-frame labels as arrays over the n objects that are not DontCare
    (kitti_dataset.py:157-176): ``type`` (n) int64 KittiType codes (indices into ``rasterize.KITTI_TYPES``), ``truncated``
    (n), ``occluded`` (n) int64, ``alpha`` (n), ``bbox`` (n, 4), ``dimensions`` (n, 3) in the file's order, ``location``
    (n, 3) in the camera frame, ``rotation_y`` (n)."""
    from .rasterize import KITTI_TYPES
    rows, types = [], []
    with open(str(path), 'r') as f:
        for line in f:
            content = line.strip().split(' ')
            if content == ['']:
                continue
            if content[0] not in KITTI_TYPES:
                raise ValueError(f'{path}: unknown object type {content[0]!r}')
            if content[0] == 'DontCare':
                continue
            types.append(KITTI_TYPES.index(content[0]))
            rows.append([float(v) for v in content[1:15]])
    a = np.array(rows, dtype=np.float64).reshape(-1, 14)
    return {'type': np.array(types, dtype=np.int64), 'truncated': a[:, 0], 'occluded': a[:, 1].astype(np.int64),
            'alpha': a[:, 2], 'bbox': a[:, 3:7], 'dimensions': a[:, 7:10], 'location': a[:, 10:13], 'rotation_y': a[:, 13]}


def read_kitti_calib(path) -> dict:
    """``calib/NNNNNN.txt`` → ``{'P0' … 'P3', 'R0_rect', 'Tr_velo_to_cam', 'Tr_imu_to_velo'}``, every matrix completed
    to 4 x 4 as kitti_dataset.py:122-155 completes it (a last row 0 0 0 1; ``R0_rect`` in the upper-left 3 x 3)."""
    calib = {}
    with open(str(path), 'r') as f:
        for line in f:
            if ':' not in line:
                continue
            k, v = line.split(':', 1)
            vals = np.array(v.split(), dtype=np.float64)
            m = np.eye(4)
            if k.strip() == 'R0_rect':
                m[:3, :3] = vals[:9].reshape(3, 3)
            else:
                m[:3, :] = vals[:12].reshape(3, 4)
            calib[k.strip()] = m
    return calib


def kitti_labels_to_velodyne(labels: dict, calib: dict) -> dict:
    """Camera-frame labels → velodyne-frame labels (kitti_dataset.py:181-195): ``dimensions[[2, 0, 1]]`` = length, width,
    height; location through ``inv(Tr_velo_to_cam)``; ``yaw = -rotation_y - pi / 2`` wrapped with ``arctan2``.  The result
    keeps the other fields and adds ``boxes`` (n, 7) f64 [x, y, z, l, w, h, yaw], the rasteriser's table."""
    c2v = np.linalg.inv(np.asarray(calib['Tr_velo_to_cam'], dtype=np.float64))
    n = labels['location'].shape[0]
    dimensions = labels['dimensions'][:, [2, 0, 1]]
    location = np.zeros((n, 3))
    yaw = np.zeros((n,))
    for k in range(n):
        tx, ty, tz = labels['location'][k]
        location[k] = (c2v @ np.array([tx, ty, tz, 1]).T)[:3]
        y = -labels['rotation_y'][k] - np.pi / 2
        yaw[k] = np.arctan2(np.sin(y), np.cos(y))
    out = dict(labels, dimensions=dimensions, location=location, rotation_y=yaw)
    out['boxes'] = np.concatenate([location, dimensions, yaw[:, None]], axis=1).reshape(-1, 7)
    return out


def is_difficulty_valid(occluded, truncated) -> np.ndarray:
    """kitti_transforms.py:48-61 over arrays: fully visible and truncated < 0.15, partly occluded and <= 0.3, or largely
    occluded and <= 0.5."""
    occ, trunc = np.asarray(occluded), np.asarray(truncated)
    return ((occ == 0) & (trunc < 0.15)) | ((occ == 1) & (trunc <= 0.3)) | ((occ == 2) & (trunc <= 0.5))


def object_range_mask(boxes, x_range, y_range) -> np.ndarray:
    """``ObjectRangeFilter`` (kitti_transforms.py:199-219): the boxes whose centre lies in the closed x and y ranges."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    return (x_range[0] <= boxes[:, 0]) & (boxes[:, 0] <= x_range[1]) & (y_range[0] <= boxes[:, 1]) & \
           (boxes[:, 1] <= y_range[1])


def select_labels(labels: dict, keep) -> dict:
    """The labels of a frame where ``keep`` (a boolean mask or an index array) says so, field by field."""
    return {k: v[keep] for k, v in labels.items()}


# ---------------------------------------------------------------------------------------------------------
# K14: instance map → targets on the device
# ---------------------------------------------------------------------------------------------------------
@torch.no_grad()
def instance_targets(instance_maps: torch.Tensor, num_queries: int, min_num_inst_pixels: int = 0,
                     packed: bool = False, check_overflow: bool = False):
    """``instance_maps`` (B, nx, ny) integer device tensor (0 = background) → ``(labels (B, Q) int64, masks)`` with
    ``masks`` (B, Q, ny, nx) f32 {0, 1} — the reference's batch contract — or, ``packed=True``, an
    :class:`ops.PackedMasks` of the B*Q maps that ``MaskBevModule.compute_loss`` accepts in their place.
    Instances are enumerated in ascending id order; ``check_overflow`` synchronises and raises ``IndexError`` like
    the reference when a scan holds more instances than ``num_queries``."""
    lib = _lib.load()
    if not instance_maps.is_cuda:
        raise MaskBevHipError('instance_targets needs a ROCm device tensor (no CPU fallback)')
    if instance_maps.dim() != 3:
        raise ValueError('instance_maps must be (B, nx, ny)')
    m = instance_maps.to(torch.int32).contiguous()
    b, nx, ny = m.shape
    dev = m.device
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ids = torch.empty((b, num_queries), dtype=torch.int32, device=dev)
    counts = torch.empty((b,), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib.mbv_instance_ids(m.data_ptr(), b, nx, ny, num_queries, int(min_num_inst_pixels), ids.data_ptr(),
                               counts.data_ptr(), status.data_ptr(), stream), 'mbv_instance_ids')
    if packed:
        words = torch.empty((b * num_queries, lib.mbv_packed_mask_words(ny, nx)), dtype=torch.int32, device=dev)
        check(lib.mbv_expand_instance_masks(m.data_ptr(), ids.data_ptr(), b, nx, ny, num_queries, None,
                                            words.data_ptr(), stream), 'mbv_expand_instance_masks')
        masks = ops.PackedMasks(words, ny, nx)
        masks.batch_shape = (b, num_queries)
    else:
        masks = torch.empty((b, num_queries, ny, nx), dtype=torch.float32, device=dev)
        check(lib.mbv_expand_instance_masks(m.data_ptr(), ids.data_ptr(), b, nx, ny, num_queries, masks.data_ptr(),
                                            None, stream), 'mbv_expand_instance_masks')
    labels = (torch.arange(num_queries, device=dev).view(1, -1) < counts.view(-1, 1)).to(torch.int64) * CAR
    if check_overflow:
        st = int(status.item())
        if st & 1:
            raise IndexError('a scan has more instances than num_queries '
                             '(semantic_kitti_transforms.py:78-80 indexes past num_pred)')
        if st & 2:
            raise MaskBevHipError('more than 4096 distinct instance ids in one scan')
    return labels, masks


class InstanceMapCollate:
    """Collate of ``(point_cloud (N, pc_dim) f32 array/tensor, instance_map (nx, ny) int array/tensor[, metadata])``
    samples into the batch ``MaskBevModule.training_step`` takes — the reference's ``MaskListCollate[Height]``
    (semantic_kitti_transforms.py:98-121) with the masks built on ``device`` by K14.  ``augmentation``: an
    ``augment.DeviceAugmentation`` (built with the grid's ranges and voxel size) applied on the device to the scans and,
    through K23c, to the maps before the targets are made; ``None``: none."""

    def __init__(self, num_queries: int, device, min_num_inst_pixels: int = 0, packed: bool = False, augmentation=None):
        self.num_queries, self.device = num_queries, torch.device(device)
        self.min_num_inst_pixels, self.packed = min_num_inst_pixels, packed
        self.augmentation = augmentation

    def __call__(self, batch: Sequence):
        pcs = [torch.as_tensor(s[0], dtype=torch.float32).to(self.device, non_blocking=True) for s in batch]
        maps = torch.stack([torch.as_tensor(np.asarray(s[1])).to(torch.int32) for s in batch]).to(self.device,
                                                                                                   non_blocking=True)
        if self.augmentation is not None:
            aug = self.augmentation.apply(pcs, instance_maps=maps)
            pcs, maps = aug.scans, aug.instance_maps
        labels, masks = instance_targets(maps, self.num_queries, self.min_num_inst_pixels, self.packed)
        if len(batch[0]) > 2:
            return pcs, (labels, masks), [s[2] for s in batch]
        return pcs, (labels, masks)


class SceneCollate:
    """Collate of ``(point_cloud (N, pc_dim) f32 array/tensor, scene[, metadata])`` samples with ``scene = (points list,
    inst list, transforms (S, 4, 4) f64, centre_inst or None)`` — the labelled scans around the sample's scan and the
    transforms that take them into its frame — into the batch ``MaskBevModule.training_step`` takes.  Beside
    :class:`InstanceMapCollate`: instead of a cached instance map, the scene is rasterised on ``device`` (K22,
    ``rasterize.SemanticKittiRasterizer``) and the maps go to K14, so no mask cache is needed and a point-level
    augmentation of the scene can come first: ``augmentation`` (an ``augment.DeviceAugmentation``, ``None``: none) runs on
    the scans (K23a / b) and its flips and rotations are folded into the scene's transforms, ``diag(A, 1, 1) @ tf``, so the
    map is rasterised from the rotated scene itself and no map is warped."""

    def __init__(self, rasterizer, num_queries: int, device, min_num_inst_pixels: int = 0, packed: bool = False,
                 augmentation=None):
        self.rasterizer, self.num_queries, self.device = rasterizer, num_queries, torch.device(device)
        self.min_num_inst_pixels, self.packed = min_num_inst_pixels, packed
        self.augmentation = augmentation

    def _up(self, t, dtype=None):
        t = torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t)
        if dtype is not None:
            t = t.to(dtype)
        elif t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float32)
        return t.to(self.device, non_blocking=True)

    def __call__(self, batch: Sequence):
        pcs = [torch.as_tensor(s[0], dtype=torch.float32).to(self.device, non_blocking=True) for s in batch]
        scene_tfs = [s[1][2] for s in batch]
        if self.augmentation is not None:
            aug = self.augmentation.apply(pcs, scene_transforms=scene_tfs)
            pcs, scene_tfs = aug.scans, aug.scene_transforms
        scenes = []
        for s, transforms in zip(batch, scene_tfs):
            points, inst, _, centre = s[1]
            scenes.append(([self._up(p) for p in points],
                           [self._up(np.asarray(i).astype(np.int64) if not isinstance(i, torch.Tensor) else i, torch.int32)
                            for i in inst], transforms,
                           None if centre is None else
                           self._up(np.asarray(centre).astype(np.int64) if not isinstance(centre, torch.Tensor) else centre,
                                    torch.int32)))
        maps = self.rasterizer.rasterize_batch(scenes)
        labels, masks = instance_targets(maps, self.num_queries, self.min_num_inst_pixels, self.packed)
        if len(batch[0]) > 2:
            return pcs, (labels, masks), [s[2] for s in batch]
        return pcs, (labels, masks)


class BankSceneCollate:
    """:class:`SceneCollate` on scene banks that stay on the device (``scene_bank.SceneBank``, K34): samples are
    ``(point_cloud (N, pc_dim) f32 array/tensor, (sequence key, scan_indices, transforms (S, 4, 4) f64, centre scan or
    None)[, metadata])`` and ``banks`` maps a sequence key to its bank.  Nothing of a scene crosses PCIe but its indices and
    matrices: the augmentation runs on the scans and folds its flips and rotations into the scene transforms as there, then
    every sequence present in the batch (a batch may mix them) takes one ``rasterize_bank`` call, and the maps go to K14."""

    def __init__(self, rasterizer, banks, num_queries: int, device, min_num_inst_pixels: int = 0, packed: bool = False,
                 augmentation=None):
        self.rasterizer, self.banks, self.num_queries, self.device = rasterizer, banks, num_queries, torch.device(device)
        self.min_num_inst_pixels, self.packed = min_num_inst_pixels, packed
        self.augmentation = augmentation

    def __call__(self, batch: Sequence):
        pcs = [torch.as_tensor(s[0], dtype=torch.float32).to(self.device, non_blocking=True) for s in batch]
        scene_tfs = [s[1][2] for s in batch]
        if self.augmentation is not None:
            aug = self.augmentation.apply(pcs, scene_transforms=scene_tfs)
            pcs, scene_tfs = aug.scans, aug.scene_transforms
        groups = {}
        for b, s in enumerate(batch):
            groups.setdefault(s[1][0], []).append(b)
        maps = None
        for key, members in groups.items():
            scenes = [(batch[b][1][1], scene_tfs[b], batch[b][1][3]) for b in members]
            if len(groups) == 1:
                maps = self.rasterizer.rasterize_bank(self.banks[key], scenes)
                break
            if maps is None:
                maps = torch.empty((len(batch), self.rasterizer.nx, self.rasterizer.ny), dtype=torch.int32, device=self.device)
            maps[torch.as_tensor(members, device=self.device)] = self.rasterizer.rasterize_bank(self.banks[key], scenes)
        labels, masks = instance_targets(maps, self.num_queries, self.min_num_inst_pixels, self.packed)
        if len(batch[0]) > 2:
            return pcs, (labels, masks), [s[2] for s in batch]
        return pcs, (labels, masks)


class BoxCollate:
    """Collate of ``(point_cloud (N, pc_dim) f32 array/tensor, boxes (n, 7) f64 [cx, cy, cz, l, w, h, theta][, metadata])``
    samples into the batch ``MaskBevModule.training_step`` takes — the reference's ``FrameMaskListCollate``
    (kitti_transforms.py:117-128) behind ``FrameScanToMask`` and ``FrameMasksToLabelInstanceMasks``, with the boxes
    rasterised on ``device`` (K24; ``rasterizer``: a ``rasterize.KittiRasterizer`` or ``WaymoRasterizer``, every box of a
    sample counts as a vehicle) and the maps expanded by K14.  Every real instance gets the label ``CAR`` = 1:
    ``KittiType.Car + 1`` there, ``TYPE_VEHICLE`` for Waymo.  ``augmentation`` (an ``augment.DeviceAugmentation``, ``None``:
    none) runs on the scans (K23) and moves the boxes on the host before they are rasterised.  ``object_range`` =
    ``(x_range, y_range)`` drops the boxes whose centre has left the closed ranges AFTER the augmentation, where the
    reference's pipeline has its ObjectRangeFilter (kitti_data_module.py:84-86); ``None``: no such filter."""

    def __init__(self, rasterizer, num_queries: int, device, min_num_inst_pixels: int = 0, packed: bool = False,
                 augmentation=None, object_range=None):
        self.rasterizer, self.num_queries, self.device = rasterizer, num_queries, torch.device(device)
        self.min_num_inst_pixels, self.packed = min_num_inst_pixels, packed
        self.augmentation, self.object_range = augmentation, object_range
        if getattr(rasterizer, 'device', None) is None:
            rasterizer.device = self.device

    def __call__(self, batch: Sequence):
        pcs = [torch.as_tensor(s[0], dtype=torch.float32).to(self.device, non_blocking=True) for s in batch]
        boxes = [np.asarray(s[1].detach().cpu().numpy() if isinstance(s[1], torch.Tensor) else s[1],
                            dtype=np.float64).reshape(-1, 7) for s in batch]
        if self.augmentation is not None:
            aug = self.augmentation.apply(pcs, boxes=boxes)
            pcs, boxes = aug.scans, aug.boxes
        if self.object_range is not None:
            boxes = [b[object_range_mask(b, *self.object_range)] for b in boxes]
        maps = self.rasterizer.rasterize_batch(boxes)
        labels, masks = instance_targets(maps, self.num_queries, self.min_num_inst_pixels, self.packed)
        if len(batch[0]) > 2:
            return pcs, (labels, masks), [s[2] for s in batch]
        return pcs, (labels, masks)
