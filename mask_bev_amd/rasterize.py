"""SemanticKITTI scene → instance-id map on the device (K22, csrc/rasterize.hip): what the reference's
``SemanticKittiRasterizer`` (mask_bev/datasets/semantic_kitti/semantic_kitti_rasterizer.py) does on the host with numpy
and one OpenCV call pair per instance, and therefore caches on disk.  The map is the input of ``batch.instance_targets``
(K14), so a training step needs neither the reference's cache nor OpenCV, and a scene can be rasterised after a
point-level augmentation: ``augment.DeviceAugmentation`` (K23) folds its flips and rotations into ``transforms``.

Where two closed-and-opened instances claim one cell the HIGHEST ID wins (the reference paints in the hash order of a
Python set); everywhere else the map equals the reference's.  Not covered: the KITTI / Waymo box rasterisers
(``cv2.drawContours``), the approximate scene branch.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import ops_rasterize
from ._lib import MaskBevHipError

TensorList = Union[torch.Tensor, Sequence[torch.Tensor]]


def scans_in_range(poses: np.ndarray, centre: int, x_range, y_range, scaling: float = 2,
                   velo_to_cam: Optional[np.ndarray] = None) -> np.ndarray:
    """Indices of the scans of a sequence that make up the scene around scan ``centre``
    (semantic_kitti_mask_dataset.py:81-92, the non-approximate branch): the scans whose position, seen from the centre
    scan, lies strictly inside ``scaling`` times the x and y ranges.  ``poses`` (N, 4, 4) f64 as ``batch.read_poses``
    returns them; with ``velo_to_cam`` (``batch.read_calib(...)['velo_to_cam']``) they are taken to the velodyne frame
    first, ``inv(velo_to_cam) @ pose @ velo_to_cam``, as the reference does."""
    poses = np.asarray(poses, dtype=np.float64)
    if velo_to_cam is not None:
        v2c = np.asarray(velo_to_cam, dtype=np.float64)
        poses = np.linalg.inv(v2c) @ poses @ v2c
    pos = poses @ np.array([0., 0., 0., 1.])
    pos = np.hstack((pos[:, :3] / pos[:, 3].reshape((-1, 1)), np.ones((pos.shape[0], 1))))
    pos = (np.linalg.inv(poses[centre]) @ pos.T).T
    in_range = (scaling * x_range[0] < pos[:, 0]) & (pos[:, 0] < x_range[1] * scaling) & \
               (scaling * y_range[0] < pos[:, 1]) & (pos[:, 1] < y_range[1] * scaling)
    return np.flatnonzero(in_range)


class SemanticKittiRasterizer:
    """The reference's constructor keywords and defaults, plus ``max_instances`` (slots of per-instance bit images in the
    workspace: nx * ceil(ny / 32) * 4 bytes each)."""

    def __init__(self, x_range, y_range, z_range, voxel_size: float, remove_unseen: bool = False, min_points: int = 1,
                 morph_kernel_size: int = 9, max_instances: int = 1024):
        k = int(morph_kernel_size)
        if k != morph_kernel_size or k % 2 == 0 or not 1 <= k <= 31:
            raise ValueError(f'morph_kernel_size must be odd and in 1 … 31, got {morph_kernel_size}')
        if not 1 <= int(max_instances) <= 65535:
            raise ValueError(f'max_instances must be in 1 … 65535, got {max_instances}')
        if not voxel_size > 0:
            raise ValueError('voxel_size must be positive')
        self.x_range, self.y_range, self.z_range = tuple(x_range), tuple(y_range), tuple(z_range)
        self.voxel_size = voxel_size
        self.nx = int((x_range[1] - x_range[0]) / voxel_size)          # the reference's expression (:29-30)
        self.ny = int((y_range[1] - y_range[0]) / voxel_size)
        if self.nx < 1 or self.ny < 1:
            raise ValueError('empty grid')
        self.remove_unseen, self.min_points = bool(remove_unseen), int(min_points)
        self.morph_kernel_size, self.max_instances = k, int(max_instances)

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _concat(points: TensorList, inst: TensorList, offsets):
        if isinstance(points, torch.Tensor):
            if isinstance(inst, (list, tuple)):
                raise ValueError('points concatenated but inst a list')
            if offsets is None:
                offsets = [0, points.shape[0]]
            return points, inst, offsets
        if len(points) != len(inst):
            raise ValueError('points and inst lists differ in length')
        for t in list(points) + list(inst):
            if not t.is_cuda:
                raise MaskBevHipError('SemanticKittiRasterizer needs ROCm device tensors (no CPU fallback)')
        counts = [int(p.shape[0]) for p in points]
        if [int(i.numel()) for i in inst] != counts:
            raise ValueError('a scan has a different number of points and labels')
        offsets = np.concatenate([[0], np.cumsum(counts)]).tolist()
        return torch.cat(list(points)), torch.cat([i.reshape(-1) for i in inst]), offsets

    @torch.no_grad()
    def rasterize(self, points: TensorList, inst: TensorList, transforms, centre_inst: Optional[torch.Tensor] = None,
                  scan_offsets=None, check_overflow: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``points`` / ``inst``: lists of per-scan device tensors ((n, 3 | 4) f32 or f64, (n) integer), or already
        concatenated with ``scan_offsets`` (S + 1); ``transforms`` (S, 4, 4) f64 array or tensor taking each scan into the
        centre scan's frame.  Returns the (nx, ny) int32 instance map on the device.  ``check_overflow`` synchronises and
        raises ``IndexError`` (more than ``max_instances`` instances) / ``MaskBevHipError`` (an id outside 0 … 65535)."""
        if self.remove_unseen and centre_inst is None:
            raise ValueError('remove_unseen=True needs the centre scan\'s instance labels (centre_inst)')
        points, inst, scan_offsets = self._concat(points, inst, scan_offsets)
        for t in (points, inst, centre_inst):
            if t is not None and not t.is_cuda:
                raise MaskBevHipError('SemanticKittiRasterizer needs ROCm device tensors (no CPU fallback)')
        dev = points.device
        tf = np.ascontiguousarray(transforms.detach().cpu().numpy() if isinstance(transforms, torch.Tensor) else transforms,
                                  dtype=np.float64).reshape(-1, 4, 4)
        # rigid transforms only: the kernel reads the upper 3 x 4 block (a product of inverses may leave 1e-17 in the last row)
        if not np.allclose(tf[:, 3, :], [0., 0., 0., 1.], rtol=0, atol=1e-12):
            raise ValueError('the last row of every transform must be 0 0 0 1')
        if isinstance(scan_offsets, torch.Tensor):
            offs = scan_offsets.to(device=dev, dtype=torch.int32)
        else:
            offs = torch.tensor([int(v) for v in scan_offsets], dtype=torch.int32, device=dev)
        if offs.numel() != tf.shape[0] + 1:
            raise ValueError(f'{tf.shape[0]} transforms for {offs.numel() - 1} scans')
        if points.dtype not in (torch.float32, torch.float64):
            points = points.to(torch.float32)
        centre = centre_inst.reshape(-1).to(torch.int32) if self.remove_unseen else None
        m, status, _ = ops_rasterize.rasterize_scene(
            points, inst.reshape(-1).to(torch.int32), offs, torch.from_numpy(tf).to(dev), centre, self.x_range,
            self.y_range, self.z_range, self.voxel_size, self.nx, self.ny, self.morph_kernel_size, self.min_points,
            self.max_instances, out=out)
        if check_overflow:
            st = int(status.item())
            if st & 1:
                raise IndexError(f'the scene holds more than max_instances = {self.max_instances} instances')
            if st & 2:
                raise MaskBevHipError('an instance id outside 0 … 65535 (SemanticKITTI ids are 16 bits)')
        return m

    def rasterize_batch(self, scenes: Sequence, check_overflow: bool = False) -> torch.Tensor:
        """``scenes``: a list of ``(points, inst, transforms[, centre_inst])`` → (B, nx, ny) int32, ready for
        ``batch.instance_targets``."""
        if len(scenes) == 0:
            raise ValueError('empty batch')
        first = scenes[0][0]
        dev = first.device if isinstance(first, torch.Tensor) else first[0].device
        if dev.type != 'cuda':
            raise MaskBevHipError('SemanticKittiRasterizer needs ROCm device tensors (no CPU fallback)')
        maps = torch.empty((len(scenes), self.nx, self.ny), dtype=torch.int32, device=dev)
        for b, scene in enumerate(scenes):
            self.rasterize(scene[0], scene[1], scene[2], scene[3] if len(scene) > 3 else None,
                           check_overflow=check_overflow, out=maps[b])
        return maps

    def get_mask_around(self, scan, scene, device=None) -> torch.Tensor:
        """The reference's call, for drop-in use: ``scan.velo_to_inv_pose``, ``scan.inst_label``, ``scene.point_cloud``
        (world frame, f64 — passed through as it is; the whole scene is one "scan" whose transform is
        ``scan.velo_to_inv_pose``), ``scene.inst_label``.  Uploads to ``device`` (default: the current ROCm device)."""
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        pc = np.ascontiguousarray(scene.point_cloud)
        if pc.dtype not in (np.float32, np.float64):
            pc = pc.astype(np.float64)
        inst = torch.from_numpy(np.asarray(scene.inst_label).astype(np.int64)).to(dev)
        centre = None
        if self.remove_unseen:
            centre = torch.from_numpy(np.asarray(scan.inst_label).astype(np.int64)).to(dev)
        return self.rasterize(torch.from_numpy(pc).to(dev), inst, np.asarray(scan.velo_to_inv_pose, dtype=np.float64)[None],
                              centre)


__all__ = ['SemanticKittiRasterizer', 'scans_in_range']
