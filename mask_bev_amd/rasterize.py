"""SemanticKITTI scene → instance-id map on the device (K22, csrc/rasterize.hip): what the reference's
``SemanticKittiRasterizer`` (mask_bev/datasets/semantic_kitti/semantic_kitti_rasterizer.py) does on the host with numpy
and one OpenCV call pair per instance, and therefore caches on disk.  The map is the input of ``batch.instance_targets``
(K14), so a training step needs neither the reference's cache nor OpenCV, and a scene can be rasterised after a
point-level augmentation: ``augment.DeviceAugmentation`` (K23) folds its flips and rotations into ``transforms``.

``rasterize_bank`` (K34) does the same for a whole batch in one native call on a ``scene_bank.SceneBank`` — the labelled points
of a sequence, kept on the device — without copying a scan: what the launcher uses for ``semantic_kitti_targets: scenes``.

Where two closed-and-opened instances claim one cell the HIGHEST ID wins (the reference paints in the hash order of a
Python set); everywhere else the map equals the reference's.  Not covered: the approximate scene branch.

KITTI / Waymo box tables → instance-id maps (K24, csrc/box_rasterize.hip): ``KittiRasterizer`` and ``WaymoRasterizer``
(mask_bev/datasets/kitti/kitti_rasterizer.py, mask_bev/datasets/waymo/waymo_rasterizer.py).  The corners of the few dozen
boxes of a frame are made on the host by ``box_vertices`` — the reference's f64 expressions and its ``np.intp``
truncation, so identical to the last bit — and one launch paints the whole batch by the fill rule of
include/maskbev_hip.h: a cell belongs to a box iff its integer point lies inside or on the closed quadrilateral of the
truncated corners, or on the integer line between two consecutive corners; a later box overwrites an earlier one.
Equality with ``cv2.drawContours(..., -1)`` is NOT pinned by any test: OpenCV draws the outline with its own line iterator
and fills spans in 16-bit fixed point, so tie cells on an edge may differ — boundary cells of a target mask only.
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

    def bank_tables(self, bank, scenes: Sequence):
        """``rasterize_bank``'s scenes as the host tables of ``ops_rasterize.rasterize_bank``: (seg_start, seg_count,
        sample_seg_offsets, transforms, centre_start, centre_count)."""
        offsets, n_scans = bank.scan_offsets, len(bank)
        index, tfs, c_start, c_count = [], [], [], []
        for scans, transforms, *rest in scenes:
            scans = np.asarray(scans, dtype=np.int64).reshape(-1)
            tf = np.asarray(transforms.detach().cpu().numpy() if isinstance(transforms, torch.Tensor) else transforms,
                            dtype=np.float64).reshape(-1, 4, 4)
            if tf.shape[0] != scans.size:
                raise ValueError(f'{tf.shape[0]} transforms for {scans.size} scans')
            if scans.size and (scans.min() < 0 or scans.max() >= n_scans):
                raise IndexError(f'a scene names a scan outside 0 … {n_scans - 1}')
            centre = rest[0] if rest else None
            if self.remove_unseen:
                if centre is None:
                    raise ValueError('remove_unseen=True needs the centre scan of every scene')
                if not 0 <= int(centre) < n_scans:
                    raise IndexError(f'centre scan {centre} outside 0 … {n_scans - 1}')
                c_start.append(offsets[int(centre)])
                c_count.append(offsets[int(centre) + 1] - offsets[int(centre)])
            else:
                c_start.append(0)
                c_count.append(-1)
            index.append(scans)
            tfs.append(tf)
        tf = np.concatenate(tfs)
        if not np.allclose(tf[:, 3, :], [0., 0., 0., 1.], rtol=0, atol=1e-12):
            raise ValueError('the last row of every transform must be 0 0 0 1')
        scans = np.concatenate(index)
        return (offsets[scans], offsets[scans + 1] - offsets[scans], np.concatenate([[0], np.cumsum([len(i) for i in index])]),
                tf, np.asarray(c_start, dtype=np.int64), np.asarray(c_count, dtype=np.int64))

    @torch.no_grad()
    def rasterize_bank(self, bank, scenes: Sequence, out: Optional[torch.Tensor] = None,
                       check_overflow: bool = False) -> torch.Tensor:
        """The scenes of a whole batch from a ``scene_bank.SceneBank`` that lives on the device, in one native call (K34):
        ``scenes`` is a list of ``(scan_indices (k), transforms (k, 4, 4) f64, centre_scan or None)`` — the scans of the bank
        that make up the sample's scene, the matrices that take them into its frame (``SceneBank.scene``) and, for
        ``remove_unseen``, the scan whose labels name the instances.  The bank is read in place: no scan is copied or
        concatenated.  Map b equals ``rasterize`` on the listed scans, bit for bit.  → (B, nx, ny) int32 on the device.
        ``check_overflow`` reads the B status words in one host copy and raises as ``rasterize`` does."""
        if len(scenes) == 0:
            raise ValueError('empty batch')
        if not bank.points.is_cuda:
            raise MaskBevHipError('SemanticKittiRasterizer needs ROCm device tensors (no CPU fallback)')
        maps, status, _ = ops_rasterize.rasterize_bank(
            bank.points, bank.inst, *self.bank_tables(bank, scenes), self.x_range, self.y_range, self.z_range,
            self.voxel_size, self.nx, self.ny, self.morph_kernel_size, self.min_points, self.max_instances, out=out)
        if check_overflow:
            st = status.cpu().numpy()
            if (st & 1).any():
                raise IndexError(f'scene {int(np.flatnonzero(st & 1)[0])} holds more than max_instances = '
                                 f'{self.max_instances} instances')
            if (st & 2).any():
                raise MaskBevHipError('an instance id outside 0 … 65535 (SemanticKITTI ids are 16 bits)')
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


# ---------------------------------------------------------------------------------------------------------
# K24: box tables
# ---------------------------------------------------------------------------------------------------------
KITTI_TYPES = ('Car', 'Van', 'Truck', 'Pedestrian', 'Person_sitting', 'Cyclist', 'Tram', 'Misc', 'DontCare')   # KittiType
KITTI_CAR, KITTI_CAR_LIKE = 0, (0, 1, 2)         # Car; Car, Van, Truck: all painted as Car (kitti_rasterizer.py:28-34)
WAYMO_TYPE_VEHICLE = 1                           # torch_waymo's Type.TYPE_VEHICLE
MAX_VERTEX = 1 << 20                             # |cell coordinate| the kernel's 64-bit products are sized for


def box_vertices(boxes, x_range, y_range, nx: int, ny: int) -> np.ndarray:
    """``boxes`` (n, 7) f64 [cx, cy, cz, l, w, h, theta] → (n, 4, 2) int32 corners in cell coordinates (x-cell, y-cell):
    ``_box_to_points``, ``_map_to`` and the ``np.intp`` truncation toward zero of kitti_rasterizer.py:49-52,60-80
    (waymo_rasterizer.py has the identical lines), expression by expression in f64, one box at a time as there."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    if not np.all(np.isfinite(boxes)):
        raise ValueError('box_vertices: a box has a non-finite entry')
    out = np.zeros((boxes.shape[0], 4, 2), dtype=np.int32)
    for k, (cx, cy, _, l, w, _, theta) in enumerate(boxes):
        points = np.zeros((4, 2))
        dl, dw = l / 2, w / 2
        d = np.array([np.cos(theta), np.sin(theta)])
        phi = theta + np.pi / 2
        d_bar = np.array([np.cos(phi), np.sin(phi)])
        points[0, :] = d * dl + d_bar * dw
        points[1, :] = - d * dl + d_bar * dw
        points[2, :] = - d * dl - d_bar * dw
        points[3, :] = d * dl - d_bar * dw
        points += [cx, cy]
        points[:, 0] = (points[:, 0] - x_range[0]) / (x_range[1] - x_range[0]) * (nx - 0) + 0
        points[:, 1] = (points[:, 1] - y_range[0]) / (y_range[1] - y_range[0]) * (ny - 0) + 0
        if not np.all(np.abs(points) <= MAX_VERTEX):                 # also catches the NaN of a zero-width range
            raise ValueError(f'box_vertices: box {k} has a corner beyond ±2^20 cells')
        out[k] = np.intp(points)
    return out


def boxes_from_cells(boxes: torch.Tensor, x_range, y_range, nx: int, ny: int) -> torch.Tensor:
    """The way back from ``box_vertices``' cell coordinates, taken at cell centres: K25's boxes (r, 5) [cx, cy, dx, dy, theta]
    in cell units (cell index i along x covers [i, i + 1) of ``(x - x_lo) / (x_hi - x_lo) * nx``, so its centre is i + 0.5)
    → (r, 5) float32 [x, y, l, w, yaw] in metres in the velodyne frame, yaw as ``box_vertices`` and
    ``batch.kitti_labels_to_velodyne`` have it (the direction of the length, counter-clockwise, in [-pi, pi)), l >= w.
    A box that K24 paints and K25 fits lands on itself up to the rasterisation.  On a grid whose cells are not square the
    axis direction is scaled per axis and the extents by the length of the scaled unit vectors.  A box of zeros (an empty
    mask) stays a box of zeros at the grid's origin cell.  Runs where ``boxes`` lives, in float64."""
    b = boxes.to(torch.float64)
    sx, sy = (float(x_range[1]) - float(x_range[0])) / nx, (float(y_range[1]) - float(y_range[0])) / ny
    c, s = torch.cos(b[:, 4]), torch.sin(b[:, 4])
    x = float(x_range[0]) + (b[:, 0] + 0.5) * sx
    y = float(y_range[0]) + (b[:, 1] + 0.5) * sy
    length = b[:, 2] * torch.hypot(c * sx, s * sy)
    width = b[:, 3] * torch.hypot(s * sx, c * sy)
    yaw = torch.atan2(s * sy, c * sx)
    swap = width > length
    yaw = torch.where(swap, yaw + np.pi / 2, yaw)
    yaw = torch.atan2(torch.sin(yaw), torch.cos(yaw))
    l, w = torch.where(swap, width, length), torch.where(swap, length, width)
    return torch.stack([x, y, l, w, yaw], dim=1).to(torch.float32)


class _BoxRasterizer:
    """What the two box rasterisers share: the reference's constructor keywords and grid sizes, the upload and the launch."""

    def __init__(self, x_range, y_range, z_range, voxel_size: float, remove_unseen: bool = False, min_points: int = 1,
                 device=None):
        if not voxel_size > 0:
            raise ValueError('voxel_size must be positive')
        self.x_range, self.y_range, self.z_range = tuple(x_range), tuple(y_range), tuple(z_range)
        self.voxel_size = voxel_size
        self.nx = int((x_range[1] - x_range[0]) / voxel_size)          # the reference's expression (:23-24)
        self.ny = int((y_range[1] - y_range[0]) / voxel_size)
        if self.nx < 1 or self.ny < 1:
            raise ValueError('empty grid')
        self.remove_unseen, self.min_points = bool(remove_unseen), int(min_points)
        self.device = None if device is None else torch.device(device)

    def _device(self) -> torch.device:
        dev = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
        if dev.type != 'cuda':
            raise MaskBevHipError(f'{type(self).__name__} needs a ROCm device (no CPU fallback), got {dev}')
        return dev

    def _paint(self, frames: Sequence) -> torch.Tensor:
        """``frames``: per frame ``(boxes (k, 7), ids (k))`` of the boxes to paint, in paint order → (B, nx, ny) int32."""
        if len(frames) == 0:
            raise ValueError('empty batch')
        dev = self._device()
        verts = np.concatenate([box_vertices(b, self.x_range, self.y_range, self.nx, self.ny) for b, _ in frames])
        ids = np.concatenate([np.asarray(i, dtype=np.int32).reshape(-1) for _, i in frames])
        offsets = np.concatenate([[0], np.cumsum([len(i) for _, i in frames])])
        return ops_rasterize.rasterize_boxes(torch.from_numpy(verts).to(dev, non_blocking=True),
                                             torch.from_numpy(ids).to(dev, non_blocking=True), offsets, self.nx, self.ny)

    @staticmethod
    def _rows(boxes) -> np.ndarray:
        if isinstance(boxes, torch.Tensor):
            boxes = boxes.detach().cpu().numpy()
        return np.asarray(boxes, dtype=np.float64).reshape(-1, 7)


class KittiRasterizer(_BoxRasterizer):
    """mask_bev/datasets/kitti/kitti_rasterizer.py.  Car, Van and Truck labels are painted (all as Car); a label's id is its
    index among those labels plus 1, counted BEFORE the range skip.  The range skip is the reference's line (:46-48) as it
    stands: it tests ``x_range[0] <= cx``, ``y_range[0] <= cy`` and the TRUTHINESS of the two upper bounds — a centre beyond
    an upper bound is still painted where it reaches the grid, and an upper bound of 0 skips every box (SURVEY.md
    Appendix B).  ``remove_unseen`` and ``min_points`` are accepted and unused, as there."""

    def _select(self, boxes, types=None):
        boxes = self._rows(boxes)
        if types is not None:
            types = np.asarray(types).reshape(-1)
            if types.shape[0] != boxes.shape[0]:
                raise ValueError('one type per box expected')
            boxes = boxes[np.isin(types, KITTI_CAR_LIKE)]
        ids = np.arange(1, boxes.shape[0] + 1, dtype=np.int32)
        keep = np.array([bool(self.x_range[0] <= b[0] and self.x_range[1] and self.y_range[0] <= b[1] and self.y_range[1])
                         for b in boxes], dtype=bool).reshape(-1)
        return boxes[keep], ids[keep]

    @torch.no_grad()
    def rasterize_batch(self, boxes: Sequence, types: Optional[Sequence] = None) -> torch.Tensor:
        """``boxes``: per frame an (n_b, 7) f64 array [cx, cy, cz, l, w, h, theta] in the velodyne frame (n_b = 0: an all-zero
        map); ``types``: per frame the (n_b) KittiType codes (indices into ``KITTI_TYPES``), ``None``: every box is car-like.
        → (B, nx, ny) int32 on the device, ready for ``batch.instance_targets``."""
        if types is not None and len(types) != len(boxes):
            raise ValueError('one type array per frame expected')
        return self._paint([self._select(b, None if types is None else types[k]) for k, b in enumerate(boxes)])

    def get_mask(self, frame) -> dict:
        """The reference's call, for drop-in use: ``frame.labels`` with ``type``, ``location``, ``dimensions`` and
        ``rotation_y`` → ``{KittiType.Car: (ny, nx) int32 device tensor}`` (a view of the (nx, ny) map)."""
        labels = list(frame.labels)
        boxes = np.array([[*l.location, *l.dimensions, l.rotation_y] for l in labels], dtype=np.float64).reshape(-1, 7)
        types = np.array([int(l.type) for l in labels], dtype=np.int64)
        return {KITTI_CAR: self.rasterize_batch([boxes], [types])[0].t()}


class WaymoRasterizer(_BoxRasterizer):
    """mask_bev/datasets/waymo/waymo_rasterizer.py: the ``TYPE_VEHICLE`` labels with ``num_lidar_points_in_box >=
    min_points``, in label order, id = index among them plus 1; no range skip.  Cells are indexed [y-cell][x-cell] as the
    reference's ``drawContours`` call indexes them.  The reference allocates that image as (nx, ny), which only fits a
    square grid; here the map always has the KITTI layout — (nx, ny) for K14, (ny, nx) from ``get_mask`` — so a non-square
    grid works too."""

    def _select(self, boxes, types=None, num_points=None):
        boxes = self._rows(boxes)
        keep = np.ones(boxes.shape[0], dtype=bool)
        if types is not None:
            keep &= np.asarray(types).reshape(-1) == WAYMO_TYPE_VEHICLE
        boxes = boxes[keep]
        if num_points is not None:
            boxes = boxes[np.asarray(num_points).reshape(-1)[keep] >= self.min_points]
        return boxes, np.arange(1, boxes.shape[0] + 1, dtype=np.int32)

    @torch.no_grad()
    def rasterize_batch(self, boxes: Sequence, types: Optional[Sequence] = None,
                        num_points: Optional[Sequence] = None) -> torch.Tensor:
        """``boxes``: per frame (n_b, 7) f64 [center_x, center_y, center_z, length, width, height, heading]; ``types`` /
        ``num_points``: per frame the (n_b) label types and ``num_lidar_points_in_box`` (``None``: every box is a vehicle /
        has enough points) → (B, nx, ny) int32 on the device."""
        for extra in (types, num_points):
            if extra is not None and len(extra) != len(boxes):
                raise ValueError('one type / point-count array per frame expected')
        return self._paint([self._select(b, None if types is None else types[k],
                                         None if num_points is None else num_points[k]) for k, b in enumerate(boxes)])

    def get_mask(self, frame) -> dict:
        """``frame.laser_labels`` with ``type``, ``num_lidar_points_in_box`` and ``box`` → ``{TYPE_VEHICLE: (ny, nx) int32
        device tensor}``."""
        labels = list(frame.laser_labels)
        boxes = np.array([[l.box.center_x, l.box.center_y, l.box.center_z, l.box.length, l.box.width, l.box.height,
                           l.box.heading] for l in labels], dtype=np.float64).reshape(-1, 7)
        types = np.array([int(l.type) for l in labels], dtype=np.int64)
        counts = np.array([l.num_lidar_points_in_box for l in labels], dtype=np.int64)
        return {WAYMO_TYPE_VEHICLE: self.rasterize_batch([boxes], [types], [counts])[0].t()}


__all__ = ['SemanticKittiRasterizer', 'scans_in_range', 'box_vertices', 'boxes_from_cells', 'KittiRasterizer', 'WaymoRasterizer',
           'KITTI_TYPES', 'KITTI_CAR', 'KITTI_CAR_LIKE', 'WAYMO_TYPE_VEHICLE']
