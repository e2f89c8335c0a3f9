"""The scene bank of a SemanticKITTI sequence: the instance-labelled points of every scan, kept in device memory so that
``rasterize.SemanticKittiRasterizer.rasterize_bank`` (K34, csrc/rasterize.hip) can rasterise the scenes of a whole batch
from it in place.  With it the launcher trains and tests on the dataset as downloaded (``velodyne/``, ``labels/``,
``poses.txt``, ``calib.txt``): no mask cache, none of the reference's host rasterisation.

A sample's scene is the labelled points of the scans around its scan (``rasterize.scans_in_range``, often hundreds), each
taken into its frame by ``inv(pose_v[centre]) @ pose_v[s]``.  The bank stores every scan's points ONCE, in the scan's own
frame; a scene is a list of scan indices — ranges of the bank — and as many 4 x 4 matrices.

Memory (an ESTIMATE from the dataset's published proportions, not a measurement): cars are a few per cent of the about
120 000 points of a scan, so some thousand points a scan at 16 bytes each (12 of coordinates, 4 of id): tens of MB for a
sequence of 4 500 scans, a few GB at most for all ten training sequences.  ``SceneBank.load`` prints the real number of bytes
of every bank it puts on a device."""
from __future__ import annotations

import pathlib
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .batch import read_semantic_kitti_label, read_velodyne_bin
from .rasterize import scans_in_range

CAR_RAW = 10                         # the raw SemanticKITTI id of a (static) car; 252, moving car, is another class there
BUILD_COMMAND = 'python train_mask_bev_amd.py --config CONFIG --data-root ROOT --build-scene-bank'


class SceneBank:
    """``points`` (n, 3) f32, every scan in its own frame; ``inst`` (n) int32 instance ids, never 0; ``scan_offsets``
    (S + 1) int64: scan s owns ``points[scan_offsets[s]:scan_offsets[s + 1]]``; ``classes``: the raw semantic ids kept.
    ``points`` and ``inst`` may be numpy arrays (a bank just built) or tensors (a loaded bank: on the device it was loaded
    to, where they stay); ``scan_offsets`` is always on the host, and next to the points as ``device_offsets``."""

    def __init__(self, points, inst, scan_offsets, classes=(CAR_RAW,), device=None):
        self.scan_offsets = np.ascontiguousarray(scan_offsets, dtype=np.int64).reshape(-1)
        self.classes = tuple(int(c) for c in np.asarray(classes).reshape(-1))
        if isinstance(points, torch.Tensor):
            self.points, self.inst = points.to(torch.float32).reshape(-1, 3), inst.to(torch.int32).reshape(-1)
        else:
            self.points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3))
            self.inst = torch.from_numpy(np.ascontiguousarray(inst, dtype=np.int32).reshape(-1))
        if device is not None:
            self.points, self.inst = self.points.to(device), self.inst.to(device)
        self.points, self.inst = self.points.contiguous(), self.inst.contiguous()
        n = self.points.shape[0]
        if (self.inst.numel() != n or self.scan_offsets.size < 1 or self.scan_offsets[0] != 0 or self.scan_offsets[-1] != n
                or (np.diff(self.scan_offsets) < 0).any()):
            raise ValueError('SceneBank: scan_offsets must ascend from 0 to the number of points, one label per point')
        self.device_offsets = torch.from_numpy(self.scan_offsets).to(self.points.device)

    def __len__(self) -> int:
        """The number of scans."""
        return self.scan_offsets.size - 1

    @property
    def device(self) -> torch.device:
        return self.points.device

    @property
    def nbytes(self) -> int:
        return self.points.numel() * 4 + self.inst.numel() * 4 + self.scan_offsets.nbytes

    def scan(self, s: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(points, inst) of scan ``s``: views of the bank."""
        a, b = int(self.scan_offsets[s]), int(self.scan_offsets[s + 1])
        return self.points[a:b], self.inst[a:b]

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def default_path(root, seq) -> pathlib.Path:
        return pathlib.Path(root).expanduser() / 'sequences' / f'{int(seq):02d}' / 'instance_points.npz'

    @classmethod
    def build(cls, scan_paths: Sequence, label_paths: Sequence, classes=(CAR_RAW,)) -> 'SceneBank':
        """Every scan of a sequence, in scan order: the points whose raw semantic id (``word & 0xFFFF``) is in ``classes`` and
        whose instance id (``word >> 16``) is not 0, in file order — what ``SemanticKittiDataset(included_labels=[CAR])``
        leaves with a non-zero ``inst_label`` there."""
        if len(scan_paths) != len(label_paths):
            raise ValueError('SceneBank.build: one label file per scan expected')
        pts, ids, counts = [], [], []
        for scan_path, label_path in zip(scan_paths, label_paths):
            if not pathlib.Path(label_path).exists():
                raise FileNotFoundError(f'SceneBank.build: {scan_path} has no label file {label_path}')
            sem, inst = read_semantic_kitti_label(label_path)
            xyz = read_velodyne_bin(scan_path)[:, :3]
            if len(sem) != len(xyz):
                raise ValueError(f'SceneBank.build: {label_path} holds {len(sem)} labels for {len(xyz)} points')
            keep = np.isin(sem, classes) & (inst != 0)
            pts.append(xyz[keep])
            ids.append(inst[keep].astype(np.int32))
            counts.append(int(keep.sum()))
        return cls(np.concatenate(pts) if pts else np.zeros((0, 3), np.float32),
                   np.concatenate(ids) if ids else np.zeros((0,), np.int32), np.concatenate([[0], np.cumsum(counts)]), classes)

    def save(self, path) -> None:
        path = pathlib.Path(path).expanduser()
        path.parent.mkdir(parents=True, exist_ok=True)
        with open(path, 'wb') as f:
            np.savez(f, points=self.points.cpu().numpy(), inst=self.inst.cpu().numpy(), scan_offsets=self.scan_offsets,
                     classes=np.asarray(self.classes, dtype=np.int64))

    @classmethod
    def load(cls, path, device, classes=(CAR_RAW,), num_scans: Optional[int] = None, verbose: bool = True) -> 'SceneBank':
        """The bank of ``path`` with its points on ``device``.  ``classes`` / ``num_scans`` (``None``: any): what the caller
        expects; a file made for other classes, or for another number of scans, is refused."""
        path = pathlib.Path(path).expanduser()
        if not path.exists():
            raise FileNotFoundError(f'Cannot find the scene bank at {path}: build it with `{BUILD_COMMAND}`')
        with np.load(path) as z:
            have = tuple(int(c) for c in z['classes'])
            want = tuple(int(c) for c in classes)
            scans = int(z['scan_offsets'].size) - 1
            if have != want:
                raise ValueError(f'{path} holds the classes {have}, not {want}: rebuild it with `{BUILD_COMMAND}`')
            if num_scans is not None and scans != int(num_scans):
                raise ValueError(f'{path} holds {scans} scans, the sequence has {int(num_scans)}: rebuild it with '
                                 f'`{BUILD_COMMAND}`')
            bank = cls(z['points'], z['inst'], z['scan_offsets'], have, device)
        if verbose:
            print(f'scene bank {path}: {len(bank)} scans, {bank.points.shape[0]} points, {bank.nbytes} bytes on {bank.device}',
                  flush=True)
        return bank

    def to(self, device) -> 'SceneBank':
        return SceneBank(self.points, self.inst, self.scan_offsets, self.classes, device)

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def scene(centre: int, poses: np.ndarray, velo_to_cam: Optional[np.ndarray], x_range, y_range
              ) -> Tuple[np.ndarray, np.ndarray]:
        """The scene around scan ``centre`` → (scan_indices (k), transforms (k, 4, 4) f64): ``rasterize.scans_in_range``'s
        choice, and ``inv(pose_v[centre]) @ pose_v[s]`` with ``pose_v = inv(velo_to_cam) @ pose @ velo_to_cam`` (``poses`` as
        ``batch.read_poses`` returns them; ``velo_to_cam`` ``None``: they are velodyne poses already), in f64 on the host."""
        poses = np.asarray(poses, dtype=np.float64)
        index = scans_in_range(poses, centre, x_range, y_range, velo_to_cam=velo_to_cam)
        if velo_to_cam is not None:
            v2c = np.asarray(velo_to_cam, dtype=np.float64)
            poses = np.linalg.inv(v2c) @ poses @ v2c
        return index, np.linalg.inv(poses[centre]) @ poses[index]


__all__ = ['SceneBank', 'CAR_RAW', 'BUILD_COMMAND']
