#!/usr/bin/env python3
"""Launcher of the MI355X-native MaskBEV path — the counterpart of /root/reference: train_mask_bev.py:34-119.

Same command line (``--config/-c``, ``--train/-t``, ``--test/-e``), same YAML files (every key of
``configs/training/**.yml`` is accepted; the model keys go to ``MaskBevModule.from_config`` unchanged), same
checkpoint folder convention (``checkpoints/<config stem>/``, ``last.ckpt`` plus the best
``<stem>-epoch=EE-<metric>=V.ckpt``; ``--test`` picks the best file by the ``val_loss=`` / ``train_loss=`` in its
name like :57-64 does).

What differs: the reference hands the loop to ``pytorch_lightning.Trainer(strategy='ddp')`` (:92-112), which is not
installed on the MI355X image.  The loop here is the built-in one: one process per GPU (``torchrun`` / RANK,
WORLD_SIZE), parameters in a :class:`mask_bev_amd.arena.ParameterArena`, the static part of the step replayed from
HIP graphs (:class:`mask_bev_amd.graph.GraphedTrainStep`), gradients averaged over RCCL by
:class:`mask_bev_amd.ddp.GradientAllReducer` underneath the backward, ``ReduceLROnPlateau`` / ``CosineAnnealingLR``
stepped once per epoch on ``train_loss`` as ``configure_optimizers`` declares (mask_bev_module.py:161-166).

Data (the reference's DataModules, /root/reference: train_mask_bev.py:68-83, are outside the hot path):
``dataset: synthetic`` (or ``--synthetic``) draws SemanticKITTI-shaped scans and box masks on the GPU
(mask_bev_amd/synthetic.py); ``dataset: semantic-kitti`` reads ``<root>/sequences/SS/velodyne/*.bin`` with the
instance-map cache ``<root>/sequences/SS/mask_cache/*.npy`` the reference's mask dataset writes
(semantic_kitti_mask_dataset.py:121-137) and builds the (labels, masks) targets on the GPU (batch.py, K14);
``dataset: kitti`` reads the KITTI object distribution as the reference's KittiDataset lays it out
(``<root>/data_object_velodyne/training/velodyne/*.bin``, ``data_object_label_2/training/label_2/*.txt``,
``data_object_calib/training/calib/*.txt``, ``train.txt`` / ``val.txt``) and rasterises each frame's Car / Van / Truck
boxes on the GPU (rasterize.KittiRasterizer, K24) in front of K14.  ``dataset: waymo`` is not read here (``torch_waymo``
frames); ``rasterize.WaymoRasterizer`` with ``batch.BoxCollate`` makes its batches from box tables.  The config's
``augmentations:`` list is applied to the training batches on the GPU (mask_bev_amd/augment.py, K23), never to validation.

``--test`` extras: ``dataset: kitti`` prints the Car BEV AP block, with ``kitti_3d: true`` (optional ``kitti_3d_extent:
[q_lo, q_hi]``) also the ``3d   AP:`` lines from heights lifted out of the scans (K31, K26b); ``dataset: semantic-kitti`` with
``--write-labels DIR`` writes the per-point instance labels of every validated scan (K31) to
``DIR/sequences/SS/predictions/NNNNNN.label``; when ``sequences/SS/labels/NNNNNN.label`` lies next to every validated scan
it also prints ``point PQ .. SQ .. RQ .. IoU .. (car; tp .. fp .. fn ..)``, the panoptic quality of those lifted labels (K32;
``panoptic_min_points``, ``panoptic_things``, ``panoptic_ignore``).  ``track_instances: true`` adds a pass on rank 0 over the
validation sequences in scan order (K33; needs ``sequences/SS/poses.txt`` and ``calib.txt``, says so in one line and skips
without them): one global instance id per object, written by ``--write-labels`` in place of the query index, and with label
files ``point LSTQ .. S_assoc .. S_cls .. (tubes .., tracks .., dropped ..)`` (``track_min_iou``, ``track_max_age``,
``track_min_cells``, ``track_max_tracks``).
"""
from __future__ import annotations

import argparse
import os
import pathlib
import re
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

os.environ.setdefault('OMP_NUM_THREADS', str(6))          # /root/reference: train_mask_bev.py:14

from mask_bev.mask_bev_module import MaskBevModule          # noqa: E402  (the reference's import line, :12)


def get_metric_from_name(path, regex):
    return float(regex.search(str(path)).group(1))


class SyntheticBatches:
    """``len`` batches per epoch of synthetic scans in the reference's batch contract, already on the device."""

    def __init__(self, config, device, rank, batches_per_epoch):
        from mask_bev_amd import synthetic
        self.syn, self.device, self.rank, self.n = synthetic, device, rank, batches_per_epoch
        vs = config['voxel_size']
        self.nx = int((config['x_range'][1] - config['x_range'][0]) / vs)
        self.ny = int((config['y_range'][1] - config['y_range'][0]) / vs)
        self.cfg = config

    def __len__(self):
        return self.n

    def batch(self, epoch, i):
        c, syn = self.cfg, self.syn
        gen = torch.Generator(device=self.device).manual_seed(int(c.get('seed', 420)) + 1000 * self.rank + 100003 * epoch + i)
        b = int(c.get('batch_size', 1))
        scans = []
        for _ in range(b):
            s = syn.lidar_scan(int(c.get('synthetic_points', 120000)), int(c.get('pc_point_dim', 4)), gen, self.device)
            if c['x_range'][0] >= 0:
                s[:, 0] = s[:, 0].abs()
            scans.append(s)
        labels, masks = syn.gt_masks(b, int(c['num_queries']), self.ny, self.nx, gen, self.device, cell=c['voxel_size'])
        return scans, (labels, masks)


def build_augmentation(config):
    """The config's ``augmentations:`` list (the reference's SemanticKITTI configurations carry one) as an on-device
    augmentation (K23), ``None`` without one."""
    spec = config.get('augmentations')
    if not spec:
        return None
    from mask_bev_amd.augment import DeviceAugmentation, make_semantic_kitti_augmentation_list
    return DeviceAugmentation(make_semantic_kitti_augmentation_list(spec), int(config.get('seed', 420)),
                              config['x_range'], config['y_range'], config['voxel_size'])


class SemanticKittiCacheBatches:
    """``.bin`` scans + the reference's ``.npy`` instance-map cache; targets are expanded on the GPU (K14).  ``augment``:
    apply the config's ``augmentations:`` (training batches only), seeded from (seed, rank, epoch, batch index)."""

    def __init__(self, config, device, rank, world, root, sequences, augment=False):
        from mask_bev_amd import batch as B
        self.B, self.device = B, device
        self.rank, self.seed = rank, int(config.get('seed', 420))
        self.augmentation = build_augmentation(config) if augment else None
        files = []
        for seq in sequences:
            d = pathlib.Path(root) / 'sequences' / f'{int(seq):02d}'
            for f in sorted((d / 'velodyne').glob('*.bin')):
                m = d / 'mask_cache' / (f.stem + '.npy')
                if m.exists():
                    files.append((f, m))
        if not files:
            raise ValueError(f'no (velodyne/*.bin, mask_cache/*.npy) pairs under {root}')
        bsz = int(config.get('batch_size', 1))
        usable = len(files) - len(files) % (world * bsz)           # drop_last, equal work per rank
        self.files = files[rank:usable:world]
        self.bsz = bsz
        self.collate = B.InstanceMapCollate(int(config['num_queries']), device,
                                            int(config.get('min_num_inst_pixels', 0)), augmentation=self.augmentation)
        self.shuffle = bool(config.get('shuffle_train', True))

    def __len__(self):
        return len(self.files) // self.bsz

    def batch(self, epoch, i):
        order = list(range(len(self.files)))
        if self.shuffle:
            g = torch.Generator().manual_seed(epoch)
            order = torch.randperm(len(order), generator=g).tolist()
        idx = order[i * self.bsz:(i + 1) * self.bsz]
        samples = []
        for j in idx:
            pc = torch.from_numpy(self.B.read_velodyne_bin(self.files[j][0]))
            pc = pc[torch.randperm(pc.shape[0])]                     # ShufflePointCloud (semantic_kitti_transforms.py:58-61)
            samples.append((pc, self.B.read_mask_cache(self.files[j][1])))
        if self.augmentation is not None:
            self.augmentation.reseed(self.seed, self.rank, epoch, i)
        return self.collate(samples)


def build_kitti_augmentation(config):
    """The ``augmentations:`` list of a KITTI configuration (kitti_mask_augmentations.py's names).  With
    ``device_object_augmentation: true`` the whole list runs, ``object_sample`` and ``object_noise`` on the device (K28) with
    the bank of ``object_bank:`` or ``<dataset_root>/samples.npz`` (``--build-object-bank`` writes it).  Without that key
    training goes on without the two after one line."""
    spec = config.get('augmentations')
    if not spec:
        return None
    from mask_bev_amd.augment import DeviceAugmentation, make_kitti_augmentation_list
    if config.get('device_object_augmentation', False):
        from mask_bev_amd.object_augment import ObjectBank, make_kitti_object_augmentation_list
        bank = ObjectBank.load(config['object_bank']) if config.get('object_bank') else None
        return DeviceAugmentation(make_kitti_object_augmentation_list(spec, bank), int(config.get('seed', 420)),
                                  config['x_range'], config['y_range'], config['voxel_size'])
    left_out = [a.get('name') for a in spec if a.get('name') in ('object_sample', 'object_noise')]
    if left_out:
        print(f'warning: training without {", ".join(left_out)} (not provided: samples.pkl / mmdet3d collision search)',
              flush=True)
    spec = [a for a in spec if a.get('name') not in ('object_sample', 'object_noise')]
    return DeviceAugmentation(make_kitti_augmentation_list(spec), int(config.get('seed', 420)),
                              config['x_range'], config['y_range'], config['voxel_size']) if spec else None


class KittiObjectBatches:
    """KITTI object frames (kitti_dataset.py, kitti_data_module.py:53-105): ``.bin`` scan, ``label_2`` and ``calib`` of the
    frames listed in ``<root>/<split>.txt``; labels taken to the velodyne frame, optionally filtered by difficulty
    (``filter_difficulty``), Car / Van / Truck boxes rasterised on the GPU (K24) and expanded to targets (K14).  The
    range filter acts after the augmentation, as there."""

    def __init__(self, config, device, rank, world, root, split, augment=False):
        from mask_bev_amd import batch as B
        from mask_bev_amd.rasterize import KITTI_CAR_LIKE, KittiRasterizer
        import numpy as np
        self.B, self.np, self.device, self.car_like = B, np, device, KITTI_CAR_LIKE
        self.rank, self.seed = rank, int(config.get('seed', 420))
        self.augmentation = build_kitti_augmentation(config) if augment else None
        root = pathlib.Path(root).expanduser()
        with open(root / f'{split}.txt', 'r') as f:
            frames = [int(line.strip()) for line in f if line.strip()]
        self.dirs = {k: root / f'data_object_{k}' / 'training' / d
                     for k, d in (('velodyne', 'velodyne'), ('label_2', 'label_2'), ('calib', 'calib'))}
        if not frames:
            raise ValueError(f'{root / (split + ".txt")} lists no frame')
        bsz = int(config.get('batch_size', 1))
        usable = len(frames) - len(frames) % (world * bsz)           # drop_last, equal work per rank
        self.frames, self.bsz = frames[rank:usable:world], bsz
        self.filter_difficulty = bool(config.get('filter_difficulty', False))
        rasterizer = KittiRasterizer(config['x_range'], config['y_range'], config['z_range'], config['voxel_size'],
                                     bool(config.get('remove_unseen', False)), int(config.get('min_num_points', 1)),
                                     device=device)
        self.collate = B.BoxCollate(rasterizer, int(config['num_queries']), device,
                                    int(config.get('min_num_inst_pixels', 0)), augmentation=self.augmentation,
                                    object_range=(config['x_range'], config['y_range']))
        self.shuffle = bool(config.get('shuffle_train', True))

    def __len__(self):
        return len(self.frames) // self.bsz

    def sample(self, frame, shuffle_points=True):
        B, np = self.B, self.np
        name = f'{frame:06d}'
        pc = torch.from_numpy(B.read_velodyne_bin(self.dirs['velodyne'] / f'{name}.bin'))
        if shuffle_points:
            pc = pc[torch.randperm(pc.shape[0])]                     # ShufflePointCloud (kitti_transforms.py:35-38)
        labels = B.kitti_labels_to_velodyne(B.read_kitti_label(self.dirs['label_2'] / f'{name}.txt'),
                                            B.read_kitti_calib(self.dirs['calib'] / f'{name}.txt'))
        keep = np.isin(labels['type'], self.car_like)
        if self.filter_difficulty:
            keep &= B.is_difficulty_valid(labels['occluded'], labels['truncated'])
        return pc, labels['boxes'][keep]

    def batch(self, epoch, i):
        order = list(range(len(self.frames)))
        if self.shuffle:
            g = torch.Generator().manual_seed(epoch)
            order = torch.randperm(len(order), generator=g).tolist()
        samples = [self.sample(self.frames[j]) for j in order[i * self.bsz:(i + 1) * self.bsz]]
        if self.augmentation is not None:
            self.augmentation.reseed(self.seed, self.rank, epoch, i)
        return self.collate(samples)


def kitti_bev_evaluation(model, config, device, root, split='val', score_threshold=0.0, box_method=None):
    """Car BEV AP (easy / moderate / hard at overlaps 0.7 and 0.5) of ``model`` on every frame of ``<root>/<split>.txt``:
    ``model.predict`` per batch, an oriented box per kept mask (``Predictions.kitti_predictions``), then the KITTI protocol on
    the device (K26, K27; ``mask_bev_amd.kitti_eval.eval_kitti``).  ``box_method`` (default: the configuration's
    ``kitti_box_method``, else ``moment``): ``moment`` — K25's moment-axis box of all set cells; ``min_area_rect`` — the
    minimum-area rectangle of the mask's largest component (K30a + K30b), the reference's recipe.  All labels of a frame take
    part, unfiltered: the protocol itself decides what counts at which difficulty.  With the configuration's ``kitti_3d: true``
    (default false) the scans go to ``kitti_predictions`` as well, every box gets the z-extent of the points inside
    its mask (K31; ``kitti_3d_extent: [q_lo, q_hi]`` takes histogram quantiles instead of the extremes) and a ``3d   AP:``
    line follows every ``bev  AP:`` line (K26b).  Returns the result (a string with ``.metrics``)."""
    from mask_bev_amd.predict import BOX_METHODS
    method = box_method if box_method is not None else config.get('kitti_box_method', 'moment')
    if method not in BOX_METHODS:
        raise ValueError(f'kitti_box_method must be one of {BOX_METHODS}, got {method!r}')
    from mask_bev_amd import batch as B
    from mask_bev_amd.kitti_eval import eval_kitti
    with_3d = bool(config.get('kitti_3d', False))
    extent = tuple(config['kitti_3d_extent']) if config.get('kitti_3d_extent') else 'minmax'
    frames = KittiObjectBatches(dict(config, shuffle_train=False, batch_size=1), device, 0, 1, root, split)
    bsz = max(1, int(config.get('batch_size', 1)))
    labels, predictions = [], []
    for start in range(0, len(frames.frames), bsz):
        scans = []
        for frame in frames.frames[start:start + bsz]:
            name = f'{frame:06d}'
            scans.append(torch.from_numpy(B.read_velodyne_bin(frames.dirs['velodyne'] / f'{name}.bin')).to(device))
            labels.append(B.kitti_labels_to_velodyne(B.read_kitti_label(frames.dirs['label_2'] / f'{name}.txt'),
                                                     B.read_kitti_calib(frames.dirs['calib'] / f'{name}.txt')))
        pred = model.predict(scans, score_threshold)
        lift = dict(scans=scans, module=model, extent=extent) if with_3d else {}
        predictions += pred.kitti_predictions(config['x_range'], config['y_range'], config['voxel_size'], method=method, **lift)
    return eval_kitti(labels, predictions, device=device)


def write_point_labels(model, config, device, files, out_dir, score_threshold=0.0, semantic_id=10):
    """Per-point instance labels of every scan of ``files`` — the (``.bin``, cache) pairs of a
    :class:`SemanticKittiCacheBatches` — in SemanticKITTI's layout: ``model.predict`` per batch, the instance map lifted to
    the points (K31, ``Predictions.lift``), one ``<out_dir>/sequences/SS/predictions/NNNNNN.label`` per scan (``uint32``:
    query + 1 in the upper 16 bits, ``semantic_id`` in the lower, 0 for an unlabelled point).  Returns the paths written."""
    from mask_bev_amd import batch as B
    from mask_bev_amd.predict import write_semantic_kitti_labels
    bsz = max(1, int(config.get('batch_size', 1)))
    written = []
    for start in range(0, len(files), bsz):
        part = [f for f, _ in files[start:start + bsz]]
        scans = [torch.from_numpy(B.read_velodyne_bin(f)).to(device) for f in part]
        pred = model.predict(scans, score_threshold)
        for f, labels in zip(part, pred.lift(scans, model).per_scan()):
            d = pathlib.Path(out_dir) / 'sequences' / f.parent.parent.name / 'predictions'
            d.mkdir(parents=True, exist_ok=True)
            write_semantic_kitti_labels(d / (f.stem + '.label'), labels, semantic_id)
            written.append(d / (f.stem + '.label'))
    return written


def semantic_kitti_label_path(scan_path):
    """``sequences/SS/velodyne/NNNNNN.bin`` → ``sequences/SS/labels/NNNNNN.label``, the ground truth next to a scan."""
    scan_path = pathlib.Path(scan_path)
    return scan_path.parent.parent / 'labels' / (scan_path.stem + '.label')


def panoptic_settings(config):
    """The configuration's ``panoptic_min_points`` (default 50), ``panoptic_things`` (default [[10]]: raw label 10, car, is
    thing class 1; one list of raw semantic ids per thing class) and ``panoptic_ignore`` (default [0, 1, 252])."""
    things = config.get('panoptic_things', [[10]])
    things = tuple(tuple(int(i) for i in (t if isinstance(t, (list, tuple)) else [t])) for t in things)
    ignore = tuple(int(i) for i in config.get('panoptic_ignore', [0, 1, 252]))
    return int(config.get('panoptic_min_points', 50)), things, ignore


def point_panoptic_evaluation(model, config, device, files, score_threshold=0.0):
    """Panoptic quality of the lifted point labels over ``files`` — the (``.bin``, cache) pairs of a
    :class:`SemanticKittiCacheBatches` — against ``sequences/SS/labels/NNNNNN.label``: ``model.predict`` per batch, the lift
    to the points (K31), the per-frame counts on the device (K32, ``metrics.DevicePanopticQuality``).  Returns the metric
    after the last update (``compute()`` sums the ranks: call it on every rank), or ``None`` when a label file is missing.
    ``panoptic_max_gt`` (default 256, at most 1024): the ground-truth segments a scan may hold."""
    import numpy as np
    from mask_bev_amd import batch as B
    from mask_bev_amd.metrics import DevicePanopticQuality, semantic_kitti_class_lut
    labels = [semantic_kitti_label_path(f) for f, _ in files]
    if not labels or not all(p.exists() for p in labels):
        return None
    min_points, things, ignore = panoptic_settings(config)
    metric = DevicePanopticQuality(len(things) + 1, semantic_kitti_class_lut(things, ignore), min_points=min_points,
                                   max_gt=int(config.get('panoptic_max_gt', 256)))
    bsz = max(1, int(config.get('batch_size', 1)))
    for start in range(0, len(files), bsz):
        scans = [torch.from_numpy(B.read_velodyne_bin(f)).to(device) for f, _ in files[start:start + bsz]]
        words = [torch.from_numpy(np.fromfile(str(p), dtype='<u4').view(np.int32)).to(device) for p in labels[start:start + bsz]]
        pred = model.predict(scans, score_threshold)
        pred.panoptic_points(pred.lift(scans, model), words, metric)
    return metric


def format_point_panoptic(result, things=((10,),)):
    """The ``point PQ`` line of ``--test`` from ``DevicePanopticQuality.compute()``."""
    pc = result['per_class']
    what = 'car' if tuple(tuple(t) for t in things) == ((10,),) else f'{len(things)} thing classes'
    return (f'point PQ {result["pq"]:.4f} SQ {result["sq"]:.4f} RQ {result["rq"]:.4f} IoU {result["iou"]:.4f} '
            f'({what}; tp {sum(pc["tp"][1:])} fp {sum(pc["fp"][1:])} fn {sum(pc["fn"][1:])})')


def tracking_settings(config):
    """``track_min_iou`` (0.3), ``track_max_age`` (2), ``track_min_cells`` (4), ``track_max_tracks`` (256): the arguments of
    :class:`mask_bev_amd.tracking.InstanceTracker`."""
    return dict(min_iou=float(config.get('track_min_iou', 0.3)), max_age=int(config.get('track_max_age', 2)),
                min_cells=int(config.get('track_min_cells', 4)), max_tracks=int(config.get('track_max_tracks', 256)))


def sequence_tracking(model, config, device, root, sequences, out_dir=None, score_threshold=0.0, semantic_id=10):
    """``track_instances: true``: one pass over the scans of ``sequences`` in scan order, on ONE rank — predict, the tracker
    step on the BEV instance maps (K33a; the tracker is reset at every sequence change, the ego motion comes from
    ``poses.txt`` and ``calib.txt`` of the sequence), the lift to the points (K31) and the per-point track ids.  With
    ``labels/NNNNNN.label`` next to every scan the tube association (K33b) per sequence and the panoptic IoU (K32) over the
    same frames; with ``out_dir`` the ``.label`` files carry the track id + 1 as the instance id.  Returns ``None`` — after
    one line that says why — when a sequence lacks ``poses.txt`` or ``calib.txt``, else ``{'tracks', 'dropped', 'frames',
    'written'}`` plus, with labels, ``{'lstq', 's_assoc', 's_cls', 'tubes'}``.  Not pinned: parity with semantic-kitti-api's
    4D evaluator (not installed), and any LSTQ on real SemanticKITTI (none has been measured)."""
    import numpy as np
    from mask_bev_amd import batch as B
    from mask_bev_amd.metrics import (DevicePanopticQuality, DeviceTubeAssociation, lstq, panoptic_quality,
                                      semantic_kitti_class_lut)
    from mask_bev_amd.predict import write_semantic_kitti_labels
    from mask_bev_amd.tracking import InstanceTracker, velodyne_poses
    files = SemanticKittiCacheBatches(dict(config, shuffle_train=False, batch_size=1), device, 0, 1, root, sequences).files
    by_seq = {}
    for f, _ in files:
        by_seq.setdefault(f.parent.parent, []).append(f)
    missing = [d for d in by_seq if not ((d / 'poses.txt').exists() and (d / 'calib.txt').exists())]
    if missing:
        print(f'track_instances: skipped, poses.txt or calib.txt is missing under {missing[0]}', flush=True)
        return None
    have_labels = all(semantic_kitti_label_path(f).exists() for f, _ in files)
    min_points, things, ignore = panoptic_settings(config)
    lut = semantic_kitti_class_lut(things, ignore)
    settings = tracking_settings(config)
    tracker = InstanceTracker(config['x_range'], config['y_range'], config['voxel_size'], int(config['num_queries']),
                              device=device, **settings)
    tubes = DeviceTubeAssociation(len(things) + 1, lut, id_limit=int(config.get('track_id_limit', 1024)),
                                  max_tracks=int(config.get('track_tube_tracks', 4096)))
    quality = DevicePanopticQuality(len(things) + 1, lut, min_points=min_points, max_gt=int(config.get('panoptic_max_gt', 256)))
    bsz = max(1, int(config.get('batch_size', 1)))
    out = dict(tracks=0, dropped=0, frames=0, written=[])
    assoc_sum, n_tubes = 0.0, 0
    for seq_dir, scans_of in by_seq.items():
        poses = velodyne_poses(B.read_poses(seq_dir / 'poses.txt'), B.read_calib(seq_dir / 'calib.txt'))
        tracker.reset()
        tubes.reset()
        for start in range(0, len(scans_of), bsz):
            part = scans_of[start:start + bsz]
            scans = [torch.from_numpy(B.read_velodyne_bin(f)).to(device) for f in part]
            pred = model.predict(scans, score_threshold)
            query_track = pred.track(tracker, poses=poses[[int(f.stem) for f in part]])
            lifted = pred.lift(scans, model)
            ids = pred.point_tracks(lifted, query_track)
            if have_labels:
                words = [torch.from_numpy(np.fromfile(str(semantic_kitti_label_path(f)), dtype='<u4').view(np.int32)).to(device)
                         for f in part]
                tubes.update(ids, words[0] if len(words) == 1 else torch.cat(words))
                pred.panoptic_points(lifted, words, quality)
            if out_dir is not None:
                for f, labels, tracks in zip(part, lifted.per_scan(), torch.split(ids, list(lifted.lengths))):
                    d = pathlib.Path(out_dir) / 'sequences' / seq_dir.name / 'predictions'
                    d.mkdir(parents=True, exist_ok=True)
                    write_semantic_kitti_labels(d / (f.stem + '.label'), labels, semantic_id, instance_ids=tracks)
                    out['written'].append(d / (f.stem + '.label'))
        counts = tracker.counters()
        out['tracks'] += counts['tracks']
        out['dropped'] += counts['dropped']
        out['frames'] += counts['frames']
        if have_labels:
            res = tubes.compute()                  # per sequence: SemanticKITTI's instance ids are unique inside one only
            assoc_sum += res['s_assoc'] * res['tubes']
            n_tubes += res['tubes']
    if have_labels:
        s_assoc, s_cls = assoc_sum / max(n_tubes, 1), 0.0
        if quality.state is not None:              # this rank's sums alone: compute() would wait for the other ranks
            stats, iou_sum, conf, over = (x.cpu().numpy() for x in quality.state)
            if int(over[0]) > 0:
                raise RuntimeError(f'track_instances: {int(over[0])} scans hold more than panoptic_max_gt ground-truth segments')
            s_cls = panoptic_quality(stats[:, 0], stats[:, 1], stats[:, 2], iou_sum, conf)['iou']
        out.update(lstq=lstq(s_assoc, s_cls), s_assoc=s_assoc, s_cls=s_cls, tubes=n_tubes)
    return out


def format_point_lstq(result):
    """The ``point LSTQ`` line of ``--test`` from :func:`sequence_tracking`."""
    return (f'point LSTQ {result["lstq"]:.4f} S_assoc {result["s_assoc"]:.4f} S_cls {result["s_cls"]:.4f} '
            f'(tubes {result["tubes"]}, tracks {result["tracks"]}, dropped {result["dropped"]})')


def object_bank_path(config, root):
    """``object_bank:``, else ``samples.npz`` under the ``dataset_root`` of the list's ``object_sample`` entry, else under ``root``."""
    from mask_bev_amd.object_augment import ObjectBank
    if config.get('object_bank'):
        return pathlib.Path(config['object_bank']).expanduser()
    for a in config.get('augmentations') or []:
        if a.get('name') == 'object_sample' and a.get('dataset_root'):
            return ObjectBank.default_path(a['dataset_root'])
    return ObjectBank.default_path(root)


def build_object_bank(config, device, root, split='train', min_points=5):
    """The bank ``object_sample`` pastes from (scripts/generate_kitti_object_sampler.py): every labelled box of the split's
    frames, as this launcher selects them, that holds at least ``min_points`` points; written to ``object_bank_path``."""
    from mask_bev_amd.object_augment import ObjectBank
    frames = KittiObjectBatches(dict(config, shuffle_train=False, batch_size=1), device, 0, 1, root, split)
    bank = ObjectBank.build((frames.sample(f, shuffle_points=False) for f in frames.frames), min_points, device)
    path = object_bank_path(config, root)
    bank.save(path)
    print(f'object bank: {len(bank)} samples, {len(bank.points)} points from {len(frames.frames)} frames -> {path}', flush=True)
    return path


def format_layer_metrics(logged, layer):
    """One line of ``--test`` per decoder layer from the module's logged values (mask_bev_module.py:209-224)."""
    names = ('map', 'map_50', 'map_75', 'mar_100')
    parts = [f'{n} {logged[f"val_mAP_{layer}_{n}"]:.4f}' for n in names]
    parts += [f'mIoU {logged[f"val_mIoU_layer_{layer}"]:.4f}', f'cls_AP {logged[f"val_cls_mAP_layer_{layer}"]:.4f}']
    return f'layer {layer}: ' + ' '.join(parts)


def save_checkpoint(model, optimizer, path, epoch, metric_name, metric):
    torch.save({'state_dict': model.state_dict(), 'hyper_parameters': dict(getattr(model, 'hparams', {})),
                'optimizer_states': [optimizer.state_dict()], 'epoch': epoch, metric_name: metric}, path)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--config', '-c', type=str, help='Config file for current run', required=True)
    parser.add_argument('--train', '-t', action='store_true', help='Train the model')
    parser.add_argument('--test', '-e', action='store_true', help='Test the model')
    # extensions of this launcher
    parser.add_argument('--synthetic', action='store_true', help='synthetic scans instead of a dataset on disk')
    parser.add_argument('--data-root', default=None, help='default: data/SemanticKITTI, data/KITTI for dataset: kitti')
    parser.add_argument('--max-epochs', type=int, default=1000)
    parser.add_argument('--max-steps', type=int, default=-1, help='stop after this many optimizer steps (-1: no limit)')
    parser.add_argument('--steps-per-epoch', type=int, default=100, help='synthetic data: batches per epoch')
    parser.add_argument('--compute-dtype', default=None, choices=[None, 'fp32', 'bf16', 'fp16'])
    parser.add_argument('--no-graph', action='store_true', help='launch every kernel eagerly (no HIP-graph replay)')
    parser.add_argument('--checkpoint-root', default='checkpoints')
    parser.add_argument('--build-object-bank', action='store_true',
                        help='dataset: kitti: write the object bank of object_sample from the training split and exit')
    parser.add_argument('--write-labels', default=None, metavar='DIR',
                        help='dataset: semantic-kitti with --test: write the per-point instance labels of every validated '
                             'scan to DIR/sequences/SS/predictions/NNNNNN.label')
    args = parser.parse_args(argv)

    is_training, is_testing = args.train, args.test
    if is_training is False and is_testing is False:
        is_training = True

    config_path = pathlib.Path(args.config)
    exp_name = config_path.stem
    checkpoint_folder_path = pathlib.Path(args.checkpoint_root).joinpath(exp_name)
    if not config_path.exists():
        raise ValueError(f'Could not find config at path {config_path}')
    with open(config_path, 'r') as f:
        config: dict = yaml.safe_load(f)
    if args.compute_dtype:
        config['compute_dtype'] = args.compute_dtype

    limit_val_batches = config.get('limit_val_batches', 1.0)
    check_metric = 'val_loss' if (limit_val_batches > 0 and not args.synthetic
                                  and config.get('dataset', 'semantic-kitti') != 'synthetic') else 'train_loss'
    if is_testing:
        regex = re.compile(r'(?:val|train)_loss=([0-9]+\.?[0-9]*)')
        checkpoints = [f for f in checkpoint_folder_path.iterdir() if not f.name.startswith('last')]
        best_checkpoint = min(checkpoints, key=lambda x: get_metric_from_name(x, regex))
        print(f'Testing from {best_checkpoint}')
        config['checkpoint'] = str(best_checkpoint)
        config['batch_size'] = config.get('test_batch_size', config.get('batch_size', 1))
        config['num_workers'] = config.get('test_num_workers', config.get('num_workers', 0))

    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if not torch.cuda.is_available():
        raise SystemExit('train_mask_bev_amd.py needs an MI355X (the product path has no CPU fallback)')
    dev_index = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev_index)
    device = torch.device('cuda', dev_index)
    if args.build_object_bank:
        if config.get('dataset', 'semantic-kitti') != 'kitti':
            raise ValueError('--build-object-bank needs dataset: kitti')
        build_object_bank(config, device, args.data_root or 'data/KITTI')
        return
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        backend = os.environ.get('MBV_DIST_BACKEND', 'nccl')       # 'nccl' is RCCL on ROCm
        dist.init_process_group(backend, **({'device_id': device} if backend == 'nccl' else {}))

    model = MaskBevModule.from_config(config, checkpoint_folder_path).to(device)
    model.log_scalars = False
    model.flatten_parameters()         # fp16 compute: this also creates the device-side loss scaler
    opt_cfg = model.configure_optimizers()
    optimizer, scheduler = opt_cfg['optimizer'], opt_cfg['lr_scheduler']

    reducer = None
    if world > 1:
        from mask_bev_amd.ddp import GradientAllReducer
        reducer = GradientAllReducer(model, bucket_mb=64.0)

    dataset_name = 'synthetic' if args.synthetic else config.get('dataset', 'semantic-kitti')
    if dataset_name == 'synthetic':
        data = SyntheticBatches(config, device, rank, args.steps_per_epoch)
        val = None
    elif dataset_name == 'semantic-kitti':
        args.data_root = args.data_root or 'data/SemanticKITTI'
        data = SemanticKittiCacheBatches(config, device, rank, world, args.data_root,
                                         config.get('train_sequences', [0, 1, 2, 3, 4, 5, 6, 7, 9, 10]), augment=True)
        val = SemanticKittiCacheBatches(dict(config, shuffle_train=False), device, rank, world, args.data_root,
                                        config.get('val_sequences', [8])) if limit_val_batches > 0 else None
    elif dataset_name == 'kitti':
        args.data_root = args.data_root or 'data/KITTI'
        data = KittiObjectBatches(config, device, rank, world, args.data_root, 'train', augment=True)
        val = KittiObjectBatches(dict(config, shuffle_train=False), device, rank, world, args.data_root,
                                 'val') if limit_val_batches > 0 else None
    elif dataset_name == 'waymo':
        raise NotImplementedError('dataset: waymo is not read by this launcher (torch_waymo frames); build batches from '
                                  'box tables with mask_bev_amd.rasterize.WaymoRasterizer and mask_bev_amd.batch.BoxCollate')
    else:
        raise NotImplementedError(dataset_name)

    def validate(epoch):
        if val is None:
            return None
        model.eval()
        tot, n = 0.0, 0
        with torch.no_grad():
            for i in range(len(val)):
                tot += float(model.validation_step(val.batch(epoch, i), i))
                n += 1
        model.train()
        v = tot / max(1, n)
        if world > 1:                  # every rank validates its own shard: the monitored value is the mean over ranks
            from mask_bev_amd.ddp import reduce_scalars
            v = reduce_scalars({'val_loss': torch.tensor(v, device=device)})['val_loss']
        return float(v)

    if is_training:
        model.train()
        if rank == 0:
            checkpoint_folder_path.mkdir(parents=True, exist_ok=True)
        graphed, step_count, best = None, 0, float('inf')
        # EarlyStopping(check_metric, patience=30) of the reference's Trainer (train_mask_bev.py:100): stop after 30
        # epochs without an improvement of the monitored metric (Lightning's default min_delta = 0, mode = 'min')
        es_best, es_wait, es_patience = float('inf'), 0, 30
        for epoch in range(args.max_epochs):
            model.current_epoch = epoch
            t0, loss_sum, n_steps = time.perf_counter(), None, 0
            n_batches = int(len(data) * float(config.get('limit_train_batches', 1.0))) if isinstance(
                config.get('limit_train_batches', 1.0), float) else int(config.get('limit_train_batches'))
            for i in range(max(1, n_batches)):
                batch = data.batch(epoch, i)
                if not args.no_graph and getattr(model, '_arena', None) is not None:
                    if graphed is None:
                        from mask_bev_amd.graph import GraphedTrainStep
                        if reducer is not None:
                            reducer.no_sync(True)
                        graphed = GraphedTrainStep(model, optimizer, batch, reducer=reducer)
                    loss = graphed.step(batch)
                else:
                    if reducer is not None:
                        reducer.sync_buffers()
                    loss = model.training_step(batch, i)
                    model.scale_loss(loss).backward()
                    if reducer is not None:
                        reducer.finish(optimizer)
                    optimizer.step()
                    optimizer.zero_grad(set_to_none=False)
                # accumulate on the device: the graphed step returns ONE static tensor that every replay overwrites,
                # so keeping references would average N aliases of the last batch's loss (the reference monitors the
                # epoch mean of train_loss, mask_bev_module.py:296 `self.log('train_loss', ..., on_epoch=True)`)
                loss_sum = loss.detach().clone() if loss_sum is None else loss_sum + loss.detach()
                n_steps += 1
                step_count += 1
                if 0 < args.max_steps <= step_count:
                    break
            train_loss = float(loss_sum) / max(1, n_steps)
            if world > 1:
                from mask_bev_amd.ddp import reduce_scalars
                train_loss = reduce_scalars({'train_loss': torch.tensor(train_loss, device=device)})['train_loss']
            val_loss = validate(epoch)
            monitored = val_loss if (check_metric == 'val_loss' and val_loss is not None) else train_loss
            if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
                scheduler.step(train_loss)                          # monitor 'train_loss', interval 'epoch'
            else:
                scheduler.step()
            if rank == 0:
                dt = time.perf_counter() - t0
                print(f'epoch {epoch}: train_loss {train_loss:.6f}'
                      + (f' val_loss {val_loss:.6f}' if val_loss is not None else '')
                      + f'  {n_steps * int(config.get("batch_size", 1)) * world / dt:.1f} scans/s', flush=True)
                save_checkpoint(model, optimizer, checkpoint_folder_path / 'last.ckpt', epoch, check_metric, monitored)
                if monitored < best:
                    best = monitored
                    for old in checkpoint_folder_path.glob(f'{exp_name}-epoch=*'):
                        old.unlink()
                    save_checkpoint(model, optimizer, checkpoint_folder_path /
                                    f'{exp_name}-epoch={epoch:02d}-{check_metric}={monitored:.6f}.ckpt', epoch,
                                    check_metric, monitored)
            if monitored < es_best:
                es_best, es_wait = monitored, 0
            else:
                es_wait += 1
            if es_wait >= es_patience:         # `monitored` is rank-reduced, so every rank stops at the same epoch
                if rank == 0:
                    print(f'early stopping: {check_metric} did not improve in {es_patience} epochs '
                          f'(best {es_best:.6f})', flush=True)
                break
            if 0 < args.max_steps <= step_count:
                break
        if graphed is not None:
            graphed.close()

    if is_testing:
        # the reference runs trainer.validate then trainer.test (train_mask_bev.py:118-119); MaskBevModule defines no
        # test_step, so the test pass has nothing of its own to run: validation is the whole of it
        layers = tuple(range(model.num_layers))    # the reference attaches its metrics to all ten decoder outputs (:85-98)
        if val is not None:
            # what trainer.validate logs there: COCO mask AP (K29), mIoU and class AP of every decoder layer
            model.enable_metrics(layers=layers, train=False, val=True, mask_map='device')
        v = validate(0)
        if val is not None:
            model.on_validation_epoch_end()            # every rank: the mask AP gathers the states of all ranks
        if rank == 0:
            print(f'val_loss {v}' if v is not None else 'no validation data configured')
            if val is not None:
                for layer in layers:
                    print(format_layer_metrics(model.logged, layer), flush=True)
            if dataset_name == 'kitti' and val is not None:
                # what the reference's mask_to_pred + eval_kitti are for: boxes from the predicted masks, KITTI BEV AP
                # (`kitti_3d: true`: with the heights lifted from the scans, and the 3D AP lines)
                print(kitti_bev_evaluation(model, config, device, args.data_root,
                                           box_method=config.get('kitti_box_method', 'moment')), end='', flush=True)
        if dataset_name == 'semantic-kitti' and val is not None:
            # point-level panoptic quality of the lifted labels, when the ground truth lies next to every validated scan
            have = all(semantic_kitti_label_path(f).exists() for f, _ in val.files)
            if world > 1:                              # every rank or none: compute() sums the ranks
                flag = torch.tensor([int(have)], device=device)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                have = bool(int(flag))
            metric = point_panoptic_evaluation(model, config, device, val.files) if have else None
            if metric is not None:
                result = metric.compute()
                if rank == 0:
                    print(format_point_panoptic(result, panoptic_settings(config)[1]), flush=True)
        tracked = None
        track = dataset_name == 'semantic-kitti' and val is not None and bool(config.get('track_instances', False))
        if track and rank == 0:
            # global instance ids over the validation sequences (K33), LSTQ of the predicted thing classes when labels exist
            tracked = sequence_tracking(model, config, device, args.data_root, config.get('val_sequences', [8]),
                                        out_dir=args.write_labels)
            if tracked is not None and 'lstq' in tracked:
                print(format_point_lstq(tracked), flush=True)
            if tracked is not None and args.write_labels:
                print(f'wrote {len(tracked["written"])} label files with track ids under {args.write_labels}', flush=True)
        if track and world > 1 and args.write_labels:
            flag = torch.tensor([int(tracked is not None)], device=device)
            dist.broadcast(flag, 0)                    # rank 0 wrote every scan with its track id, or nobody did
            if int(flag) and tracked is None:
                tracked = {}
        if args.write_labels and dataset_name == 'semantic-kitti' and val is not None and tracked is None:
            paths = write_point_labels(model, config, device, val.files, args.write_labels)     # every rank: its own scans
            print(f'wrote {len(paths)} label files under {args.write_labels}', flush=True)

    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
