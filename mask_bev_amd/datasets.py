"""The launcher's data readers (the reference's DataModules are outside the hot path): synthetic scans, SemanticKITTI scans with
the instance-map cache or with scene banks, KITTI object frames, as batches in the reference's batch contract with the targets built on the device."""
import pathlib

import numpy as np
import torch

from . import batch as B
from . import synthetic as syn
from .augment import DeviceAugmentation, make_kitti_augmentation_list, make_semantic_kitti_augmentation_list
from .object_augment import ObjectBank, make_kitti_object_augmentation_list
from .rasterize import KITTI_CAR_LIKE, KittiRasterizer, SemanticKittiRasterizer
from .scene_bank import SceneBank


def shard(items, rank, world, bsz):
    """This rank's share of ``items``: drop_last to a multiple of ``world * bsz`` (equal work per rank), then strided by rank."""
    usable = len(items) - len(items) % (world * bsz)
    return items[rank:usable:world]


def epoch_order(n, epoch, shuffle):
    """The order in which an epoch visits ``n`` samples: a permutation seeded by the epoch alone, the same on every rank."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(epoch)).tolist() if shuffle else range(n)


class SyntheticBatches:
    """``len`` batches per epoch of synthetic scans in the reference's batch contract, already on the device."""

    def __init__(self, config, device, rank, batches_per_epoch):
        self.cfg, self.device, self.rank, self.n = config, device, rank, batches_per_epoch
        self.nx, self.ny = (int((config[k][1] - config[k][0]) / config['voxel_size']) for k in ('x_range', 'y_range'))

    def __len__(self):
        return self.n

    def batch(self, epoch, i):
        c = self.cfg
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


class ShardedBatches:
    """What the on-disk readers share: this rank's shard of ``items`` and batch ``i`` of an epoch: the reader's ``collate`` of the
    ``sample(item)`` pairs in the epoch's order, points shuffled, the augmentation seeded from (seed, rank, epoch, batch index)."""

    def __init__(self, config, rank, world, items, augmentation):
        self.rank, self.seed, self.augmentation = rank, int(config.get('seed', 420)), augmentation
        self.bsz, self.shuffle = int(config.get('batch_size', 1)), bool(config.get('shuffle_train', True))
        self.items = shard(items, rank, world, self.bsz)

    def __len__(self):
        return len(self.items) // self.bsz

    def batch(self, epoch, i):
        order = epoch_order(len(self.items), epoch, self.shuffle)
        samples = [self.sample(self.items[j]) for j in order[i * self.bsz:(i + 1) * self.bsz]]
        samples = [(pc[torch.randperm(pc.shape[0])], target) for pc, target in samples]     # the reference's ShufflePointCloud
        if self.augmentation is not None:
            self.augmentation.reseed(self.seed, self.rank, epoch, i)
        return self.collate(samples)


def build_augmentation(config):
    """The ``augmentations:`` list of a SemanticKITTI configuration as an on-device augmentation (K23), ``None`` without one."""
    spec = config.get('augmentations')
    if not spec:
        return None
    return DeviceAugmentation(make_semantic_kitti_augmentation_list(spec), int(config.get('seed', 420)),
                              config['x_range'], config['y_range'], config['voxel_size'])


def semantic_kitti_files(root, sequences):
    """The (``velodyne/NNNNNN.bin``, ``mask_cache/NNNNNN.npy``) pairs of ``sequences`` under ``root``, in scan order."""
    files = []
    for seq in sequences:
        d = pathlib.Path(root) / 'sequences' / f'{int(seq):02d}'
        for f in sorted((d / 'velodyne').glob('*.bin')):
            m = d / 'mask_cache' / (f.stem + '.npy')
            if m.exists():
                files.append((f, m))
    if not files:
        raise ValueError(f'no (velodyne/*.bin, mask_cache/*.npy) pairs under {root}')
    return files


class SemanticKittiCacheBatches(ShardedBatches):
    """``.bin`` scans + the reference's ``.npy`` instance-map cache (``files``: this rank's pairs); targets are expanded on
    the GPU (K14).  ``augment``: apply the config's ``augmentations:`` (training batches only)."""

    def __init__(self, config, device, rank, world, root, sequences, augment=False):
        files = semantic_kitti_files(root, sequences)
        super().__init__(config, rank, world, files, build_augmentation(config) if augment else None)
        self.device, self.files = device, self.items
        self.collate = B.InstanceMapCollate(int(config['num_queries']), device,
                                            int(config.get('min_num_inst_pixels', 0)), augmentation=self.augmentation)

    def sample(self, pair):
        return torch.from_numpy(B.read_velodyne_bin(pair[0])), B.read_mask_cache(pair[1])


def scene_sequences(root, sequences):
    """Those of ``sequences`` under ``root`` that lie there as downloaded — ``velodyne/``, ``labels/``, ``poses.txt``,
    ``calib.txt`` — as (sequence number, folder) pairs."""
    found = []
    for seq in sequences:
        d = pathlib.Path(root).expanduser() / 'sequences' / f'{int(seq):02d}'
        if (d / 'velodyne').is_dir() and (d / 'labels').is_dir() and (d / 'poses.txt').exists() and (d / 'calib.txt').exists():
            found.append((int(seq), d))
    if not found:
        raise ValueError(f'no sequence with velodyne/, labels/, poses.txt and calib.txt among {list(sequences)} under {root}')
    return found


def scene_rasterizer(config):
    """The rasteriser of a SemanticKITTI configuration, as the reference's data module builds its own."""
    return SemanticKittiRasterizer(config['x_range'], config['y_range'], config['z_range'], config['voxel_size'],
                                   bool(config.get('remove_unseen', False)), int(config.get('min_num_points', 1)))


class SceneSequence:
    """One sequence as the scene readers use it: ``scans`` (the ``.bin`` paths in scan order), ``poses`` (S, 4, 4) f64 in the
    velodyne frame, and ``bank``, loaded from ``SceneBank.default_path`` when the file is there, else built from the label
    files (and saved when ``save``)."""

    def __init__(self, root, seq, folder, device, save=False, build_only=False):
        self.seq, self.folder = seq, folder
        self.scans = sorted((folder / 'velodyne').glob('*.bin'))
        poses, v2c = B.read_poses(folder / 'poses.txt'), B.read_calib(folder / 'calib.txt')['velo_to_cam']
        if len(poses) != len(self.scans):
            raise ValueError(f'{folder}: {len(poses)} poses for {len(self.scans)} scans')
        self.poses = np.linalg.inv(v2c) @ poses @ v2c
        path = SceneBank.default_path(root, seq)
        if path.exists() and not build_only:
            self.bank = SceneBank.load(path, device, num_scans=len(self.scans))
        else:
            bank = SceneBank.build(self.scans, [folder / 'labels' / (f.stem + '.label') for f in self.scans])
            if save:
                bank.save(path)
                print(f'scene bank: {len(bank)} scans, {bank.points.shape[0]} points -> {path}', flush=True)
            self.bank = bank if build_only else bank.to(device)
            if not build_only:
                print(f'scene bank of sequence {seq:02d} built: {len(bank)} scans, {bank.points.shape[0]} points, '
                      f'{bank.nbytes} bytes on {self.bank.device}', flush=True)

    def scene(self, centre, config):
        """(scan_indices, transforms) of the scene around scan ``centre``."""
        return SceneBank.scene(centre, self.poses, None, config['x_range'], config['y_range'])


class SemanticKittiSceneBatches(ShardedBatches):
    """SemanticKITTI as downloaded, without a mask cache (``semantic_kitti_targets: scenes``): ``.bin`` scans, and targets
    rasterised per batch from the sequences' scene banks on the GPU (K34) and expanded by K14.  ``files``: this rank's
    ``(scan path, None)`` pairs.  ``augment``: apply the config's ``augmentations:`` (training batches only); its flips and
    rotations go into the scene transforms, so no map is warped."""

    def __init__(self, config, device, rank, world, root, sequences, augment=False):
        save = bool(config.get('save_scene_bank', False)) and rank == 0
        self.sequences = {seq: SceneSequence(root, seq, d, device, save) for seq, d in scene_sequences(root, sequences)}
        items = [(seq, k, f) for seq, s in self.sequences.items() for k, f in enumerate(s.scans)]
        super().__init__(config, rank, world, items, build_augmentation(config) if augment else None)
        self.config, self.device, self.files = config, device, [(f, None) for _, _, f in self.items]
        self.rasterizer = scene_rasterizer(config)
        self.collate = B.BankSceneCollate(self.rasterizer, {seq: s.bank for seq, s in self.sequences.items()},
                                          int(config['num_queries']), device, int(config.get('min_num_inst_pixels', 0)),
                                          augmentation=self.augmentation)

    def sample(self, item):
        seq, k, path = item
        index, transforms = self.sequences[seq].scene(k, self.config)
        return torch.from_numpy(B.read_velodyne_bin(path)), (seq, index, transforms, k)


def build_scene_banks(config, root, sequences):
    """``--build-scene-bank``: the banks of ``sequences`` written next to their scans."""
    for seq, d in scene_sequences(root, sequences):
        SceneSequence(root, seq, d, None, save=True, build_only=True)
    return [SceneBank.default_path(root, seq) for seq, _ in scene_sequences(root, sequences)]


def build_mask_cache(config, device, root, sequences, overwrite=False, batch_size=8):
    """``--build-mask-cache``: every scan of ``sequences`` rasterised through its sequence's bank (K34) and written as the
    reference's mask cache, ``sequences/SS/mask_cache/NNNNNN.npy`` = ``np.save`` of the (nx, ny) int64 map.  Files that exist
    are left alone unless ``overwrite``.  Returns the paths written."""
    rasterizer, written = scene_rasterizer(config), []
    for seq, d in scene_sequences(root, sequences):
        s = SceneSequence(root, seq, d, device)
        (d / 'mask_cache').mkdir(exist_ok=True)
        todo = [(k, d / 'mask_cache' / (f.stem + '.npy')) for k, f in enumerate(s.scans)]
        todo = [(k, p) for k, p in todo if overwrite or not p.exists()]
        for i in range(0, len(todo), batch_size):
            part = todo[i:i + batch_size]
            maps = rasterizer.rasterize_bank(s.bank, [(*s.scene(k, config), k) for k, _ in part]).cpu().numpy()
            for (_, p), m in zip(part, maps):
                np.save(p, m.astype(np.int64))
                written.append(p)
        print(f'mask cache: sequence {seq:02d}, {len(todo)} of {len(s.scans)} scans written', flush=True)
    return written


def build_kitti_augmentation(config):
    """The ``augmentations:`` list of a KITTI configuration (kitti_mask_augmentations.py's names).  With
    ``device_object_augmentation: true`` the whole list runs, ``object_sample`` and ``object_noise`` on the device (K28) with the
    bank of ``object_bank:`` or ``<dataset_root>/samples.npz``; without that key training goes on without the two after one line."""
    spec = config.get('augmentations')
    if not spec:
        return None
    if config.get('device_object_augmentation', False):
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


class KittiFrames:
    """The KITTI object tree as the reference's KittiDataset lays it out (kitti_dataset.py): ``frames``, the numbers listed
    in ``<root>/<split>.txt``, and ``dirs``, the folders of their ``.bin`` scan, ``label_2`` and ``calib`` files."""

    def __init__(self, root, split, filter_difficulty=False):
        root, self.filter_difficulty = pathlib.Path(root).expanduser(), filter_difficulty
        with open(root / f'{split}.txt', 'r') as f:
            self.frames = [int(line.strip()) for line in f if line.strip()]
        self.dirs = {k: root / f'data_object_{k}' / 'training' / k for k in ('velodyne', 'label_2', 'calib')}
        if not self.frames:
            raise ValueError(f'{root / (split + ".txt")} lists no frame')

    def scan(self, frame):
        return self.dirs['velodyne'] / f'{frame:06d}.bin'

    def labels(self, frame):
        """All labels of a frame, taken to the velodyne frame."""
        return B.kitti_labels_to_velodyne(B.read_kitti_label(self.dirs['label_2'] / f'{frame:06d}.txt'),
                                          B.read_kitti_calib(self.dirs['calib'] / f'{frame:06d}.txt'))

    def sample(self, frame):
        """(points, Car / Van / Truck boxes) of a frame, with ``filter_difficulty`` only the boxes of a valid difficulty."""
        pc, labels = torch.from_numpy(B.read_velodyne_bin(self.scan(frame))), self.labels(frame)
        keep = np.isin(labels['type'], KITTI_CAR_LIKE)
        if self.filter_difficulty:
            keep &= B.is_difficulty_valid(labels['occluded'], labels['truncated'])
        return pc, labels['boxes'][keep]


class KittiObjectBatches(ShardedBatches):
    """KITTI object frames (kitti_data_module.py:53-105; ``frames``: this rank's of a :class:`KittiFrames`), optionally filtered by
    difficulty, the boxes rasterised on the GPU (K24) and expanded to targets (K14); the range filter follows the augmentation."""

    def __init__(self, config, device, rank, world, root, split, augment=False):
        augmentation = build_kitti_augmentation(config) if augment else None
        self.tree = KittiFrames(root, split, bool(config.get('filter_difficulty', False)))
        super().__init__(config, rank, world, self.tree.frames, augmentation)
        self.device, self.frames, self.dirs = device, self.items, self.tree.dirs
        rasterizer = KittiRasterizer(config['x_range'], config['y_range'], config['z_range'], config['voxel_size'],
                                     bool(config.get('remove_unseen', False)), int(config.get('min_num_points', 1)),
                                     device=device)
        self.collate = B.BoxCollate(rasterizer, int(config['num_queries']), device,
                                    int(config.get('min_num_inst_pixels', 0)), augmentation=self.augmentation,
                                    object_range=(config['x_range'], config['y_range']))

    def sample(self, frame):
        return self.tree.sample(frame)


def object_bank_path(config, root):
    """``object_bank:``, else ``samples.npz`` under the ``dataset_root`` of the ``object_sample`` entry, else under ``root``."""
    if config.get('object_bank'):
        return pathlib.Path(config['object_bank']).expanduser()
    for a in config.get('augmentations') or []:
        if a.get('name') == 'object_sample' and a.get('dataset_root'):
            return ObjectBank.default_path(a['dataset_root'])
    return ObjectBank.default_path(root)


def build_object_bank(config, device, root, split='train', min_points=5):
    """The bank ``object_sample`` pastes from (scripts/generate_kitti_object_sampler.py): every labelled box of the split's
    frames, as the launcher selects them, that holds at least ``min_points`` points; written to ``object_bank_path``."""
    tree = KittiFrames(root, split, bool(config.get('filter_difficulty', False)))
    bank = ObjectBank.build((tree.sample(f) for f in tree.frames), min_points, device)
    path = object_bank_path(config, root)
    bank.save(path)
    print(f'object bank: {len(bank)} samples, {len(bank.points)} points from {len(tree.frames)} frames -> {path}', flush=True)
    return path
