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

``semantic_kitti_targets: scenes`` (default ``cache``) needs no mask cache: the dataset as downloaded is enough
(``sequences/SS/velodyne/``, ``labels/``, ``poses.txt``, ``calib.txt``).  The instance-labelled points of every sequence stay on
the GPU as a scene bank (mask_bev_amd/scene_bank.py; ``sequences/SS/instance_points.npz`` when there, else built from the label
files, and saved with ``save_scene_bank: true``), and each batch's instance maps are rasterised from it in one native call (K34).
``--build-scene-bank`` writes the banks of the train and validation sequences and exits; ``--build-mask-cache`` [``--overwrite``]
writes the reference's ``mask_cache/NNNNNN.npy`` files from them and exits.

``weight_average: ema | mean`` (or ``--weight-average``; K43, ``weight_average_decay``, ``weight_average_warmup``,
``weight_average_every``, ``weight_average_start_epoch``) keeps an averaged copy of the arena's weights, updated on the device
behind every optimizer step from the start epoch on: validation — and so the monitored ``val_loss`` and the choice of the best
checkpoint — runs on the averaged weights, every checkpoint gains a ``weight_average`` entry beside the live ``state_dict``,
and ``--test`` loads the averaged weights when the key is set and the checkpoint has the entry, saying so in one
``weight average: ..`` line.  Module buffers are not averaged.  Without the key nothing changes.

``--test`` extras: ``dataset: kitti`` prints the Car BEV AP block, with ``kitti_3d: true`` (optional ``kitti_3d_extent:
[q_lo, q_hi]``) also the ``3d   AP:`` lines from heights lifted out of the scans (K31, K26b); ``dataset: semantic-kitti`` with
``--write-labels DIR`` writes the per-point instance labels of every validated scan (K31) to
``DIR/sequences/SS/predictions/NNNNNN.label``; when ``sequences/SS/labels/NNNNNN.label`` lies next to every validated scan
it also prints ``point PQ .. SQ .. RQ .. IoU .. (car; tp .. fp .. fn ..)``, the panoptic quality of those lifted labels (K32;
``panoptic_min_points``, ``panoptic_things``, ``panoptic_ignore``).  ``track_instances: true`` adds a pass on rank 0 over the
validation sequences in scan order (K33; needs ``sequences/SS/poses.txt`` and ``calib.txt``, says so in one line and skips
without them): one global instance id per object, written by ``--write-labels`` in place of the query index, and with label
files ``point LSTQ .. S_assoc .. S_cls .. (tubes .., tracks .., dropped ..)`` (``track_min_iou``, ``track_max_age``,
``track_min_cells``, ``track_max_tracks``; ``track_motion: true`` runs the tracker with its constant-velocity motion model and
gated re-association, K37 — ``track_velocity_gain``, ``track_gate`` metres, ``track_max_speed`` metres per frame — and the
parenthesis then ends ``, gated ..``; ``track_occlusion: true`` computes a BEV visibility map of every scan and lets a track
that goes unmatched out of the sensor's sight keep its age, K38 — ``track_occlusion_z_top`` metres in the sensor frame,
``track_hidden_fraction`` [num, den], ``track_max_hold`` frames — and the parenthesis then ends ``, held ..``; ``track_fuse: true``
fuses the tracked footprints over time in a rolling world grid, K39 — ``track_fuse_cap``, ``track_fuse_min_count``, and with
``track_motion`` ``track_fuse_static_speed`` metres per frame — lifts, labels and renders from the fused map, and the parenthesis
then ends ``, fused``).  ``predict_resolve: true`` (K42; ``predict_nms_iou`` [num, den], ``predict_min_overlap`` [num, den],
``predict_min_cells``, ``predict_exclusive_masks``) reconciles the kept queries of every prediction of these passes with each
other — greedy mask NMS, then Mask2Former's overlap filter on the rebuilt instance map — and prints one ``resolved predictions:
..`` line in front of the results it changes; the defaults 1/2 and 4/5 are conventions, not tuned here.  ``lift_ground: true`` (K35; ``lift_ground_radius`` metres, ``lift_ground_clearance``,
``lift_max_height``, ``lift_z_floor``) makes every one of these lifts label only the returns above a ground estimate made from
the scan, lets the 3D boxes stand on it, and prints one ``ground-aware lift: ..`` line in front of the results it changes.
``--render DIR`` (K36; ``render_scale``, ``render_alpha``, ``render_boxes``) adds a last pass on rank 0 that writes one BEV frame
per validation scan, composed on the device: ``DIR/sequences/SS/bev/NNNNNN.png`` for ``dataset: semantic-kitti`` (returns per
cell, the predicted instances coloured by query — by track id with ``track_instances: true`` — and the contour of the mask
cache's instances where the file exists), ``DIR/NNNNNN.png`` for ``dataset: kitti`` (with the predicted and the label boxes).
"""
import argparse
import contextlib
import os
import pathlib
import re
import sys
import time

import torch
import torch.distributed as dist
import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

os.environ.setdefault('OMP_NUM_THREADS', str(6))          # /root/reference: train_mask_bev.py:14

from mask_bev.mask_bev_module import MaskBevModule          # noqa: E402  (the reference's import line, :12)
from mask_bev_amd import datasets, evaluate                 # noqa: E402
from mask_bev_amd.optimizers import ClipStats, clip_gradients   # noqa: E402


def get_metric_from_name(path, regex):
    return float(regex.search(str(path)).group(1))


def save_checkpoint(model, optimizer, path, epoch, metric_name, metric, average=None):
    ckpt = {'state_dict': model.state_dict(), 'hyper_parameters': dict(getattr(model, 'hparams', {})),
            'optimizer_states': [optimizer.state_dict()], 'epoch': epoch, metric_name: metric}
    if average is not None:
        # 'state_dict' stays the LIVE weights, which the optimizer state belongs to; the averaged ones travel beside them
        ckpt['weight_average'] = average.state_dict()
    torch.save(ckpt, path)


def validate(model, val, epoch, device, world, average=None):
    if val is None:
        return None
    model.eval()
    tot = 0.0
    # with a weight average (K43) the monitored val_loss is the averaged weights': swapped in for the pass, back after it
    with torch.no_grad(), (average.applied() if average is not None else contextlib.nullcontext()):
        for i in range(len(val)):
            tot += float(model.validation_step(val.batch(epoch, i), i))
    model.train()
    v = tot / max(1, len(val))
    if world > 1:                  # every rank validates its own shard: the monitored value is the mean over ranks
        from mask_bev_amd.ddp import reduce_scalars
        v = reduce_scalars({'val_loss': torch.tensor(v, device=device)})['val_loss']
    return float(v)


def train(args, config, model, optimizer, scheduler, reducer, data, val, device, rank, world, checkpoint_folder_path, check_metric,
          average=None):
    model.train()
    if rank == 0:
        checkpoint_folder_path.mkdir(parents=True, exist_ok=True)
    exp_name = checkpoint_folder_path.name
    graphed, step_count, best = None, 0, float('inf')
    # EarlyStopping(check_metric, patience=30) of the reference's Trainer (train_mask_bev.py:100): stop after 30
    # epochs without an improvement of the monitored metric (Lightning's default min_delta = 0, mode = 'min')
    es_best, es_wait, es_patience = float('inf'), 0, 30
    # a flat optimizer with clipping (K41) keeps the last step's gradient norm and clip coefficient on the device
    clipping = getattr(optimizer, 'max_grad_norm', None) is not None
    clip_val = config.get('gradient_clip_val', None)
    # a weight average (K43) starts at `weight_average_start_epoch` (SWA: average the tail of the run only): before it there
    # are no updates, validation reads the live weights and the checkpoints carry no average
    average_start, averaging = int(config.get('weight_average_start_epoch', 0)), None
    for epoch in range(args.max_epochs):
        model.current_epoch = epoch
        if average is not None and epoch == average_start:
            average.reset()
            averaging = average
            if graphed is not None:
                graphed.average = average
        t0, loss_sum, n_steps = time.perf_counter(), None, 0
        clip_stats = ClipStats()
        n_batches = int(len(data) * float(config.get('limit_train_batches', 1.0))) if isinstance(
            config.get('limit_train_batches', 1.0), float) else int(config.get('limit_train_batches'))
        for i in range(max(1, n_batches)):
            batch = data.batch(epoch, i)
            if not args.no_graph and getattr(model, '_arena', None) is not None:
                if graphed is None:
                    from mask_bev_amd.graph import GraphedTrainStep
                    if reducer is not None:
                        reducer.no_sync(True)
                    graphed = GraphedTrainStep(model, optimizer, batch, reducer=reducer, average=averaging)
                loss = graphed.step(batch)
            else:
                if reducer is not None:
                    reducer.sync_buffers()
                loss = model.training_step(batch, i)
                model.scale_loss(loss).backward()
                if reducer is not None:
                    reducer.finish(optimizer)
                clip_gradients(optimizer, model.parameters(), clip_val)     # per-tensor optimizers; a flat one clips itself
                optimizer.step()
                if averaging is not None:
                    averaging.update()
                optimizer.zero_grad(set_to_none=False)
            # accumulate on the device: the graphed step returns ONE static tensor that every replay overwrites,
            # so keeping references would average N aliases of the last batch's loss (the reference monitors the
            # epoch mean of train_loss, mask_bev_module.py:296 `self.log('train_loss', ..., on_epoch=True)`)
            loss_sum = loss.detach().clone() if loss_sum is None else loss_sum + loss.detach()
            if clipping:           # views of the optimizer's record, which the next step overwrites: summed on the device too
                clip_stats.add(optimizer.grad_norm, optimizer.clip_coef)
            n_steps += 1
            step_count += 1
            if 0 < args.max_steps <= step_count:
                break
        train_loss = float(loss_sum) / max(1, n_steps)
        if world > 1:
            from mask_bev_amd.ddp import reduce_scalars
            train_loss = reduce_scalars({'train_loss': torch.tensor(train_loss, device=device)})['train_loss']
        val_loss = validate(model, val, epoch, device, world, averaging)
        monitored = val_loss if (check_metric == 'val_loss' and val_loss is not None) else train_loss
        if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
            scheduler.step(train_loss)                          # monitor 'train_loss', interval 'epoch'
        else:
            scheduler.step()
        if rank == 0:
            dt = time.perf_counter() - t0
            print(f'epoch {epoch}: train_loss {train_loss:.6f}'
                  + (f' val_loss {val_loss:.6f}' if val_loss is not None else '')
                  + (' ' + clip_stats.line(n_steps) if clipping else '')
                  + f'  {n_steps * int(config.get("batch_size", 1)) * world / dt:.1f} scans/s', flush=True)
            save_checkpoint(model, optimizer, checkpoint_folder_path / 'last.ckpt', epoch, check_metric, monitored, averaging)
            if monitored < best:
                best = monitored
                for old in checkpoint_folder_path.glob(f'{exp_name}-epoch=*'):
                    old.unlink()
                save_checkpoint(model, optimizer, checkpoint_folder_path /
                                f'{exp_name}-epoch={epoch:02d}-{check_metric}={monitored:.6f}.ckpt', epoch,
                                check_metric, monitored, averaging)
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


def load_averaged_weights(model, average, checkpoint_path, rank):
    """--test with `weight_average` set: the checkpoint's averaged weights (K43) take the place of the live ones in the model,
    when the checkpoint has them.  Buffers stay the live ones.  Prints what was loaded in one line."""
    if average is None:
        return False
    entry = torch.load(checkpoint_path, map_location='cpu', weights_only=False).get('weight_average')
    if entry is None:
        return False
    average.load_state_dict(entry)
    with torch.no_grad():
        model._arena.param.copy_(average.avg)
    model._arena.refresh_shadow()
    if rank == 0:
        print(f'weight average: {average.mode}, ' + (f'decay {average.decay:g}, ' if average.mode == 'ema' else '')
              + f'{int(average.num_updates)} updates', flush=True)
    return True


def test(args, config, model, val, dataset_name, device, rank, world):
    """The reference runs trainer.validate then trainer.test (train_mask_bev.py:118-119); MaskBevModule defines no test_step
    (SURVEY Appendix B), so the test pass has nothing of its own to run: validation, then the extras of mask_bev_amd/evaluate.py."""
    lifting = evaluate.lift_settings(config)   # None unless `lift_ground: true` (K35)
    resolving = evaluate.resolve_settings(config)   # None unless `predict_resolve: true` (K42)
    layers = tuple(range(model.num_layers))    # the reference attaches its metrics to all ten decoder outputs (:85-98)
    if val is not None:
        # what trainer.validate logs there: COCO mask AP (K29), mIoU and class AP of every decoder layer
        model.enable_metrics(layers=layers, train=False, val=True, mask_map='device')
    v = validate(model, val, 0, device, world)
    if val is not None:
        model.on_validation_epoch_end()            # every rank: the mask AP gathers the states of all ranks
    if rank == 0:
        print(f'val_loss {v}' if v is not None else 'no validation data configured')
        if val is not None:
            for layer in layers:
                print(evaluate.format_layer_metrics(model.logged, layer), flush=True)
        if resolving is not None and val is not None:
            print(evaluate.format_resolve_settings(resolving), flush=True)
        if dataset_name == 'kitti' and val is not None:
            # what the reference's mask_to_pred + eval_kitti are for: boxes from the predicted masks, KITTI BEV AP
            # (`kitti_3d: true`: with the heights lifted from the scans, and the 3D AP lines)
            if lifting is not None and config.get('kitti_3d', False):
                print(evaluate.format_lift_settings(lifting, config['voxel_size']), flush=True)
            print(evaluate.kitti_bev_evaluation(model, config, device, args.data_root), end='', flush=True)
    if args.render and rank == 0 and val is not None and dataset_name == 'kitti':
        tree = datasets.KittiFrames(args.data_root, 'val')
        paths = evaluate.render_frames(model, config, device, [tree.scan(f) for f in tree.frames], args.render, dataset='kitti',
                                       label_boxes=[tree.labels(f)['boxes'] for f in tree.frames])
        print(f'wrote {len(paths)} frames under {args.render}', flush=True)
    if dataset_name != 'semantic-kitti' or val is None:
        return
    if lifting is not None and rank == 0:
        print(evaluate.format_lift_settings(lifting, config['voxel_size']), flush=True)
    # point-level panoptic quality of the lifted labels, when the ground truth lies next to every validated scan
    have = all(evaluate.semantic_kitti_label_path(f).exists() for f, _ in val.files)
    if world > 1:                              # every rank or none: compute() sums the ranks
        flag = torch.tensor([int(have)], device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        have = bool(int(flag))
    metric = evaluate.point_panoptic_evaluation(model, config, device, val.files) if have else None
    if metric is not None:
        result = metric.compute()
        if rank == 0:
            print(evaluate.format_point_panoptic(result, evaluate.panoptic_settings(config)[1]), flush=True)
    tracked = None
    track = bool(config.get('track_instances', False))
    if track and rank == 0:
        # global instance ids over the validation sequences (K33), LSTQ of the predicted thing classes when labels exist
        tracked = evaluate.sequence_tracking(model, config, device, args.data_root, config.get('val_sequences', [8]),
                                             out_dir=args.write_labels)
        if tracked is not None and 'lstq' in tracked:
            print(evaluate.format_point_lstq(tracked), flush=True)
        if tracked is not None and args.write_labels:
            print(f'wrote {len(tracked["written"])} label files with track ids under {args.write_labels}', flush=True)
    if track and world > 1 and args.write_labels:
        flag = torch.tensor([int(tracked is not None)], device=device)
        dist.broadcast(flag, 0)                    # rank 0 wrote every scan with its track id, or nobody did
        if int(flag) and tracked is None:
            tracked = {}
    if args.write_labels and tracked is None:
        paths = evaluate.write_point_labels(model, config, device, val.files, args.write_labels)     # every rank: its own scans
        print(f'wrote {len(paths)} label files under {args.write_labels}', flush=True)
    if args.render and rank == 0:
        scans_of = [f for seq in config.get('val_sequences', [8])
                    for f in sorted((pathlib.Path(args.data_root) / 'sequences' / f'{int(seq):02d}' / 'velodyne').glob('*.bin'))]
        paths = evaluate.render_frames(model, config, device, scans_of, args.render)
        print(f'wrote {len(paths)} frames under {args.render}', flush=True)


def build_parser():
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
    parser.add_argument('--gradient-clip-val', type=float, default=None,
                        help='clip the global 2-norm of the gradient at this value (overrides the YAML gradient_clip_val)')
    parser.add_argument('--weight-average', default=None, choices=['ema', 'mean'],
                        help='keep an averaged copy of the weights, validate and checkpoint it (overrides the YAML weight_average)')
    parser.add_argument('--no-graph', action='store_true', help='launch every kernel eagerly (no HIP-graph replay)')
    parser.add_argument('--checkpoint-root', default='checkpoints')
    parser.add_argument('--build-object-bank', action='store_true',
                        help='dataset: kitti: write the object bank of object_sample from the training split and exit')
    parser.add_argument('--build-scene-bank', action='store_true',
                        help='dataset: semantic-kitti: write sequences/SS/instance_points.npz of the train and validation '
                             'sequences and exit')
    parser.add_argument('--build-mask-cache', action='store_true',
                        help='dataset: semantic-kitti: write sequences/SS/mask_cache/NNNNNN.npy of the train and validation '
                             'sequences through the scene banks and exit')
    parser.add_argument('--overwrite', action='store_true', help='--build-mask-cache: rewrite the files that exist')
    parser.add_argument('--write-labels', default=None, metavar='DIR',
                        help='dataset: semantic-kitti with --test: write the per-point instance labels of every validated '
                             'scan to DIR/sequences/SS/predictions/NNNNNN.label')
    parser.add_argument('--render', default=None, metavar='DIR',
                        help='with --test: write one BEV frame per validated scan, composed on the GPU, to '
                             'DIR/sequences/SS/bev/NNNNNN.png (dataset: semantic-kitti) or DIR/NNNNNN.png (dataset: kitti)')
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.render and not args.test:
        parser.error('--render needs --test')

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
    if args.gradient_clip_val is not None:
        config['gradient_clip_val'] = args.gradient_clip_val
    if args.weight_average is not None:
        config['weight_average'] = args.weight_average

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
        datasets.build_object_bank(config, device, args.data_root or 'data/KITTI')
        return
    if args.build_scene_bank or args.build_mask_cache:
        if config.get('dataset', 'semantic-kitti') != 'semantic-kitti':
            raise ValueError('--build-scene-bank and --build-mask-cache need dataset: semantic-kitti')
        root = args.data_root or 'data/SemanticKITTI'
        sequences = list(dict.fromkeys(list(config.get('train_sequences', [0, 1, 2, 3, 4, 5, 6, 7, 9, 10]))
                                      + list(config.get('val_sequences', [8]))))         # each sequence once
        if args.build_scene_bank:
            datasets.build_scene_banks(config, root, sequences)
        if args.build_mask_cache:
            datasets.build_mask_cache(config, device, root, sequences, args.overwrite)
        return
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        backend = os.environ.get('MBV_DIST_BACKEND', 'nccl')       # 'nccl' is RCCL on ROCm
        dist.init_process_group(backend, **({'device_id': device} if backend == 'nccl' else {}))

    model = MaskBevModule.from_config(config, checkpoint_folder_path).to(device)
    model.log_scalars = False
    model.flatten_parameters()         # fp16 compute: this also creates the device-side loss scaler
    opt_cfg = model.configure_optimizers()
    optimizer, scheduler = opt_cfg['optimizer'], opt_cfg['lr_scheduler']
    average = model.make_weight_average()      # None unless `weight_average: ema | mean` (K43)

    reducer = None
    if world > 1:
        from mask_bev_amd.ddp import GradientAllReducer
        reducer = GradientAllReducer(model, bucket_mb=64.0)

    dataset_name = 'synthetic' if args.synthetic else config.get('dataset', 'semantic-kitti')
    if dataset_name == 'synthetic':
        data = datasets.SyntheticBatches(config, device, rank, args.steps_per_epoch)
        val = None
    elif dataset_name == 'semantic-kitti':
        args.data_root = args.data_root or 'data/SemanticKITTI'
        targets = config.get('semantic_kitti_targets', 'cache')
        if targets not in ('cache', 'scenes'):
            raise ValueError(f'semantic_kitti_targets must be cache or scenes, got {targets}')
        reader = datasets.SemanticKittiSceneBatches if targets == 'scenes' else datasets.SemanticKittiCacheBatches
        data = reader(config, device, rank, world, args.data_root,
                      config.get('train_sequences', [0, 1, 2, 3, 4, 5, 6, 7, 9, 10]), augment=True)
        val = reader(dict(config, shuffle_train=False), device, rank, world, args.data_root,
                     config.get('val_sequences', [8])) if limit_val_batches > 0 else None
    elif dataset_name == 'kitti':
        args.data_root = args.data_root or 'data/KITTI'
        data = datasets.KittiObjectBatches(config, device, rank, world, args.data_root, 'train', augment=True)
        val = datasets.KittiObjectBatches(dict(config, shuffle_train=False), device, rank, world, args.data_root,
                                          'val') if limit_val_batches > 0 else None
    elif dataset_name == 'waymo':
        raise NotImplementedError('dataset: waymo is not read by this launcher (torch_waymo frames); build batches from '
                                  'box tables with mask_bev_amd.rasterize.WaymoRasterizer and mask_bev_amd.batch.BoxCollate')
    else:
        raise NotImplementedError(dataset_name)

    if is_training:
        train(args, config, model, optimizer, scheduler, reducer, data, val, device, rank, world, checkpoint_folder_path,
              check_metric, average)
    if is_testing:
        load_averaged_weights(model, average, config['checkpoint'], rank)
        test(args, config, model, val, dataset_name, device, rank, world)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
