"""What ``--test`` runs after the validation loss, one pass over the scans per feature: KITTI BEV / 3D AP (K25-K27, K30, K31),
per-point labels (K31), their panoptic quality (K32), tracking with LSTQ (K33), BEV frames as PNG files (K36); the settings and printed lines of each.  With
``predict_resolve: true`` every one of these passes predicts with mask NMS and the overlap filter among the kept queries (K42).  With
``lift_ground: true`` every lift labels only the returns above a ground estimate made from the scan itself (K35)."""
import pathlib

import numpy as np
import torch

from . import batch as B
from .datasets import KittiFrames, semantic_kitti_files
from .kitti_eval import eval_kitti
from .metrics import DevicePanopticQuality, DeviceTubeAssociation, lstq, semantic_kitti_class_lut
from .predict import BOX_METHODS, GroundSettings, ResolveSettings, write_semantic_kitti_labels
from .tracking import FootprintFusion, FusionSettings, InstanceTracker, MotionSettings, OcclusionSettings, velodyne_poses


def resolve_settings(config):
    """``predict_resolve: true``: the :class:`~mask_bev_amd.predict.ResolveSettings` (K42: mask NMS and the overlap filter among
    the kept queries) from ``predict_nms_iou`` ([1, 2]; null: no NMS), ``predict_min_overlap`` ([4, 5]; null: only the cell
    count), ``predict_min_cells`` (1) and ``predict_exclusive_masks`` (false); ``None`` without the key.  The defaults are the
    conventional mask-NMS IoU and Mask2Former's OVERLAP_THRESHOLD, not tuned here."""
    if not bool(config.get('predict_resolve', False)):
        return None
    ratio = lambda key, default: None if config.get(key, default) is None else tuple(config.get(key, default))
    return ResolveSettings(nms_iou=ratio('predict_nms_iou', (1, 2)), min_overlap=ratio('predict_min_overlap', (4, 5)),
                           min_cells=config.get('predict_min_cells', 1),
                           exclusive=bool(config.get('predict_exclusive_masks', False)))


def format_resolve_settings(settings):
    """The line ``--test`` prints in front of the results that ``predict_resolve: true`` changes."""
    ratio = lambda r: 'off' if r is None else f'{r[0]}/{r[1]}'
    return (f'resolved predictions: nms_iou {ratio(settings.nms_iou)}, min_overlap {ratio(settings.min_overlap)}, '
            f'min_cells {settings.min_cells}' + (', exclusive masks' if settings.exclusive else ''))


def predictions(model, scan_paths, bsz, device, score_threshold=0.0, resolve=None):
    """``(paths, scans, pred)`` per batch of ``bsz`` of ``scan_paths``: the scans on the device and ``model.predict`` of them —
    the one place ``--test`` predicts; ``resolve``: :func:`resolve_settings` of the configuration (K42)."""
    bsz = max(1, int(bsz))
    for start in range(0, len(scan_paths), bsz):
        part = scan_paths[start:start + bsz]
        scans = [torch.from_numpy(B.read_velodyne_bin(f)).to(device) for f in part]
        if resolve is None:
            yield part, scans, model.predict(scans, score_threshold)
        else:
            yield part, scans, model.predict(scans, score_threshold, resolve=resolve)


def semantic_kitti_label_path(scan_path):
    """``sequences/SS/velodyne/NNNNNN.bin`` → ``sequences/SS/labels/NNNNNN.label``, the ground truth next to a scan."""
    scan_path = pathlib.Path(scan_path)
    return scan_path.parent.parent / 'labels' / (scan_path.stem + '.label')


def read_label_words(path, device):
    """The ``uint32`` words of a ``.label`` file as an int32 tensor on the device, as K32 and K33 take them."""
    return torch.from_numpy(np.fromfile(str(path), dtype='<u4').view(np.int32)).to(device)


def prediction_label_path(out_dir, scan_path):
    """``sequences/SS/velodyne/NNNNNN.bin`` → ``<out_dir>/sequences/SS/predictions/NNNNNN.label``; creates the folder."""
    scan_path = pathlib.Path(scan_path)
    d = pathlib.Path(out_dir) / 'sequences' / scan_path.parent.parent.name / 'predictions'
    d.mkdir(parents=True, exist_ok=True)
    return d / (scan_path.stem + '.label')


def lift_settings(config):
    """The ground-aware lift of the configuration (K35), ``None`` when off: ``lift_ground`` (default false) switches it on;
    ``lift_ground_radius`` (metres, default 1.6), ``lift_ground_clearance`` (default 0.3), ``lift_max_height`` and ``lift_z_floor``
    (default none) fill a :class:`~mask_bev_amd.predict.GroundSettings`.  With a ``voxel_size`` in the configuration the radius
    is checked here: more than 32 cells raises ``ValueError``.  The defaults rest on geometry, not on measurement."""
    if not bool(config.get('lift_ground', False)):
        return None
    opt = lambda key: None if config.get(key) is None else float(config[key])
    settings = GroundSettings(radius_m=float(config.get('lift_ground_radius', 1.6)),
                              clearance=float(config.get('lift_ground_clearance', 0.3)), max_height=opt('lift_max_height'),
                              z_floor=opt('lift_z_floor'))
    if config.get('voxel_size') is not None:
        settings.radius_cells(config['voxel_size'])
    return settings


def format_lift_settings(settings, voxel_size):
    """The line ``--test`` prints in front of the results a ground-aware lift changes."""
    extra = ''.join(f', {name} {value:g} m' for name, value in (('max height', settings.max_height), ('z floor', settings.z_floor))
                    if value is not None)
    return (f'ground-aware lift: radius {settings.radius_m:g} m ({settings.radius_cells(voxel_size)} cells), clearance '
            f'{settings.clearance:g} m{extra}')


def _ground(config):
    """``pred.lift``'s keyword for the configuration: nothing when the ground-aware lift is off."""
    settings = lift_settings(config)
    return {} if settings is None else dict(ground=settings)


def kitti_bev_evaluation(model, config, device, root, split='val', score_threshold=0.0, box_method=None):
    """Car BEV AP (easy / moderate / hard at overlaps 0.7 and 0.5) of ``model`` on every frame of ``<root>/<split>.txt``:
    ``model.predict`` per batch, an oriented box per kept mask (``Predictions.kitti_predictions``), then the KITTI protocol on
    the device (K26, K27; ``kitti_eval.eval_kitti``).  ``box_method`` (default: the configuration's ``kitti_box_method``, else
    ``moment``): ``moment`` — K25's moment-axis box of all set cells; ``min_area_rect`` — the minimum-area rectangle of the
    mask's largest component (K30), the reference's recipe.  All labels of a frame take part, unfiltered: the protocol decides
    what counts at which difficulty.  With ``kitti_3d: true`` every box gets the z-extent of the points inside its mask (K31;
    ``kitti_3d_extent: [q_lo, q_hi]``: histogram quantiles instead of the extremes) and a ``3d   AP:`` line follows every
    ``bev  AP:`` line (K26b); with ``lift_ground: true`` as well only the returns above the estimated ground count and the
    boxes stand on it (K35, ``bottom='ground'``).  Returns the result (a string with ``.metrics``)."""
    method = box_method if box_method is not None else config.get('kitti_box_method', 'moment')
    if method not in BOX_METHODS:
        raise ValueError(f'kitti_box_method must be one of {BOX_METHODS}, got {method!r}')
    with_3d = bool(config.get('kitti_3d', False))
    extent = tuple(config['kitti_3d_extent']) if config.get('kitti_3d_extent') else 'minmax'
    ground = _ground(config)
    tree = KittiFrames(root, split)
    labels, scan_paths, boxes = [tree.labels(f) for f in tree.frames], [tree.scan(f) for f in tree.frames], []
    for _, scans, pred in predictions(model, scan_paths, config.get('batch_size', 1), device, score_threshold,
                                        resolve=resolve_settings(config)):
        lift = dict(scans=scans, module=model, extent=extent) if with_3d else {}
        if with_3d and ground:
            lift.update(ground=ground['ground'], bottom='ground')
        boxes += pred.kitti_predictions(config['x_range'], config['y_range'], config['voxel_size'], method=method, **lift)
    return eval_kitti(labels, boxes, device=device)


def write_point_labels(model, config, device, files, out_dir, score_threshold=0.0, semantic_id=10):
    """Per-point instance labels of every scan of ``files`` — the (``.bin``, cache) pairs of a ``SemanticKittiCacheBatches``:
    ``model.predict`` per batch, the instance map lifted to the points (K31), one :func:`prediction_label_path` file per scan
    (``uint32``: query + 1 in the upper 16 bits, ``semantic_id`` in the lower, 0 = unlabelled).  ``lift_ground: true``: only the
    returns above the estimated ground are labelled (:func:`lift_settings`).  Returns the paths written."""
    written = []
    ground = _ground(config)
    for part, scans, pred in predictions(model, [f for f, _ in files], config.get('batch_size', 1), device, score_threshold,
                                        resolve=resolve_settings(config)):
        for f, labels in zip(part, pred.lift(scans, model, **ground).per_scan()):
            written.append(prediction_label_path(out_dir, f))
            write_semantic_kitti_labels(written[-1], labels, semantic_id)
    return written


def panoptic_settings(config):
    """The configuration's ``panoptic_min_points`` (default 50), ``panoptic_things`` (default [[10]]: raw label 10, car, is
    thing class 1; one list of raw semantic ids per thing class) and ``panoptic_ignore`` (default [0, 1, 252])."""
    things = config.get('panoptic_things', [[10]])
    things = tuple(tuple(int(i) for i in (t if isinstance(t, (list, tuple)) else [t])) for t in things)
    ignore = tuple(int(i) for i in config.get('panoptic_ignore', [0, 1, 252]))
    return int(config.get('panoptic_min_points', 50)), things, ignore


def panoptic_metric(config):
    """The K32 metric of :func:`panoptic_settings` and ``panoptic_max_gt`` (default 256: the segments a scan may hold)."""
    min_points, things, ignore = panoptic_settings(config)
    return DevicePanopticQuality(len(things) + 1, semantic_kitti_class_lut(things, ignore), min_points=min_points,
                                 max_gt=int(config.get('panoptic_max_gt', 256)))


def point_panoptic_evaluation(model, config, device, files, score_threshold=0.0):
    """Panoptic quality of the lifted point labels over ``files`` (as in :func:`write_point_labels`) against the ground truth
    next to the scans: ``model.predict`` per batch, the lift to the points (K31), the per-frame counts on the device (K32).  Returns
    the metric (``compute()`` sums the ranks: call it on every rank), or ``None`` when a label file is missing."""
    scans_of = [f for f, _ in files]
    if not scans_of or not all(semantic_kitti_label_path(f).exists() for f in scans_of):
        return None
    metric = panoptic_metric(config)
    ground = _ground(config)
    for part, scans, pred in predictions(model, scans_of, config.get('batch_size', 1), device, score_threshold,
                                        resolve=resolve_settings(config)):
        words = [read_label_words(semantic_kitti_label_path(f), device) for f in part]
        pred.panoptic_points(pred.lift(scans, model, **ground), words, metric)
    return metric


def format_point_panoptic(result, things=((10,),)):
    """The ``point PQ`` line of ``--test`` from ``DevicePanopticQuality.compute()``."""
    pc = result['per_class']
    what = 'car' if tuple(tuple(t) for t in things) == ((10,),) else f'{len(things)} thing classes'
    return (f'point PQ {result["pq"]:.4f} SQ {result["sq"]:.4f} RQ {result["rq"]:.4f} IoU {result["iou"]:.4f} '
            f'({what}; tp {sum(pc["tp"][1:])} fp {sum(pc["fp"][1:])} fn {sum(pc["fn"][1:])})')


def tracking_settings(config):
    """``track_min_iou`` (0.3), ``track_max_age`` (2), ``track_min_cells`` (4), ``track_max_tracks`` (256): ``InstanceTracker``'s.
    ``track_motion: true`` adds ``motion``, a ``MotionSettings`` (K37) from ``track_velocity_gain`` (0.5), ``track_gate`` (3.0 m)
    and ``track_max_speed`` (6.0 m per frame); without the key the result is what it was.  ``track_occlusion: true`` adds
    ``occlusion``, an ``OcclusionSettings`` (K38) from ``track_occlusion_z_top`` (-0.2 m), ``track_hidden_fraction`` ([1, 2]) and
    ``track_max_hold`` (10 frames); without the key the result is what it was."""
    out = dict(min_iou=float(config.get('track_min_iou', 0.3)), max_age=int(config.get('track_max_age', 2)),
               min_cells=int(config.get('track_min_cells', 4)), max_tracks=int(config.get('track_max_tracks', 256)))
    if bool(config.get('track_motion', False)):
        out['motion'] = MotionSettings(gain=float(config.get('track_velocity_gain', 0.5)), gate_m=float(config.get('track_gate', 3.0)),
                                       max_speed=float(config.get('track_max_speed', 6.0)))
    if bool(config.get('track_occlusion', False)):
        out['occlusion'] = OcclusionSettings(z_top=float(config.get('track_occlusion_z_top', -0.2)),
                                             hidden_fraction=tuple(config.get('track_hidden_fraction', (1, 2))),
                                             max_hold=int(config.get('track_max_hold', 10)))
    return out


def fusion_settings(config):
    """``track_fuse: true``: the ``FusionSettings`` (K39) from ``track_fuse_cap`` (8), ``track_fuse_min_count`` (2) and, with
    ``track_motion: true`` only, ``track_fuse_static_speed`` (0.5 m per frame: a query faster than that is passed through, not
    accumulated); ``None`` without the key."""
    if not bool(config.get('track_fuse', False)):
        return None
    speed = float(config.get('track_fuse_static_speed', 0.5)) if bool(config.get('track_motion', False)) else None
    return FusionSettings(cap=int(config.get('track_fuse_cap', 8)), min_count=int(config.get('track_fuse_min_count', 2)),
                          static_speed=speed)


def _fusion(config, device):
    settings = fusion_settings(config)
    if settings is None:
        return None
    return FootprintFusion(config['x_range'], config['y_range'], config['voxel_size'], int(config['num_queries']), settings,
                           device=device)


def _track(pred, tracker, fusion, poses, vis):
    """The tracker step of a batch and, with ``fusion``, K39 behind it → (the predictions to lift, label and render from,
    query_track)."""
    if fusion is None:
        return pred, pred.track(tracker, poses=poses, visibility=vis)
    rec = tracker.update(pred.instance_map, poses=poses, record=True, **({} if vis is None else dict(visibility=vis)))
    return pred.fused(fusion, rec.query_track, poses=poses, visibility=vis, query_velocity=rec.query_velocity)[0], rec.query_track


def sequence_tracking(model, config, device, root, sequences, out_dir=None, score_threshold=0.0, semantic_id=10):
    """``track_instances: true``: one pass over the scans of ``sequences`` in scan order, on ONE rank — predict, the tracker step
    on the BEV instance maps (K33a; reset at every sequence change, the ego motion from the sequence's ``poses.txt`` and
    ``calib.txt``), the lift to the points (K31) and the per-point track ids.  With ``labels/NNNNNN.label`` next to every scan the
    tube association (K33b) per sequence and the panoptic IoU (K32) of this rank alone over the same frames; with ``out_dir`` the
    ``.label`` files carry the track id + 1 as the instance id.  Returns ``None`` — after one line that says why — when a
    sequence lacks ``poses.txt`` or ``calib.txt``, else ``{'tracks', 'dropped', 'frames', 'written'}`` (with ``track_motion: true``
    the tracker runs K37's motion model and ``'gated'`` is added; with ``track_occlusion: true`` the visibility map of every
    batch is computed from the scans already read, K38, and ``'held'`` is added) plus, with labels,
    ``{'lstq', 's_assoc', 's_cls', 'tubes'}``.  With ``track_fuse: true`` (K39, :func:`fusion_settings`) the tracker still steps on
    the model's own maps, but the lift, the written labels, the tube association and the panoptic IoU come from the fused
    predictions (``Predictions.fused``), and ``'fused': True`` is added.  Not pinned: parity with semantic-kitti-api's 4D evaluator, LSTQ on real data."""
    by_seq = {}
    for f, _ in semantic_kitti_files(root, sequences):
        by_seq.setdefault(f.parent.parent, []).append(f)
    missing = [d for d in by_seq if not ((d / 'poses.txt').exists() and (d / 'calib.txt').exists())]
    if missing:
        print(f'track_instances: skipped, poses.txt or calib.txt is missing under {missing[0]}', flush=True)
        return None
    have_labels = all(semantic_kitti_label_path(f).exists() for scans_of in by_seq.values() for f in scans_of)
    tracker = InstanceTracker(config['x_range'], config['y_range'], config['voxel_size'], int(config['num_queries']),
                              device=device, **tracking_settings(config))
    fusion = _fusion(config, device)
    quality = panoptic_metric(config)
    tubes = DeviceTubeAssociation(quality.num_classes, quality.class_lut('cpu'), id_limit=int(config.get('track_id_limit', 1024)),
                                  max_tracks=int(config.get('track_tube_tracks', 4096)))      # the same classes as `quality`
    out = dict(tracks=0, dropped=0, frames=0, written=[])
    ground = _ground(config)
    assoc_sum, n_tubes = 0.0, 0
    for seq_dir, scans_of in by_seq.items():
        poses = velodyne_poses(B.read_poses(seq_dir / 'poses.txt'), B.read_calib(seq_dir / 'calib.txt'))
        tracker.reset()
        tubes.reset()
        if fusion is not None:
            fusion.reset()
        for part, scans, pred in predictions(model, scans_of, config.get('batch_size', 1), device, score_threshold,
                                        resolve=resolve_settings(config)):
            vis = pred.visibility(scans, model, tracker.occlusion) if tracker.occlusion is not None else None
            pred, query_track = _track(pred, tracker, fusion, poses[[int(f.stem) for f in part]], vis)
            lifted = pred.lift(scans, model, **ground)
            ids = pred.point_tracks(lifted, query_track)
            if have_labels:
                words = [read_label_words(semantic_kitti_label_path(f), device) for f in part]
                tubes.update(ids, words[0] if len(words) == 1 else torch.cat(words))
                pred.panoptic_points(lifted, words, quality)
            if out_dir is not None:
                for f, labels, tracks in zip(part, lifted.per_scan(), torch.split(ids, list(lifted.lengths))):
                    out['written'].append(prediction_label_path(out_dir, f))
                    write_semantic_kitti_labels(out['written'][-1], labels, semantic_id, instance_ids=tracks)
        counts = tracker.counters()
        for key in ('tracks', 'dropped', 'frames') + tuple(k for k in ('gated', 'held') if k in counts):
            out[key] = out.get(key, 0) + counts[key]
        if have_labels:
            res = tubes.compute()                  # per sequence: SemanticKITTI's instance ids are unique inside one only
            assoc_sum += res['s_assoc'] * res['tubes']
            n_tubes += res['tubes']
    if fusion is not None:
        out['fused'] = True
    if have_labels:
        s_assoc = assoc_sum / max(n_tubes, 1)
        s_cls = quality.compute(reduce=False)['iou'] if quality.frames else 0.0     # compute() would wait for the other ranks
        out.update(lstq=lstq(s_assoc, s_cls), s_assoc=s_assoc, s_cls=s_cls, tubes=n_tubes)
    return out


def format_point_lstq(result):
    """The ``point LSTQ`` line of ``--test`` from :func:`sequence_tracking`."""
    gated = f', gated {result["gated"]}' if 'gated' in result else ''                  # K37: with ``track_motion: true`` only
    held = f', held {result["held"]}' if 'held' in result else ''                      # K38: with ``track_occlusion: true`` only
    fused = ', fused' if result.get('fused') else ''                                   # K39: with ``track_fuse: true`` only
    return (f'point LSTQ {result["lstq"]:.4f} S_assoc {result["s_assoc"]:.4f} S_cls {result["s_cls"]:.4f} '
            f'(tubes {result["tubes"]}, tracks {result["tracks"]}, dropped {result["dropped"]}{gated}{held}{fused})')


def format_layer_metrics(logged, layer):
    """One line of ``--test`` per decoder layer from the module's logged values (mask_bev_module.py:209-224)."""
    parts = [f'{n} {logged[f"val_mAP_{layer}_{n}"]:.4f}' for n in ('map', 'map_50', 'map_75', 'mar_100')]
    parts += [f'mIoU {logged[f"val_mIoU_layer_{layer}"]:.4f}', f'cls_AP {logged[f"val_cls_mAP_layer_{layer}"]:.4f}']
    return f'layer {layer}: ' + ' '.join(parts)


def render_settings(config):
    """The :class:`~mask_bev_amd.render.RenderSettings` of a configuration: ``render_scale`` (pixels per cell, default 2) and
    ``render_alpha`` (0 .. 256, default 128); everything else keeps its default."""
    from .render import RenderSettings
    return RenderSettings(scale=int(config.get('render_scale', 2)), alpha=int(config.get('render_alpha', 128)))


def render_frame_path(out_dir, scan_path, dataset):
    """``dataset: semantic-kitti``: ``sequences/SS/velodyne/NNNNNN.bin`` → ``<out_dir>/sequences/SS/bev/NNNNNN.png``; ``kitti``:
    ``<out_dir>/NNNNNN.png``.  Creates the folder."""
    scan_path, d = pathlib.Path(scan_path), pathlib.Path(out_dir)
    if dataset == 'semantic-kitti':
        d = d / 'sequences' / scan_path.parent.parent.name / 'bev'
    d.mkdir(parents=True, exist_ok=True)
    return d / (scan_path.stem + '.png')


def _cached_maps(part, shape, device):
    """The mask-cache maps next to the scans ``part`` as one (B, ny, nx) int32 device map (a scan without a file: background),
    ``None`` when no scan has one."""
    paths = [pathlib.Path(f).parent.parent / 'mask_cache' / (pathlib.Path(f).stem + '.npy') for f in part]
    if not any(p.exists() for p in paths):
        return None
    ny, nx = shape
    maps = [np.asarray(B.read_mask_cache(p)).astype(np.int32) if p.exists() else np.zeros((nx, ny), np.int32) for p in paths]
    if any(m.shape != (nx, ny) for m in maps):
        raise ValueError(f'render_frames: a mask cache next to {part[0]} is not the (nx, ny) = {(nx, ny)} map of the configuration')
    return torch.from_numpy(np.stack(maps)).to(device).permute(0, 2, 1).contiguous()       # the cache is (nx, ny)


def render_frames(model, config, device, scan_paths, out_dir, dataset='semantic-kitti', label_boxes=None, score_threshold=0.0):
    """``--render DIR``: one PNG per scan of ``scan_paths`` (:func:`render_frame_path`), composed on the device (K36,
    ``Predictions.render``) from ``model.predict`` per batch: the returns per cell underneath, every predicted instance in its
    colour (:func:`render_settings`).  ``dataset='semantic-kitti'`` — ``scan_paths`` in scan order: the contour of the mask
    cache's instances where ``mask_cache/NNNNNN.npy`` lies next to a scan; with ``track_instances: true`` the colours are the
    track ids of an ``InstanceTracker`` of this pass's own, reset at every sequence change (K33a; ``poses.txt`` and
    ``calib.txt`` of the sequence, without them one line says so and the colours are the query indices); with ``track_fuse: true``
    in addition the frames are drawn from the fused predictions (K39).  ``dataset='kitti'``:
    with ``render_boxes`` (default true) the predicted boxes and ``label_boxes`` — per scan an (n, 7) array in the velodyne
    frame — in a second colour.  Returns the paths written."""
    from .render import write_png
    settings, written = render_settings(config), []
    if dataset == 'kitti':
        with_boxes = bool(config.get('render_boxes', True))
        ranges = (config['x_range'], config['y_range'], config['voxel_size'])
        start = 0
        for part, scans, pred in predictions(model, list(scan_paths), config.get('batch_size', 1), device, score_threshold,
                                        resolve=resolve_settings(config)):
            gt = None if (label_boxes is None or not with_boxes) else list(label_boxes[start:start + len(part)])
            start += len(part)
            frames = pred.render(settings, scans=scans, module=model, boxes='pred' if with_boxes else None, gt_boxes=gt,
                                 ranges=ranges if with_boxes else None).cpu().numpy()
            for f, frame in zip(part, frames):
                written.append(render_frame_path(out_dir, f, dataset))
                write_png(written[-1], frame)
        return written
    by_seq = {}
    for f in scan_paths:
        by_seq.setdefault(pathlib.Path(f).parent.parent, []).append(pathlib.Path(f))
    track = bool(config.get('track_instances', False))
    if track and any(not ((d / 'poses.txt').exists() and (d / 'calib.txt').exists()) for d in by_seq):
        print('render: poses.txt or calib.txt is missing, colours are query indices', flush=True)
        track = False
    tracker = InstanceTracker(config['x_range'], config['y_range'], config['voxel_size'], int(config['num_queries']),
                              device=device, **tracking_settings(config)) if track else None
    fusion = _fusion(config, device) if track else None
    for seq_dir, scans_of in by_seq.items():
        if track:
            poses = velodyne_poses(B.read_poses(seq_dir / 'poses.txt'), B.read_calib(seq_dir / 'calib.txt'))
            tracker.reset()
            if fusion is not None:
                fusion.reset()
        for part, scans, pred in predictions(model, scans_of, config.get('batch_size', 1), device, score_threshold,
                                        resolve=resolve_settings(config)):
            vis = pred.visibility(scans, model, tracker.occlusion) if track and tracker.occlusion is not None else None
            query_track = None
            if track:
                pred, query_track = _track(pred, tracker, fusion, poses[[int(f.stem) for f in part]], vis)
            frames = pred.render(settings, scans=scans, module=model, query_track=query_track,
                                 gt_maps=_cached_maps(part, pred.grid_hw, device)).cpu().numpy()
            for f, frame in zip(part, frames):
                written.append(render_frame_path(out_dir, f, dataset))
                write_png(written[-1], frame)
    return written
