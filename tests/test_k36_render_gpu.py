"""K36 (csrc/render.hip) through the C ABI and what is built on it: ``ops.cell_counts``, ``ops.render_bev``,
``Predictions.render``, the launcher's ``--render``.

Image and ``skipped`` BIT-equal to the plain-loop restatement (tests/render_ref.py), written into poisoned buffers between
canaries.  The grid is 37 x 29 cells (gx x gy): at scale 3 a row is 111 pixels = 333 bytes, at scale 2 it is 222 bytes — no
multiple of 4 either — so quads of four pixels straddle cells, rows and the two scans; at scale 1 the whole image is
2 * 29 * 37 = 2146 pixels, no multiple of 4, so the last quad is short.  No tolerances."""
import types

import numpy as np
import pytest
import torch

from tests import render_ref as R
from tests.util_cfg import tiny_kwargs

pytestmark = pytest.mark.gpu
GX, GY, B, Q, P = 37, 29, 2, 6, 5
PAD, CANARY = 256, 0xA5
BAD_ARG, UNSUPPORTED = -1, -3


def _dev(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _pack(rgb):
    return int(rgb[0]) | (int(rgb[1]) << 8) | (int(rgb[2]) << 16)


def _raw_render(lib, device, batch, gy, gx, scale, flip_rows=False, counts=None, density_lut=None, instance_map=None, num_queries=0,
                id_table=None, palette=None, alpha=128, untracked_rgb=(128, 128, 128), gt_map=None, gt_background=0,
                gt_rgb=(255, 255, 255), box_corners=None, box_rgb=None, box_offsets=None, line=2):
    """mbv_render_bev into a poisoned image and a poisoned ``skipped`` between canaries → (rc, image, skipped) on the host."""
    from mask_bev_amd.ops_core import _ptr, _stream
    n = batch * gy * scale * gx * scale * 3
    raw = torch.full((PAD + (n + 255) // 256 * 256 + PAD,), CANARY, dtype=torch.uint8, device=device)
    raw[PAD:PAD + n] = 0x5a
    raw_s = torch.full((64 + batch + 64,), 0x5a5a5a5a, dtype=torch.int32, device=device)
    t = {k: _dev(v, device) for k, v in dict(counts=counts, density_lut=density_lut, instance_map=instance_map, id_table=id_table,
                                             palette=palette, gt_map=gt_map, box_corners=box_corners, box_rgb=box_rgb,
                                             box_offsets=box_offsets).items()}
    rc = lib.mbv_render_bev(batch, gx, gy, scale, 1 if flip_rows else 0, _ptr(t['counts']), _ptr(t['density_lut']),
                            _ptr(t['instance_map']), num_queries, _ptr(t['id_table']), _ptr(t['palette']),
                            0 if palette is None else len(palette), alpha, _pack(untracked_rgb), _ptr(t['gt_map']), gt_background,
                            _pack(gt_rgb), _ptr(t['box_corners']), _ptr(t['box_rgb']), _ptr(t['box_offsets']),
                            0 if box_corners is None else len(box_corners), line, raw[PAD:].data_ptr(),
                            raw_s[64:].data_ptr(), _stream())
    torch.cuda.synchronize()
    host, host_s = raw.cpu().numpy(), raw_s.cpu().numpy()
    assert np.all(host[:PAD] == CANARY) and np.all(host[PAD + n:] == CANARY), 'the kernel wrote outside the image'
    assert np.all(host_s[:64] == 0x5a5a5a5a) and np.all(host_s[64 + batch:] == 0x5a5a5a5a)
    return rc, host[PAD:PAD + n].reshape(batch, gy * scale, gx * scale, 3), host_s[64:64 + batch]


def _check(lib, device, scale, **tables):
    want, want_skipped = R.render(B, GY, GX, scale, **tables)
    rc, got, skipped = _raw_render(lib, device, B, GY, GX, scale, **tables)
    assert rc == 0
    bad = np.argwhere(np.any(got != want, axis=-1))
    assert len(bad) == 0, f'{len(bad)} pixels differ, the first at (b, row, column) {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}'
    assert np.array_equal(skipped, want_skipped)
    return got, skipped


def _layers(seed=36):
    """Every layer's tables on the 37 x 29 grid, keyed by layer."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 40, (B, GY, GX)).astype(np.int32)
    counts[rng.random((B, GY, GX)) < 0.4] = 0
    counts[0, 0, 0], counts[1, GY - 1, GX - 1], counts[1, 3, 3] = 40000, 2 ** 31 - 1, -5
    lut = rng.integers(0, 256, (16, 3)).astype(np.uint8)
    imap = np.full((B, GY, GX), -1, np.int32)
    for b in range(B):
        for q in range(Q + 2):                                   # Q and Q + 1 are not queries: not drawn
            y, x = rng.integers(0, GY - 4), rng.integers(0, GX - 5)
            imap[b, y:y + 4, x:x + 5] = q
    imap[1, GY - 1, :] = 2
    ids = np.array([[0, -1, P, 3 * P + 2, 1, -1], [7, 2, -1, 0, 2 ** 31 - 1, 4]], np.int32)          # untracked, modulo, shared ids
    palette = rng.integers(0, 256, (P, 3)).astype(np.uint8)
    gt = np.zeros((B, GY, GX), np.int32)
    gt[0, 0:5, 0:6], gt[0, GY - 3:GY, GX - 4:GX] = 1, 2            # corners: two borders each
    gt[0, 10:14, 0:3], gt[0, 10:14, 3:9] = 3, 4                    # adjacent segments with different ids, one on a border
    gt[0, 20, 20] = 5                                              # a one-cell segment
    gt[1, 0, 8:20], gt[1, GY - 1, 8:20], gt[1, 6:20, GX - 1] = 6, 7, 8
    gt[1, 5:9, 5:9], gt[1, 6:8, 6:8] = 9, 0                         # a ring: background inside
    H, W = 2 * GY, 2 * GX                                          # half-pixel units at scale 1; _boxes scales them
    return dict(density=dict(counts=counts, density_lut=lut),
                instances=dict(instance_map=imap, num_queries=Q, id_table=ids, palette=palette, density_lut=lut),
                contour=dict(gt_map=gt, density_lut=lut)), (H, W)


def _boxes(scale, many=0, seed=5):
    """Scan 0 has no box; scan 1: axis-aligned, rotated, partly outside, wholly outside, degenerate, beyond the bound, two
    overlapping ones — and ``many`` more small rotated boxes in front of those.  Half-pixel units."""
    rng = np.random.default_rng(seed)
    s = scale
    H, W = 2 * GY * s, 2 * GX * s

    def rot(cx, cy, hl, hw, yaw):
        d, e = np.array([np.cos(yaw), np.sin(yaw)]), np.array([-np.sin(yaw), np.cos(yaw)])
        c = np.array([cx, cy])
        return np.floor(np.array([c + hl * d + hw * e, c - hl * d + hw * e, c - hl * d - hw * e, c + hl * d - hw * e]) + 0.5)

    rows = [rot(rng.uniform(0, W), rng.uniform(0, H), rng.uniform(1, 9 * s), rng.uniform(1, 5 * s), rng.uniform(0, np.pi))
            for _ in range(many)]
    rows += [np.array([[8 * s, 6 * s], [30 * s, 6 * s], [30 * s, 20 * s], [8 * s, 20 * s]]),                  # axis-aligned
             rot(0.5 * W, 0.5 * H, 14 * s, 6 * s, 0.6),                                                     # rotated
             rot(W - 2 * s, 0.3 * H, 10 * s, 4 * s, 2.0),                                                   # partly outside
             rot(-40 * s, -30 * s, 6 * s, 3 * s, 0.3),                                                      # wholly outside
             np.array([[21 * s + 1, 41 * s]] * 4),                                                          # a dot
             np.array([[4, 4], [16385, 4], [16385, 40], [4, 40]]),                                          # beyond the bound
             rot(0.55 * W, 0.5 * H, 12 * s, 5 * s, -0.4), rot(0.5 * W, 0.55 * H, 3 * s, 3 * s, 0.0)]         # overlapping: later rows win
    corners = np.asarray(rows, dtype=np.int32).reshape(-1, 4, 2)
    return dict(box_corners=corners, box_rgb=rng.integers(0, 256, (len(corners), 3)).astype(np.uint8),
                box_offsets=np.array([0, 0, len(corners)], np.int32))


def _all(scale, many=0):
    layers, _ = _layers()
    tables = {}
    for part in layers.values():
        tables.update(part)
    tables.update(_boxes(scale, many))
    return tables


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('scale', [1, 2, 3])
def test_all_layers_at_every_scale(device, scale, flip):
    from mask_bev_amd import _lib
    got, skipped = _check(_lib.load(), device, scale, flip_rows=flip, **_all(scale))
    assert skipped.tolist() == [0, 1] and got.shape == (B, GY * scale, GX * scale, 3)


def test_each_layer_alone_and_none(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    layers, _ = _layers()
    lut = layers['density']['density_lut']
    rc, base, skipped = _raw_render(lib, device, B, GY, GX, 2, density_lut=lut)
    assert rc == 0 and np.all(base == lut[0]) and skipped.tolist() == [0, 0]
    rc, black, _ = _raw_render(lib, device, B, GY, GX, 2)                      # nothing at all: black
    assert rc == 0 and not black.any()
    for name, tables in layers.items():
        got, _ = _check(lib, device, 2, **tables)
        assert not np.array_equal(got, base), name
    boxes = _boxes(2)
    got, skipped = _check(lib, device, 2, density_lut=lut, **boxes)
    assert not np.array_equal(got, base) and skipped.tolist() == [0, 1]
    assert np.all(got[0] == lut[0])                                            # scan 0 has no box
    # an instance map without an id table: the colours are the queries'
    inst = dict(layers['instances'], id_table=None)
    _check(lib, device, 2, **inst)


@pytest.mark.parametrize('alpha,line', [(0, 1), (128, 2), (256, 5)])
def test_alpha_and_line(device, alpha, line):
    from mask_bev_amd import _lib
    _check(_lib.load(), device, 1, alpha=alpha, line=line, **_all(1))
    if line == 5:
        _check(_lib.load(), device, 3, alpha=alpha, line=line, flip_rows=True, **_all(3))


def test_more_boxes_than_a_chunk(device):
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    chunk = ops.RENDER_BOX_CHUNK
    assert lib.mbv_render_box_chunk() == chunk
    tables = _all(2, many=chunk + 7)                               # the special boxes lie in the second chunk
    assert tables['box_offsets'][2] - tables['box_offsets'][1] > chunk + 7
    got, skipped = _check(lib, device, 2, **tables)
    assert skipped.tolist() == [0, 1]
    # every pixel of the last row's outline has its colour, whatever lies underneath: later rows win
    r = len(tables['box_corners']) - 1
    hit = [(py, px) for py in range(2 * GY) for px in range(2 * GX) if R.box_hit(tables['box_corners'][r], 2 * px + 1, 2 * py + 1, 2)]
    assert len(hit) > 8 and all(np.array_equal(got[1, py, px], tables['box_rgb'][r]) for py, px in hit)


def test_cell_counts(device):
    from mask_bev_amd import ops
    lut = np.stack([np.arange(16)] * 3, 1).astype(np.uint8) * 16
    rng = np.random.default_rng(3)
    pc_range, voxel, grid = [-3.0, 1.5, -2.0, -3.0 + GX * 0.5, 1.5 + GY * 0.75, 2.0], [0.5, 0.75, 2.0], [GX, GY, 2]
    geom = types.SimpleNamespace(pc_range=pc_range, voxel_size=voxel, grid=grid)
    lo, hi = np.array(pc_range[:3]), np.array(pc_range[3:])
    wild = (lo + hi) / 2 + (rng.uniform(0, 1, (3001, 3)) * 2 - 1) * (hi - lo) / 2 * 1.1          # a tenth outside
    wild = np.concatenate([wild, rng.uniform(0, 1, (3001, 1))], 1).astype(np.float32)
    wild[::97, rng.integers(0, 3)] = np.nan
    wild[5], wild[6], wild[7] = [np.inf, 2, 0, 0], [lo[0], 2, 0, 0], [0, 2, hi[2], 0]
    same = np.tile(np.array([[1.26, 9.1, 0.3, 0.5]], np.float32), (40000, 1))
    for scans in ([wild, np.zeros((0, 4), np.float32), same], [same[:7, :3], wild[:500, :3]]):
        dev_scans = [torch.from_numpy(s).to(device) for s in scans]
        for prefilter in (True, False):
            got = ops.cell_counts(dev_scans, geom, prefilter=prefilter)
            want = R.cell_counts(scans, pc_range, voxel, grid, prefilter)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert want[0].max() == 7 and R.cell_counts(scans, pc_range, voxel, grid, True).sum() < sum(len(s) for s in scans)
    scans = [wild, np.zeros((0, 4), np.float32), same]
    counts = ops.cell_counts([torch.from_numpy(s).to(device) for s in scans], geom)
    want = R.cell_counts(scans, pc_range, voxel, grid)
    assert not want[1].any() and want[2].max() == 40000 and (want[2] > 0).sum() == 1
    # the picture of those counts: the cell of 40 000 returns is level 15, the empty scan is level 0 everywhere
    image, skipped = ops.render_bev(3, (GY, GX), device, scale=1, counts=counts, density_lut=torch.from_numpy(lut).to(device))
    ref, _ = R.render(3, GY, GX, 1, counts=want, density_lut=lut)
    assert np.array_equal(image.cpu().numpy(), ref) and skipped.tolist() == [0, 0, 0]
    assert ref[2].max() == 240 and not ref[1].any()
    with pytest.raises(ops.MaskBevHipError):
        ops.cell_counts([torch.zeros(4, 4)], geom)


def test_ops_render_bev_and_argument_errors(device):
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    tables = _all(3)
    want, want_skipped = R.render(B, GY, GX, 3, flip_rows=True, line=3, **tables)
    dev_tables = {k: (_dev(v, device) if isinstance(v, np.ndarray) else v) for k, v in tables.items()}
    image, skipped = ops.render_bev(B, (GY, GX), device, scale=3, flip_rows=True, line=3, **dev_tables)
    assert image.dtype == torch.uint8 and image.is_cuda and np.array_equal(image.cpu().numpy(), want)
    assert np.array_equal(skipped.cpu().numpy(), want_skipped)
    # the library's statuses
    lut = tables['density_lut']
    assert _raw_render(lib, device, 1, 8, 513, 8, density_lut=lut)[0] == UNSUPPORTED       # 4104 pixels wide
    assert _raw_render(lib, device, 1, 8, 8, 9, density_lut=lut)[0] == BAD_ARG
    assert _raw_render(lib, device, 1, 8, 8, 0, density_lut=lut)[0] == BAD_ARG
    assert _raw_render(lib, device, 1, 8, 8, 1, counts=np.zeros((1, 8, 8), np.int32))[0] == BAD_ARG
    assert _raw_render(lib, device, 1, 8, 8, 1, instance_map=np.zeros((1, 8, 8), np.int32), num_queries=1)[0] == BAD_ARG
    assert _raw_render(lib, device, B, GY, GX, 1, line=33, **_boxes(1))[0] == BAD_ARG
    assert _raw_render(lib, device, B, GY, GX, 1, alpha=257, **tables)[0] == BAD_ARG
    # and the wrapper's
    with pytest.raises(ops.MaskBevHipError):
        ops.render_bev(1, (8, 513), device, scale=8)
    with pytest.raises(ValueError):
        ops.render_bev(1, (8, 8), device, scale=9)
    with pytest.raises(ValueError):
        ops.render_bev(1, (8, 8), device, alpha=300)
    with pytest.raises(ops.MaskBevHipError):
        ops.render_bev(B, (GY, GX), device, counts=dev_tables['counts'].cpu(), density_lut=dev_tables['density_lut'])
    with pytest.raises(ops.MaskBevHipError):
        ops.render_bev(B, (GY, GX), device, instance_map=dev_tables['instance_map'][:, :-1], palette=dev_tables['palette'])
    with pytest.raises(ValueError):
        ops.render_bev(B, (GY, GX), device, box_corners=dev_tables['box_corners'])


def test_predictions_render(device):
    from mask_bev_amd import ops
    from mask_bev_amd.predict import Predictions
    from mask_bev_amd.render import RenderSettings, box_corners
    layers, _ = _layers()
    imap = _dev(layers['instances']['instance_map'], device)
    labels = torch.ones((B, Q), dtype=torch.int32, device=device)
    pred = Predictions(labels, torch.ones((B, Q), device=device), labels.bool(), None, None, None, imap, (GY, GX))
    pc_range, voxel, grid = [-3.0, 1.5, -2.0, -3.0 + GX * 0.5, 1.5 + GY * 0.5, 2.0], [0.5, 0.5, 4.0], [GX, GY, 1]
    geom = types.SimpleNamespace(pc_range=pc_range, voxel_size=voxel, grid=grid)
    rng = np.random.default_rng(8)
    scans = [torch.from_numpy((np.array(pc_range[:3]) + rng.uniform(0, 1, (n, 3)) * (np.array(pc_range[3:]) - np.array(pc_range[:3])))
                              .astype(np.float32)).to(device) for n in (700, 333)]
    ranges = ((pc_range[0], pc_range[3]), (pc_range[1], pc_range[4]))
    gt_boxes = [np.array([[2.0, 6.0, 0.0, 4.0, 1.8, 1.5, 0.3]]), np.zeros((0, 7))]
    track = _dev(layers['instances']['id_table'], device)
    gt = _dev(layers['contour']['gt_map'], device)
    settings = RenderSettings(scale=3, alpha=100, line=3, palette_size=16, palette_seed=2, flip_rows=True)
    image = pred.render(settings, scans=scans, module=geom, query_track=track, gt_maps=gt.long(), gt_boxes=gt_boxes, ranges=ranges)
    lut, palette = settings.tables(device)
    corners = box_corners(gt_boxes[0], ranges[0], ranges[1], GX, GY, 3)
    direct, skipped = ops.render_bev(B, (GY, GX), device, scale=3, flip_rows=True, counts=ops.cell_counts(scans, geom),
                                     density_lut=lut, instance_map=imap, num_queries=Q, id_table=track, palette=palette, alpha=100,
                                     untracked_rgb=settings.untracked_rgb, gt_map=gt, gt_rgb=settings.gt_rgb,
                                     box_corners=_dev(corners, device),
                                     box_rgb=_dev(np.array([settings.gt_box_rgb], np.uint8), device),
                                     box_offsets=_dev(np.array([0, 1, 1], np.int32), device), line=3)
    assert image.shape == (B, 3 * GY, 3 * GX, 3) and image.dtype == torch.uint8 and image.is_cuda
    assert torch.equal(image, direct) and skipped.tolist() == [0, 0]
    host = image.cpu().numpy()
    assert (host == np.array(settings.gt_box_rgb, np.uint8)).all(-1)[0].sum() > 20          # the label box is there
    assert (host == np.array(settings.gt_rgb, np.uint8)).all(-1).sum() > 20                 # and the contour
    # the defaults draw the instance map alone; the restatement agrees with the whole route
    plain = pred.render()
    want, _ = R.render(B, GY, GX, 2, density_lut=np.asarray(RenderSettings().density_lut, np.uint8),
                       instance_map=layers['instances']['instance_map'], num_queries=Q,
                       palette=RenderSettings().tables(device)[1].cpu().numpy())
    assert np.array_equal(plain.cpu().numpy(), want)
    # boxes='pred': the outlines of Predictions.boxes on top of the label boxes, rows grouped by scan
    m = layers['instances']['instance_map']
    dense = torch.from_numpy(np.stack([[m[b] == q for q in range(Q)] for b in range(B)]).reshape(B * Q, GY, GX)).to(device)
    with_masks = Predictions(labels, pred.scores, pred.keep, ops.pack_binary_masks(dense), None, None, imap, (GY, GX))
    image = with_masks.render(settings, boxes='pred', gt_boxes=gt_boxes, ranges=ranges + (0.5,))
    out = with_masks.boxes(ranges[0], ranges[1], 0.5)
    rows, scan = out['boxes'].cpu().numpy(), out['scan'].cpu().numpy()
    assert (scan == 0).sum() > 0 and (scan == 1).sum() > 0
    parts = [corners, box_corners(rows[scan == 0], ranges[0], ranges[1], GX, GY, 3),
             box_corners(rows[scan == 1], ranges[0], ranges[1], GX, GY, 3)]
    rgb = np.array([settings.gt_box_rgb] + [settings.box_rgb] * (len(rows)), np.uint8)
    direct, _ = ops.render_bev(B, (GY, GX), device, scale=3, flip_rows=True, density_lut=lut, instance_map=imap, num_queries=Q,
                               palette=palette, alpha=100, box_corners=_dev(np.concatenate(parts), device), box_rgb=_dev(rgb, device),
                               box_offsets=_dev(np.array([0, 1 + len(parts[1]), 1 + len(rows)], np.int32), device), line=3)
    assert torch.equal(image, direct)
    assert (image.cpu().numpy() == np.array(settings.box_rgb, np.uint8)).all(-1).sum() > 50
    with pytest.raises(ops.MaskBevHipError):
        Predictions(labels, pred.scores, pred.keep, None, None, None, None, (GY, GX)).render()
    with pytest.raises(ValueError):
        pred.render(scans=scans)
    with pytest.raises(ValueError):
        pred.render(gt_boxes=gt_boxes)


def _launcher_tree(device, tmp_path):
    """The tiny model's checkpoint, a four-scan sequence as downloaded with a mask cache beside it, and two configurations:
    ``tiny.yml`` (tracking on) and ``plain/tiny.yml`` (no tracking, scale 3, read without the cache) → (launcher, common arguments,
    the cache folder)."""
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from tests import scene_bank_util as U
    kw = tiny_kwargs()
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    data = tmp_path / 'data'
    poses, scans, words = U.drive(np.random.default_rng(3), 4, [(4.0, 3.5), (-3.0, -4.5)], 3.5, (kw['x_range'][1], kw['y_range'][1]))
    U.write_sequence(data / 'sequences' / '08', poses, scans, words)
    cache = data / 'sequences' / '08' / 'mask_cache'               # the tracking pass of --test lists (scan, cache) pairs
    cache.mkdir()
    gt = np.zeros((80, 80), np.int64)
    gt[10:22, 30:39] = 1
    for i in range(4):
        np.save(cache / f'{i:06d}.npy', gt)
    ck = tmp_path / 'ckpt' / 'tiny'
    ck.mkdir(parents=True)
    launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'], ck / 'tiny-epoch=00-val_loss=9.000000.ckpt', 0,
                             'val_loss', 9.0)
    cfg = dict(kw, dataset='semantic-kitti', batch_size=2, val_sequences=[8], train_sequences=[8], panoptic_min_points=1,
               track_instances=True, track_min_cells=2, track_max_tracks=32)
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(cfg))
    (tmp_path / 'plain').mkdir()                                   # the checkpoint folder is named after the file's stem
    (tmp_path / 'plain' / 'tiny.yml').write_text(yaml.safe_dump(dict(cfg, track_instances=False, render_scale=3, render_alpha=200,
                                                                     semantic_kitti_targets='scenes')))
    return launcher, ['--test', '--data-root', str(data), '--checkpoint-root', str(tmp_path / 'ckpt')], cache


def test_launcher_renders_frames(device, tmp_path, capsys):
    """``--test --render DIR`` on the tiny model and a four-scan sequence: one PNG per scan, the same bytes on a second run,
    with ``track_instances: true``; then without tracking, at another scale, the contour only where a cache file exists."""
    from mask_bev_amd.render import RenderSettings, read_png
    launcher, common, cache = _launcher_tree(device, tmp_path)
    runs = []
    for name in ('a', 'b'):
        assert launcher.main(['--config', str(tmp_path / 'tiny.yml'), '--render', str(tmp_path / name)] + common) == 0
        out = capsys.readouterr().out
        assert f'wrote 4 frames under {tmp_path / name}' in out
        assert len([l for l in out.splitlines() if l.startswith('point LSTQ')]) == 1         # the tracking pass of --test ran too
        files = sorted((tmp_path / name / 'sequences' / '08' / 'bev').glob('*.png'))
        assert [f.name for f in files] == [f'{i:06d}.png' for i in range(4)]
        runs.append([f.read_bytes() for f in files])
        assert all(read_png(f).shape == (160, 160, 3) for f in files)
    assert runs[0] == runs[1]
    frames = np.stack([read_png(f) for f in files])
    assert len(np.unique(frames.reshape(-1, 3), axis=0)) > 2                   # returns at more than one level
    white = lambda f: (f == np.array(RenderSettings().gt_rgb, np.uint8)).all(-1)
    assert all(white(f).sum() == 2 * 24 + 2 * 18 - 4 for f in frames)          # the cache's instance, outlined, in every frame
    # without tracking, at another scale, read without the cache, which is left next to the first two scans only
    for i in (2, 3):
        (cache / f'{i:06d}.npy').unlink()
    assert launcher.main(['--config', str(tmp_path / 'plain' / 'tiny.yml'), '--render', str(tmp_path / 'c')] + common) == 0
    capsys.readouterr()
    files = sorted((tmp_path / 'c' / 'sequences' / '08' / 'bev').glob('*.png'))
    frames = [read_png(f) for f in files]
    assert len(frames) == 4 and all(f.shape == (240, 240, 3) for f in frames)
    white = [white(f) for f in frames]
    # the cache is (nx, ny): x-cells 10 .. 21 are columns, y-cells 30 .. 38 rows; an outline of a 36 x 27 pixel rectangle
    assert white[0].sum() == white[1].sum() == 2 * 36 + 2 * 27 - 4 and white[0][90:117, 30:66].sum() == white[0].sum()
    assert white[2].sum() == 0 and white[3].sum() == 0


def test_launcher_lines_are_those_of_a_run_without_the_flag(device, tmp_path, capsys):
    """The ``val_loss``, ``point PQ`` and ``point LSTQ`` lines of ``--test --render DIR`` are identical to those of a run without
    the flag.

    KNOWN TO FAIL NOW AND THEN on the ``val_loss`` line (it failed in one of five runs of this file on an MI355X), for a reason
    that has nothing to do with the flag: the render pass runs after all three lines are printed, yet ``val_loss`` itself is not
    bit-reproducible between two ``--test`` runs of one process.  Measured with this tree, seven runs in a row, none but the
    sixth with ``--render``:
    90.62866973876953, 90.62867736816406 (x 4), 90.62866973876953 (with the flag), 90.62866973876953; an earlier pair gave
    90.6286735534668 then 90.62867736816406.  The values are neighbouring f32 losses of the two validation batches (the
    printed number is their mean); the forward pass sums with float atomics (K2's and K3's statistics), whose order is not
    fixed.  The ``point PQ`` and ``point LSTQ`` lines were identical in all of these runs and are asserted first."""
    launcher, common, _ = _launcher_tree(device, tmp_path)
    lines = {}
    for name, extra in (('without', []), ('with', ['--render', str(tmp_path / 'frames')])):
        assert launcher.main(['--config', str(tmp_path / 'tiny.yml')] + extra + common) == 0
        out = capsys.readouterr().out.splitlines()
        lines[name] = {key: [l for l in out if l.startswith(key)] for key in ('val_loss ', 'point PQ', 'point LSTQ')}
        print(name, lines[name])
        assert all(len(v) == 1 for v in lines[name].values())
    assert lines['with']['point PQ'] == lines['without']['point PQ']
    assert lines['with']['point LSTQ'] == lines['without']['point LSTQ']
    assert lines['with']['val_loss '] == lines['without']['val_loss ']


def test_launcher_renders_kitti_frames(device, tmp_path, capsys):
    """``dataset: kitti``: ``--test --render DIR`` writes ``DIR/NNNNNN.png`` with the label boxes outlined; ``render_boxes: false``
    draws none."""
    import os
    import shutil
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.render import RenderSettings, read_png
    sample = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kitti_object_sample')
    rng = np.random.default_rng(2)
    for k in ('velodyne', 'label_2', 'calib'):
        d = tmp_path / f'data_object_{k}' / 'training' / k
        d.mkdir(parents=True)
        for frame in (0, 1):
            if k == 'velodyne':
                rng.uniform([0, -10, -3, 0], [20, 10, 1, 1], (2000 + frame, 4)).astype(np.float32).tofile(d / f'{frame:06d}.bin')
            else:
                shutil.copy(os.path.join(sample, k, '000000.txt'), d / f'{frame:06d}.txt')
    (tmp_path / 'val.txt').write_text('000000\n000001\n')
    (tmp_path / 'train.txt').write_text('000000\n000001\n')
    kw = dict(tiny_kwargs(), x_range=[0, 20], y_range=[-10, 10], z_range=[-3, 1], dataset='kitti', batch_size=2)
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    green = np.array(RenderSettings().gt_box_rgb, np.uint8)
    for name, extra in (('boxes', {}), ('bare', {'render_boxes': False})):
        ck = tmp_path / 'ckpt' / name
        ck.mkdir(parents=True)
        launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'], ck / f'{name}-epoch=00-val_loss=1.000000.ckpt', 0,
                                 'val_loss', 1.0)
        (tmp_path / f'{name}.yml').write_text(yaml.safe_dump(dict(kw, **extra)))
        out_dir = tmp_path / f'frames_{name}'
        assert launcher.main(['--config', str(tmp_path / f'{name}.yml'), '--test', '--data-root', str(tmp_path), '--checkpoint-root',
                              str(tmp_path / 'ckpt'), '--render', str(out_dir)]) == 0
        assert f'wrote 2 frames under {out_dir}' in capsys.readouterr().out
        files = sorted(out_dir.glob('*.png'))
        assert [f.name for f in files] == ['000000.png', '000001.png']
        frames = [read_png(f) for f in files]
        assert all(f.shape == (160, 160, 3) for f in frames)
        outlined = [int((f == green).all(-1).sum()) for f in frames]
        # two of the sample frame's labels lie inside 0 .. 20 m x -10 .. 10 m: a car of 3.35 m x 1.57 m and a 1.2 m x 1.89 m box
        assert all(n > 60 for n in outlined) if not extra else outlined == [0, 0]
