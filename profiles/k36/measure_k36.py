"""K36 measurement: the BEV frame of a batch composed on the device — ``ops.cell_counts`` (K36a), ``ops.render_bev`` (K36b) and
the copy of the (B, H, W, 3) uint8 image to the host — against what the same picture costs without it: ``Predictions.cpu()``,
the scans copied to the host, the bit-packed masks unpacked and the layers composed with numpy.  B = 4 scans of 120 000
synthetic points, a 512 x 512 grid of 0.16 m cells at scale 2 (1024 x 1024 pixels), 100 queries of which 40 own a rectangle, 64
boxes per scan.  The host route follows the same integer rule (counts, level table, blend, contour, box outlines by the
clamped-projection form of the distance test) written with whole-array numpy operations, and its picture is compared with the
device's.  No real scan is read anywhere.  Prints one JSON line and writes it to the path given as the first argument (default:
k36_measure.json beside this file).  ``--dry`` builds tiny inputs on the CPU, runs the host route once and stops (no timing)."""
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mask_bev_amd.predict import Predictions, unpack_bits                 # noqa: E402
from mask_bev_amd.render import RenderSettings, box_corners               # noqa: E402

DRY = '--dry' in sys.argv
args = [a for a in sys.argv[1:] if a != '--dry']
dev = torch.device('cpu' if DRY else 'cuda:0')
B, N, G, S, Q, OWNED, BOXES = (2, 2000, 64, 2, 12, 6, 8) if DRY else (4, 120000, 512, 2, 100, 40, 64)
VS = 0.16
HALF = G * VS / 2
GEOM = types.SimpleNamespace(pc_range=[-HALF, -HALF, -3.0, HALF, HALF, 1.0], voxel_size=[VS, VS, 4.0], grid=[G, G, 1])
RANGES = ((-HALF, HALF), (-HALF, HALF))
settings = RenderSettings(scale=S)
rng = np.random.default_rng(36)


def make_inputs():
    scans = [((rng.random((N, 4)) * 2 - 1) * np.array([HALF * 1.05, HALF * 1.05, 2.0, 0.5]) + np.array([0, 0, -1.0, 0.5]))
             .astype(np.float32) for _ in range(B)]
    imap = np.full((B, G, G), -1, np.int32)
    masks = np.zeros((B, Q, G, G), np.float32)
    gt = np.zeros((B, G, G), np.int32)
    boxes, scores = [], np.zeros((B, Q), np.float32)
    for b in range(B):
        for k, q in enumerate(rng.permutation(Q)[:OWNED]):
            scores[b, q] = (k + 1) / OWNED                        # painted later = higher score: the map both routes arrive at
            h, w = rng.integers(8, 30), rng.integers(8, 30)
            y, x = rng.integers(0, G - h), rng.integers(0, G - w)
            masks[b, q, y:y + h, x:x + w] = 1
            imap[b, y:y + h, x:x + w] = q
            gt[b, y + 1:y + h, x:x + w - 1] = q + 1
        xy = (rng.random((BOXES, 2)) * 2 - 1) * HALF * 0.95
        boxes.append(np.concatenate([xy, np.full((BOXES, 1), -1.0), rng.uniform(3.5, 5.0, (BOXES, 1)), rng.uniform(1.6, 2.0, (BOXES, 1)),
                                     np.full((BOXES, 1), 1.5), rng.uniform(-np.pi, np.pi, (BOXES, 1))], 1))
    return scans, imap, masks, gt, boxes, scores


def host_compose(scans, words, keep, scores, gt, corners, offsets, lut, palette):
    """The picture on the host from what ``Predictions.cpu()`` and the scans hold: counts by K1's rule in numpy f32, the
    instance map from the unpacked masks (the kept query of the highest score per cell), then the four layers."""
    f = np.float32
    lo, hi, vs = np.asarray(GEOM.pc_range[:3], f), np.asarray(GEOM.pc_range[3:], f), np.asarray(GEOM.voxel_size, f)
    counts = np.zeros((B, G, G), np.int64)
    for b, p in enumerate(scans):
        p = p[:, :3]
        q = np.floor((p - lo) / vs)
        ok = np.all((q >= 0) & (q < np.asarray(GEOM.grid, f)) & (lo < p) & (p < hi), axis=1)
        np.add.at(counts[b], (q[ok, 1].astype(np.int64), q[ok, 0].astype(np.int64)), 1)
    dense = unpack_bits(words, G, G).reshape(B, Q, G, G).numpy()
    order = np.where(keep, scores, -1.0).astype(np.float32)
    best = np.argmax(dense * (order[:, :, None, None] + np.float32(2.0)), axis=1)
    imap = np.where(dense.any(axis=1), best, -1)
    up = lambda m: np.repeat(np.repeat(m, S, axis=1), S, axis=2)
    level = np.zeros((B, G, G), np.int64)
    for k in range(31):
        level += (counts >> k) > 0
    img = lut.astype(np.int64)[np.minimum(up(level), 15)]
    q = up(imap)
    col = palette.astype(np.int64)[np.maximum(q, 0) % len(palette)]
    img = np.where((q >= 0)[..., None], (img * (256 - settings.alpha) + col * settings.alpha + 128) >> 8, img)
    g = up(gt).astype(np.int64)
    pad = np.zeros((B, G * S + 2, G * S + 2), np.int64)
    pad[:, 1:-1, 1:-1] = g
    edge = (pad[:, 1:-1, :-2] != g) | (pad[:, 1:-1, 2:] != g) | (pad[:, :-2, 1:-1] != g) | (pad[:, 2:, 1:-1] != g)
    img = np.where(((g != 0) & edge)[..., None], np.asarray(settings.gt_rgb, np.int64), img)
    line2 = settings.line * settings.line
    for b in range(B):
        for r in range(offsets[b], offsets[b + 1]):
            c = corners[r].astype(np.int64)
            x0, x1 = max((c[:, 0].min() - settings.line) // 2 - 1, 0), min((c[:, 0].max() + settings.line) // 2 + 1, G * S - 1)
            y0, y1 = max((c[:, 1].min() - settings.line) // 2 - 1, 0), min((c[:, 1].max() + settings.line) // 2 + 1, G * S - 1)
            if x1 < x0 or y1 < y0:
                continue
            px, py = 2 * np.arange(x0, x1 + 1)[None, :] + 1, 2 * np.arange(y0, y1 + 1)[:, None] + 1
            hit = np.zeros((y1 - y0 + 1, x1 - x0 + 1), bool)
            for k in range(4):
                (ax, ay), (bx, by) = c[k], c[(k + 1) % 4]
                ux, uy, vx, vy = bx - ax, by - ay, px - ax, py - ay
                d, L = ux * vx + uy * vy, ux * ux + uy * uy
                t = np.clip(d, 0, L)
                hit |= 4 * (L * L * (vx * vx + vy * vy) - 2 * t * d * L + t * t * L) <= line2 * L * L       # L > 0; fits int64 here
            img[b, y0:y1 + 1, x0:x1 + 1][hit] = np.asarray(settings.box_rgb, np.int64)
    return img.astype(np.uint8)


scans, imap, masks, gt, boxes, scores_np = make_inputs()
corners = np.concatenate([box_corners(b, RANGES[0], RANGES[1], G, G, S) for b in boxes])
offsets = np.arange(B + 1, dtype=np.int32) * BOXES
lut_np = np.asarray(settings.density_lut, np.uint8)
keep_np = masks.any(axis=(2, 3))

if DRY:
    from mask_bev_amd.render import instance_palette
    bits = masks.reshape(B * Q, -1).astype(np.int64)
    n_words = (G * G + 31) // 32
    padded = np.zeros((B * Q, n_words * 32), np.int64)
    padded[:, :G * G] = bits
    words = (padded.reshape(B * Q, n_words, 32) << np.arange(32)).sum(-1)
    words = torch.from_numpy(np.where(words >= 2 ** 31, words - 2 ** 32, words).astype(np.int32))
    img = host_compose(scans, words, keep_np, scores_np, gt, corners, offsets, lut_np, instance_palette(settings.palette_size))
    print('dry run:', img.shape, img.dtype, int(img.sum()))
    sys.exit(0)

from mask_bev_amd import ops                                              # noqa: E402

dev_scans = [torch.from_numpy(s).to(dev) for s in scans]
packed = ops.pack_binary_masks(torch.from_numpy(masks.reshape(B * Q, G, G)).to(dev))
pred = Predictions(torch.from_numpy(keep_np.astype(np.int32)).to(dev), torch.from_numpy(scores_np).to(dev),
                   torch.from_numpy(keep_np).to(dev), packed, torch.from_numpy(masks.sum((2, 3)).astype(np.int32)).to(dev),
                   torch.from_numpy(scores_np).to(dev), torch.from_numpy(imap).to(dev), (G, G))
lut, palette = settings.tables(dev)
gt_dev, corners_dev = torch.from_numpy(gt).to(dev), torch.from_numpy(corners).to(dev)
rgb_dev = torch.from_numpy(np.tile(np.asarray(settings.box_rgb, np.uint8), (len(corners), 1))).to(dev)
offsets_dev = torch.from_numpy(offsets).to(dev)
state = {}


def k36a():
    state['counts'] = ops.cell_counts(dev_scans, GEOM)


def k36b():
    state['image'], state['skipped'] = ops.render_bev(
        B, (G, G), dev, scale=S, counts=state['counts'], density_lut=lut, instance_map=pred.instance_map, num_queries=Q,
        palette=palette, alpha=settings.alpha, gt_map=gt_dev, gt_rgb=settings.gt_rgb, box_corners=corners_dev, box_rgb=rgb_dev,
        box_offsets=offsets_dev, line=settings.line)


def timed_alternating(fns, iters, reps, warm):
    """Every function ``iters`` times between two events, the functions taking turns, ``reps`` rounds → {name: [ms per call]}."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    return ms


def stats(ms, **extra):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), **extra)


def wall(fn, reps):
    """Host clock around a call that ends with its result on the host (or in a synchronise)."""
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


k36a()
k36b()
pinned = torch.empty(state['image'].shape, dtype=torch.uint8).pin_memory()
ms = timed_alternating({'k36a_cell_counts': k36a, 'k36b_render_bev': k36b,
                        'image_to_pinned_host': lambda: pinned.copy_(state['image'], non_blocking=True)}, 50, 7, 5)


def device_route():
    k36a()
    k36b()
    return state['image'].cpu().numpy()


def host_route():
    host = pred.cpu()
    host_scans = [s.cpu().numpy() for s in dev_scans]
    return host_compose(host_scans, host.masks.words, host.keep.numpy(), host.scores.numpy(), gt, corners, offsets, lut_np,
                        palette.cpu().numpy())


def host_copies_only():
    pred.cpu()
    [s.cpu() for s in dev_scans]


got, want = device_route(), host_route()
pixels = int(np.prod(got.shape[:3]))
bytes_b = 12 * B * G * G + 3 * pixels                  # K36b: three int32 cell maps read once, the image written once
res = dict(batch=B, points_per_scan=N, grid=[G, G], scale=S, image=list(got.shape), queries=Q, owned_queries_per_scan=OWNED,
           boxes_per_scan=BOXES, real_scans_used=False, skipped=state['skipped'].tolist(),
           device_and_host_pictures_equal=bool(np.array_equal(got, want)),
           pixels_that_differ=int(np.any(got != want, axis=-1).sum()),
           ms_per_call_by_events={k: stats(v, iters=50, reps=7) for k, v in ms.items()},
           k36b_needed_bytes=bytes_b,
           k36b_bytes_per_second=bytes_b / (statistics.median(ms['k36b_render_bev']) * 1e-3),
           image_bytes=3 * pixels,
           ms_wall_with_result_on_host=dict(device_route_k36a_k36b_copy=stats(wall(device_route, 7), reps=7),
                                            host_route_pred_cpu_unpack_numpy=stats(wall(host_route, 3), reps=3),
                                            host_route_copies_alone=stats(wall(host_copies_only, 7), reps=7)))
target = args[0] if args else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'k36_measure.json')
with open(target, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
