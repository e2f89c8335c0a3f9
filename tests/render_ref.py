"""K36 restated (include/maskbev_hip.h, K36): numpy f32 for the cell rule, Python integers for everything else, plain loops over
points, pixels and boxes.  Independent of the product's code: nothing of mask_bev_amd is imported here.  ``render_vectorised``
is a second formulation of the same rule (whole-image numpy operations, object-dtype integers for the segment test) that
tests/test_render_cpu.py holds against the loops."""
import numpy as np

CORNER_BOUND = 16384


def cell_counts(scans, pc_range, voxel_size, grid, prefilter=True):
    """``scans``: list of (N_i, 3 | 4) f32 arrays; ``pc_range`` = (x_min, y_min, z_min, x_max, y_max, z_max), ``voxel_size`` =
    (vx, vy, vz), ``grid`` = (gx, gy, gz) → (B, gy, gx) int32.  K1's rule, one f32 operation at a time."""
    f = np.float32
    lo, hi, vs = np.asarray(pc_range[:3], dtype=f), np.asarray(pc_range[3:], dtype=f), np.asarray(voxel_size, dtype=f)
    gx, gy, gz = (int(g) for g in grid)
    out = np.zeros((len(scans), gy, gx), dtype=np.int32)
    for b, scan in enumerate(scans):
        p = np.asarray(scan, dtype=f)[:, :3]
        with np.errstate(all='ignore'):
            q = np.floor((p - lo) / vs)                                       # f32 subtract, f32 divide, floor: one rounding each
            ok = np.all((q >= 0) & (q < np.asarray([gx, gy, gz], dtype=f)), axis=1)      # NaN fails every compare
            if prefilter:
                ok &= np.all((lo < p) & (p < hi), axis=1)
        assert q.dtype == f
        np.add.at(out[b], (q[ok, 1].astype(np.int64), q[ok, 0].astype(np.int64)), 1)
    return out


def bit_length_level(c):
    return min(max(int(c), 0).bit_length(), 15)


def segment_hit(ax, ay, bx, by, px, py, line):
    ux, uy, vx, vy = bx - ax, by - ay, px - ax, py - ay
    d, length2 = ux * vx + uy * vy, ux * ux + uy * uy
    if d <= 0:
        return 4 * (vx * vx + vy * vy) <= line * line
    if d >= length2:
        return 4 * ((px - bx) ** 2 + (py - by) ** 2) <= line * line
    cross = ux * vy - uy * vx
    return 4 * cross * cross <= line * line * length2


def box_hit(corners, px, py, line):
    c = [(int(x), int(y)) for x, y in corners]
    return any(segment_hit(*c[k], *c[(k + 1) % 4], px, py, line) for k in range(4))


def render(batch, gy, gx, scale, flip_rows=False, counts=None, density_lut=None, instance_map=None, num_queries=0,
           id_table=None, palette=None, alpha=128, untracked_rgb=(128, 128, 128), gt_map=None, gt_background=0,
           gt_rgb=(255, 255, 255), box_corners=None, box_rgb=None, box_offsets=None, line=2):
    """→ (image (B, gy * scale, gx * scale, 3) uint8, skipped (B) int32).  Arrays or None, as the kernel takes them."""
    s, H, W = int(scale), gy * int(scale), gx * int(scale)
    image = np.zeros((batch, H, W, 3), dtype=np.uint8)
    skipped = np.zeros((batch,), dtype=np.int32)
    n_boxes = 0 if box_corners is None else len(box_corners)

    def gt_at(b, py, px):
        if py < 0 or py >= H or px < 0 or px >= W:
            return int(gt_background)
        return int(gt_map[b, py // s, px // s])

    for b in range(batch):
        rows = []
        if n_boxes:
            r0, r1 = max(int(box_offsets[b]), 0), min(int(box_offsets[b + 1]), n_boxes)
            for r in range(r0, r1):
                if np.abs(np.asarray(box_corners[r], dtype=np.int64)).max() > CORNER_BOUND:
                    skipped[b] += 1
                else:
                    rows.append(r)
        for py in range(H):
            for px in range(W):
                cy, cx = py // s, px // s
                rgb = [0, 0, 0]
                if density_lut is not None:
                    c = int(counts[b, cy, cx]) if counts is not None else 0
                    rgb = [int(v) for v in density_lut[bit_length_level(c)]]
                if instance_map is not None:
                    q = int(instance_map[b, cy, cx])
                    if 0 <= q < num_queries:
                        ident = int(id_table[b, q]) if id_table is not None else q
                        col = palette[ident % len(palette)] if ident >= 0 else untracked_rgb
                        rgb = [(rgb[k] * (256 - alpha) + int(col[k]) * alpha + 128) >> 8 for k in range(3)]
                if gt_map is not None:
                    v = gt_at(b, py, px)
                    if v != int(gt_background) and any(gt_at(b, py + dy, px + dx) != v
                                                       for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0))):
                        rgb = [int(k) for k in gt_rgb]
                for r in rows:
                    if box_hit(box_corners[r], 2 * px + 1, 2 * py + 1, int(line)):
                        rgb = [int(k) for k in box_rgb[r]]
                image[b, H - 1 - py if flip_rows else py, px] = rgb
    return image, skipped


def render_vectorised(batch, gy, gx, scale, flip_rows=False, counts=None, density_lut=None, instance_map=None, num_queries=0,
                      id_table=None, palette=None, alpha=128, untracked_rgb=(128, 128, 128), gt_map=None, gt_background=0,
                      gt_rgb=(255, 255, 255), box_corners=None, box_rgb=None, box_offsets=None, line=2):
    """The same rule on whole images: ``np.repeat`` for the cells of the pixels, a padded map for the contour, and for the
    boxes the point-to-segment rule written with a clamped projection parameter instead of three cases:
    t = clamp(d, 0, L); L^2 |v|^2 - 2 t d L + t^2 L  is  L^2 times the squared distance, so the test is
    4 (L^2 |v|^2 - 2 t d L + t^2 L) <= line^2 L^2 for L > 0 and 4 |v|^2 <= line^2 for L = 0.  Exact Python integers."""
    s, H, W = int(scale), gy * int(scale), gx * int(scale)
    up = lambda m: np.repeat(np.repeat(np.asarray(m), s, axis=1), s, axis=2)
    img = np.zeros((batch, H, W, 3), dtype=np.int64)
    if density_lut is not None:
        c = np.maximum(up(counts), 0).astype(np.int64) if counts is not None else np.zeros((batch, H, W), np.int64)
        level = np.zeros_like(c)
        for k in range(31):
            level += (c >> k) > 0
        img = np.asarray(density_lut, dtype=np.int64)[np.minimum(level, 15)]
    if instance_map is not None:
        q = up(instance_map).astype(np.int64)
        draw = (q >= 0) & (q < num_queries)
        qq = np.where(draw, q, 0)
        ident = qq if id_table is None else np.take_along_axis(
            np.asarray(id_table, dtype=np.int64).reshape(batch, -1), qq.reshape(batch, -1), axis=1).reshape(batch, H, W) \
            if num_queries > 0 else qq
        col = np.where((ident >= 0)[..., None], np.asarray(palette, dtype=np.int64)[np.where(ident >= 0, ident, 0) % len(palette)],
                       np.asarray(untracked_rgb, dtype=np.int64))
        img = np.where(draw[..., None], (img * (256 - alpha) + col * alpha + 128) >> 8, img)
    if gt_map is not None:
        g = up(gt_map).astype(np.int64)
        pad = np.full((batch, H + 2, W + 2), int(gt_background), dtype=np.int64)
        pad[:, 1:-1, 1:-1] = g
        edge = (pad[:, 1:-1, :-2] != g) | (pad[:, 1:-1, 2:] != g) | (pad[:, :-2, 1:-1] != g) | (pad[:, 2:, 1:-1] != g)
        img = np.where(((g != gt_background) & edge)[..., None], np.asarray(gt_rgb, dtype=np.int64), img)
    skipped = np.zeros((batch,), dtype=np.int32)
    n_boxes = 0 if box_corners is None else len(box_corners)
    if n_boxes:
        px = (2 * np.arange(W) + 1).astype(object)[None, :]
        py = (2 * np.arange(H) + 1).astype(object)[:, None]
        for b in range(batch):
            for r in range(max(int(box_offsets[b]), 0), min(int(box_offsets[b + 1]), n_boxes)):
                c = [(int(x), int(y)) for x, y in box_corners[r]]
                if max(abs(v) for xy in c for v in xy) > CORNER_BOUND:
                    skipped[b] += 1
                    continue
                hit = np.zeros((H, W), dtype=bool)
                for k in range(4):
                    (ax, ay), (bx, by) = c[k], c[(k + 1) % 4]
                    ux, uy = bx - ax, by - ay
                    vx, vy = px - ax + 0 * py, py - ay + 0 * px
                    d, L = ux * vx + uy * vy, ux * ux + uy * uy
                    vv = vx * vx + vy * vy
                    if L == 0:
                        hit |= (4 * vv <= line * line).astype(bool)
                    else:
                        t = np.where(d < 0, 0, np.where(d > L, L, d))
                        hit |= (4 * (L * L * vv - 2 * t * d * L + t * t * L) <= line * line * L * L).astype(bool)
                img[b][hit] = np.asarray(box_rgb[r], dtype=np.int64)
    img = img.astype(np.uint8)
    return (img[:, ::-1].copy() if flip_rows else img), skipped
