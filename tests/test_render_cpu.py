"""K36 on the host: the restatement against a second formulation, the PNG writer, the palette, the box corners, the binding."""
import os

import numpy as np
import pytest

from tests import render_ref as R


def scene(rng, batch, gy, gx, scale, q_num=6, p_num=5, n_boxes=(0, 5)):
    """Random tables of every layer on a (gy, gx) grid: what both formulations (and the kernel) take."""
    counts = rng.integers(0, 9, (batch, gy, gx)).astype(np.int32)
    counts[rng.random((batch, gy, gx)) < 0.3] = 0
    counts.reshape(-1)[0] = 40000
    imap = rng.integers(-1, q_num + 2, (batch, gy, gx)).astype(np.int32)
    ids = rng.integers(-1, 3 * p_num, (batch, q_num)).astype(np.int32)
    gt = np.zeros((batch, gy, gx), np.int32)
    gt[:, 1:gy // 2, 1:gx // 2] = 3
    gt[:, 1:gy // 2, gx // 2:gx - 1] = 4
    gt[0, 0, :] = 7
    gt[-1, gy - 1, gx - 1] = 9
    H, W = gy * scale, gx * scale
    corners, offsets = [], [0]
    for n in n_boxes:
        for _ in range(n):
            c, half, yaw = rng.uniform(0, 2 * max(H, W), 2), rng.uniform(2, max(H, W), 2), rng.uniform(0, np.pi)
            d, e = np.array([np.cos(yaw), np.sin(yaw)]), np.array([-np.sin(yaw), np.cos(yaw)])
            corners.append(np.rint([c + half[0] * d + half[1] * e, c - half[0] * d + half[1] * e, c - half[0] * d - half[1] * e,
                                    c + half[0] * d - half[1] * e]))
        offsets.append(len(corners))
    corners = np.asarray(corners, dtype=np.int32).reshape(-1, 4, 2)
    return dict(counts=counts, density_lut=rng.integers(0, 256, (16, 3)).astype(np.uint8), instance_map=imap, num_queries=q_num,
                id_table=ids, palette=rng.integers(0, 256, (p_num, 3)).astype(np.uint8), gt_map=gt, box_corners=corners,
                box_rgb=rng.integers(0, 256, (len(corners), 3)).astype(np.uint8), box_offsets=np.asarray(offsets, np.int32))


@pytest.mark.parametrize('flip', [False, True])
def test_restatement_agrees_with_the_vectorised_formulation(flip):
    rng = np.random.default_rng(36)
    tables = scene(rng, 2, 6, 8, 3)
    tables['box_corners'][1] = [[10, 10], [10, 10], [10, 10], [10, 10]]                 # a dot
    tables['box_corners'][2] = [[4, 4], [40, 4], [40, 30], [20000, 30]]                 # beyond the bound
    for line, alpha in ((1, 0), (2, 128), (5, 256)):
        a = R.render(2, 6, 8, 3, flip_rows=flip, line=line, alpha=alpha, **tables)
        b = R.render_vectorised(2, 6, 8, 3, flip_rows=flip, line=line, alpha=alpha, **tables)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[1].tolist() == [0, 1] and a[0].shape == (2, 18, 24, 3)
    # all layers off: the uniform first colour of the table; and each layer changes something
    lut = tables['density_lut']
    base = R.render(2, 6, 8, 3, density_lut=lut)[0]
    assert np.all(base == lut[0])
    for keys in (('counts',), ('instance_map', 'num_queries', 'palette'), ('gt_map',), ('box_corners', 'box_rgb', 'box_offsets')):
        one = R.render(2, 6, 8, 3, density_lut=lut, **{k: tables[k] for k in keys})[0]
        assert not np.array_equal(one, base), keys


def test_cell_counts_restatement_edges():
    rng, grid, vs = (-4.0, -3.0, -2.0, 4.0, 3.0, 2.0), (8, 6, 1), (1.0, 1.0, 4.0)
    pts = np.array([[-4.0, 0.5, 0.0], [-3.5, 0.5, 0.0], [3.999, 2.999, 1.9], [4.0, 0.0, 0.0], [np.nan, 0.0, 0.0],
                    [0.0, 0.0, 2.0], [0.0, 0.0, -2.0]], np.float32)
    on = R.cell_counts([pts], rng, vs, grid, True)
    off = R.cell_counts([pts], rng, vs, grid, False)
    assert on.sum() == 2 and on[0, 3, 0] == 1 and on[0, 5, 7] == 1
    assert off.sum() == 4 and off[0, 3, 0] == 2 and off[0, 3, 4] == 1       # x == x_min and z == z_min are cells without the filter


@pytest.mark.parametrize('shape', [(5, 7, 3), (1, 1, 3)])
def test_png_round_trip(tmp_path, shape):
    from mask_bev_amd.render import png_bytes, read_png, write_png
    img = np.random.default_rng(1).integers(0, 256, shape).astype(np.uint8)
    path = tmp_path / 'a.png'
    write_png(path, img)
    data = path.read_bytes()
    assert data == png_bytes(img) and data[:8] == b'\x89PNG\r\n\x1a\n'
    got = read_png(path)
    assert got.dtype == np.uint8 and np.array_equal(got, img)
    path.write_bytes(data[:-20] + bytes([data[-20] ^ 1]) + data[-19:])
    with pytest.raises(ValueError):
        read_png(path)
    with pytest.raises(ValueError):
        write_png(path, img[..., :2])


def test_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from mask_bev_amd.render import write_png
    for shape in ((5, 7, 3), (1, 1, 3)):
        img = np.random.default_rng(2).integers(0, 256, shape).astype(np.uint8)
        write_png(tmp_path / 'b.png', img)
        with Image.open(tmp_path / 'b.png') as im:
            assert im.mode == 'RGB' and np.array_equal(np.asarray(im), img)


def test_instance_palette():
    from mask_bev_amd.render import instance_palette
    a, b = instance_palette(256, 0), instance_palette(256, 0)
    assert a.dtype == np.uint8 and a.shape == (256, 3) and np.array_equal(a, b)
    assert np.array_equal(instance_palette(64, 0), a[:64])
    assert len({tuple(c) for c in a[:64].tolist()}) == 64 and len({tuple(c) for c in a.tolist()}) == 256
    assert not np.array_equal(instance_palette(64, 1), a[:64])
    assert a.max(1).min() >= 176 and a.min(1).max() <= 79                   # mid-bright: a strong and a weak channel each
    with pytest.raises(ValueError):
        instance_palette(0)


def test_box_corners_dyadic_cases():
    from mask_bev_amd.render import box_corners
    xr, yr = (-8.0, 8.0), (-4.0, 4.0)                                       # 0.5 m cells on a 32 x 16 grid
    # an axis-aligned 4 m x 2 m box at the origin, scale 1: cells x 16 +- 4, y 8 +- 2; half-pixels: twice that
    got = box_corners([[0.0, 0.0, 4.0, 2.0, 0.0]], xr, yr, 32, 16, 1)
    assert got.dtype == np.int32 and got.tolist() == [[[40, 20], [24, 20], [24, 12], [40, 12]]]
    # the same as (n, 7) at scale 3
    got = box_corners(np.array([[0.0, 0.0, -1.0, 4.0, 2.0, 1.5, 0.0]]), xr, yr, 32, 16, 3)
    assert got.tolist() == [[[120, 60], [72, 60], [72, 36], [120, 36]]]
    # a quarter turn: the length runs along y.  Centre (1, -1) m is cell (18, 6); x 18 -+ 2 cells, y 6 +- 4 cells
    got = box_corners([[1.0, -1.0, 4.0, 2.0, np.pi / 2]], xr, yr, 32, 16, 1)
    assert got.tolist() == [[[32, 20], [32, 4], [40, 4], [40, 20]]]
    # floor(v + 0.5): 0.125 m is a quarter cell, half a half-pixel at scale 1, and rounds up; so does -0.5
    got = box_corners([[0.125, 0.125, 0.0, 0.0, 0.0]], xr, yr, 32, 16, 1)
    assert got.tolist() == [[[33, 17]] * 4]
    got = box_corners([[-8.125, 0.0, 0.0, 0.0, 0.0]], xr, yr, 32, 16, 1)
    assert got[0, 0].tolist() == [0, 16]
    assert box_corners(np.zeros((0, 7)), xr, yr, 32, 16, 2).shape == (0, 4, 2)
    assert box_corners([[1e30, 0.0, 1.0, 1.0, 0.0]], xr, yr, 32, 16, 2)[0, 0, 0] == 2 ** 30
    with pytest.raises(ValueError):
        box_corners([[np.nan, 0.0, 1.0, 1.0, 0.0]], xr, yr, 32, 16, 2)
    with pytest.raises(ValueError):
        box_corners(np.zeros((2, 6)), xr, yr, 32, 16, 2)


def test_binding_and_build():
    from mask_bev_amd import _lib, build, ops_render
    header = open(os.path.join(os.path.dirname(build.PKG_DIR), 'include', 'maskbev_hip.h')).read()
    for name, n_args in (('mbv_cell_counts', 20), ('mbv_render_bev', 25), ('mbv_render_box_chunk', 0)):
        assert name in _lib.SIGNATURES and name + '(' in header
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.ABI_VERSION == 59
    assert 'render.hip' in build.sources()
    assert build.FILE_FLAGS['render.hip'] == ['-ffp-contract=off']
    # the cell rule has one copy, in the header both files include
    csrc = os.path.join(build.PKG_DIR, 'csrc')
    for name in ('render.hip', 'point_lift.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "point_cell.hpp"' in text and 'bool point_cell(' not in text
    assert 'bool point_cell(' in open(os.path.join(csrc, 'point_cell.hpp')).read()
    assert ops_render.RENDER_BOX_CHUNK == 64


def test_settings_and_facade():
    from mask_bev_amd import ops
    from mask_bev_amd.render import RenderSettings
    assert callable(ops.cell_counts) and callable(ops.render_bev)
    s = RenderSettings()
    assert (s.scale, s.alpha, s.line, s.flip_rows) == (2, 128, 2, False) and len(s.density_lut) == 16
    for bad in (dict(scale=0), dict(scale=9), dict(alpha=257), dict(line=0), dict(line=33), dict(density_lut=[(0, 0, 0)] * 15)):
        with pytest.raises(ValueError):
            RenderSettings(**bad)


def test_launcher_render_flag():
    import train_mask_bev_amd as launcher
    args = launcher.build_parser().parse_args(['--config', 'x.yml', '--test', '--render', 'frames'])
    assert args.render == 'frames' and args.test
    assert launcher.build_parser().parse_args(['--config', 'x.yml', '--test']).render is None
    with pytest.raises(SystemExit) as e:
        launcher.main(['--config', 'x.yml', '--render', 'frames'])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        launcher.main(['--config', 'x.yml', '--train', '--render', 'frames'])
