"""K39 (mbv_fuse_frames and mbv_masks_from_map, csrc/fuse.hip) through the C ABI, and what is built on it: ``ops.fuse_frames``,
``ops.masks_from_map``, ``tracking.FootprintFusion``, ``Predictions.fused`` and the launcher's ``track_fuse`` key.

After every frame EVERY output and every element of the state equals the numpy restatement (tests/fuse_ref.py) exactly, into
outputs and a fresh state filled with garbage."""
import numpy as np
import pytest
import torch

from tests import fuse_ref as F
from tests import track_ref as R
from tests.fuse_util import call, dev, gpu_runner, same_state
from tests.util_cfg import random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
C = F.WALK
SETTINGS = (4, 2, 1, 2)                       # cap, hit, miss, min_count of the random walk


@pytest.fixture(scope='module')
def lib():
    from mask_bev_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def walk_frames():
    return F.random_walk()


@pytest.mark.parametrize('vis,vel,queries', [(True, True, True), (False, True, True), (True, False, True), (True, True, False)])
def test_k39a_random_walk(lib, device, walk_frames, vis, vel, queries):
    """12 frames, 40 x 48 (S = 68), Q = 8: frame by frame against the restatement, then all 12 in ONE call from a fresh state,
    then that call again: equal, bit for bit."""
    frames = [dict(fr, vis=fr['vis'] if vis else None, vel=fr['vel'] if vel else None) for fr in walk_frames]
    args = (C['x_lo'], C['y_lo'], C['voxel']) + SETTINGS + (C['static_speed'],)
    outs, states = gpu_runner(lib, device, queries)(frames, C['h'], C['w'], *args)
    assert states[-1]['owner'].shape == (68, 68) and int(states[-1]['window'][2]) == 12 and (states[-1]['owner'] >= 0).any()
    assert any((o[0] >= 0).any() for o in outs)
    one = F.fresh_state(C['h'], C['w'])
    rc, ids, qs = call(lib, device, one, frames, *args, queries=queries)
    assert rc == 0 and np.array_equal(ids, np.stack([o[0] for o in outs]))
    assert not queries or np.array_equal(qs, np.stack([o[1] for o in outs]))
    same_state(one, states[-1])
    again = F.fresh_state(C['h'], C['w'])
    rc, ids2, qs2 = call(lib, device, again, frames, *args, queries=queries)
    assert rc == 0 and ids.tobytes() == ids2.tobytes() and (not queries or qs.tobytes() == qs2.tobytes())
    same_state(one, again)


def test_k39a_scroll_wrap_and_pose_jump(lib, device):
    F.scenario_scroll_and_wrap(gpu_runner(lib, device))
    F.scenario_pose_jump(gpu_runner(lib, device))


def test_k39a_identity_is_the_track_map(lib, device):
    """cap = hit = miss = min_count = 1, no visibility, identity poses, x_lo and y_lo multiples of the voxel: fused_ids is
    mbv_track_frames' track_map bit for bit, fused_queries the instance map on present queries."""
    from tests.track_util import call as track_call
    maps = np.stack([im for im, _ in R.scripted_scene()])
    ident = np.stack([R.IDENTITY] * len(maps))
    pr = {k: v for k, v in R.SCRIPT_PARAMS.items() if k != 'p'}
    rc, qt, track_map = track_call(lib, device, R.fresh_state(R.H0, R.W0, R.SCRIPT_PARAMS['p']), maps, ident, R.X_LO0, R.Y_LO0,
                                   R.VOXEL0, entry='plain', **pr)
    assert rc == 0 and (track_map >= 0).any()
    frames = [dict(imap=im, qt=q, m=R.IDENTITY, n=R.IDENTITY) for im, q in zip(maps, qt)]
    state = F.fresh_state(R.H0, R.W0)
    rc, ids, qs = call(lib, device, state, frames, R.X_LO0, R.Y_LO0, R.VOXEL0, 1, 1, 1, 1)
    assert rc == 0 and ids.tobytes() == track_map.tobytes()
    assert np.array_equal(qs, np.where(track_map >= 0, maps, -1))


@pytest.mark.parametrize('passed', [False, True])
def test_k39a_bridging(lib, device, passed):
    F.scenario_bridging(gpu_runner(lib, device), passed)


def test_k39a_moving_query_and_invalid_pose(lib, device):
    F.scenario_moving(gpu_runner(lib, device))
    F.scenario_invalid_pose(gpu_runner(lib, device))


def test_k39_completion_and_fused_predictions(lib, device):
    """The left half is seen, then the right half with the left unknown: the fused footprint is the whole rectangle, and
    through ``Predictions.fused(...).boxes(...)`` K25's box has the whole length where the unfused one has half."""
    from mask_bev_amd import ops
    from mask_bev_amd.predict import Predictions
    from mask_bev_amd.tracking import FootprintFusion, FusionSettings
    frames, outs = F.scenario_completion(gpu_runner(lib, device))
    maps = dev(np.stack([fr['imap'] for fr in frames]), device)
    qt = dev(np.stack([fr['qt'] for fr in frames]), device)
    vis = dev(np.stack([fr['vis'] for fr in frames]), device)
    b, q = 6, 3
    labels = torch.ones((b, q), dtype=torch.int32, device=device)
    scores = torch.full((b, q), 0.9, dtype=torch.float32, device=device)
    masks, areas = ops.masks_from_map(maps, q)
    pred = Predictions(labels, scores, labels > 0, masks, areas, scores.clone(), maps, (16, 24))
    fusion = FootprintFusion((0.0, 24.0), (0.0, 16.0), 1.0, q, FusionSettings(cap=8, hit=1, miss=1, min_count=2), device=device)
    first, ids_a = Predictions(labels[:4], scores[:4], labels[:4] > 0, None, None, None, maps[:4], (16, 24)).fused(
        fusion, qt[:4], visibility=vis[:4])
    last, ids_b = Predictions(labels[4:], scores[4:], labels[4:] > 0, None, None, scores[4:], maps[4:], (16, 24)).fused(
        fusion, qt[4:], poses=np.stack([np.eye(4)] * 2), visibility=vis[4:])
    got = torch.cat([ids_a, ids_b]).cpu().numpy()
    assert np.array_equal(got, np.stack([o[0] for o in outs]))
    assert np.array_equal(torch.cat([first.instance_map, last.instance_map]).cpu().numpy(), np.stack([o[1] for o in outs]))
    assert last.labels is labels[4:] or torch.equal(last.labels, labels[4:])
    assert last.areas.cpu().tolist() == [[0, 0, 48], [0, 0, 48]] and pred.areas[4:].cpu().tolist() == [[0, 0, 24], [0, 0, 24]]
    rng = ((0.0, 24.0), (0.0, 16.0), 1.0)
    whole, half = last.boxes(*rng), Predictions(labels[4:], scores[4:], labels[4:] > 0, ops.PackedMasks(
        pred.masks.words[4 * q:], 16, 24), pred.areas[4:], None, maps[4:], (16, 24)).boxes(*rng)
    for out, length, cx in ((whole, 12.0, 10.0), (half, 6.0, 13.0)):
        assert out['query'].tolist() == [2, 2] and out['cells'].tolist() == [int(length) * 4] * 2
        bx = out['boxes'].cpu().numpy()
        assert np.allclose(bx[:, 2], length, atol=1e-3) and np.allclose(bx[:, 3], 4.0, atol=1e-3), bx
        assert np.allclose(bx[:, 0], cx, atol=1e-3) and np.allclose(bx[:, 1], 8.0, atol=1e-3), bx
    # ops.fuse_frames with static_speed None ignores a velocity; a wrong store raises
    state = ops.FusionState.fresh(16, 24, device)
    ident = dev(np.stack([R.IDENTITY] * 6), device)
    vel = torch.full((6, q, 2), 9.0, dtype=torch.float64, device=device)
    res = ops.fuse_frames(maps, qt, ident, ident, state, 0.0, 0.0, 1.0, FusionSettings(), visibility=vis, query_velocity=vel)
    assert np.array_equal(res.ids.cpu().numpy(), got)
    through = ops.fuse_frames(maps, qt, ident, ident, ops.FusionState.fresh(16, 24, device), 0.0, 0.0, 1.0,
                              FusionSettings(static_speed=1.0), visibility=vis, query_velocity=vel, queries=False)
    assert through.queries is None and np.array_equal(through.ids.cpu().numpy(), np.where(maps.cpu().numpy() >= 0, 5, -1))
    with pytest.raises(ops.MaskBevHipError):
        ops.fuse_frames(maps, qt, ident, ident, ops.FusionState.fresh(8, 8, device), 0.0, 0.0, 1.0)


@pytest.mark.parametrize('w', [40, 64])
def test_k39b_masks_from_map(lib, device, w):
    """Against mbv_pack_binary_masks of the dense one-hot masks, word for word, and against the restatement; values outside
    [0, Q) set nothing; outputs pre-filled with garbage."""
    from mask_bev_amd import ops
    from mask_bev_amd.ops_core import _ptr, _stream
    f, h, q = 3, 37, 5
    rng = np.random.default_rng(w)
    maps = rng.integers(-1, q, (f, h, w)).astype(np.int32)
    maps[rng.random(maps.shape) < 0.05] = q
    maps[0, 0, :3] = [-7, 2 ** 31 - 1, -2 ** 31]
    maps[1, 5:9] = 3                                                   # whole words of one query
    d_maps = dev(maps, device)
    n_words = lib.mbv_packed_mask_words(h, w)
    words = torch.full((f * q, n_words), 0x5a5a5a5a, dtype=torch.int32, device=device)
    areas = torch.full((f, q), 0x5a5a5a5a, dtype=torch.int32, device=device)
    assert lib.mbv_masks_from_map(_ptr(d_maps), f, h, w, q, _ptr(words), _ptr(areas), _stream()) == 0
    dense = torch.stack([(d_maps == k) for k in range(q)], dim=1).reshape(f * q, h, w).float()
    want = ops.pack_binary_masks(dense)
    assert tuple(want.words.shape) == (f * q, n_words) and torch.equal(words, want.words)
    ref_words, ref_areas = F.masks_from_map(maps, q)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), ref_words)
    assert np.array_equal(areas.cpu().numpy(), ref_areas) and np.array_equal(ref_areas, dense.sum((1, 2)).reshape(f, q).cpu().numpy())
    pm, ar = ops.masks_from_map(d_maps, q)
    assert (pm.h, pm.w) == (h, w) and torch.equal(pm.words, words) and torch.equal(ar, areas)
    # error codes; nothing is written
    keep = words.clone()
    call_ = lambda ff=f, hh=h, qq=q, m=d_maps, wd=words: lib.mbv_masks_from_map(_ptr(m), ff, hh, w, qq, _ptr(wd), _ptr(areas), _stream())
    assert call_(ff=0, m=None) == 0 and call_(qq=0, wd=None) == 0
    assert call_(ff=-1) == BAD_ARG and call_(hh=0) == BAD_ARG and call_(m=None) == BAD_ARG and call_(wd=None) == BAD_ARG
    assert call_(qq=1025) == UNSUPPORTED and call_(ff=65536) == UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(words, keep)


def test_k39a_error_codes(lib, device):
    """Odd S, S too small, Q > 1024, F * H * W = 0 and cap < 1 give the documented code, and nothing is written."""
    frames = [F.still_frame(F.rect_map(8, 8, [(0, 2, 6, 2, 6)]), [3])]
    args = (0.0, 0.0, 1.0)

    def run(s=16, q_num=None, settings=(4, 1, 1, 1), speed=0.0, fr=frames):
        state = F.fresh_state(8, 8, 16)
        state['owner'][:], state['count'][:], state['window'][:] = 11, 2, (5, 6, 7, 0)       # frames != 0: goes in as it is
        before = F.copy_state(state)
        rc, ids, qs = call(lib, device, state, fr, *args, *settings, speed, s=s, q_num=q_num, always=True)
        if rc != 0 or not fr[0]['imap'].size:
            same_state(state, before)
            assert (ids == 0x5a5a5a5a).all() and (qs == 0x5a5a5a5a).all()
        return rc

    assert run() == 0
    assert run(s=15) == UNSUPPORTED and run(s=14) == UNSUPPORTED and run(s=8194) == UNSUPPORTED       # 16 is the smallest for 8 x 8
    assert run(q_num=1025) == UNSUPPORTED
    for bad in ((0, 1, 1, 1), (4, 0, 1, 1), (4, 1, -1, 1), (4, 1, 1, 0)):
        assert run(settings=bad) == BAD_ARG, bad
    assert run(speed=-1.0) == BAD_ARG and run(speed=float('nan')) == BAD_ARG and run(s=-2) == BAD_ARG
    empty = [dict(frames[0], imap=np.zeros((0, 8), np.int32))]
    assert run(fr=empty) == 0                                          # H * W == 0: MBV_OK, nothing written
    from mask_bev_amd.ops_core import _ptr, _stream
    z = torch.zeros(4, dtype=torch.int64, device=device)
    assert lib.mbv_fuse_frames(None, None, None, None, None, None, 0, 8, 8, 16, 0.0, 0.0, 1.0, 1, 4, 1, 1, 1, 0.0, None, None, None,
                               None, None, _stream()) == 0                                # F == 0 whatever the pointers are
    assert lib.mbv_fuse_frames(None, None, None, None, None, None, 1, 8, 8, 16, 0.0, 0.0, 1.0, 1, 4, 1, 1, 1, 0.0, None, None, _ptr(z),
                               None, None, _stream()) == BAD_ARG
    assert lib.mbv_fuse_frames(None, None, None, None, None, None, 1, 8, 8, 16, 0.0, 0.0, 0.0, 1, 4, 1, 1, 1, 0.0, None, None, _ptr(z),
                               None, None, _stream()) == BAD_ARG                          # voxel 0
    torch.cuda.synchronize()
    assert not z.any()


def test_launcher_track_fuse_key(device, tmp_path, capsys):
    """``track_fuse: true`` on ``--test``: the ``point LSTQ`` line's parenthesis ends ``, fused)``; without the key the line has
    the old form."""
    import re
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd.mask_bev_module import MaskBevModule
    kw = tiny_kwargs()
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    seq = tmp_path / 'data' / 'sequences' / '08'
    for sub in ('velodyne', 'mask_cache', 'labels'):
        (seq / sub).mkdir(parents=True)
    scans = random_scans(kw, [1500, 1201, 900, 700], seed=3)
    for i, s in enumerate(scans):
        s.numpy().tofile(seq / 'velodyne' / f'{i:06d}.bin')
        imap = np.zeros((80, 80), dtype=np.int32)
        imap[10:22, 10:19], imap[40:52, 30:39] = 1, 2
        np.save(seq / 'mask_cache' / f'{i:06d}.npy', imap)
        words = np.full(s.shape[0], (3 << 16) | 10, np.uint32)
        words[::4] = 40
        words.astype('<u4').tofile(seq / 'labels' / f'{i:06d}.label')
    tr = np.array([[0.0, -1.0, 0.0, 0.1], [0.0, 0.0, -1.0, -0.2], [1.0, 0.0, 0.0, 0.3], [0.0, 0.0, 0.0, 1.0]])
    cam = [tr @ R.pose_2d(0.3 * k, 0.05 * k, 0.01 * k) @ np.linalg.inv(tr) for k in range(4)]
    np.savetxt(seq / 'poses.txt', np.stack([p[:3].reshape(-1) for p in cam]))
    (seq / 'calib.txt').write_text('P0: ' + ' '.join(['0'] * 12) + '\nTr: ' + ' '.join(repr(float(v)) for v in tr[:3].reshape(-1)) + '\n')
    base = dict(kw, dataset='semantic-kitti', batch_size=2, val_sequences=[8], train_sequences=[8], panoptic_min_points=1,
                track_instances=True, track_min_cells=2, track_max_tracks=32)
    base = {k: (list(v) if isinstance(v, tuple) else v) for k, v in base.items()}
    ck = tmp_path / 'ckpt' / 'tiny'
    ck.mkdir(parents=True)
    launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'], ck / 'tiny-epoch=00-val_loss=1.000000.ckpt', 0,
                             'val_loss', 1.0)
    argv = ['--config', str(tmp_path / 'tiny.yml'), '--test', '--data-root', str(tmp_path / 'data'), '--checkpoint-root',
            str(tmp_path / 'ckpt')]
    old_form = r'point LSTQ (\S+) S_assoc (\S+) S_cls (\S+) \(tubes (\d+), tracks (\d+), dropped (\d+)\)'
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(base))
    assert launcher.main(argv) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('point LSTQ')]
    assert len(lines) == 1 and re.fullmatch(old_form, lines[0]) and 'fused' not in lines[0], lines
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(dict(base, track_fuse=True, track_fuse_cap=4, track_fuse_min_count=1)))
    assert launcher.main(argv) == 0
    fused = capsys.readouterr().out.splitlines()
    got = [re.fullmatch(old_form[:-2] + r', fused\)', l) for l in fused if l.startswith('point LSTQ')]
    assert len(got) == 1 and got[0], fused
    # the tracker ran on the unfused maps: its counts (tracks, dropped) are the plain run's.  Nothing else is compared: the
    # lift and the labels come from the fused map, and ``val_loss`` is not bit-reproducible between two runs of one process
    # (tests/test_k36_render_gpu.py says why)
    want = re.fullmatch(old_form, lines[0])
    assert got[0].group(5) == want.group(5) and got[0].group(6) == want.group(6)
