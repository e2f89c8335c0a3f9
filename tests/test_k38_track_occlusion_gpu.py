"""K38b (mbv_track_frames_occluded, csrc/track.hip) through the C ABI, and what is built on it: ``ops.track_frames(occlusion=,
visibility=)``, ``tracking.InstanceTracker(occlusion=)``, ``Predictions.visibility`` / ``Predictions.track(visibility=)`` and
the launcher's ``track_occlusion`` key.

After every frame EVERY output and every element of the state — ``live_held`` and ``occlusion_counters`` included — equals
the numpy restatement (tests/track_occlusion_ref.py), the integers exactly, the f64 tables bit for bit, into outputs, state
tails and a workspace filled with garbage; where no track may be held the step equals ``mbv_track_frames_motion`` and, with
gain = gate = 0 in addition, ``mbv_track_frames``."""
import numpy as np
import pytest
import torch

from tests import track_motion_ref as M
from tests import track_occlusion_ref as O
from tests import track_ref as R
from tests import visibility_ref as V
from tests.track_util import call, dev, same_state, walk
from tests.util_cfg import random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
STEP = {k: v for k, v in O.OCC_PARAMS.items() if k != 'p'}
IDENT = R.IDENTITY


@pytest.fixture(scope='module')
def lib():
    from mask_bev_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('motion', [True, False])
def test_k38b_random_walk(lib, device, motion):
    """12 frames, 48 x 40, Q = 8, P = 16, random visibility bytes, a turning and moving ego."""
    frames, x_lo, y_lo = O.random_walk(380)
    pr = dict(STEP, **({} if motion else dict(gain=0.0, gate=0.0)))
    end, _ = walk(lib, device, frames, 48, 40, x_lo, y_lo, 0.5, p=O.OCC_PARAMS['p'], entry='occluded', **pr)
    assert end['counters'][2] == 12 and end['occlusion_counters'][0] > 0 and end['occlusion_counters'][1] == 0


def test_k38b_identity_where_nothing_may_be_held(lib, device):
    """The same walk: visibility == NULL and max_hold == 0 equal mbv_track_frames_motion; with gain = gate = 0 in addition
    they equal mbv_track_frames."""
    frames, x_lo, y_lo = O.random_walk(380)
    k37 = {k: v for k, v in STEP.items() if k not in ('hold_num', 'hold_den', 'max_hold')}
    k33 = {k: v for k, v in k37.items() if k not in ('gain', 'gate', 'max_shift')}
    for off in ('no map', 'max_hold 0'):
        pr = dict(STEP, max_hold=0) if off == 'max_hold 0' else STEP
        a, b = O.fresh_state(48, 40, 16), M.fresh_state(48, 40, 16)
        a0, c = O.fresh_state(48, 40, 16), R.fresh_state(48, 40, 16)
        for im, m, n, vis in frames:
            v = None if off == 'no map' else vis[None]
            rc, qt, tm, qv = call(lib, device, a, im[None], m[None], x_lo, y_lo, 0.5, ns=n[None], vis=v, entry='occluded', **pr)
            rc2, qt2, tm2, qv2 = call(lib, device, b, im[None], m[None], x_lo, y_lo, 0.5, ns=n[None], entry='motion', **k37)
            assert rc == 0 and rc2 == 0
            assert qt.tobytes() == qt2.tobytes() and tm.tobytes() == tm2.tobytes() and qv.tobytes() == qv2.tobytes()
            for key in b:
                assert a[key].tobytes() == b[key].tobytes(), (off, key)
            assert not a['live_held'].any() and not a['occlusion_counters'].any()
            rc, qt, tm, qv = call(lib, device, a0, im[None], m[None], x_lo, y_lo, 0.5, ns=n[None], vis=v, entry='occluded',
                                  **dict(pr, gain=0.0, gate=0.0))
            rc3, (kqt,), (ktm,) = call(lib, device, c, im[None], m[None], x_lo, y_lo, 0.5, entry='plain', **k33)
            assert rc3 == 0
            assert rc == 0 and qt[0].tobytes() == kqt.tobytes() and tm[0].tobytes() == ktm.tobytes()
            for key in c:
                assert a0[key].tobytes() == c[key].tobytes(), (off, key)
            assert not a0['live_held'].any() and not a0['vel'].any() and not qv.any()


GAP = dict(STEP, q_num=8, gain=0.0, gate=0.0, max_shift=0)
ARGS2 = (O.H2, O.W2, 0.0, 0.0, 1.0)
GAP4 = dict(GAP, q_num=4)                                              # for the hand-written states with P = 4


def _first_object(tracks):
    return [int(qt[2]) if k < 3 else (int(qt[5]) if k > 7 else None) for k, qt in enumerate(tracks)]


def test_k38b_scenario_a_hidden_object_keeps_its_id(lib, device):
    """Present in frames 0 – 2, absent in 3 – 7 with its footprint's visibility 0 and max_age = 2, back in frame 8: the same
    id.  The same maps through mbv_track_frames_motion give a new one."""
    frames = O.gap_scene(False)
    end, tracks = walk(lib, device, frames, *ARGS2, p=8, entry='occluded', **GAP)
    assert _first_object(tracks) == [1, 1, 1, None, None, None, None, None, 1]
    assert end['occlusion_counters'].tolist() == [5, 0] and end['counters'].tolist() == [2, 2, 9, 0]
    state = M.fresh_state(O.H2, O.W2, 8)
    k37 = {k: v for k, v in GAP.items() if k not in ('hold_num', 'hold_den', 'max_hold')}
    plain = []
    for im, m, n, _ in frames:
        rc, qt, _, _ = call(lib, device, state, im[None], m[None], 0.0, 0.0, 1.0, ns=n[None], entry='motion', **k37)
        assert rc == 0
        plain.append(qt[0])
    assert _first_object(plain) == [1, 1, 1, None, None, None, None, None, 2] and state['counters'].tolist() == [2, 3, 9, 0]


def test_k38b_scenario_b_seen_empty_footprint_dies(lib, device):
    """The same, the footprint PASSED while the object is absent: the track dies exactly as in K33a."""
    frames = O.gap_scene(True)
    end, tracks = walk(lib, device, frames, *ARGS2, p=8, entry='occluded', **GAP)
    assert _first_object(tracks) == [1, 1, 1, None, None, None, None, None, 2]
    assert end['occlusion_counters'].tolist() == [0, 0] and end['counters'].tolist() == [2, 3, 9, 0]
    k33 = R.fresh_state(O.H2, O.W2, 8)
    for k, (im, m, _, _) in enumerate(frames):
        rc, (kqt,), _ = call(lib, device, k33, im[None], m[None], 0.0, 0.0, 1.0, 8, GAP['min_iou'], GAP['max_age'], GAP['min_cells'],
                             entry='plain')
        assert rc == 0
        assert np.array_equal(kqt, tracks[k])
    for key in k33:
        assert np.array_equal(end[key], k33[key]), key


def test_k38b_max_hold_reached_mid_gap(lib, device):
    frames = O.gap_scene(False)
    end, tracks = walk(lib, device, frames, *ARGS2, p=8, entry='occluded', **dict(GAP, max_hold=2))     # held in 3 and 4, aged in 5 and 6, gone in 7
    assert _first_object(tracks)[-1] == 2 and end['occlusion_counters'].tolist() == [2, 0]
    end, tracks = walk(lib, device, frames, *ARGS2, p=8, entry='occluded', **dict(GAP, max_hold=3))     # held in 3 – 5, aged in 6 and 7, back in 8
    assert _first_object(tracks)[-1] == 1 and end['occlusion_counters'].tolist() == [3, 0]


def _hand_state(p, footprints, frame=3, seen=2, held=0, vel=None):
    """A 16 x 20 state written by hand: footprints {t: (rows, columns)}; every track last seen in frame `seen`."""
    s = O.fresh_state(O.H2, O.W2, p)
    n = len(footprints)
    for t, (ys, xs) in footprints.items():
        s['state_map'][ys, xs] = t
        iy, ix = np.nonzero(s['state_map'] == t)
        s['pos'][t] = [ix.mean() + 0.5, iy.mean() + 0.5]
    s['live_id'][:n], s['live_seen'][:n], s['live_held'][:n] = np.arange(n) + 10, seen, held
    s['counters'][:] = [n, 10 + n, frame, 0]
    if vel is not None:
        s['vel'][:n] = np.asarray(vel, np.float64)
    return s


EMPTY = np.full((O.H2, O.W2), -1, np.int32)


def test_k38b_fraction_boundary(lib, device):
    """A footprint of 20 cells at 1 / 2 and of 21 cells at 2 / 3: hidden * den == area * num holds the track, one hidden
    cell fewer does not."""
    for foot, area, num, den in ((O.FOOT, 20, 1, 2), ((slice(4, 7), slice(6, 13)), 21, 2, 3)):
        start = _hand_state(4, {0: foot}, frame=5, seen=2)              # one more unheld frame and it is gone: 5 - 2 > 2
        cells = np.argwhere(start['state_map'] == 0)
        assert len(cells) == area
        for hidden, held in ((area * num // den, True), (area * num // den - 1, False)):
            assert (hidden * den == area * num) == held
            vis = np.full((O.H2, O.W2), 3, np.uint8)
            vis[cells[:hidden, 0], cells[:hidden, 1]] = 0
            end, _ = walk(lib, device, [(EMPTY, IDENT, IDENT, vis)], *ARGS2, p=4, entry='occluded', start=start, **dict(GAP4, hold_num=num, hold_den=den))
            assert end['occlusion_counters'].tolist() == [int(held), 0] and end['counters'][0] == int(held)
            assert end['live_held'][0] == int(held) and end['live_seen'][0] == (3 if held else -1)


def test_k38b_footprint_warped_off_the_grid_is_not_held(lib, device):
    """The ego jumps 100 m: the warped footprint has no cell, area_t = 0, and nothing is hidden of nothing."""
    start = _hand_state(4, {0: O.FOOT}, frame=5, seen=2)
    far = np.array([[1.0, 0.0, 100.0], [0.0, 1.0, 0.0]])
    vis = np.zeros((O.H2, O.W2), np.uint8)
    end, _ = walk(lib, device, [(EMPTY, far, M.invert(far), vis)], *ARGS2, p=4, entry='occluded', start=start, **GAP4)
    assert end['occlusion_counters'].tolist() == [0, 0] and end['counters'].tolist() == [0, 11, 6, 0]
    # the same frame without the jump holds it
    end, _ = walk(lib, device, [(EMPTY, IDENT, IDENT, vis)], *ARGS2, p=4, entry='occluded', start=start, **GAP4)
    assert end['occlusion_counters'].tolist() == [1, 0] and end['counters'].tolist() == [1, 11, 6, 0]


def test_k38b_held_tracks_fill_the_list_and_are_dropped(lib, device):
    """P = 4: four hidden tracks that would all have aged out, three new objects: one slot is left, three held tracks are
    dropped and counted."""
    feet = {t: (slice(1 + 3 * t, 3 + 3 * t), slice(1, 5)) for t in range(4)}
    start = _hand_state(4, feet, frame=5, seen=2)
    im = EMPTY.copy()
    for q in range(3):
        im[2 + 4 * q:5 + 4 * q, 12:16] = q
    vis = np.zeros((O.H2, O.W2), np.uint8)
    end, tracks = walk(lib, device, [(im, IDENT, IDENT, vis)], *ARGS2, p=4, entry='occluded', start=start, **dict(GAP, q_num=3))
    assert end['counters'].tolist() == [4, 17, 6, 3] and end['occlusion_counters'].tolist() == [4, 0]
    assert end['live_id'].tolist() == [14, 15, 16, 10] and end['live_held'].tolist() == [0, 0, 0, 1]
    assert tracks[0].tolist() == [14, 15, 16]


def test_k38b_held_track_coasts_with_the_motion_model(lib, device):
    """Motion on: a held track's footprint moves by its whole-cell shift and its pos by its velocity, frame after frame."""
    start = _hand_state(4, {0: O.FOOT}, frame=5, seen=2, vel=[(1.0, -1.0)])
    vis = np.zeros((O.H2, O.W2), np.uint8)
    pr = dict(GAP4, gain=0.5, gate=2.0, max_shift=4)
    end, _ = walk(lib, device, [(EMPTY, IDENT, IDENT, vis)] * 3, *ARGS2, p=4, entry='occluded', start=start, **pr)
    want = np.full((O.H2, O.W2), -1, np.int32)
    want[1:5, 9:14] = 0                                                  # rows 4 – 7 up three, columns 6 – 10 right three
    assert np.array_equal(end['state_map'], want)
    assert end['pos'][0].tolist() == [start['pos'][0][0] + 3.0, start['pos'][0][1] - 3.0] and end['vel'][0].tolist() == [1.0, -1.0]
    assert end['live_held'][0] == 3 and end['live_seen'][0] == 5 and end['occlusion_counters'].tolist() == [3, 0]


def test_k38b_five_frames_in_one_call(lib, device):
    frames, x_lo, y_lo = O.random_walk(381, frames=5)
    end, tracks = walk(lib, device, frames, 48, 40, x_lo, y_lo, 0.5, p=16, entry='occluded', **STEP)
    one = O.fresh_state(48, 40, 16)
    maps, ms, ns, vis = (np.stack([f[k] for f in frames]) for k in range(4))
    rc, qt, tm, qv = call(lib, device, one, maps, ms, x_lo, y_lo, 0.5, ns=ns, vis=vis, entry='occluded', **STEP)
    assert rc == 0 and np.array_equal(qt, np.stack(tracks))
    same_state(one, end)
    again = O.fresh_state(48, 40, 16)
    rc, qt2, _, qv2 = call(lib, device, again, maps, ms, x_lo, y_lo, 0.5, ns=ns, vis=vis, entry='occluded', track_map=False, **STEP)
    assert rc == 0 and qt.tobytes() == qt2.tobytes() and qv.tobytes() == qv2.tobytes()
    same_state(one, again)


def test_k38b_error_codes(lib, device):
    from mask_bev_amd.ops_core import _ptr, _stream
    h, w, q, p = 8, 8, 4, 4
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=device)
    maps, ms, ns, vis = i32(1, h, w), f64(1, 2, 3), f64(1, 2, 3), torch.zeros((1, h, w), dtype=torch.uint8, device=device)
    sm, lid, seen, held, cnt, qt = i32(h, w), i32(p), i32(p), i32(p), i32(4), i32(1, q)
    pos, vel, mc, oc, qv = f64(p, 2), f64(p, 2), i32(2), i32(2), f64(1, q, 2)
    ws = torch.zeros((lib.mbv_track_frames_occluded_workspace_bytes(h, w, q, p),), dtype=torch.uint8, device=device)

    def call(f=1, qq=q, pp=p, gain=0.5, num=1, den=2, hold=10, vis=vis, held=held, oc=oc, mc=mc, ws_bytes=None):
        return lib.mbv_track_frames_occluded(_ptr(maps), _ptr(ms), _ptr(ns), _ptr(vis), f, h, w, 0.0, 0.0, 1.0, qq, pp, 0.3, 2, 4, gain,
                                             3.0, 4, num, den, hold, _ptr(sm), _ptr(lid), _ptr(seen), _ptr(held), _ptr(cnt),
                                             _ptr(pos), _ptr(vel), _ptr(mc), _ptr(oc), _ptr(qt), None, _ptr(qv), _ptr(ws),
                                             ws.numel() if ws_bytes is None else ws_bytes, _stream())

    assert call() == 0 and call(vis=None) == 0 and call(hold=0) == 0 and call(num=2, den=2) == 0 and call(f=0, oc=None) == 0
    for bad in (dict(num=0), dict(num=-1), dict(num=3, den=2), dict(den=0), dict(hold=-1), dict(held=None), dict(oc=None),
                dict(mc=None), dict(gain=2.0), dict(f=-1)):
        assert call(**bad) == BAD_ARG, bad
    assert call(qq=5) == UNSUPPORTED and call(pp=1025) == UNSUPPORTED
    assert call(ws_bytes=ws.numel() - 1) == WORKSPACE
    assert ws.numel() > lib.mbv_track_frames_motion_workspace_bytes(h, w, q, p)
    assert call(ws_bytes=lib.mbv_track_frames_motion_workspace_bytes(h, w, q, p)) == WORKSPACE
    assert lib.mbv_track_frames_occluded_workspace_bytes(h, w, 5, 4) == 0
    torch.cuda.synchronize()


def test_k38b_tracker_and_predictions_track(lib, device):
    """Scenario A through ``InstanceTracker(occlusion=)`` and ``Predictions.track(visibility=)``: the ids of the direct call."""
    from mask_bev_amd import ops
    from mask_bev_amd.predict import Predictions
    from mask_bev_amd.tracking import InstanceTracker, OcclusionSettings
    frames = O.gap_scene(False)
    _, want = walk(lib, device, frames, *ARGS2, p=8, entry='occluded', **GAP)
    want = np.stack(want)
    maps, vis = dev(np.stack([f[0] for f in frames]), device), dev(np.stack([f[3] for f in frames]), device)
    make = lambda **kw: InstanceTracker((0.0, float(O.W2)), (0.0, float(O.H2)), 1.0, 8, max_tracks=8, min_iou=GAP['min_iou'],
                                        max_age=GAP['max_age'], min_cells=GAP['min_cells'], device=device, **kw)
    tracker = make(occlusion=OcclusionSettings(hidden_fraction=(1, 2), max_hold=10))
    ids = tracker.update(maps[:4], visibility=vis[:4])
    pred = Predictions(labels=None, scores=None, keep=None, masks=None, areas=None, mask_scores=None, instance_map=maps[4:],
                       grid_hw=(O.H2, O.W2))
    last = pred.track(tracker, visibility=vis[4:])
    assert np.array_equal(ids.cpu().numpy(), want[:4]) and np.array_equal(last.cpu().numpy(), want[4:])
    assert tracker.counters() == dict(live=2, tracks=2, frames=9, dropped=0, held=5)
    assert not tracker.state.occlusion.live_held.any()
    # no map: nothing is held, K33a's ids; off unless passed
    tracker.reset()
    none = tracker.update(maps).cpu().numpy()
    plain = make()
    assert np.array_equal(none, plain.update(maps).cpu().numpy()) and tracker.counters()['held'] == 0
    assert tracker.counters()['tracks'] == 3 == plain.counters()['tracks'] and 'held' not in plain.counters()
    with pytest.raises(ops.MaskBevHipError):
        plain.update(maps, visibility=vis)
    with pytest.raises(ops.MaskBevHipError):
        tracker.update(maps, visibility=vis[:, :4])


def test_launcher_track_occlusion_key(device, tmp_path, capsys):
    """``track_occlusion: true`` on ``--test``: the ``point LSTQ`` line's parenthesis ends ``, held <n>``, and the numbers are
    the restatement's on the same predictions with the restated visibility maps; without the key the line has the old form."""
    import re
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd.batch import read_calib, read_poses
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.predict import voxel_geometry
    from mask_bev_amd.tracking import cur_from_prev_2d, velodyne_poses
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
    path = ck / 'tiny-epoch=00-val_loss=1.000000.ckpt'
    launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'], path, 0, 'val_loss', 1.0)
    argv = ['--config', str(tmp_path / 'tiny.yml'), '--test', '--data-root', str(tmp_path / 'data'), '--checkpoint-root',
            str(tmp_path / 'ckpt')]
    old_form = r'point LSTQ (\S+) S_assoc (\S+) S_cls (\S+) \(tubes (\d+), tracks (\d+), dropped (\d+)\)'
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(base))
    assert launcher.main(argv) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('point LSTQ')]
    assert len(lines) == 1 and re.fullmatch(old_form, lines[0]) and 'held' not in lines[0], lines
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(dict(base, track_occlusion=True, track_occlusion_z_top=-0.5,
                                                           track_hidden_fraction=[1, 3], track_max_hold=2)))
    assert launcher.main(argv) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('point LSTQ')]
    got = [re.fullmatch(old_form[:-2] + r', held (\d+)\)', l) for l in lines]
    assert len(got) == 1 and got[0], lines
    # the restatement on the predictions of the model as the launcher loads it
    loaded = MaskBevModule.from_config(dict(base, checkpoint=str(path))).to(device)
    loaded.log_scalars = False
    loaded.flatten_parameters()
    geom = voxel_geometry(loaded)
    ocx, ocy = V.origin_cell(geom.pc_range, geom.voxel_size, (0.0, 0.0, 0.0))
    vis = V.visibility_map([s.numpy() for s in scans], geom.pc_range, geom.voxel_size, geom.grid, ocx, ocy, 0.0, -0.5)
    poses = velodyne_poses(read_poses(seq / 'poses.txt'), read_calib(seq / 'calib.txt'))
    voxel = kw['voxel_size']
    ref = O.fresh_state(80, 80, 32)
    for start in (0, 2):
        pred = loaded.predict([s.to(device) for s in scans[start:start + 2]])
        assert pred.visibility([s.to(device) for s in scans[start:start + 2]], loaded,
                               launcher_settings()).cpu().numpy().tobytes() == vis[start:start + 2].tobytes()
        maps = pred.instance_map.cpu().numpy()
        for k in range(2):
            i = start + k
            m = R.IDENTITY if i == 0 else R.prev_from_cur(poses[i - 1], poses[i])
            O.step(ref, maps[k], m, cur_from_prev_2d(m), vis[i], kw['x_range'][0], kw['y_range'][0], voxel, kw['num_queries'], 0.3, 2, 2,
                   0.0, 0.0, 0, 1, 3, 2)
    assert int(got[0].group(5)) == int(ref['counters'][1]) > 0 and int(got[0].group(6)) == int(ref['counters'][3])
    assert int(got[0].group(7)) == int(ref['occlusion_counters'][0])


def launcher_settings():
    from mask_bev_amd.tracking import OcclusionSettings
    return OcclusionSettings(z_top=-0.5, hidden_fraction=(1, 3), max_hold=2)
