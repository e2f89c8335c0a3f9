"""K37 without a GPU: the numpy restatement (tests/track_motion_ref.py) against its plain-loop pieces, the scripted moving
scene's properties on the restatement (3 ids where K33a gives out 16; gain = gate = 0 equals K33a exactly), and the host
side — MotionSettings / InstanceTracker argument checks, the computed inverse transforms, the launcher keys, the binding."""
import os

import numpy as np
import pytest
import torch

from tests import track_motion_ref as M
from tests import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_pieces(state, im, q_num, x_lo, y_lo, voxel, min_cells, gate, max_shift, log):
    """The plain-loop advect, centroids and gate walk against what `M.step` logged for the same frame; `state` is the
    state BEFORE the step."""
    p = state['live_id'].shape[0]
    n_live = int(min(max(int(state['counters'][0]), 0), p))
    assert np.array_equal(M.plain_advect(state['state_map'], n_live, state['vel'], voxel, max_shift), log['moved'])
    plain_c = M.plain_centroids(im, q_num, x_lo, y_lo, voxel)
    assert set(plain_c) == set(np.nonzero(log['area_q'])[0].tolist())
    for q, (x, y) in plain_c.items():
        assert (x, y) == (float(log['c_q'][q, 0]), float(log['c_q'][q, 1]))          # bit for bit
    if gate > 0 and n_live > 0:
        assert M.plain_gate(plain_c, log['pred'], log['open_q'], log['open_t'], gate) == log['gate_taken']
    else:
        assert log['gate_taken'] == []


def _walk_ref(frames, h, w, x_lo, y_lo, voxel, q_num, p, min_iou, max_age, min_cells, gain, gate, max_shift, pieces=True):
    state, out = M.fresh_state(h, w, p), []
    for im, m, n in frames:
        before, log = M.copy_state(state), {}
        res = M.step(state, im, m, n, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells, gain, gate, max_shift, log=log)
        if pieces:
            _check_pieces(before, im, q_num, x_lo, y_lo, voxel, min_cells, gate, max_shift, log)
        out.append(res + (log['gated'],))
    return state, out


@pytest.mark.parametrize('ego', [True, False])
def test_scripted_moving_scene_on_the_restatement(ego):
    pr = M.MOTION_PARAMS
    frames = M.moving_scene(ego)
    end, out = _walk_ref(frames, M.H1, M.W1, M.X_LO1, M.Y_LO1, M.VOXEL1, **pr)
    # three objects, three ids over eight frames; the two moving cars are picked up by the gate in frame 1, never again
    assert end['counters'].tolist() == [3, 3, 8, 0] and end['motion_counters'].tolist() == [2, 0]
    assert [o[3] for o in out] == [0, 2, 0, 0, 0, 0, 0, 0]
    ids = {}
    for k, (qt, _, qv, _) in enumerate(out):
        shown = [0, 2] if k == 4 else [0, 1, 2]                       # the oncoming car (1) is missed in frame 4
        for j in shown:
            ids.setdefault(j, set()).add(int(qt[(j + k) % 4]))
        assert int(qt[(3 + k) % 4]) == -1
        parked = qv[(0 + k) % 4]
        assert float(np.hypot(*parked)) < 0.15
    assert all(len(v) == 1 for v in ids.values()) and len(set.union(*ids.values())) == 3
    if not ego:                                                        # the oncoming car: 3 m per frame towards -x
        for k in (5, 6, 7):
            assert out[k][2][(1 + k) % 4].tolist() == [-3.0, 0.0]
    # K33a on the same frames: a new id for every moving car in every frame
    k33 = R.fresh_state(M.H1, M.W1, pr['p'])
    for im, m, _ in frames:
        R.step(k33, im, m, M.X_LO1, M.Y_LO1, M.VOXEL1, pr['q_num'], pr['min_iou'], pr['max_age'], pr['min_cells'])
    assert int(k33['counters'][1]) == 16


def _identity_on(frames, h, w, x_lo, y_lo, voxel, q_num, p, min_iou, max_age, min_cells):
    a, b = M.fresh_state(h, w, p), R.fresh_state(h, w, p)
    for im, m, n in frames:
        qa = M.step(a, im, m, n, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells, 0.0, 0.0, 16)
        qb = R.step(b, im, m, x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells)
        assert np.array_equal(qa[0], qb[0]) and np.array_equal(qa[1], qb[1])
        for key in b:
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
        assert not a['vel'].any() and not qa[2].any() and not a['motion_counters'].any()


def test_identity_property_on_the_restatement():
    pr = {k: M.MOTION_PARAMS[k] for k in ('q_num', 'p', 'min_iou', 'max_age', 'min_cells')}
    for ego in (True, False):
        _identity_on(M.moving_scene(ego), M.H1, M.W1, M.X_LO1, M.Y_LO1, M.VOXEL1, **pr)
    _identity_on([(im, m, M.invert(m)) for im, m in R.scripted_scene()], R.H0, R.W0, R.X_LO0, R.Y_LO0, R.VOXEL0, **R.SCRIPT_PARAMS)
    for frames, pr in R.constructed_cases().values():
        _identity_on([(im, m, M.invert(m)) for im, m in frames], 6, 8, 0.0, 0.0, 1.0, **pr)
    scene, x_lo, y_lo = R.random_scene(3, 33, 65, 8, frames=4)
    _identity_on([(im, m, M.invert(m)) for im, m in scene], 33, 65, x_lo, y_lo, 0.5, 8, 8, 0.3, 1, 4)


@pytest.mark.parametrize('seed', range(4))
def test_restatement_pieces_agree_on_random_moving_scenes(seed):
    h, w, q = (37, 53, 6) if seed % 2 else (40, 48, 8)
    frames, x_lo, y_lo = M.random_moving_scene(seed, h, w, q, frames=5)
    end, out = _walk_ref(frames, h, w, x_lo, y_lo, 0.5, q, 12, 0.3, 2, 4, 0.5, 3.0, 6)
    assert int(end['counters'][1]) >= 2 and np.isfinite(end['vel']).all()
    # a small max_shift and a wide gate: other branches of the same pieces
    _walk_ref(frames, h, w, x_lo, y_lo, 0.5, q, 12, 0.3, 2, 4, 1.0, 8.0, 1)


def test_motion_settings_and_tracker_arguments():
    from mask_bev_amd import ops, tracking
    from mask_bev_amd.tracking import InstanceTracker, MotionSettings
    assert tracking.MotionSettings is ops.MotionSettings
    s = MotionSettings()
    assert (s.gain, s.gate_m, s.max_speed) == (0.5, 3.0, 6.0)
    assert s.max_shift(0.5) == 12 and s.max_shift(0.16) == 37 and MotionSettings(max_speed=0.0).max_shift(0.5) == 0
    for bad in (dict(gain=-0.1), dict(gain=1.5), dict(gain=float('nan')), dict(gate_m=-1.0), dict(gate_m=float('inf')),
                dict(max_speed=-1.0), dict(max_speed=float('nan'))):
        with pytest.raises(ValueError):
            MotionSettings(**bad)
    with pytest.raises(ValueError):
        InstanceTracker((0, 8), (0, 8), 1.0, 4, max_tracks=4, device='cpu', motion=dict(gain=0.5))
    plain = InstanceTracker((0, 8), (0, 8), 1.0, 4, max_tracks=4, device='cpu')
    assert plain.motion is None and plain.state.motion is None
    t = InstanceTracker((0, 8), (0, 8), 1.0, 4, max_tracks=4, device='cpu', motion=MotionSettings(gain=0.25))
    rec = t.state.motion
    assert rec.pos.shape == (4, 2) and rec.pos.dtype == torch.float64 and rec.vel.shape == (4, 2) and rec.vel.dtype == torch.float64
    assert rec.motion_counters.shape == (2,) and rec.motion_counters.dtype == torch.int32
    assert not rec.pos.any() and not rec.vel.any() and not rec.motion_counters.any()
    assert t.counters() == dict(live=0, tracks=0, frames=0, dropped=0, gated=0)
    assert ops.TrackState.fresh(4, 4, 4, 'cpu').motion is None
    # the kernels need a GPU: a missing one, or a missing motion record, is an error and never another path
    maps, ms = torch.zeros((1, 8, 8), dtype=torch.int32), torch.zeros((1, 2, 3), dtype=torch.float64)
    with pytest.raises(ops.MaskBevHipError):
        t.update(maps)
    with pytest.raises(ops.MaskBevHipError):
        ops.track_frames(maps, ms, ops.TrackState.fresh(8, 8, 4, 'cpu'), 0.0, 0.0, 1.0, 4, motion=MotionSettings())


def test_inverse_transforms():
    from mask_bev_amd import ops
    from mask_bev_amd.tracking import cur_from_prev_2d, prev_from_cur_2d
    rng = np.random.default_rng(37)
    ms = []
    for k in range(16):
        a, b = R.pose_2d(*rng.uniform(-50, 50, 2), rng.uniform(-3, 3)), R.pose_2d(*rng.uniform(-50, 50, 2), rng.uniform(-3, 3))
        ms.append(prev_from_cur_2d(a, b))
    ms = np.stack(ms)
    got = ops.invert_transforms(torch.from_numpy(ms)).numpy()
    assert got.shape == (16, 2, 3) and got.dtype == np.float64
    for m, n in zip(ms, got):
        want = np.linalg.inv(np.vstack([m, [0.0, 0.0, 1.0]]))[:2]
        # a rigid map with a shift below 150 m: both inverses are a few roundings of numbers of that size away from exact
        assert np.abs(n - want).max() <= 1e-12 * 150
        assert np.array_equal(cur_from_prev_2d(m), want)
    ident = ops.invert_transforms(torch.from_numpy(R.IDENTITY[None].copy())).numpy()[0]
    assert np.array_equal(np.abs(ident), R.IDENTITY)                   # exact, up to the sign of a zero


def test_tracking_settings_keys():
    from mask_bev_amd.evaluate import format_point_lstq, tracking_settings
    from mask_bev_amd.tracking import MotionSettings
    base = dict(min_iou=0.3, max_age=2, min_cells=4, max_tracks=256)
    assert tracking_settings({}) == base
    assert tracking_settings(dict(track_motion=False, track_gate=9.0)) == base
    got = tracking_settings(dict(track_motion=True))
    assert got.pop('motion') == MotionSettings() and got == base
    got = tracking_settings(dict(track_motion=True, track_velocity_gain=0.25, track_gate=4, track_max_speed=8, track_max_age=3))
    assert got['motion'] == MotionSettings(gain=0.25, gate_m=4.0, max_speed=8.0) and got['max_age'] == 3
    with pytest.raises(ValueError):
        tracking_settings(dict(track_motion=True, track_velocity_gain=2.0))
    res = dict(lstq=0.5, s_assoc=0.25, s_cls=1.0, tubes=3, tracks=7, dropped=1)
    assert format_point_lstq(res) == 'point LSTQ 0.5000 S_assoc 0.2500 S_cls 1.0000 (tubes 3, tracks 7, dropped 1)'
    assert format_point_lstq(dict(res, gated=4)) == 'point LSTQ 0.5000 S_assoc 0.2500 S_cls 1.0000 (tubes 3, tracks 7, dropped 1, gated 4)'


def test_binding_table_and_header():
    from mask_bev_amd import _lib, build, ops
    names = ('mbv_track_frames_motion', 'mbv_track_frames_motion_workspace_bytes')
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    for name in names:
        assert name in _lib.SIGNATURES and name + '(' in header
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [30, 4]
    assert _lib.ABI_VERSION == 59 and build.FILE_FLAGS['track.hip'] == ['-ffp-contract=off']
    for name in ('TrackMotion', 'MotionSettings', 'invert_transforms'):
        assert hasattr(ops, name)
