"""K37 (the tracker step with the constant-velocity motion model and the gated second stage, csrc/track.hip) through the C
ABI, and what is built on it: ``ops.track_frames(motion=)``, ``tracking.InstanceTracker(motion=)``, ``Predictions.track`` and
the launcher's ``track_motion`` key.

After every frame EVERY output and every element of the state and of the motion record equals the numpy restatement
(tests/track_motion_ref.py) — the integers exactly, ``pos`` / ``vel`` / ``query_velocity`` bit for bit as f64 — into outputs,
state tails and a workspace filled with garbage; with gain = gate = 0 the step equals ``mbv_track_frames``."""
import numpy as np
import pytest
import torch

from tests import track_motion_ref as M
from tests import track_ref as R
from tests import track_util
from tests.track_util import call, dev, same_state, walk
from tests.util_cfg import random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
STEP_PARAMS = {k: v for k, v in M.MOTION_PARAMS.items() if k != 'p'}          # `M.step` takes P from the state


def test_k37_scripted_moving_scene(device):
    """Three objects, two of them too fast for K33a's overlap: 3 ids over 8 frames (K33a gives out 16), after every frame
    everything equal to the restatement, and one call of 8 frames equal to eight calls of one."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    pr = M.MOTION_PARAMS
    for ego in (True, False):
        frames = M.moving_scene(ego)
        end, _ = walk(lib, device, frames, M.H1, M.W1, M.X_LO1, M.Y_LO1, M.VOXEL1, **pr, entry='motion')
        assert end['counters'].tolist() == [3, 3, 8, 0] and end['motion_counters'].tolist() == [2, 0]
        one = M.fresh_state(M.H1, M.W1, pr['p'])
        maps, ms, ns = (np.stack([f[k] for f in frames]) for k in range(3))
        rc, qt, tm, qv = call(lib, device, one, maps, ms, M.X_LO1, M.Y_LO1, M.VOXEL1, pr['q_num'], pr['min_iou'], pr['max_age'],
                              pr['min_cells'], pr['gain'], pr['gate'], pr['max_shift'], ns=ns, entry='motion')
        assert rc == 0
        same_state(one, end)
        ref = M.fresh_state(M.H1, M.W1, pr['p'])
        for k, (im, m, n) in enumerate(frames):
            rqt, rtm, rqv = M.step(ref, im, m, n, M.X_LO1, M.Y_LO1, M.VOXEL1, **STEP_PARAMS)
            assert np.array_equal(qt[k], rqt) and np.array_equal(tm[k], rtm) and qv[k].tobytes() == rqv.tobytes()
        assert sorted(set(qt[qt >= 0].tolist())) == [0, 1, 2]
        # twice: bit-equal
        again = M.fresh_state(M.H1, M.W1, pr['p'])
        rc, qt2, tm2, qv2 = call(lib, device, again, maps, ms, M.X_LO1, M.Y_LO1, M.VOXEL1, pr['q_num'], pr['min_iou'],
                                 pr['max_age'], pr['min_cells'], pr['gain'], pr['gate'], pr['max_shift'], ns=ns, entry='motion',
                                 track_map=False)
        assert rc == 0 and qt.tobytes() == qt2.tobytes() and qv.tobytes() == qv2.tobytes()
        same_state(one, again)


def _identity(lib, device, frames, h, w, x_lo, y_lo, voxel, q_num, p, min_iou, max_age, min_cells):
    a, b = M.fresh_state(h, w, p), R.fresh_state(h, w, p)
    for im, m in frames:
        rc, qt, tm, qv = call(lib, device, a, im[None], np.asarray(m)[None], x_lo, y_lo, voxel, q_num, min_iou, max_age, min_cells,
                              0.0, 0.0, 16, ns=M.invert(m)[None], entry='motion')
        assert rc == 0
        rc, (kqt,), (ktm,) = call(lib, device, b, im[None], np.asarray(m)[None], x_lo, y_lo, voxel, q_num, min_iou, max_age,
                                  min_cells, entry='plain')
        assert rc == 0
        assert qt[0].tobytes() == kqt.tobytes() and tm[0].tobytes() == ktm.tobytes()
        for k in b:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert not a['vel'].any() and not qv.any() and not a['motion_counters'].any()


def test_k37_identity_with_gain_and_gate_zero(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    _identity(lib, device, R.scripted_scene(), R.H0, R.W0, R.X_LO0, R.Y_LO0, R.VOXEL0, **R.SCRIPT_PARAMS)
    for frames, pr in R.constructed_cases().values():
        _identity(lib, device, frames, 6, 8, 0.0, 0.0, 1.0, **pr)
    scene, x_lo, y_lo = R.random_scene(3, 33, 65, 8, frames=4)
    _identity(lib, device, scene, 33, 65, x_lo, y_lo, 0.5, 8, 8, 0.3, 1, 4)


def _hand_state(p, footprints, pos, vel, frame=1):
    """A 6 x 8 state written by hand: footprints {t: [(iy, ix), ..]}, every track seen in frame 0."""
    s = M.fresh_state(6, 8, p)
    n = len(pos)
    for t, cells in footprints.items():
        for iy, ix in cells:
            s['state_map'][iy, ix] = t
    s['live_id'][:n], s['live_seen'][:n] = np.arange(n) + 10, 0
    s['counters'][:] = [n, 10 + n, frame, 0]
    s['pos'][:n], s['vel'][:n] = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    return s


def _grid(cells):
    im = np.full((6, 8), -1, np.int32)
    for q, where in cells.items():
        for iy, ix in where:
            im[iy, ix] = q
    return im


ARGS68 = (6, 8, 0.0, 0.0, 1.0)                                         # h, w, x_lo, y_lo, voxel


def test_k37_advect_edge_cases(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    empty, ident = _grid({}), R.IDENTITY
    sq = lambda iy, ix: [(iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1)]
    walk = lambda start, im, max_shift, gain=0.5: track_util.walk(lib, device, [(im, ident, ident)], *ARGS68, 4, 4, 0.3, 2, 1, gain,
                                                                   0.0, max_shift, start=start, entry='motion')[0]
    # two tracks shifted onto the same cells: the smaller index wins, the other has no cell left; both coast
    end = walk(_hand_state(4, {0: sq(1, 0), 1: sq(1, 2)}, [(1.0, 2.0), (3.0, 2.0)], [(2.0, 0.0), (0.0, 0.0)]), empty, 4)
    assert np.array_equal(end['state_map'], _grid({0: sq(1, 2)})) and end['counters'][0] == 2
    assert end['pos'][:2].tolist() == [[3.0, 2.0], [3.0, 2.0]] and end['vel'][:2].tolist() == [[2.0, 0.0], [0.0, 0.0]]
    # ... and the larger index moved onto the smaller: still the smaller wins
    end = walk(_hand_state(4, {0: sq(1, 2), 1: sq(1, 0)}, [(3.0, 2.0), (1.0, 2.0)], [(0.0, 0.0), (2.0, 0.0)]), empty, 4)
    assert np.array_equal(end['state_map'], _grid({0: sq(1, 2)}))
    # a shift that carries part of a footprint off the grid, in x and (negative) in y
    end = walk(_hand_state(4, {0: sq(0, 6)}, [(7.0, 1.0)], [(1.0, -1.0)]), empty, 4)
    assert np.array_equal(end['state_map'], _grid({0: [(0, 7)]}))
    # |shift| > max_shift gives 0 for both components; rint(2.5) = 2 is inside max_shift = 2
    end = walk(_hand_state(4, {0: sq(1, 0)}, [(1.0, 2.0)], [(3.0, 1.0)]), empty, 2)
    assert np.array_equal(end['state_map'], _grid({0: sq(1, 0)})) and end['vel'][0].tolist() == [3.0, 1.0]
    end = walk(_hand_state(4, {0: sq(1, 0)}, [(1.0, 2.0)], [(2.5, -0.5)]), empty, 2)
    assert np.array_equal(end['state_map'], _grid({0: sq(1, 2)}))
    # a NaN and an inf velocity component: no shift (the other component's neither), the tracks are matched where they
    # stand and the stored velocity is finite
    start = _hand_state(4, {0: sq(0, 0), 1: sq(3, 4)}, [(1.0, 1.0), (5.0, 4.0)], [(np.nan, 1.0), (2.0, -np.inf)])
    end = walk(start, _grid({2: sq(0, 0), 0: sq(3, 4)}), 4)
    assert end['live_id'][:2].tolist() == [11, 10] and end['counters'].tolist() == [2, 12, 2, 0]
    assert np.isfinite(end['vel']).all() and not end['vel'].any() and end['pos'][:2].tolist() == [[5.0, 4.0], [1.0, 1.0]]


def test_k37_gate_order(device):
    """Integer geometry (voxel 1, single cells, centroids at .5): d2 is exact.  The tracks have no footprint, so step 3
    matches nothing and step 3b decides."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    ident = R.IDENTITY
    walk = lambda start, im, gate, q=4: track_util.walk(lib, device, [(im, ident, ident)], *ARGS68, q, 4, 0.3, 2, 1, 0.5, gate, 4,
                                                         start=start, entry='motion')[0]
    zero = [(0.0, 0.0)]
    # two queries equidistant (d2 = 4 = gate^2, accepted) from one track: the smaller q takes it
    im = _grid({1: [(2, 1)], 3: [(2, 5)]})
    end = walk(_hand_state(4, {}, [(3.5, 2.5)], zero), im, 2.0)
    assert end['live_id'][:2].tolist() == [10, 11] and end['motion_counters'].tolist() == [1, 0]
    assert end['vel'][0].tolist() == [-1.0, 0.0]                       # 0.5 * (1.5 - 3.5)
    # just below: nobody is inside the gate; and gate = 0 switches the stage off
    for gate in (1.9999999, 0.0):
        end = walk(_hand_state(4, {}, [(3.5, 2.5)], zero), im, gate)
        assert end['live_id'][:3].tolist() == [11, 12, 10] and end['motion_counters'].tolist() == [0, 0]
    # one query equidistant from two tracks: the smaller t is taken, the other coasts
    end = walk(_hand_state(4, {}, [(1.5, 2.5), (5.5, 2.5)], zero * 2), _grid({2: [(2, 3)]}), 2.0)
    assert end['live_id'][:2].tolist() == [10, 11] and end['live_seen'][:2].tolist() == [1, 0]
    # a nearer pair goes first: query 3 is 1 away from track 1, query 0 is 2 away from both tracks → 0 gets track 0
    end = walk(_hand_state(4, {}, [(1.5, 0.5), (5.5, 0.5)], zero * 2), _grid({0: [(0, 3)], 3: [(0, 6)]}), 2.0)
    assert end['live_id'][:2].tolist() == [10, 11] and end['motion_counters'].tolist() == [2, 0]
    # a query matched in step 3 takes no part: query 0 overlaps track 0's footprint; track 1 (no footprint) lies ON query
    # 0's centroid and 2 away from query 1, which takes it
    foot = [(2, 0), (2, 1)]
    end = walk(_hand_state(4, {0: foot}, [(1.0, 2.5), (1.0, 2.5)], zero * 2), _grid({0: foot, 1: [(2, 3)]}), 2.5)
    assert end['live_id'][:2].tolist() == [10, 11] and end['motion_counters'].tolist() == [1, 0]
    assert end['pos'][:2].tolist() == [[1.0, 2.5], [3.5, 2.5]]


@pytest.mark.parametrize('seed', [0, 1])
def test_k37_odd_grid_random_moving_scenes(device, seed):
    """37 x 53 = 1961 cells: 8 blocks of 256, the last with 169 threads in use."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    frames, x_lo, y_lo = M.random_moving_scene(40 + seed, 37, 53, 6, frames=5)
    end, _ = walk(lib, device, frames, 37, 53, x_lo, y_lo, 0.5, 6, 12, 0.3, 2, 4, 0.5, 3.0, 6, entry='motion')
    assert end['counters'][1] >= 2 and end['counters'][2] == 5


def test_k37_table_limits(device):
    """Q = 300, P = 1024 on 64 x 64: about 40 moving rectangles and scattered cells over 4 frames, min_cells = 1: tables past
    256 entries, hundreds of gate candidates per track and several match rounds in both stages."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    frames, x_lo, y_lo = M.random_moving_scene(37, 64, 64, 300, frames=4, rects=40)
    rng = np.random.default_rng(38)
    noisy = []
    for im, m, n in frames:
        im = im.copy()
        at = rng.random(im.shape) < 0.12
        im[at] = rng.integers(0, 300, int(at.sum()))
        noisy.append((im, m, n))
    end, _ = walk(lib, device, noisy, 64, 64, x_lo, y_lo, 0.5, 300, 1024, 0.05, 2, 1, 0.5, 3.0, 6, entry='motion')
    assert end['counters'][0] > 300 and end['counters'][1] > 300 and end['motion_counters'][0] > 50


def test_k37_smallest_tables(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    ident = R.IDENTITY
    # Q = P = 1: an object that moves two cells per frame: the gate takes it in frames 1 and 2 (velocity 1.0, then 1.5 cells
    # per frame, so the footprint shifted by one cell still misses it in frame 2), the overlap in frame 3
    frames = [(_grid({0: [(2, 2 * k), (3, 2 * k)]}), ident, ident) for k in range(4)]
    end, _ = walk(lib, device, frames, *ARGS68, 1, 1, 0.3, 2, 1, 0.5, 3.0, 4, entry='motion')
    assert end['counters'].tolist() == [1, 1, 4, 0] and end['motion_counters'].tolist() == [2, 0]
    assert end['vel'].tolist() == [[1.75, 0.0]]
    # Q = 0: nothing is ever present; a track written by hand coasts and then dies
    start = _hand_state(2, {0: [(1, 1)]}, [(1.5, 1.5)], [(1.0, 0.0)])
    end, _ = walk(lib, device, [(_grid({}), ident, ident)] * 3, *ARGS68, 0, 2, 0.3, 1, 1, 0.5, 3.0, 4, start=start, entry='motion')
    assert end['counters'].tolist() == [0, 11, 4, 0] and not end['pos'].any()


def test_k37_error_codes(device):
    from mask_bev_amd import _lib
    from mask_bev_amd.ops_core import _ptr, _stream
    lib = _lib.load()
    h, w, q, p = 8, 8, 4, 4
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=device)
    maps, ms, ns = i32(1, h, w), f64(1, 2, 3), f64(1, 2, 3)
    sm, lid, seen, cnt, qt = i32(h, w), i32(p), i32(p), i32(4), i32(1, q)
    pos, vel, mc, qv = f64(p, 2), f64(p, 2), i32(2), f64(1, q, 2)
    ws = torch.zeros((lib.mbv_track_frames_motion_workspace_bytes(h, w, q, p),), dtype=torch.uint8, device=device)

    def call(f=1, hh=h, ww=w, qq=q, pp=p, age=2, cells=4, gain=0.5, gate=3.0, shift=4, maps=maps, ns=ns, pos=pos, vel=vel, mc=mc,
             qv=qv, ws_bytes=None, ws=ws):
        return lib.mbv_track_frames_motion(_ptr(maps), _ptr(ms), _ptr(ns), f, hh, ww, 0.0, 0.0, 1.0, qq, pp, 0.3, age, cells, gain,
                                           gate, shift, _ptr(sm), _ptr(lid), _ptr(seen), _ptr(cnt), _ptr(pos), _ptr(vel), _ptr(mc),
                                           _ptr(qt), None, _ptr(qv), _ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                           _stream())

    nan, inf = float('nan'), float('inf')
    assert call() == 0 and call(gain=0.0, gate=0.0, shift=0) == 0 and call(gain=1.0) == 0
    assert lib.mbv_track_frames_motion(None, None, None, 0, h, w, 0.0, 0.0, 1.0, q, p, 0.3, 2, 4, 0.5, 3.0, 4, None, None, None, None,
                                       None, None, None, None, None, None, None, 0, _stream()) == 0
    for bad in (dict(gain=-0.01), dict(gain=1.01), dict(gain=nan), dict(gain=inf), dict(gate=-1.0), dict(gate=nan), dict(gate=inf),
                dict(shift=-1), dict(pos=None), dict(vel=None), dict(mc=None), dict(ns=None), dict(qv=None), dict(maps=None),
                dict(cells=0), dict(age=-1), dict(f=-1), dict(hh=-1)):
        assert call(**bad) == BAD_ARG, bad
    assert call(qq=5) == UNSUPPORTED and call(pp=1025) == UNSUPPORTED and call(hh=1025, ww=1024) == UNSUPPORTED
    assert call(ws_bytes=ws.numel() - 1) == WORKSPACE and call(ws=None, ws_bytes=1 << 30) == WORKSPACE
    assert ws.numel() > lib.mbv_track_frames_workspace_bytes(h, w, q, p)
    assert call(ws_bytes=lib.mbv_track_frames_workspace_bytes(h, w, q, p)) == WORKSPACE
    assert lib.mbv_track_frames_motion_workspace_bytes(h, w, 5, 4) == 0
    assert lib.mbv_track_frames_motion_workspace_bytes(1025, 1024, 4, 4) == 0
    assert lib.mbv_track_frames_motion_workspace_bytes(1024, 1024, 300, 1024) > 0
    torch.cuda.synchronize()


def test_k37_tracker_and_predictions_track(device):
    """The scripted scene through ``InstanceTracker(motion=)``: poses on the host (both transforms computed there), then
    ``prev_from_cur`` as a device tensor (the inverse computed on the device), and ``Predictions.track``."""
    from mask_bev_amd import ops
    from mask_bev_amd.predict import Predictions
    from mask_bev_amd.tracking import InstanceTracker, MotionSettings, cur_from_prev_2d, prev_from_cur_2d
    pr = M.MOTION_PARAMS
    frames = M.moving_scene(True)
    maps = dev(np.stack([f[0] for f in frames]), device)
    poses = np.stack([R.pose_2d(0.8 * k, 0.0, 0.03 * k) for k in range(8)])
    settings = MotionSettings(gain=pr['gain'], gate_m=pr['gate'], max_speed=8.0)            # floor(8 / 0.5) = 16 cells
    make = lambda: InstanceTracker((M.X_LO1, M.X_LO1 + M.W1 * M.VOXEL1), (M.Y_LO1, M.Y_LO1 + M.H1 * M.VOXEL1), M.VOXEL1, pr['q_num'],
                                   max_tracks=pr['p'], min_iou=pr['min_iou'], max_age=pr['max_age'], min_cells=pr['min_cells'],
                                   device=device, motion=settings)
    tracker = make()
    assert (tracker.h, tracker.w) == (M.H1, M.W1)
    ref, want, want_v = M.fresh_state(M.H1, M.W1, pr['p']), [], []
    for k in range(8):
        m = R.IDENTITY if k == 0 else prev_from_cur_2d(poses[k - 1], poses[k])
        qt, _, qv = M.step(ref, frames[k][0], m, cur_from_prev_2d(m), M.X_LO1, M.Y_LO1, M.VOXEL1, **STEP_PARAMS)
        want.append(qt)
        want_v.append(qv)
    want, want_v = np.stack(want), np.stack(want_v)
    ids = tracker.update(maps[:3], poses=poses[:3])
    rec = tracker.update(maps[3:6], poses=poses[3:6], record=True)
    pred = Predictions(labels=None, scores=None, keep=None, masks=None, areas=None, mask_scores=None, instance_map=maps[6:],
                       grid_hw=(M.H1, M.W1))
    last = pred.track(tracker, poses=poses[6:])
    assert np.array_equal(ids.cpu().numpy(), want[:3]) and np.array_equal(last.cpu().numpy(), want[6:])
    assert rec.track_map is None and np.array_equal(rec.query_track.cpu().numpy(), want[3:6])
    assert rec.query_velocity.cpu().numpy().tobytes() == want_v[3:6].tobytes()
    assert tracker.counters() == dict(live=3, tracks=3, frames=8, dropped=0, gated=2)
    assert tracker.state.motion.vel.cpu().numpy().tobytes() == ref['vel'].tobytes()
    # the transforms as a device tensor: the inverse is computed on the device, the same ids
    other = make()
    ms = dev(np.stack([R.IDENTITY if k == 0 else prev_from_cur_2d(poses[k - 1], poses[k]) for k in range(8)]), device)
    out = other.update(maps, prev_from_cur=ms, track_map=True)
    assert np.array_equal(out.query_track.cpu().numpy(), want) and out.query_velocity.shape == (8, pr['q_num'], 2)
    assert np.abs(out.query_velocity.cpu().numpy() - want_v).max() < 1e-9
    assert other.counters()['tracks'] == 3
    # without a motion model the same frames take 16 ids, and the record holds no velocity
    plain = InstanceTracker((M.X_LO1, M.X_LO1 + M.W1 * M.VOXEL1), (M.Y_LO1, M.Y_LO1 + M.H1 * M.VOXEL1), M.VOXEL1, pr['q_num'],
                            max_tracks=pr['p'], min_iou=pr['min_iou'], max_age=pr['max_age'], min_cells=pr['min_cells'], device=device)
    assert plain.update(maps, poses=poses, record=True).query_velocity is None
    assert plain.counters() == dict(live=7, tracks=16, frames=8, dropped=0)
    other.reset()
    assert other.counters() == dict(live=0, tracks=0, frames=0, dropped=0, gated=0) and not other.state.motion.pos.any()
    with pytest.raises(ops.MaskBevHipError):
        ops.track_frames(maps, ms, ops.TrackState.fresh(M.H1, M.W1, pr['p'], device), M.X_LO1, M.Y_LO1, M.VOXEL1, pr['q_num'],
                         motion=settings)


def test_launcher_track_motion_key(device, tmp_path, capsys):
    """``track_motion: true`` on ``--test``: the ``point LSTQ`` line's parenthesis gains ``, gated <n>``, and the numbers are
    the restatement's on the same predictions; without the key the line has exactly the old form."""
    import re
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd.batch import read_calib, read_poses
    from mask_bev_amd.mask_bev_module import MaskBevModule
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
    assert len(lines) == 1 and re.fullmatch(old_form, lines[0]) and 'gated' not in lines[0], lines
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(dict(base, track_motion=True, track_velocity_gain=0.5, track_gate=4.0,
                                                           track_max_speed=3.0)))
    assert launcher.main(argv) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('point LSTQ')]
    got = [re.fullmatch(old_form[:-2] + r', gated (\d+)\)', l) for l in lines]
    assert len(got) == 1 and got[0], lines
    # the restatement on the predictions of the model as the launcher loads it
    loaded = MaskBevModule.from_config(dict(base, checkpoint=str(path))).to(device)
    loaded.log_scalars = False
    loaded.flatten_parameters()
    poses = velodyne_poses(read_poses(seq / 'poses.txt'), read_calib(seq / 'calib.txt'))
    voxel = kw['voxel_size']
    ref = M.fresh_state(80, 80, 32)
    for start in (0, 2):
        maps = loaded.predict([s.to(device) for s in scans[start:start + 2]]).instance_map.cpu().numpy()
        for k in range(2):
            i = start + k
            m = R.IDENTITY if i == 0 else R.prev_from_cur(poses[i - 1], poses[i])
            M.step(ref, maps[k], m, cur_from_prev_2d(m), kw['x_range'][0], kw['y_range'][0], voxel, kw['num_queries'], 0.3, 2, 2, 0.5,
                   4.0, int(np.floor(3.0 / voxel)))
    assert int(got[0].group(5)) == int(ref['counters'][1]) > 0 and int(got[0].group(6)) == int(ref['counters'][3])
    assert int(got[0].group(7)) == int(ref['motion_counters'][0])
