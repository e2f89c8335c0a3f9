"""K38b without a GPU: the numpy restatement (tests/track_occlusion_ref.py) against its plain-loop pieces and against K37's
restatement where no track may be held, the two scripted gap scenes, the host records and settings, the launcher's keys and
the declaration of the entry points."""
import os

import numpy as np
import pytest
import torch

from tests import track_motion_ref as M
from tests import track_occlusion_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = {k: v for k, v in O.OCC_PARAMS.items() if k != 'p'}


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('motion', [True, False])
def test_numpy_step_equals_the_plain_pieces(seed, motion):
    frames, x_lo, y_lo = O.random_walk(380 + seed)
    pr = dict(STEP, **({} if motion else dict(gain=0.0, gate=0.0)))
    state = O.fresh_state(48, 40, O.OCC_PARAMS['p'])
    held_total = 0
    for im, m, n, vis in frames:
        before = O.copy_state(state)
        log = {}
        O.step(state, im, m, n, vis, x_lo, y_lo, 0.5, log=log, **pr)
        n_live = int(before['counters'][0])
        area, hidden = O.plain_hidden(log['warped'], vis, O.OCC_PARAMS['p'])
        assert area == log['area_t'].tolist() and hidden == log['hidden'].tolist()
        n_present = int(np.count_nonzero(np.bincount(im[(im >= 0) & (im < pr['q_num'])], minlength=pr['q_num']) >= pr['min_cells']))
        occluded, appended, dropped = O.plain_hold(n_live, set(log['t_taken']), before['live_seen'], before['live_held'], area, hidden,
                                                   True, log['frame'], pr['max_age'], O.OCC_PARAMS['p'] - n_present, pr['hold_num'],
                                                   pr['hold_den'], pr['max_hold'])
        assert occluded == log['occluded']
        assert [t for t, _, _ in appended] == [t for t in range(n_live) if log['t_new'][t] >= 0]
        for t, seen, held in appended:
            at = int(log['t_new'][t])
            assert (int(state['live_seen'][at]), int(state['live_held'][at]), int(state['live_id'][at])) == \
                (seen, held, int(before['live_id'][t]))
        assert int(state['counters'][3]) - int(before['counters'][3]) == dropped
        assert int(state['occlusion_counters'][0]) - int(before['occlusion_counters'][0]) == len(occluded)
        assert not state['live_held'][int(state['counters'][0]):].any() and state['occlusion_counters'][1] == 0
        held_total += len(occluded)
    assert held_total > 0                                           # the walk does hold tracks


@pytest.mark.parametrize('off', ['no map', 'max_hold 0'])
def test_identity_with_k37_when_nothing_may_be_held(off):
    frames, x_lo, y_lo = O.random_walk(385)
    pr = dict(STEP, max_hold=0) if off == 'max_hold 0' else STEP
    k37 = {k: v for k, v in STEP.items() if k not in ('hold_num', 'hold_den', 'max_hold')}
    a, b = O.fresh_state(48, 40, 16), M.fresh_state(48, 40, 16)
    for im, m, n, vis in frames:
        got = O.step(a, im, m, n, None if off == 'no map' else vis, x_lo, y_lo, 0.5, **pr)
        want = M.step(b, im, m, n, x_lo, y_lo, 0.5, **k37)
        for g, w_ in zip(got, want):
            assert g.tobytes() == w_.tobytes()
        for key in b:
            assert a[key].tobytes() == b[key].tobytes(), key
        assert not a['live_held'].any() and not a['occlusion_counters'].any()


def _ids(frames, query_of, **over):
    """The id of the gap scene's first object per frame (None while it is absent), and the final state."""
    pr = dict(STEP, q_num=8, max_age=2, min_cells=4, gain=0.0, gate=0.0, max_shift=0, **over)
    state = O.fresh_state(O.H2, O.W2, 8)
    ids = []
    for k, (im, m, n, vis) in enumerate(frames):
        qt, _, _ = O.step(state, im, m, n, vis, 0.0, 0.0, 1.0, **pr)
        q = query_of(k)
        ids.append(None if q is None else int(qt[q]))
    return ids, state


def test_gap_scenes_by_the_restatement():
    query_of = lambda k: 2 if k < 3 else (5 if k > 7 else None)
    # A: out of sight while absent: the same id after five frames, five holds
    ids, end = _ids(O.gap_scene(False), query_of)
    assert ids == [1, 1, 1, None, None, None, None, None, 1] and end['occlusion_counters'].tolist() == [5, 0]
    assert end['counters'].tolist() == [2, 2, 9, 0] and not end['live_held'].any()
    # ... and without the map (K37's step) a new one
    ids, end = _ids([f[:3] + (None,) for f in O.gap_scene(False)], query_of)
    assert ids == [1, 1, 1, None, None, None, None, None, 2] and end['counters'].tolist() == [2, 3, 9, 0]
    # B: the footprint is seen empty while absent: the track dies as in K33a
    ids, end = _ids(O.gap_scene(True), query_of)
    assert ids == [1, 1, 1, None, None, None, None, None, 2] and end['occlusion_counters'].tolist() == [0, 0]
    # max_hold reached mid-gap: frames 3 and 4 held, 5 and 6 aged, gone in frame 7
    ids, end = _ids(O.gap_scene(False), query_of, max_hold=2)
    assert ids[-1] == 2 and end['occlusion_counters'].tolist() == [2, 0]
    ids, end = _ids(O.gap_scene(False), query_of, max_hold=3)
    assert ids[-1] == 1 and end['occlusion_counters'].tolist() == [3, 0]   # frames 3 – 5 held, 6 and 7 aged: still there in 8


def test_occlusion_settings_and_tracker_arguments():
    from mask_bev_amd import ops, tracking
    from mask_bev_amd.tracking import InstanceTracker, MotionSettings, OcclusionSettings
    assert tracking.OcclusionSettings is ops.OcclusionSettings
    s = OcclusionSettings()
    assert (s.z_top, s.hidden_fraction, s.max_hold, s.origin) == (-0.2, (1, 2), 10, (0.0, 0.0, 0.0))
    for bad in (dict(hidden_fraction=(0, 2)), dict(hidden_fraction=(3, 2)), dict(hidden_fraction=(1, 0)), dict(max_hold=-1),
                dict(z_top=float('nan')), dict(origin=(0.0, float('inf'), 0.0)), dict(origin=(0.0, 0.0))):
        with pytest.raises(ValueError):
            OcclusionSettings(**bad)
    with pytest.raises(ValueError):
        InstanceTracker((0, 8), (0, 8), 1.0, 4, max_tracks=4, device='cpu', occlusion=dict(max_hold=3))
    plain = InstanceTracker((0, 8), (0, 8), 1.0, 4, max_tracks=4, device='cpu')
    assert plain.occlusion is None and plain.state.occlusion is None and plain.counters() == dict(live=0, tracks=0, frames=0, dropped=0)
    t = InstanceTracker((0, 8), (0, 8), 1.0, 4, max_tracks=4, device='cpu', occlusion=OcclusionSettings(max_hold=3))
    rec = t.state.occlusion
    assert rec.live_held.shape == (4,) and rec.live_held.dtype == torch.int32 and rec.occlusion_counters.shape == (2,)
    assert not rec.live_held.any() and not rec.occlusion_counters.any() and t.state.motion is not None
    assert t.counters() == dict(live=0, tracks=0, frames=0, dropped=0, held=0)
    both = InstanceTracker((0, 8), (0, 8), 1.0, 4, max_tracks=4, device='cpu', motion=MotionSettings(), occlusion=OcclusionSettings())
    assert both.counters() == dict(live=0, tracks=0, frames=0, dropped=0, gated=0, held=0)
    # the kernels need a GPU; a map for a tracker without occlusion settings is an error, never ignored
    maps, vis = torch.zeros((1, 8, 8), dtype=torch.int32), torch.zeros((1, 8, 8), dtype=torch.uint8)
    with pytest.raises(ops.MaskBevHipError):
        t.update(maps, visibility=vis)
    with pytest.raises(ops.MaskBevHipError):
        plain.update(maps, visibility=vis)
    with pytest.raises(ops.MaskBevHipError):
        ops.track_frames(maps, torch.zeros((1, 2, 3), dtype=torch.float64), ops.TrackState.fresh(8, 8, 4, 'cpu'), 0.0, 0.0, 1.0, 4,
                         visibility=vis)


def test_tracking_settings_keys_and_the_lstq_line():
    from mask_bev_amd.evaluate import format_point_lstq, tracking_settings
    from mask_bev_amd.tracking import OcclusionSettings
    base = dict(min_iou=0.3, max_age=2, min_cells=4, max_tracks=256)
    assert tracking_settings(dict(track_occlusion=False, track_max_hold=3)) == base
    got = tracking_settings(dict(track_occlusion=True))
    assert got.pop('occlusion') == OcclusionSettings() and got == base
    got = tracking_settings(dict(track_occlusion=True, track_occlusion_z_top=-0.5, track_hidden_fraction=[2, 3], track_max_hold=5))
    assert got['occlusion'] == OcclusionSettings(z_top=-0.5, hidden_fraction=(2, 3), max_hold=5)
    with pytest.raises(ValueError):
        tracking_settings(dict(track_occlusion=True, track_hidden_fraction=[3, 2]))
    res = dict(lstq=0.5, s_assoc=0.25, s_cls=1.0, tubes=3, tracks=7, dropped=1)
    assert format_point_lstq(dict(res, held=6)) == 'point LSTQ 0.5000 S_assoc 0.2500 S_cls 1.0000 (tubes 3, tracks 7, dropped 1, held 6)'
    assert format_point_lstq(dict(res, gated=4, held=6)).endswith('(tubes 3, tracks 7, dropped 1, gated 4, held 6)')


def test_binding_table_and_header():
    from mask_bev_amd import _lib, ops
    from mask_bev_amd.predict import Predictions
    names = ('mbv_track_frames_occluded', 'mbv_track_frames_occluded_workspace_bytes')
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    for name in names:
        assert name in _lib.SIGNATURES and name + '(' in header
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [36, 4]
    assert [len(_lib.SIGNATURES[n][1]) for n in ('mbv_track_frames', 'mbv_track_frames_motion')] == [22, 30]   # unchanged
    for name in ('TrackOcclusion', 'OcclusionSettings', 'visibility_map'):
        assert hasattr(ops, name)
    assert hasattr(Predictions, 'visibility')
