"""K39 without a GPU: the numpy restatement (tests/fuse_ref.py) against its plain-loop version, the scenarios on the
restatement, and the host side: FootprintFusion's transforms, the settings, the launcher keys, the binding table."""
import os

import numpy as np
import pytest
import torch

from tests import fuse_ref as F
from tests import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('vis,vel', [(True, True), (False, True), (True, False)])
def test_restatement_equals_plain_loops(vis, vel):
    c = F.WALK
    frames = [dict(fr, vis=fr['vis'] if vis else None, vel=fr['vel'] if vel else None) for fr in F.random_walk()]
    a, b = F.fresh_state(c['h'], c['w']), F.fresh_state(c['h'], c['w'])
    assert a['owner'].shape == (68, 68)
    args = (c['x_lo'], c['y_lo'], c['voxel'], 4, 2, 1, 2, c['static_speed'])
    for k, fr in enumerate(frames):
        (ids, qs), = F.run(a, [fr], *args)
        (pids, pqs), = F.run(b, [fr], *args, fn=F.plain_step)
        assert ids.dtype == np.int32 and np.array_equal(ids, pids) and np.array_equal(qs, pqs), k
        for key in a:
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (k, key)
    assert int(a['window'][2]) == 12 and (a['owner'] >= 0).any() and a['window'][0] < 0


def test_walk_turns_past_pi_and_goes_negative():
    frames = F.random_walk()
    m = frames[-1]['m']
    assert 0.3 * 11 > np.pi and abs(np.hypot(m[0, 0], m[1, 0]) - 1.0) < 1e-12
    assert any(np.isnan(fr['vel']).any() for fr in frames) and any((fr['qt'] < 0).any() for fr in frames)
    assert any(((fr['imap'] >= 8) | (fr['imap'] < -1)).any() for fr in frames)
    for fr in frames:
        assert np.allclose(np.vstack([fr['m'], [0, 0, 1]]) @ np.vstack([fr['n'], [0, 0, 1]]), np.eye(3), atol=1e-12)


def test_masks_restatement_equals_plain_loops():
    rng = np.random.default_rng(1)
    for h, w in ((5, 40), (3, 64)):
        maps = rng.integers(-2, 6, (2, h, w)).astype(np.int32)
        words, areas = F.masks_from_map(maps, 4)
        pw, pa = F.plain_masks_from_map(maps, 4)
        assert words.dtype == np.uint32 and words.shape == (8, F.packed_words(h, w))
        assert np.array_equal(words, pw) and np.array_equal(areas, pa)
        assert int(areas.sum()) == int(((maps >= 0) & (maps < 4)).sum())


def test_scenarios_on_the_restatement():
    F.scenario_scroll_and_wrap(F.ref_runner)
    F.scenario_pose_jump(F.ref_runner)
    F.scenario_bridging(F.ref_runner, passed=False)
    F.scenario_bridging(F.ref_runner, passed=True)
    F.scenario_completion(F.ref_runner)
    F.scenario_moving(F.ref_runner)
    F.scenario_invalid_pose(F.ref_runner)


def test_identity_settings_give_the_track_map():
    """cap = hit = miss = min_count = 1, identity poses, grid origin on cell borders: fused_ids is K33a's track_map."""
    state, fused = R.fresh_state(R.H0, R.W0, 4), F.fresh_state(R.H0, R.W0)
    for imap, _ in R.scripted_scene():
        qt, track_map = R.step(state, imap, R.IDENTITY, R.X_LO0, R.Y_LO0, R.VOXEL0, **{k: v for k, v in R.SCRIPT_PARAMS.items() if k != 'p'})
        ids, qs = F.step(fused, imap, qt, R.IDENTITY, R.IDENTITY, R.X_LO0, R.Y_LO0, R.VOXEL0, 1, 1, 1, 1)
        assert np.array_equal(ids, track_map) and np.array_equal(qs, np.where(track_map >= 0, imap, -1))


def test_footprint_fusion_transforms_follow_the_chain():
    from mask_bev_amd.tracking import FootprintFusion, cur_from_prev_2d, prev_from_cur_2d
    fusion = FootprintFusion((-20.0, 4.0), (-4.0, 16.0), 0.5, 8, device='cpu')
    assert (fusion.h, fusion.w) == (40, 48) and tuple(fusion.state.owner.shape) == (68, 68)
    poses = np.stack([R.pose_2d(0.7 * k + 3.0, -0.4 * k, 0.31 * k + 0.2) for k in range(9)])
    m1, n1 = fusion.transforms(4, poses[:4])
    m2, n2 = fusion.transforms(5, poses[4:])                           # the origin is remembered between calls
    m, n = np.concatenate([m1, m2]), np.concatenate([n1, n2])
    chain = np.eye(3)
    for k in range(9):
        if k:
            chain = chain @ np.vstack([prev_from_cur_2d(poses[k - 1], poses[k]), [0.0, 0.0, 1.0]])
        assert np.allclose(m[k], chain[:2], rtol=0, atol=1e-12), k
        assert np.array_equal(n[k], cur_from_prev_2d(m[k]))
    assert np.allclose(m[0], R.IDENTITY, rtol=0, atol=1e-15)         # inv(origin) @ origin, rounded
    fusion.reset()
    assert np.allclose(fusion.transforms(1, poses[5:6])[0][0], R.IDENTITY, rtol=0, atol=1e-15)
    still_m, still_n = fusion.transforms(2)
    assert np.array_equal(still_m, np.stack([R.IDENTITY] * 2)) and np.array_equal(still_n, still_m)
    bad = fusion.transforms(1, world_from_cur=np.array([[[1.0, 0.0, np.nan], [0.0, 1.0, 0.0]]]))[1]
    assert np.isnan(bad).all()


def test_settings_validation_and_store_size():
    from mask_bev_amd import ops
    from mask_bev_amd.tracking import FootprintFusion, FusionSettings
    s = FusionSettings()
    assert (s.cap, s.hit, s.miss, s.min_count, s.static_speed) == (8, 1, 1, 2, None)
    assert FusionSettings(miss=0, static_speed=0).static_speed == 0.0
    for bad in (dict(cap=0), dict(hit=0), dict(miss=-1), dict(min_count=0), dict(static_speed=-1.0), dict(static_speed=float('nan')),
                dict(static_speed=float('inf')), dict(cap=2 ** 31)):
        with pytest.raises(ValueError):
            FusionSettings(**bad)
    for h, w in ((40, 48), (8, 8), (3, 4), (500, 500), (1024, 1024), (1, 1), (0, 0)):
        assert ops.fusion_store_size(h, w) == F.store_size(h, w), (h, w)
    assert ops.fusion_store_size(40, 48) == 68 and ops.fusion_store_size(3, 4) == 10
    with pytest.raises(ValueError):
        FootprintFusion((0.0, 8.0), (0.0, 8.0), 1.0, 2000, device='cpu')
    with pytest.raises(ValueError):
        FootprintFusion((0.0, 8.0), (0.0, 8.0), 1.0, 4, settings=dict(cap=3), device='cpu')
    fusion = FootprintFusion((0.0, 8.0), (0.0, 8.0), 1.0, 4, device='cpu')
    with pytest.raises(ops.MaskBevHipError):                           # no CPU fallback
        fusion.update(torch.zeros((1, 8, 8), dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(ops.MaskBevHipError):
        ops.masks_from_map(torch.zeros((1, 8, 8), dtype=torch.int32), 4)


def test_launcher_keys_and_the_lstq_line():
    from mask_bev_amd.evaluate import format_point_lstq, fusion_settings, tracking_settings
    from mask_bev_amd.tracking import FusionSettings
    assert fusion_settings(dict()) is None and fusion_settings(dict(track_fuse=False, track_fuse_cap=3)) is None
    assert fusion_settings(dict(track_fuse=True)) == FusionSettings()
    assert fusion_settings(dict(track_fuse=True, track_fuse_cap=5, track_fuse_min_count=3, track_fuse_static_speed=0.25)) == \
        FusionSettings(cap=5, min_count=3)                             # the static speed needs track_motion
    assert fusion_settings(dict(track_fuse=True, track_motion=True, track_fuse_static_speed=0.25)).static_speed == 0.25
    assert fusion_settings(dict(track_fuse=True, track_motion=True)).static_speed == 0.5
    with pytest.raises(ValueError):
        fusion_settings(dict(track_fuse=True, track_fuse_cap=0))
    assert 'fuse' not in ''.join(tracking_settings(dict(track_fuse=True)))     # the tracker's own settings are untouched
    res = dict(lstq=0.5, s_assoc=0.25, s_cls=1.0, tubes=3, tracks=7, dropped=1)
    assert format_point_lstq(res) == 'point LSTQ 0.5000 S_assoc 0.2500 S_cls 1.0000 (tubes 3, tracks 7, dropped 1)'
    assert format_point_lstq(dict(res, fused=True)).endswith('(tubes 3, tracks 7, dropped 1, fused)')
    assert format_point_lstq(dict(res, gated=4, held=6, fused=True)).endswith('(tubes 3, tracks 7, dropped 1, gated 4, held 6, fused)')


def test_binding_table_header_and_flags():
    from mask_bev_amd import _lib, build, ops
    from mask_bev_amd.predict import Predictions
    header = open(os.path.join(ROOT, 'include', 'maskbev_hip.h')).read()
    for name, n_args in (('mbv_fuse_frames', 25), ('mbv_masks_from_map', 8)):
        assert name in _lib.SIGNATURES and name + '(' in header
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert build.FILE_FLAGS['fuse.hip'] == ['-ffp-contract=off'] and 'fuse.hip' in build.sources()
    for name in ('FusionSettings', 'FusionState', 'FusedFrames', 'fuse_frames', 'masks_from_map'):
        assert hasattr(ops, name)
    assert hasattr(Predictions, 'fused') and 'mask_scores' in Predictions.fused.__doc__


def test_turning_footprint_figures_of_the_documents():
    """The scene behind the nearest-cell figures README, INTEGRATION and DESIGN quote, and the figures themselves — a record of
    the RESTATEMENT (the kernels are held against it elsewhere), so that the documents change when the rule does.  Nothing is
    read out in frame 0 (count 1 < min_count 2); afterwards what is read out on detected cells never exceeds either set."""
    rows = F.turning_footprint()
    assert rows[0] == (32, 0, 0) and len(rows) == 12
    for detected, fused, both in rows[1:]:
        assert 0 < both <= min(detected, fused)
    span = lambda rs, k: (min(r[k] for r in rs[1:]), max(r[k] for r in rs[1:]))
    assert span(rows, 0) == (30, 32) and span(rows, 1) == (29, 32)             # 0.05 rad and 0.5 m a frame
    fast = F.turning_footprint(yaw_step=0.1)
    assert span(fast, 0) == (31, 33) and span(fast, 1) == (29, 34)
    assert all(r == (32, 32, 32) for r in F.turning_footprint(yaw_step=0.0, drive=0.3)[1:])       # a pure translation: exact
