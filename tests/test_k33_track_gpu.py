"""K33 (the tracker step and tube association, csrc/track.hip) through the C ABI, and what is built on it:
``ops.track_frames`` / ``tube_accumulate`` / ``tube_scores``, ``tracking.InstanceTracker``, ``Predictions.track`` /
``point_tracks`` and ``metrics.DeviceTubeAssociation``.

After every frame EVERY output and every element of the state equals the numpy restatement (tests/track_ref.py) as exact
integers, into outputs, state tails and a workspace filled with garbage; two runs are bit-equal; the tube tables equal the
restatement and the f64 scores agree with exact fractions to 1e-12 relative (the fixed-order sum of at most 1024 terms of a
few correctly rounded operations each: about 1e-13)."""
import numpy as np
import pytest
import torch

from tests import track_ref as R
from tests.track_util import call, dev, same_state, walk
from tests.util_cfg import random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3


def test_k33_scripted_and_constructed_scenes(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    pr = R.SCRIPT_PARAMS
    end, _ = walk(lib, device, R.scripted_scene(), R.H0, R.W0, R.X_LO0, R.Y_LO0, R.VOXEL0, pr['q_num'], pr['p'], pr['min_iou'],
                  pr['max_age'], pr['min_cells'], entry='plain')
    assert end['counters'].tolist() == [4, 7, 6, 2]                    # by the restatement: 7 ids, 2 drops by capacity
    for frames, pr in R.constructed_cases().values():
        walk(lib, device, frames, 6, 8, 0.0, 0.0, 1.0, pr['q_num'], pr['p'], pr['min_iou'], pr['max_age'], pr['min_cells'], entry='plain')


@pytest.mark.parametrize('qp', [(8, 8), (4, 4)])
@pytest.mark.parametrize('hw', [(40, 48), (33, 65)])
def test_k33_random_scenes(device, hw, qp):
    from mask_bev_amd import _lib
    lib = _lib.load()
    for seed in range(3):
        frames, x_lo, y_lo = R.random_scene(100 * hw[0] + 10 * qp[0] + seed, hw[0], hw[1], qp[0], frames=5)
        end, _ = walk(lib, device, frames, hw[0], hw[1], x_lo, y_lo, 0.5, qp[0], qp[1], 0.3, 1, 4, entry='plain')
        assert end['counters'][1] >= 2 and end['counters'][2] == 5


def test_k33_table_limits(device):
    """Q = 300, P = 1024 on 64 x 64: scattered cells, so that thousands of pairs tie; three frames under a shift of a cell."""
    from mask_bev_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(33)
    frames = []
    for k in range(3):
        im = rng.integers(-1, 300, (64, 64)).astype(np.int32)
        im[8 * k:8 * k + 20, 10:30] = 7 + k                            # and one solid object that moves with the shift
        frames.append((im, np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.0]]) if k else R.IDENTITY))
    end, _ = walk(lib, device, frames, 64, 64, -16.0, -16.0, 0.5, 300, 1024, 0.05, 2, 4, entry='plain')
    assert end['counters'][0] > 300 and end['counters'][1] > 400


def test_k33_degenerate_frames(device):
    from mask_bev_amd import _lib
    lib = _lib.load()
    h, w, q, p = 40, 48, 8, 8
    scene, x_lo, y_lo = R.random_scene(5, h, w, q, frames=3)
    args = (h, w, x_lo, y_lo, 0.5, q, p, 0.3, 2, 4)
    empty = np.full((h, w), -1, np.int32)
    # the first frame of a fresh tracker under a transform that means nothing yet; then an empty map; then the scene again
    far = np.array([[1.0, 0.0, 1e6], [0.0, 1.0, -1e6]])
    nan = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]])
    mid, _ = walk(lib, device, [(scene[0][0], far), (empty, R.IDENTITY), scene[1]], *args, entry='plain')
    assert mid['counters'][0] > 0
    # everything mapped off the grid, and a NaN / inf transform: no match, all births, the old tracks coast
    walk(lib, device, [(scene[2][0], far)], *args, start=mid, entry='plain')
    walk(lib, device, [(scene[2][0], nan)], *args, start=mid, entry='plain')
    # values out of range in the instance map and in a corrupted state: results change, addresses never
    bad_map = scene[2][0].copy()
    bad_map[::5, ::3] = q
    bad_map[1::7, ::4] = 2 ** 30
    bad_map[2::7, 1::4] = -5
    broken = R.copy_state(mid)
    broken['state_map'][::4, ::5] = p
    broken['state_map'][1::4, ::5] = 2 ** 30
    broken['state_map'][2::4, ::5] = -9
    broken['state_map'][3::4, ::5] = int(mid['counters'][0])          # just past n_live
    walk(lib, device, [(bad_map, scene[2][1])], *args, start=broken, entry='plain')
    for n_live in (-3, p + 5):                                         # a stored n_live outside [0, P] is clamped
        odd = R.copy_state(mid)
        odd['counters'][0] = n_live
        odd['live_id'][:], odd['live_seen'][:] = np.arange(p) + 50, 1
        got, ref = R.copy_state(odd), R.copy_state(odd)
        rc, qt, tm = call(lib, device, got, scene[2][0][None], scene[2][1][None], *args[2:5], q, 0.3, 2, 4, entry='plain')
        rqt, rtm = R.step(ref, scene[2][0], scene[2][1], *args[2:5], q, 0.3, 2, 4)
        assert rc == 0 and np.array_equal(qt[0], rqt) and np.array_equal(tm[0], rtm)
        for k in ('state_map', 'counters'):
            assert np.array_equal(got[k], ref[k])
        n = int(ref['counters'][0])
        assert np.array_equal(got['live_id'][:n], ref['live_id'][:n]) and np.array_equal(got['live_seen'][:n], ref['live_seen'][:n])


def test_k33_frames_in_one_call_and_twice(device):
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    h, w, q, p = 33, 65, 8, 8
    scene, x_lo, y_lo = R.random_scene(9, h, w, q, frames=3)
    maps, ms = np.stack([f[0] for f in scene]), np.stack([f[1] for f in scene])
    one = R.fresh_state(h, w, p)
    rc, qt, tm = call(lib, device, one, maps, ms, x_lo, y_lo, 0.5, q, 0.3, 2, 4, entry='plain')
    assert rc == 0
    three, parts = R.fresh_state(h, w, p), []
    for k in range(3):
        rc, a, b = call(lib, device, three, maps[k:k + 1], ms[k:k + 1], x_lo, y_lo, 0.5, q, 0.3, 2, 4, entry='plain')
        assert rc == 0
        parts.append((a[0], b[0]))
    same_state(one, three)
    assert all(np.array_equal(qt[k], parts[k][0]) and np.array_equal(tm[k], parts[k][1]) for k in range(3))
    again = R.fresh_state(h, w, p)
    rc, qt2, tm2 = call(lib, device, again, maps, ms, x_lo, y_lo, 0.5, q, 0.3, 2, 4, entry='plain')
    assert rc == 0 and qt.tobytes() == qt2.tobytes() and tm.tobytes() == tm2.tobytes()
    assert all(one[k].tobytes() == again[k].tobytes() for k in one)
    # without a track map, and the wrapper with the tracker on top: the same ids
    none = R.fresh_state(h, w, p)
    rc, qt3, _ = call(lib, device, none, maps, ms, x_lo, y_lo, 0.5, q, 0.3, 2, 4, track_map=False, entry='plain')
    assert rc == 0 and np.array_equal(qt, qt3)
    same_state(one, none)
    from mask_bev_amd.tracking import InstanceTracker
    tracker = InstanceTracker((x_lo, x_lo + w * 0.5), (y_lo, y_lo + h * 0.5), 0.5, q, max_tracks=p, device=device)
    ids = tracker.update(dev(maps[:2], device), prev_from_cur=ms[:2])
    rec = tracker.update(dev(maps[2:], device), prev_from_cur=dev(ms[2:], device), track_map=True)
    assert np.array_equal(ids.cpu().numpy(), qt[:2]) and np.array_equal(rec.query_track.cpu().numpy(), qt[2:])
    assert np.array_equal(rec.track_map.cpu().numpy(), tm[2:])
    c = tracker.counters()
    assert [c['live'], c['tracks'], c['frames'], c['dropped']] == one['counters'].tolist()
    tracker.reset()
    assert tracker.counters() == dict(live=0, tracks=0, frames=0, dropped=0)
    with pytest.raises(ops.MaskBevHipError):
        ops.track_frames(torch.from_numpy(maps), torch.from_numpy(ms), ops.TrackState.fresh(h, w, p, 'cpu'), x_lo, y_lo, 0.5, q)


def test_k33_error_codes(device):
    from mask_bev_amd import _lib
    from mask_bev_amd.ops_core import _ptr, _stream
    lib = _lib.load()
    h, w, q, p = 8, 8, 4, 4
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)
    maps, ms = i32(1, h, w), torch.zeros((1, 2, 3), dtype=torch.float64, device=device)
    sm, lid, seen, cnt, qt = i32(h, w), i32(p), i32(p), i32(4), i32(1, q)
    ws = torch.zeros((lib.mbv_track_frames_workspace_bytes(h, w, q, p),), dtype=torch.uint8, device=device)

    def call(f=1, hh=h, ww=w, qq=q, pp=p, age=2, cells=4, maps=maps, cnt=cnt, ws_bytes=None, ws=ws):
        return lib.mbv_track_frames(_ptr(maps), _ptr(ms), f, hh, ww, 0.0, 0.0, 1.0, qq, pp, 0.3, age, cells, _ptr(sm), _ptr(lid),
                                    _ptr(seen), _ptr(cnt), _ptr(qt), None, _ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                    _stream())

    assert call() == 0
    assert lib.mbv_track_frames(None, None, 0, h, w, 0.0, 0.0, 1.0, q, p, 0.3, 2, 4, None, None, None, None, None, None, None, 0,
                                _stream()) == 0
    assert call(qq=5) == UNSUPPORTED and call(pp=1025, qq=4) == UNSUPPORTED and call(hh=1025, ww=1024) == UNSUPPORTED
    assert call(cells=0) == BAD_ARG and call(age=-1) == BAD_ARG and call(f=-1) == BAD_ARG and call(hh=-1) == BAD_ARG
    assert call(maps=None) == BAD_ARG and call(cnt=None) == BAD_ARG
    assert call(ws_bytes=ws.numel() - 1) == WORKSPACE and call(ws=None, ws_bytes=1 << 30) == WORKSPACE
    assert lib.mbv_track_frames_workspace_bytes(h, w, 5, 4) == 0 and lib.mbv_track_frames_workspace_bytes(1024, 1024, 300, 1024) > 0
    torch.cuda.synchronize()
    # K33b
    lut = i32(4)
    big = lambda n: torch.zeros((n,), dtype=torch.int64, device=device)
    tube = lambda total=8, c=2, i=4, t=4, pred=i32(8): lib.mbv_tube_accumulate(
        _ptr(pred), _ptr(i32(8)), total, _ptr(lut), 4, c, i, t, _ptr(big(16)), _ptr(big(8)), _ptr(i32(64)), _ptr(big(2)), _stream())
    assert tube() == 0 and tube(total=0, pred=None) == 0
    assert tube(c=17) == UNSUPPORTED and tube(i=65537) == UNSUPPORTED and tube(c=16, i=65536, t=4096) == UNSUPPORTED
    assert tube(c=0) == BAD_ARG and tube(i=0) == BAD_ARG and tube(t=0) == BAD_ARG and tube(total=-1) == BAD_ARG
    assert tube(pred=None) == BAD_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize('cit', [(3, 8, 6), (2, 1024, 4096), (2, 4097, 4097)])
def test_k33_tube_tables_and_scores(device, cit):
    """Three batches into the running tables: the tables equal the restatement, the overflow counters included; the scores
    agree with exact fractions to 1e-12 relative.  (2, 1024, 4096): both size tables in LDS; (2, 4097, 4097): neither."""
    from mask_bev_amd import ops
    from mask_bev_amd.metrics import DeviceTubeAssociation
    c, i, t = cit
    ref = R.fresh_tables(c, i, t)
    tables = ops.TubeTables.zeros(c, i, t, device)
    everything = [R.random_elements(seed, n, c, i, t) for seed, n in ((1, 5000), (2, 1), (3, 70001))]
    lut = everything[0][2]
    for pred, words, _ in everything:
        R.tube_accumulate(ref, pred, words, lut, c, i, t)
        ops.tube_accumulate(dev(pred, device), dev(words.view(np.int32), device), dev(lut, device), tables)
    for k in ('gt_size', 'pred_size', 'pair', 'overflow'):
        got = getattr(tables, k).cpu().numpy()
        assert got.dtype == ref[k].dtype and np.array_equal(got, ref[k]), k
    assert ref['overflow'].min() > 0 and (ref['pair'] > 0).sum() > 20
    scores = ops.tube_scores(tables)
    again = ops.tube_scores(tables)
    assoc, class_assoc, class_tubes = (x.cpu().numpy() for x in (scores.assoc, scores.class_assoc, scores.class_tubes))
    assert assoc.tobytes() == again.assoc.cpu().numpy().tobytes()
    exact, over = R.plain_tube(np.concatenate([e[0] for e in everything]), np.concatenate([e[1] for e in everything]), lut, c, i, t)
    assert over == ref['overflow'].tolist() and set(exact) == set(np.nonzero(ref['gt_size'])[0].tolist())
    for r in range(assoc.shape[0]):
        want = float(exact.get(r, 0))
        assert abs(assoc[r] - want) <= 1e-12 * want, (r, assoc[r], want)
    rassoc, rclass, rtubes = R.tube_scores(ref, c, i)
    assert np.array_equal(class_tubes, rtubes) and class_tubes.dtype == np.int32
    for k in range(c):
        want = float(sum((v for r, v in exact.items() if r // i == k - 1), 0))
        assert abs(class_assoc[k] - want) <= 1e-12 * want, (k, class_assoc[k], want)
    # the metric: it raises on the overflow, and gives the mean over the tubes without one
    metric = DeviceTubeAssociation(c, lut, id_limit=i, max_tracks=t, tables=tables)
    with pytest.raises(ops.MaskBevHipError):
        metric.compute()
    tables.overflow.zero_()
    res = metric.compute()
    want = float(sum(exact.values(), 0) / len(exact))
    assert res['tubes'] == len(exact) and abs(res['s_assoc'] - want) <= 1e-12 * want and res['overflow'] == [0, 0]
    with pytest.raises(ops.MaskBevHipError):
        ops.tube_accumulate(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), dev(lut, device), tables)


def test_k33_predict_track_lift_and_tubes(device):
    """A tiny random-weight model: predict → Predictions.track → lift → point_tracks → DeviceTubeAssociation equals the
    restatements applied to the copied-back instance map and point queries."""
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.metrics import DeviceTubeAssociation
    from mask_bev_amd.tracking import InstanceTracker, prev_from_cur_2d
    torch.manual_seed(0)
    kw = dict(tiny_kwargs(nx=96, ny=96, q=8), compute_dtype='fp32')
    model = MaskBevModule(**kw).to(device).train()
    model.log_scalars = False
    scans = [x.to(device) for x in random_scans(kw, [3000, 2400, 2600], seed=4)]
    pred = model.predict(scans)
    x_lo, y_lo, voxel = float(kw['x_range'][0]), float(kw['y_range'][0]), float(kw['voxel_size'])
    tracker = InstanceTracker(kw['x_range'], kw['y_range'], voxel, 8, max_tracks=16, min_cells=2, device=device)
    assert (tracker.h, tracker.w) == (96, 96)
    poses = np.stack([R.pose_2d(0.4 * k, 0.1 * k, 0.02 * k) for k in range(3)])
    qt = pred.track(tracker, poses=poses)
    lifted = pred.lift(scans, model)
    ids = pred.point_tracks(lifted, qt)
    # the restatement on the copied-back maps
    ref = R.fresh_state(96, 96, 16)
    maps = pred.instance_map.cpu().numpy()
    want = []
    for k in range(3):
        m = R.IDENTITY if k == 0 else prev_from_cur_2d(poses[k - 1], poses[k])
        want.append(R.step(ref, maps[k], m, x_lo, y_lo, voxel, 8, 0.3, 2, 2)[0])
    want = np.stack(want)
    assert np.array_equal(qt.cpu().numpy(), want)
    assert np.array_equal(tracker.state.counters.cpu().numpy(), ref['counters'])
    pq = lifted.point_query.cpu().numpy()
    scan = np.repeat(np.arange(3), lifted.lengths)
    want_ids = np.where(pq >= 0, want[scan, np.maximum(pq, 0)], -1).astype(np.int32)
    got_ids = ids.cpu().numpy()
    assert got_ids.dtype == np.int32 and np.array_equal(got_ids, want_ids)
    assert (want >= 0).sum() >= 2 and (want_ids >= 0).any(), 'no query is tracked onto a point: the test needs another seed'
    # ground truth: the predicted ids themselves, shifted by one and with every third point ignored: S_assoc from the tables
    words = np.where(want_ids >= 0, ((want_ids.astype(np.int64) % 5 + 1) << 16) | 10, 40).astype(np.uint32)
    words[::3] = 0
    lut = np.zeros(64, np.int32)
    lut[10], lut[0] = 1, -1
    metric = DeviceTubeAssociation(2, lut, id_limit=8, max_tracks=64)
    metric.update(ids, dev(words.view(np.int32), device))
    res = metric.compute()
    exact, over = R.plain_tube(want_ids, words, lut, 2, 8, 64)
    assert over == [0, 0] and res['tubes'] == len(exact)
    if exact:
        want_s = float(sum(exact.values(), 0) / len(exact))
        assert abs(res['s_assoc'] - want_s) <= 1e-12 * want_s


def test_launcher_tracks_sequences(device, tmp_path, capsys):
    """``track_instances: true`` on ``--test``: without poses.txt / calib.txt one line and no LSTQ; with them and label files
    one ``point LSTQ`` line, and ``--write-labels`` writes track ids that the restatement gives on the same predictions."""
    import re
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.tracking import velodyne_poses
    kw = tiny_kwargs()
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    seq = tmp_path / 'data' / 'sequences' / '08'
    (seq / 'velodyne').mkdir(parents=True)
    (seq / 'mask_cache').mkdir()
    (seq / 'labels').mkdir()
    scans = random_scans(kw, [1500, 1201, 900, 700], seed=3)
    for i, s in enumerate(scans):
        s.numpy().tofile(seq / 'velodyne' / f'{i:06d}.bin')
        imap = np.zeros((80, 80), dtype=np.int32)
        imap[10:22, 10:19], imap[40:52, 30:39] = 1, 2
        np.save(seq / 'mask_cache' / f'{i:06d}.npy', imap)
        words = np.full(s.shape[0], (3 << 16) | 10, np.uint32)            # one car tube over everything
        words[::4] = 40
        words.astype('<u4').tofile(seq / 'labels' / f'{i:06d}.label')
    cfg = dict(kw, dataset='semantic-kitti', batch_size=2, val_sequences=[8], train_sequences=[8], panoptic_min_points=1,
               track_instances=True, track_min_cells=2, track_max_tracks=32)
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}
    ck = tmp_path / 'ckpt' / 'tiny'
    ck.mkdir(parents=True)
    path = ck / 'tiny-epoch=00-val_loss=1.000000.ckpt'
    launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'], path, 0, 'val_loss', 1.0)
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(cfg))
    out_dir = tmp_path / 'out'
    argv = ['--config', str(tmp_path / 'tiny.yml'), '--test', '--data-root', str(tmp_path / 'data'), '--checkpoint-root',
            str(tmp_path / 'ckpt'), '--write-labels', str(out_dir)]
    assert launcher.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len([l for l in lines if l.startswith('track_instances: skipped')]) == 1
    assert not [l for l in lines if l.startswith('point LSTQ')] and [l for l in lines if l.startswith('point PQ')]
    plain = [np.fromfile(str(out_dir / 'sequences' / '08' / 'predictions' / f'{i:06d}.label'), '<u4') for i in range(4)]
    # the sequence's poses (camera frame) and calibration
    tr = np.array([[0.0, -1.0, 0.0, 0.1], [0.0, 0.0, -1.0, -0.2], [1.0, 0.0, 0.0, 0.3], [0.0, 0.0, 0.0, 1.0]])
    velo = [R.pose_2d(0.3 * k, 0.05 * k, 0.01 * k) for k in range(4)]
    cam = [tr @ p @ np.linalg.inv(tr) for p in velo]
    np.savetxt(seq / 'poses.txt', np.stack([p[:3].reshape(-1) for p in cam]))
    (seq / 'calib.txt').write_text('P0: ' + ' '.join(['0'] * 12) + '\nTr: ' + ' '.join(repr(float(v)) for v in tr[:3].reshape(-1)) + '\n')
    assert launcher.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    got = [re.fullmatch(r'point LSTQ (\S+) S_assoc (\S+) S_cls (\S+) \(tubes (\d+), tracks (\d+), dropped (\d+)\)', l)
           for l in lines if l.startswith('point LSTQ')]
    assert len(got) == 1 and got[0], lines
    pq_at = [i for i, l in enumerate(lines) if l.startswith('point PQ')]
    assert len(pq_at) == 1 and lines[pq_at[0] + 1].startswith('point LSTQ')
    # one sequence, one rank: both passes see the same batches, so this rank's IoU alone is the IoU summed over the ranks
    assert got[0].group(3) == re.search(r' IoU (\S+) ', lines[pq_at[0]]).group(1)
    assert any(l.startswith('wrote 4 label files with track ids') for l in lines)
    # the restatement on the predictions of the model as the launcher loads it
    loaded = MaskBevModule.from_config(dict(cfg, checkpoint=str(path))).to(device)
    loaded.log_scalars = False
    loaded.flatten_parameters()
    from mask_bev_amd.batch import read_calib, read_poses
    poses = velodyne_poses(read_poses(seq / 'poses.txt'), read_calib(seq / 'calib.txt'))
    assert np.allclose(poses, np.stack(velo), rtol=0, atol=1e-9)
    ref, ids, all_words = R.fresh_state(80, 80, 32), [], []
    for start in (0, 2):
        part = [s.to(device) for s in scans[start:start + 2]]
        pred = loaded.predict(part)
        per = [p.cpu().numpy() for p in pred.lift(part, loaded).per_scan()]
        maps = pred.instance_map.cpu().numpy()
        for k in range(2):
            i = start + k
            m = R.IDENTITY if i == 0 else R.prev_from_cur(poses[i - 1], poses[i])
            qt = R.step(ref, maps[k], m, kw['x_range'][0], kw['y_range'][0], kw['voxel_size'], kw['num_queries'], 0.3, 2, 2)[0]
            ids.append(np.where(per[k] >= 0, qt[np.maximum(per[k], 0)], -1))
            all_words.append(np.fromfile(str(seq / 'labels' / f'{i:06d}.label'), '<u4'))
    for i in range(4):
        written = np.fromfile(str(out_dir / 'sequences' / '08' / 'predictions' / f'{i:06d}.label'), '<u4')
        assert np.array_equal(written, np.where(ids[i] >= 0, ((ids[i] + 1) << 16) | 10, 0).astype(np.uint32))
        assert not np.any((written != 0) & (plain[i] == 0))               # a tracked point is a labelled point
    assert int(got[0].group(5)) == int(ref['counters'][1]) > 0 and int(got[0].group(6)) == int(ref['counters'][3])
    from mask_bev_amd.metrics import semantic_kitti_class_lut
    exact, over = R.plain_tube(np.concatenate(ids), np.concatenate(all_words), semantic_kitti_class_lut(), 2, 1024, 4096)
    assert over == [0, 0] and int(got[0].group(4)) == len(exact) == 1
    assert abs(float(got[0].group(2)) - float(sum(exact.values()) / len(exact))) <= 5.1e-5      # four printed decimals
    s_assoc, s_cls = float(got[0].group(2)), float(got[0].group(3))
    assert abs(float(got[0].group(1)) - np.sqrt(s_assoc * s_cls)) <= 1e-3
