"""``scene_bank.SceneBank`` on the host: what ``build`` keeps, the file round trip, what ``load`` refuses, and the scene of a
scan (indices and matrices).  No GPU."""
import numpy as np
import pytest
import torch

from tests import scene_bank_util as U

N_SCANS = 12


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """Two sequences of 12 scans; scan 5 of sequence 00 has no kept point at all."""
    root = tmp_path_factory.mktemp('kitti')
    rng = np.random.default_rng(7)
    seqs = {}
    for seq, empty in ((0, 5), (3, None)):
        poses, scans, words = U.drive(rng, N_SCANS, [(4.0, 3.0), (-3.0, -4.0)], 3.0, (9.0, 9.0), n_car=90 + 7 * seq,
                                      empty_scan=empty)
        U.write_sequence(root / 'sequences' / f'{seq:02d}', poses, scans, words)
        seqs[seq] = (poses, scans, words)
    return root, seqs


def _paths(root, seq):
    d = root / 'sequences' / f'{seq:02d}'
    scans = sorted((d / 'velodyne').glob('*.bin'))
    return scans, [d / 'labels' / (f.stem + '.label') for f in scans]


def test_build_equals_the_numpy_filter(tree):
    from mask_bev_amd.scene_bank import SceneBank
    root, seqs = tree
    for seq, (_, scans, words) in seqs.items():
        bank = SceneBank.build(*_paths(root, seq))
        want = [U.kept(s, w) for s, w in zip(scans, words)]
        counts = [len(i) for _, i in want]
        assert len(bank) == N_SCANS and bank.classes == (10,)
        assert bank.scan_offsets.dtype == np.int64 and np.array_equal(bank.scan_offsets, np.concatenate([[0], np.cumsum(counts)]))
        assert bank.points.dtype == torch.float32 and bank.inst.dtype == torch.int32
        assert np.array_equal(bank.points.numpy(), np.concatenate([p for p, _ in want]))
        assert np.array_equal(bank.inst.numpy(), np.concatenate([i for _, i in want]))
        assert set(np.unique(bank.inst.numpy())) == {1, 2}             # 7 (moving car), 5 (person) and 0 never
        assert all(0 < c < len(w) for c, w in zip(counts, words) if c)  # the filter drops something in every scan
        if seq == 0:
            assert counts[5] == 0 and len(bank.scan(5)[1]) == 0 and min(counts[:5] + counts[6:]) > 0
        for k in (0, 5, 11):
            p, i = bank.scan(k)
            assert np.array_equal(p.numpy(), want[k][0]) and np.array_equal(i.numpy(), want[k][1])


def test_save_and_load_round_trip(tree, tmp_path, capsys):
    from mask_bev_amd.scene_bank import SceneBank
    root, _ = tree
    bank = SceneBank.build(*_paths(root, 3))
    assert SceneBank.default_path(tmp_path, 3) == tmp_path / 'sequences' / '03' / 'instance_points.npz'
    path = SceneBank.default_path(tmp_path, 3)
    bank.save(path)
    back = SceneBank.load(path, 'cpu', num_scans=N_SCANS)
    assert torch.equal(back.points, bank.points) and torch.equal(back.inst, bank.inst)
    assert np.array_equal(back.scan_offsets, bank.scan_offsets) and back.classes == bank.classes
    assert torch.equal(back.device_offsets, torch.from_numpy(bank.scan_offsets)) and back.device == torch.device('cpu')
    assert f'{bank.points.shape[0] * 16 + (N_SCANS + 1) * 8} bytes' in capsys.readouterr().out    # the real size, printed


def test_load_refuses_another_bank(tree, tmp_path):
    from mask_bev_amd.scene_bank import BUILD_COMMAND, SceneBank
    root, _ = tree
    path = tmp_path / 'bank.npz'
    SceneBank.build(*_paths(root, 0)).save(path)
    with pytest.raises(ValueError, match='classes') as e:
        SceneBank.load(path, 'cpu', classes=(10, 252))
    assert BUILD_COMMAND in str(e.value)
    with pytest.raises(ValueError, match=f'{N_SCANS} scans') as e:
        SceneBank.load(path, 'cpu', num_scans=N_SCANS + 1)
    assert BUILD_COMMAND in str(e.value) and '--build-scene-bank' in BUILD_COMMAND
    with pytest.raises(FileNotFoundError) as e:
        SceneBank.load(tmp_path / 'none.npz', 'cpu')
    assert BUILD_COMMAND in str(e.value)


def test_a_missing_label_file_is_named(tree, tmp_path):
    from mask_bev_amd.scene_bank import SceneBank
    rng = np.random.default_rng(1)
    poses, scans, words = U.drive(rng, 3, [(2.0, 2.0)], 3.0, (9.0, 9.0))
    words[1] = None
    U.write_sequence(tmp_path / 'sequences' / '00', poses, scans, words)
    with pytest.raises(FileNotFoundError, match='000001.label'):
        SceneBank.build(*_paths(tmp_path, 0))


def test_scene_of_a_looping_trajectory():
    """The vehicle drives a circle: the scene around scan 0 holds the scans before AND after it on the loop."""
    from mask_bev_amd.rasterize import scans_in_range
    from mask_bev_amd.scene_bank import SceneBank
    n, radius = 12, 10.0
    velo = np.stack([U.pose_2d(radius * np.cos(2 * np.pi * k / n), radius * np.sin(2 * np.pi * k / n), 2 * np.pi * k / n + np.pi / 2)
                     for k in range(n)])
    cam = np.stack([U.TR @ p @ np.linalg.inv(U.TR) for p in velo])
    x_range, y_range = (-4.0, 4.0), (-3.5, 3.5)
    for centre in (0, 6, 11):
        index, tf = SceneBank.scene(centre, cam, U.TR, x_range, y_range)
        assert np.array_equal(index, scans_in_range(cam, centre, x_range, y_range, velo_to_cam=U.TR))
        assert centre in index and 1 < len(index) < n
        assert tf.dtype == np.float64 and tf.shape == (len(index), 4, 4)
        assert np.abs(tf - np.linalg.inv(velo[centre]) @ velo[index]).max() <= 1e-12
        if centre in (0, 11):                                   # not a contiguous range: a slice of the bank would not do
            assert np.any(np.diff(index) > 1), index
    index, _ = SceneBank.scene(0, cam, U.TR, x_range, y_range)
    assert index.tolist() == [0, 1, 11]
    # velodyne poses passed as they are give the same scene
    index_v, tf_v = SceneBank.scene(0, velo, None, x_range, y_range)
    assert np.array_equal(index_v, index) and np.abs(tf_v - np.linalg.inv(velo[0]) @ velo[index]).max() <= 1e-12
