"""Synthetic SemanticKITTI sequences for the scene-bank tests (tests/test_scene_bank_cpu.py, tests/test_k34_rasterize_bank_gpu.py):
static "cars" (squares of random points) in a world frame, an ego vehicle that drives past them, every scan in its own frame,
label words as the dataset stores them, ``poses.txt`` in the camera frame and ``calib.txt``."""
import numpy as np

TR = np.array([[0.0, -1.0, 0.0, 0.1], [0.0, 0.0, -1.0, -0.2], [1.0, 0.0, 0.0, 0.3], [0.0, 0.0, 0.0, 1.0]])     # velo_to_cam


def pose_2d(x, y, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    m = np.eye(4)
    m[:2, :2] = [[c, -s], [s, c]]
    m[0, 3], m[1, 3] = x, y
    return m


def into_frame(xyz, pose):
    """World points (n, 3) f64 seen from the frame whose pose (frame → world) is ``pose`` → (n, 3) f32."""
    inv = np.linalg.inv(pose)
    return (np.asarray(xyz, dtype=np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)


def square(rng, centre, side, n, z=-1.0):
    p = np.empty((n, 3))
    p[:, :2] = np.asarray(centre, dtype=np.float64) + (rng.random((n, 2)) - 0.5) * side
    p[:, 2] = z + 0.3 * rng.random(n)
    return p


def drive(rng, n_scans, cars, side, half, n_car=100, n_other=100, step=(0.3, 0.05, 0.01), empty_scan=None):
    """→ (velodyne poses (S, 4, 4), scans [(n, 4) f32], words [(n) u32]).  ``cars``: world centres, ids 1, 2, ...; every scan sees
    ``n_car`` points of every car as ``id << 16 | 10`` and ``n_other`` more inside ±``half``, a quarter each of a moving car
    ``7 << 16 | 252``, a person ``5 << 16 | 30``, a car without an instance ``0 << 16 | 10`` and road ``40``.  The points are
    shuffled, so the kept ones are not a prefix.  In scan ``empty_scan`` the car points are road: it has no kept point."""
    poses = np.stack([pose_2d(step[0] * k, step[1] * k, step[2] * k) for k in range(n_scans)])
    scans, words = [], []
    for k in range(n_scans):
        xyz = [square(rng, c, side, n_car) for c in cars]
        w = [np.full(n_car, ((i + 1) << 16) | 10, np.uint32) for i in range(len(cars))]
        if k == empty_scan:
            w = [np.full(n_car, 40, np.uint32) for _ in cars]
        other = np.empty((n_other, 3))
        other[:, :2] = (rng.random((n_other, 2)) * 2 - 1) * np.asarray(half, dtype=np.float64)
        other[:, 2] = -1.0
        xyz.append(other)
        w.append(np.resize(np.array([(7 << 16) | 252, (5 << 16) | 30, (0 << 16) | 10, 40], np.uint32), n_other))
        xyz, w = np.concatenate(xyz), np.concatenate(w)
        order = rng.permutation(len(w))
        scan = np.zeros((len(w), 4), np.float32)
        scan[:, :3] = into_frame(xyz[order], poses[k])
        scan[:, 3] = rng.random(len(w))
        scans.append(scan)
        words.append(w[order])
    return poses, scans, words


def write_sequence(folder, velo_poses, scans, words):
    """The sequence as downloaded; ``words[k] is None`` leaves scan k without a label file."""
    (folder / 'velodyne').mkdir(parents=True)
    (folder / 'labels').mkdir()
    for k, (scan, w) in enumerate(zip(scans, words)):
        scan.astype('<f4').tofile(folder / 'velodyne' / f'{k:06d}.bin')
        if w is not None:
            w.astype('<u4').tofile(folder / 'labels' / f'{k:06d}.label')
    cam = [TR @ p @ np.linalg.inv(TR) for p in velo_poses]
    np.savetxt(folder / 'poses.txt', np.stack([p[:3].reshape(-1) for p in cam]))
    (folder / 'calib.txt').write_text('P0: ' + ' '.join(['0'] * 12) + '\nTr: ' + ' '.join(repr(float(v)) for v in TR[:3].reshape(-1)) + '\n')


def kept(scan, w):
    """The three-line filter a bank is checked against: static car (raw id 10) with an instance id."""
    sem, inst = w & 0xFFFF, w >> 16
    keep = (sem == 10) & (inst != 0)
    return scan[keep, :3], inst[keep].astype(np.int32)
