"""What K39's GPU tests share (tests/test_k39_fuse_gpu.py): one caller of mbv_fuse_frames into poisoned memory and the walk of a
scene through the kernel and the restatement (tests/fuse_ref.py) side by side."""
import numpy as np
import torch

from tests import fuse_ref as F

POISON = 0x5a5a5a5a


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def call(lib, device, state, frames, x_lo, y_lo, voxel, cap, hit, miss, min_count, static_speed=0.0, queries=True, s=None, q_num=None,
         always=False):
    """mbv_fuse_frames on the F frame dicts (imap, qt, m, n, vis, vel; vis / vel of the first frame decide whether the call
    gets them) into poisoned outputs; `state` (host dict) is stepped.  A state that has seen no frame goes in with garbage in
    owner, count, the window's corner and its reserved word (an invalid frame must leave a later state as it is).  `always`: the
    device's state comes back whatever the return code is.  → (rc, fused_ids, fused_queries or None)"""
    from mask_bev_amd.ops_core import _ptr, _stream
    maps = np.stack([np.asarray(fr['imap'], np.int32) for fr in frames])
    f, h, w = maps.shape
    qt = np.stack([np.asarray(fr['qt'], np.int32) for fr in frames])
    q_num = qt.shape[1] if q_num is None else q_num
    host = F.copy_state(state)
    if int(host['window'][2]) == 0:
        host['owner'][:], host['count'][:], host['window'][:2], host['window'][3] = POISON, -POISON, (1 << 50) + 12345, POISON
    on_device = {k: dev(v, device) for k, v in host.items()}
    d_maps, d_qt = dev(maps, device), dev(qt, device)
    d_m = dev(np.stack([np.asarray(fr['m'], np.float64) for fr in frames]), device)
    d_n = dev(np.stack([np.asarray(fr['n'], np.float64) for fr in frames]), device)
    d_vis = dev(np.stack([fr['vis'] for fr in frames]).astype(np.uint8), device) if frames[0].get('vis') is not None else None
    d_vel = dev(np.stack([fr['vel'] for fr in frames]).astype(np.float64), device) if frames[0].get('vel') is not None else None
    ids = torch.full((f, h, w), POISON, dtype=torch.int32, device=device)
    qs = torch.full((f, h, w), POISON, dtype=torch.int32, device=device) if queries else None
    rc = lib.mbv_fuse_frames(_ptr(d_maps), _ptr(d_qt), _ptr(d_m), _ptr(d_n), _ptr(d_vis), _ptr(d_vel), f, h, w,
                             host['owner'].shape[0] if s is None else s, x_lo, y_lo, voxel, q_num, cap, hit, miss, min_count,
                             static_speed, _ptr(on_device['owner']), _ptr(on_device['count']), _ptr(on_device['window']), _ptr(ids),
                             _ptr(qs), _stream())
    torch.cuda.synchronize()
    if rc == 0 or always:
        for k, t in on_device.items():
            state[k] = t.cpu().numpy()
    return rc, ids.cpu().numpy(), qs.cpu().numpy() if queries else None


def same_state(a, b):
    assert set(a) == set(b)
    for k in b:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (k, a[k], b[k])


def gpu_runner(lib, device, queries=True):
    """A `runner` of tests/fuse_ref.py's scenarios on the kernel, frame by frame (F = 1); after every frame all outputs and
    every state element equal the restatement's."""
    def runner(frames, h, w, x_lo, y_lo, v, cap, hit, miss, min_count, static_speed=0.0):
        got, ref, outs, states = F.fresh_state(h, w), F.fresh_state(h, w), [], []
        for k, fr in enumerate(frames):
            rc, ids, qs = call(lib, device, got, [fr], x_lo, y_lo, v, cap, hit, miss, min_count, static_speed, queries=queries)
            (rids, rqs), = F.run(ref, [fr], x_lo, y_lo, v, cap, hit, miss, min_count, static_speed)
            assert rc == 0
            assert ids.dtype == np.int32 and np.array_equal(ids[0], rids), k
            assert not queries or np.array_equal(qs[0], rqs), k
            same_state(got, ref)
            outs.append((ids[0], qs[0] if queries else rqs))
            states.append(F.copy_state(got))
        return outs, states
    return runner
