"""numpy restatement of K23 (csrc/augment.hip), written from the reference's transform classes
(mask_bev/augmentations/semantic_kitti_mask_augmentations.py:44-161) and the text of include/maskbev_hip.h — the hash, the
uniform / normal / drop rules, the op program in f64 with an f32 store after each op, the permutation as a stable argsort of
the restated keys, the warp rule.  The normal is taken in f64 here: the GPU tests allow for the kernel's f32 logf / sqrtf /
cosf in their tolerance."""
import numpy as np

OP_LINEAR, OP_JITTER, OP_DROP, OP_SHUFFLE, OP_DECIMATE = 1, 2, 3, 4, 5
ORDER_SLOT = 8


def pcg(v):
    v = np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF
    s = (v * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & 0xFFFFFFFF
    return ((w >> 22) ^ w) & 0xFFFFFFFF


def stream(seed, slot):
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    return int(pcg(lo ^ int(pcg((hi + slot * 0x9E3779B9) & 0xFFFFFFFF))))


def draw(seed, slot, idx, comp, j):
    idx = np.asarray(idx, dtype=np.uint64)
    return pcg((stream(seed, slot) + (idx * 8 + comp * 2 + j)) & 0xFFFFFFFF)


def normal(seed, slot, idx, comp):
    u1 = ((draw(seed, slot, idx, comp, 0) >> 8) + 1).astype(np.float64) * 2.0 ** -24
    u2 = (draw(seed, slot, idx, comp, 1) >> 8).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def run_program(pc, seed, ops):
    """One scan (n, dim) f32 through its op list → (values (n, dim) f32 of every input point, kept (n) bool)."""
    pc = np.array(pc, dtype=np.float32, copy=True)
    n, dim = pc.shape
    idx = np.arange(n)
    keep = np.ones(n, dtype=bool)
    for slot, (code, arg, p) in enumerate(ops):
        if code == OP_LINEAR:
            x, y = pc[:, 0].astype(np.float64), pc[:, 1].astype(np.float64)
            pc[:, 0] = (p[0] * x + p[1] * y).astype(np.float32)
            pc[:, 1] = (p[2] * x + p[3] * y).astype(np.float32)
        elif code == OP_JITTER:
            for c in range(dim):
                d = np.clip(p[1 + c] * normal(seed, slot, idx, c), -p[5 + c], p[5 + c])
                pc[:, c] = (pc[:, c].astype(np.float64) + p[0] * d).astype(np.float32)
            if dim == 4:
                np.clip(pc[:, 3], 0, 1, pc[:, 3])
        elif code == OP_DROP:
            keep &= (draw(seed, slot, idx, 0, 0) >> 8) >= arg
    return pc, keep


def augment_batch(scans, draws):
    """scans: list of (n, dim) f32; draws: list of (seed, ops) with ops = [(code, arg, p), ...] → list of output scans.
    A scan with a shuffle or decimate is ordered by the stable argsort of its order keys; a decimate keeps the first
    ceil(m / k) of the ordered survivors, once per decimate op."""
    out = []
    for pc, (seed, ops) in zip(scans, draws):
        vals, keep = run_program(pc, seed, ops)
        idx = np.flatnonzero(keep)
        if any(code in (OP_SHUFFLE, OP_DECIMATE) for code, _, _ in ops):
            keys = draw(seed, ORDER_SLOT, idx, 0, 0) >> 6
            idx = idx[np.argsort(keys, kind='stable')]
        m = len(idx)
        for code, arg, _ in ops:
            if code == OP_DECIMATE and arg > 1:
                m = -(-m // arg)
        out.append(vals[idx[:m]])
    return out


def warp(m, a, cx, cy):
    """(nx, ny) map under the 2 x 2 matrix ``a`` (original → augmented): the rule of mbv_warp_instance_maps.  Also returns
    the f64 source coordinates (for the distance-to-an-integer check of the GPU test)."""
    nx, ny = m.shape
    ix, iy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing='ij')
    du, dv = (ix + 0.5) - cx, (iy + 0.5) - cy
    su = (a[0, 0] * du + a[1, 0] * dv) + cx
    sv = (a[0, 1] * du + a[1, 1] * dv) + cy
    fu, fv = np.floor(su), np.floor(sv)
    ok = (fu >= 0) & (fu < nx) & (fv >= 0) & (fv < ny)
    out = np.zeros_like(m)
    out[ok] = m[fu[ok].astype(np.int64), fv[ok].astype(np.int64)]
    return out, su, sv


def rotation(theta_deg):
    c, s = np.cos(np.deg2rad(theta_deg)), np.sin(np.deg2rad(theta_deg))
    return np.array([[c, -s], [s, c]])
