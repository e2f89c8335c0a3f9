"""The dense zero-padded PillarFeatureNet in plain torch on the CPU, any dtype: the reference of the K2 float64 suite
(test_k2_paths_gpu.py), pinned to the project's oracle by test_pfn_ref_cpu.py.

It is the PFNLayer stack as the reference model evaluates it on a (V, P, C) tensor whose unused point slots are zero:
Linear without bias → BatchNorm1d over all V·P rows (training: batch statistics with the biased variance, running update
with momentum and the unbiased variance; eval: running statistics), eps 1e-3 → ReLU → max over the P slots → concat
[x, max] for every layer but the last.  Ordinary autograd; every layer's pre-activation z is returned too."""
import torch

EPS, MOMENTUM = 1e-3, 0.01


def dense_rows(rows, num_points, max_points):
    """Compact rows (K, C), pillar-major, + num_points (V,) → the zero-padded (V, P, C) tensor (differentiable in rows)."""
    n = num_points.long()
    mask = torch.arange(max_points).view(1, -1) < n.view(-1, 1)                     # (V, P)
    out = rows.new_zeros((n.shape[0], max_points, rows.shape[1]))
    return out.masked_scatter(mask.unsqueeze(-1).expand_as(out), rows)


def dense_voxels(points, pillar_points):
    """``Pillars`` fields (points (N, D), pillar_points (V, P) with -1 for an unused slot) → zero-padded (V, P, D) voxels."""
    idx = pillar_points.long()
    return points[idx.clamp_min(0)] * (idx >= 0).unsqueeze(-1).to(points.dtype)


def compact_rows(dense, num_points):
    """The real rows of a (V, P, C) tensor, pillar-major: the inverse of :func:`dense_rows`."""
    mask = torch.arange(dense.shape[1]).view(1, -1) < num_points.long().view(-1, 1)
    return dense[mask]


def decorate(voxels, num_points, coors, voxel_size, pc_range):
    """The (V, P, D + 7) decoration of mmdet3d's PillarFeatureNet (legacy, with_distance) in the dtype of ``voxels``: channels
    0-2 hold the offset from the pillar centre (the legacy aliasing), then the other point channels, the offset from the
    pillar's mean point, the centre offset again and its norm; unused slots are zero.  The pillar centre is formed from the
    f32 voxel size and range bounds the kernel ABI takes, exactly, in that dtype."""
    dt = voxels.dtype
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32).to(dt)
    n = num_points.to(dt).view(-1, 1, 1)
    xyz = voxels[:, :, :3]
    cluster = xyz - xyz.sum(1, keepdim=True) / n
    centre = torch.stack([coors[:, 3 - k].to(dt) * f32(voxel_size[k]) + f32(voxel_size[k] / 2 + pc_range[k]) for k in range(3)], -1)
    off = xyz - centre.unsqueeze(1)
    dist = (off * off).sum(-1, keepdim=True).sqrt()
    out = torch.cat([off, voxels[:, :, 3:], cluster, off, dist], -1)
    mask = torch.arange(voxels.shape[1]).view(1, -1) < num_points.long().view(-1, 1)
    return out * mask.unsqueeze(-1).to(dt)


def batch_norm(y, gamma, beta, running_mean, running_var, training, eps=EPS, momentum=MOMENTUM):
    """BatchNorm1d over the rows of y (R, U).  Returns z and the running buffers after the call (new tensors)."""
    if training:
        r = y.shape[0]
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)                                            # biased: what normalises
        with torch.no_grad():
            rm = (1 - momentum) * running_mean + momentum * mean
            rv = (1 - momentum) * running_var + momentum * var * (r / max(r - 1, 1))
    else:
        mean, var, rm, rv = running_mean, running_var, running_mean.clone(), running_var.clone()
    return (y - mean) / torch.sqrt(var + eps) * gamma + beta, rm, rv


def pfn_ref(dense, layers, training, eps=EPS, momentum=MOMENTUM):
    """dense (V, P, C); layers: a sequence of (weight (U, C_in), gamma, beta, running_mean, running_var) in the dtype of
    ``dense``.  Returns (out (V, U_last), [z_l (V, P, U_l)], [(running_mean_l, running_var_l) after the call])."""
    x = dense
    v, p, _ = x.shape
    zs, bufs = [], []
    for i, (w, g, b, rm, rv) in enumerate(layers):
        y = x @ w.t()
        z, rm2, rv2 = batch_norm(y.reshape(v * p, -1), g, b, rm, rv, training, eps, momentum)
        z = z.view(v, p, -1)
        zs.append(z)
        bufs.append((rm2, rv2))
        a = torch.relu(z)
        m = a.max(dim=1, keepdim=True)[0]
        x = m if i == len(layers) - 1 else torch.cat([a, m.expand(-1, p, -1)], dim=2)
    return x.squeeze(1), zs, bufs
