"""tests/pfn_ref.py — the dense PillarFeatureNet reference of the K2 float64 suite — pinned to the project's oracle: run in
f32 it agrees with oracle.maskbev_oracle.pfn_forward on the configuration of test_k2_pfn_gpu.py (output and running buffers
to 1e-5 relative).  There is nothing else to check it against; its float64 runs are the same code in another dtype."""
import pytest
import torch

from oracle import maskbev_oracle as O
from tests import pfn_ref as R
from tests.util_cfg import random_scans


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('pc_dim', [4, 3])
@pytest.mark.parametrize('chans,P,sizes,training', [([32, 32, 32], 8, [3000, 2000], True), ([64, 128], 4, [1500, 10, 900], True),
                                                    ([32, 32, 32], 8, [2500], False)])
def test_pfn_ref_f32_equals_the_oracle(chans, P, sizes, training, pc_dim):
    kw = dict(x_range=(-10, 10), y_range=(-10, 10), z_range=(-3, 1), voxel_size=0.25, num_queries=4, max_num_points=P,
              encoder_feat_channels=chans, backbone_embed_dim=48, head_feat_channels=128, head_out_channels=128,
              pc_point_dim=pc_dim)
    cfg = O.make_cfg(**kw)
    pre = O.ENC + '_voxel_encoder.pfn_layers.'
    sd = {k: v for k, v in O.make_state_dict(cfg, 3).items() if k.startswith(pre)}
    for k in list(sd):
        if k.endswith('running_mean'):
            sd[k] = torch.randn_like(sd[k]) * 0.1
        if k.endswith('running_var'):
            sd[k] = torch.rand_like(sd[k]) + 0.5
    voxels, nump, coors = O.voxelize(cfg, random_scans(kw, sizes, seed=P))
    bufs = {k: v.clone() for k, v in sd.items() if 'running_' in k}
    want = O.pfn_forward(cfg, sd, voxels, nump, coors, training, bn_buffers=bufs)
    # the decoration, then the stack
    dense = R.decorate(voxels, nump, coors, cfg.voxel_size3, cfg.pc_range)
    assert _rel(dense, O.pfn_decorate(cfg, voxels, nump, coors)) <= 1e-6
    layers = [tuple(sd[f'{pre}{i}.{n}'] for n in ('linear.weight', 'norm.weight', 'norm.bias', 'norm.running_mean',
                                                 'norm.running_var')) for i in range(len(chans))]
    out, zs, new = R.pfn_ref(dense, layers, training)
    assert out.shape == want.shape and len(zs) == len(chans)
    assert all(z.shape == (voxels.shape[0], P, l[0].shape[0]) for z, l in zip(zs, layers))      # (a non-last layer: half its channels)
    assert _rel(out, want) <= 1e-5
    for i, (rm, rv) in enumerate(new):
        assert _rel(rm, bufs[f'{pre}{i}.norm.running_mean']) <= 1e-5
        assert _rel(rv, bufs[f'{pre}{i}.norm.running_var']) <= 1e-5
        if not training:
            assert torch.equal(rm, layers[i][3]) and torch.equal(rv, layers[i][4])
    # the compact form and back; the Pillars-field form of the voxels
    rows = R.compact_rows(dense, nump)
    assert rows.shape[0] == int(nump.sum()) and torch.equal(R.dense_rows(rows, nump, P), dense)
    pts = voxels.reshape(-1, voxels.shape[-1])
    slots = torch.arange(voxels.shape[0] * P, dtype=torch.int32).view(-1, P)
    slots = torch.where(torch.arange(P).view(1, -1) < nump.view(-1, 1), slots, torch.full_like(slots, -1))
    assert torch.equal(R.dense_voxels(pts, slots), voxels)


def test_pfn_ref_float64_gradients_reach_every_parameter():
    """Autograd through the reference in float64: rows and all parameters get a gradient, and a pillar's unused slots carry
    the bias-only activation relu(beta - mean·scale), not zero — the padded rows take part in the statistics and in the max."""
    g = torch.Generator().manual_seed(0)
    nump = torch.tensor([3, 1, 4, 2])
    rows = torch.randn(10, 5, generator=g, dtype=torch.float64).requires_grad_()
    layers = []
    for cin, u in ((5, 8), (16, 8)):
        layers.append((torch.randn(u, cin, generator=g, dtype=torch.float64).requires_grad_(),
                       (1 + 0.1 * torch.randn(u, generator=g, dtype=torch.float64)).requires_grad_(),
                       (0.1 * torch.randn(u, generator=g, dtype=torch.float64)).requires_grad_(),
                       torch.zeros(u, dtype=torch.float64), torch.ones(u, dtype=torch.float64)))
    out, zs, new = R.pfn_ref(R.dense_rows(rows, nump, 4), layers, True)
    out.sum().backward()
    assert rows.grad is not None and float(rows.grad.abs().max()) > 0
    for w, gm, bt, _, _ in layers:
        assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in (w, gm, bt))
    z0 = zs[0].detach()
    assert torch.equal(z0[1, 1], z0[1, 3]) and torch.equal(z0[1, 1], z0[0, 3])      # every padded slot of layer 0: one value
    assert not torch.equal(z0[1, 1], torch.zeros(8, dtype=torch.float64))
    assert float((new[0][0] - 0.01 * (R.dense_rows(rows, nump, 4).detach() @ layers[0][0].detach().t()).reshape(16, 8).mean(0)).abs().max()) < 1e-15


@pytest.mark.parametrize('p,nump', [(4, [3, 1, 4, 2, 4, 1]), (8, [8, 8, 8]), (5, [2])])
def test_float64_steps_of_one_layer_compose_to_autograd(p, nump):
    """The dense steps test_k2_paths_gpu.py holds the kernels to (step_forward, step_route, step_bn: padded-row copies,
    first-index max, summed padded gradients) are, in float64, the autograd gradient of the dense layer itself."""
    from tests.test_k2_paths_gpu import _dense, _index, _spread, step_bn, step_forward, step_route
    f64 = torch.float64
    g = torch.Generator().manual_seed(p)
    n = torch.tensor(nump, dtype=torch.int32)
    v, k, u = len(nump), sum(nump), 8
    r = lambda *s: torch.randn(*s, generator=g, dtype=f64)
    y0, ypad0, t = r(k, u).requires_grad_(), r(v, u).requires_grad_(), r(v, u).requires_grad_()
    gamma, beta = (1 + 0.1 * r(u)).requires_grad_(), (0.1 * r(u)).requires_grad_()
    da, dm = r(k, u), r(v, u)
    sapad = r(v, u) * (n.view(-1, 1) < p)
    # the dense layer with autograd
    row_pillar = _index(n)[1]
    yd, mask = _dense(y0 + t[row_pillar], ypad0 + t, n, p)
    z, _, _ = R.batch_norm(yd.reshape(v * p, u), gamma, beta, torch.zeros(u, dtype=f64), torch.ones(u, dtype=f64), True)
    a = torch.relu(z).view(v, p, u)
    up = _dense(da, _spread(sapad, n, p), n, p)[0]                      # the upstream gradient of every slot
    loss = (a * up).sum() + (a.max(dim=1)[0] * dm).sum()
    gy, gypad, gt, ggamma, gbeta = torch.autograd.grad(loss, (y0, ypad0, t, gamma, beta))
    # the steps
    f = step_forward(y0.detach(), ypad0.detach(), t.detach(), gamma.detach(), beta.detach(), torch.zeros(u), torch.ones(u), n, p,
                     True, f64)
    assert float((f['m'] - a.detach().max(dim=1)[0]).abs().max()) < 1e-12
    assert float((f['y'] * f['scale'] + f['shift'] - z.detach().view(v, p, u)[mask.expand(v, p, u)].view(k, u)).abs().max()) < 1e-12
    rt = step_route(f['y'], f['y_pad'], f['scale'], f['shift'], f['mean'], f['rstd'], da, sapad, dm, n, p, f64)
    bn = step_bn(f['y'], f['y_pad'], rt['dz'], rt['dz_pad'], f['mean'], f['rstd'], gamma.detach(),
                 torch.cat([rt['d_beta'], rt['d_gamma']]), float(v * p), True, n, p, f64)
    for got, want in ((bn['dy'], gy), (bn['dy_pad'], gypad), (bn['dt'], gt), (rt['d_gamma'], ggamma), (rt['d_beta'], gbeta)):
        assert float((got - want).abs().max()) < 1e-12 * max(1.0, float(want.abs().max()))
