"""tests/loss_ref.py, the dtype-generic restatement of the loss the float64 loss-path suite (test_loss_paths_gpu.py) compares
with, pinned on the CPU: in float32 it IS the oracle's loss (same assignment, every term), and handing it its own decisions
changes nothing."""
import pytest
import torch

from oracle import maskbev_oracle as O
from tests import loss_ref as R
from tests.util_cfg import tiny_kwargs

D, B, Q, P = 3, 2, 8, 40


def _inputs(n_gt, seed):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(D, B, Q, 2, generator=g)
    masks = torch.randn(D, B, Q, 20, 18, generator=g) * 3
    labels = torch.randint(0, 2, (B, n_gt), generator=g)
    gt = (torch.rand(B, n_gt, 37, 29, generator=g) > 0.7).float()
    gt[:, -1] = 0
    return cls, masks, labels, gt


def _oracle_assignment(cfg, cls, masks, labels, gt, seed):
    """The assignment inside O.loss_dict, from a replay of its draws (get_targets_single does not return it)."""
    pts = O.PointSource(seed)
    n_samp, _, n_rand = R.counts(cfg)
    g = B * min(Q, labels.shape[1])
    out = torch.full((D, B, Q), -1, dtype=torch.long)
    for d in range(D):
        for b in range(B):
            c = pts.rand(1, cfg.num_points, 2)
            mp = O.point_sample(masks[d, b].unsqueeze(1), c.repeat(Q, 1, 1)).squeeze(1)
            gp = O.point_sample(gt[b].unsqueeze(1), c.repeat(labels.shape[1], 1, 1)).squeeze(1)
            out[d, b] = R.solve(O.match_cost(cfg, cls[d, b], mp, labels[b], gp))
        pts.rand(g, n_samp, 2)
        pts.rand(g, n_rand, 2)
    return out


@pytest.mark.parametrize('n_gt', [5, 8, 12])
def test_float32_free_mode_is_the_oracle(n_gt):
    """G < Q, G = Q, G > Q: every term of O.loss_dict bit for bit, and the oracle's assignment."""
    cfg = O.make_cfg(**tiny_kwargs())
    cfg.num_points = P
    cls, masks, labels, gt = _inputs(n_gt, n_gt)
    want = O.loss_dict(cfg, list(cls.unbind(0)), list(masks.unbind(0)), labels, gt, O.PointSource(5))
    got = R.loss_ref(R.spec(P, cfg.num_classes, cfg.class_weight), cls, masks, labels, gt, O.PointSource(5), torch.float32)
    assert list(got.loss.keys()) == list(want.keys())
    assert [k for k in want if torch.is_tensor(want[k])] == R.loss_keys(D)
    for k in want:
        if torch.is_tensor(want[k]):
            assert got.loss[k].dtype == torch.float32 and float(got.loss[k]) == float(want[k]), k
        else:
            assert got.loss[k] == want[k] == 0
    assert torch.equal(got.assignment, _oracle_assignment(cfg, cls, masks, labels, gt, 5))
    m = min(Q, n_gt)
    assert bool(((got.assignment >= 0).sum(-1) == m).all())
    assert got.cost.shape == (D * B, Q, n_gt) and got.points.shape == (D * B * m, P, 2)
    assert got.candidate_logits.shape == (D * B * m, 3 * P) and got.rows.shape == (D * B * m,)


@pytest.mark.parametrize('n_gt', [5, 8, 12])
def test_float64_teacher_forced_with_its_own_decisions_is_the_free_mode(n_gt):
    """Fed with the free mode's assignment and points, the teacher-forced mode reproduces its losses and gradients to 1e-12."""
    cfg = R.spec(P)
    cls, masks, labels, gt = _inputs(n_gt, 20 + n_gt)
    g = torch.Generator().manual_seed(1)
    w = {k: 0.5 + float(torch.rand((), generator=g)) for k in R.loss_keys(D)}
    free = R.loss_ref(cfg, cls, masks, labels, gt, O.PointSource(3), torch.float64, weights=w)
    forced = R.loss_ref(cfg, cls, masks, labels, gt, O.PointSource(3), torch.float64, assignment=free.assignment,
                        points=free.points, weights=w)
    assert free.d_cls.dtype == free.d_masks.dtype == torch.float64
    for k in R.loss_keys(D):
        assert abs(float(forced.loss[k]) - float(free.loss[k])) <= 1e-12 * abs(float(free.loss[k])), k
    for a, b in ((forced.d_cls, free.d_cls), (forced.d_masks, free.d_masks), (forced.cost, free.cost)):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    assert torch.equal(forced.points, free.points) and torch.equal(forced.rows, free.rows)
    # the gradient reaches exactly the matched maps, and every class row
    touched = free.d_masks.flatten(0, 2).abs().amax((1, 2)) > 0
    assert torch.equal(torch.nonzero(touched).squeeze(-1), free.rows)
    assert bool((free.d_cls.abs().amax(-1) > 0).all())
