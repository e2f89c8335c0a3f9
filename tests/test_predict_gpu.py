"""Inference API (mask_bev_amd/predict.py): MaskBevModule.predict against forward() + the K21 restatement of
tests/test_k21_instances_gpu.py, and GraphedPredictStep replays against eager predict — across batches, in-place weight
updates, a live training graph, and at full size."""
import collections

import pytest
import torch
import torch.nn.functional as F

from tests.test_k21_instances_gpu import check_masks, check_selection, ref_map_rows
from tests.util_cfg import random_gt, random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu


def _tiny(device, dtype='fp32', flat=False, q=8):
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(0)
    kw = dict(tiny_kwargs(nx=96, ny=96, q=q), compute_dtype=dtype)
    m = MaskBevModule(**kw).to(device).train()
    m.log_scalars = False
    if flat:
        m.flatten_parameters()
    return kw, m


def _scans(kw, device, sizes, seed):
    return [x.to(device) for x in random_scans(kw, sizes, seed=seed)]


def _eager_outputs(m, scans):
    was = m.training
    m.eval()
    with torch.no_grad():
        cls, mk, _ = m(scans)
    m.train(was)
    return cls[-1].float().cpu(), mk[-1].float().cpu()


def check_against_restatement(got, cls, mk, grid):
    """K21's outputs against the CPU restatement on the decoder output they were extracted from."""
    check_selection(got, cls, 0.0)
    v = F.interpolate(mk, grid, mode='bilinear', align_corners=False)
    check_masks(got, v.flatten(0, 1), torch.arange(v.shape[0] * v.shape[1]))
    imap, amb = ref_map_rows(v, got.scores.cpu(), got.keep.cpu())
    gm = got.instance_map.cpu()
    assert torch.equal(gm[~amb], imap[~amb].to(gm.dtype))


def assert_same(a, b, score_rtol=1e-6, frac=0.0):
    """Two Predictions of the same scans: labels / keep exact, scores to score_rtol, and at most `frac` of the mask bits and
    of the instance-map pixels different (0.0: identical)."""
    assert torch.equal(a.labels, b.labels) and torch.equal(a.keep, b.keep)
    assert torch.allclose(a.scores, b.scores, rtol=score_rtol, atol=0)
    bits = (a.masks.words ^ b.masks.words).ne(0).sum().item()
    assert bits <= frac * a.masks.words.numel() * 32, bits
    px = (a.instance_map != b.instance_map).sum().item()
    assert px <= frac * a.instance_map.numel(), px
    assert (a.areas - b.areas).abs().max().item() <= frac * a.masks.h * a.masks.w
    assert torch.allclose(a.mask_scores, b.mask_scores, rtol=1e-5 if frac else 0, atol=1e-6 if frac else 0)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
def test_predict_equals_forward_and_restatement(device, dtype):
    from mask_bev_amd.predict import grid_hw
    kw, m = _tiny(device, dtype)
    scans = _scans(kw, device, [3000, 2400], seed=1)
    got = m.predict(scans)
    cls, mk = _eager_outputs(m, scans)
    check_against_restatement(got, cls, mk, grid_hw(m))
    assert got.instance_map.shape == (2, 96, 96) and got.masks.h == 96
    # Lightning's name, with a (scans, targets) batch
    labels, gt = random_gt(kw, 2, 2, seed=3)
    again = m.predict_step((scans, (labels.to(device), gt.to(device))), 0)
    assert_same(got, again)


def test_predict_restores_mode(device):
    kw, m = _tiny(device)
    scans = _scans(kw, device, [2000], seed=2)
    m.train()
    m.predict(scans)
    assert m.training and m._encoder.training
    m.eval()
    m.predict(scans)
    assert not m.training and not m._encoder.training


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_graphed_predict_replays_match_eager(device, dtype):
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.predict import GraphedPredictStep, grid_hw
    kw, m = _tiny(device, dtype)
    batches = [_scans(kw, device, sizes, seed=s) for s, sizes in enumerate([[3000, 2500], [1200, 4100], [2600, 900]])]
    g = GraphedPredictStep(m, batches[0])
    for scans in batches:
        got = g.step(scans).clone()
        want = m.predict(scans)
        assert_same(got, want)
        cls, mk = _eager_outputs(m, scans)
        check_against_restatement(got, cls, mk, grid_hw(m))
    with pytest.raises(MaskBevHipError):
        g.step(batches[0][:1])
    g.close()


@pytest.mark.parametrize('flat', [False, True])
def test_graphed_predict_follows_optimizer_steps(device, flat):
    from mask_bev_amd.predict import GraphedPredictStep
    kw, m = _tiny(device, 'bf16', flat=flat)
    opt = m.configure_optimizers()['optimizer']
    scans = _scans(kw, device, [3000, 2500], seed=4)
    g = GraphedPredictStep(m, scans)
    before = g.step(scans).clone()
    labels, gt = random_gt(kw, 2, 3, seed=5)
    batch = (scans, (labels.to(device), gt.to(device)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                 # eager backward off the default stream (graph.py)
        for _ in range(3):
            opt.zero_grad(set_to_none=not flat)
            m.scale_loss(m.training_step(batch, 0)).backward()
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    got = g.step(scans).clone()
    want = m.predict(scans)
    assert not torch.equal(got.scores, before.scores)          # the weights did change
    assert_same(got, want)
    g.close()


def test_graphed_predict_beside_graphed_train(device):
    from mask_bev_amd.graph import GraphedTrainStep
    from mask_bev_amd.predict import GraphedPredictStep
    kw, m = _tiny(device, 'bf16', flat=True)
    m._panoptic_head._panoptic_head.num_points = 2000
    opt = m.configure_optimizers()['optimizer']
    batches = []
    for s in range(2):
        labels, gt = random_gt(kw, 2, 3, seed=10 + s)
        batches.append((_scans(kw, device, [3000, 2500 + 300 * s], seed=s), (labels.to(device), gt.to(device))))
    train = GraphedTrainStep(m, opt, batches[0])
    pred = GraphedPredictStep(m, batches[1][0])
    for it in range(2):
        b = batches[it % 2]
        with torch.no_grad():                     # the eager loss on the same weights (fresh sampling points: within 5 %)
            loss_e = float(m.training_step(b, 0))
        loss_g = float(train.step(b))
        assert abs(loss_g - loss_e) / loss_e < 0.05, (loss_g, loss_e)
        got = pred.step(batches[1][0]).clone()
        want = m.predict(batches[1][0])
        assert_same(got, want)
    pred.close()
    train.close()


def _spy_capture(make):
    from torch.utils._python_dispatch import TorchDispatchMode
    red = ('sum', 'amax', 'amin', 'max', 'min', 'mean', 'norm', 'prod', 'any', 'all', 'argmax', 'argmin', 'var', 'std',
           'logsumexp', 'count_nonzero')
    seen = collections.Counter()

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            if func.__name__.split('.')[0] in red and torch.cuda.is_current_stream_capturing():
                t = next((a for a in args if torch.is_tensor(a)), None)
                o = out[0] if isinstance(out, (tuple, list)) else out
                if t is not None and torch.is_tensor(o) and t.is_cuda and o.numel() > 0:
                    seen[(str(func), tuple(t.shape), tuple(o.shape))] = t.numel() // o.numel()
            return out

    with Spy():
        g = make()
    return g, seen


def _bench_module(device, workload, batch, dtype):
    from mask_bev_amd import synthetic
    from mask_bev_amd.mask_bev_module import MaskBevModule
    torch.manual_seed(420)
    m = MaskBevModule(**synthetic.module_kwargs(workload, batch, compute_dtype=dtype)).to(device).train()
    m.flatten_parameters()
    scans = synthetic.make_batch(workload, batch, 0, 0, device)[0]
    return m, scans


@pytest.mark.parametrize('batch,dtype', [(2, 'bf16'), (1, 'fp32')])
def test_no_multi_workgroup_aten_reduction_inside_the_predict_capture(device, batch, dtype):
    """The rule of test_graph_gpu.py for the training capture, over the predict capture."""
    from mask_bev_amd.predict import GraphedPredictStep
    m, scans = _bench_module(device, 'semantic_kitti_512', batch, dtype)
    g, seen = _spy_capture(lambda: GraphedPredictStep(m, scans))
    g.close()
    if seen:
        worst = max(seen.items(), key=lambda kv: kv[1])
        assert worst[1] <= 1024, f'{worst[0]} reduces {worst[1]} elements per output inside the predict capture'


@pytest.mark.parametrize('workload,batch,dtype', [('semantic_kitti_512', 2, 'bf16'), ('waymo_1024', 1, 'fp16')])
def test_graphed_predict_full_size(device, workload, batch, dtype):
    from mask_bev_amd import synthetic
    from mask_bev_amd.predict import GraphedPredictStep
    m, scans = _bench_module(device, workload, batch, dtype)
    g = GraphedPredictStep(m, scans)
    other = synthetic.make_batch(workload, batch, 0, 1, device)[0]
    for s in (other, scans):
        got = g.step(s).clone()
        want = m.predict(s)
        assert torch.isfinite(got.scores).all() and torch.isfinite(got.mask_scores).all()
        assert got.instance_map.min().item() >= -1 and got.instance_map.max().item() < got.labels.shape[1]
        assert_same(got, want)
    g.close()
