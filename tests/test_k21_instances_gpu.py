"""K21 instance extraction (csrc/instances.hip, predict.extract_instances) against a torch restatement on the CPU:
softmax / first argmax / F.interpolate(bilinear, align_corners=False) > 0 / argmax of score * sigmoid over kept queries."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BAND = 1e-5          # |v| at or below this: the pixel may fall on either side of the threshold


def ref_select(cls, thr):
    c = cls.float()
    label = c.argmax(-1)
    score = torch.softmax(c, -1).gather(-1, label.unsqueeze(-1)).squeeze(-1)
    return label, score, (label > 0) & (score >= thr)


def ref_rows(logits, y_lo, y_hi, H, W):
    """Rows [y_lo, y_hi) of the upsampled maps, upsample_bilinear2d's arithmetic written out (for maps too big to upsample
    whole)."""
    b, q, h, w = logits.shape
    sh, sw = torch.tensor(h / H, dtype=torch.float32), torch.tensor(w / W, dtype=torch.float32)
    y = torch.arange(y_lo, y_hi, dtype=torch.float32)
    x = torch.arange(W, dtype=torch.float32)
    fy = (sh * (y + 0.5) - 0.5).clamp(min=0)
    fx = (sw * (x + 0.5) - 0.5).clamp(min=0)
    y0, x0 = fy.long(), fx.long()
    y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)
    ly, lx = (fy - y0.float()).view(-1, 1), fx - x0.float()
    hy, hx = 1 - ly, 1 - lx
    top, bot = logits[:, :, y0], logits[:, :, y1]
    return hy * (hx * top[..., x0] + lx * top[..., x1]) + ly * (hx * bot[..., x0] + lx * bot[..., x1])


def ref_map_rows(v, score, keep):
    """v (B, Q, r, W) → instance map rows (B, r, W) and the mask of ambiguous pixels (band or a near tie)."""
    sig = torch.sigmoid(v)
    ok = keep.view(*keep.shape, 1, 1) & (v > 0)
    prod = torch.where(ok, score.view(*score.shape, 1, 1) * sig, torch.full_like(v, -1.0))
    top2 = prod.topk(min(2, prod.shape[1]), dim=1).values
    best = prod.argmax(1)
    imap = torch.where(top2[:, 0] >= 0, best, torch.full_like(best, -1))
    amb = (keep.view(*keep.shape, 1, 1) & (v.abs() <= BAND)).any(1)
    if top2.shape[1] > 1:
        amb |= (top2[:, 1] >= 0) & ((top2[:, 0] - top2[:, 1]) <= 1e-6 * top2[:, 0])
    return imap, amb


def make_inputs(B, Q, h, w, classes, seed):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(B, Q, classes, generator=g) * 2
    cls[0, 0, :] = 0.5                                     # all classes tied: label 0
    if classes > 2:
        cls[0, 1 % Q, 1:3] = 4.0                           # tie between classes 1 and 2: label 1
    logits = torch.randn(B, Q, h, w, generator=g) * 3
    logits[0, min(1, Q - 1)] = -logits[0, min(1, Q - 1)].abs() - 0.1     # an all-negative map: area 0, mask score 0
    return cls, logits


def check_selection(got, cls, thr):
    label, score, keep = ref_select(cls, thr)
    assert torch.equal(got.labels.cpu().long(), label)
    assert torch.allclose(got.scores.cpu(), score, rtol=2e-6, atol=0)
    near = (score - thr).abs() <= 2e-6 * score                # a score within its tolerance of the threshold
    assert torch.equal(got.keep.cpu()[~near], keep[~near])
    return label, score, keep


def check_masks(got, v, rows):
    """v (N, H, W): the reference maps of the rows `rows` of got.masks."""
    from mask_bev_amd.predict import unpack_bits
    H, W = v.shape[-2:]
    bits = unpack_bits(got.masks.words.cpu()[rows], H, W)
    want = v > 0
    band = v.abs() <= BAND
    assert torch.equal(bits[~band], want[~band])
    nband = band.flatten(1).sum(1)
    area = want.flatten(1).sum(1)
    got_area = got.areas.cpu().flatten()[rows].long()
    assert ((got_area - area).abs() <= nband).all()
    s = (torch.sigmoid(v.double()) * want).flatten(1).sum(1)
    ms = torch.where(area > 0, s / area.clamp(min=1), torch.zeros_like(s))
    got_ms = got.mask_scores.cpu().flatten()[rows].double()
    tol = 1e-5 * ms + nband / area.clamp(min=1)
    assert ((got_ms - ms).abs() <= tol).all(), (got_ms - ms).abs().max()
    assert (got_ms[area == 0] == 0).all() and (got_area[area == 0] <= nband[area == 0]).all()


def run_case(device, B, Q, h, w, H, W, classes, thr, cls_dtype, seed, subset=None):
    from mask_bev_amd.predict import extract_instances
    cls, logits = make_inputs(B, Q, h, w, classes, seed)
    cls = cls.to(cls_dtype)
    got = extract_instances(cls.to(device), logits.to(device), (H, W), score_threshold=thr)
    torch.cuda.synchronize()
    _, score, keep = check_selection(got, cls, thr)
    score, keep = got.scores.cpu(), got.keep.cpu()             # the map is checked against the kernel's own selection
    if subset is None:
        v = F.interpolate(logits, (H, W), mode='bilinear', align_corners=False)
        check_masks(got, v.flatten(0, 1), torch.arange(B * Q))
        imap, amb = ref_map_rows(v, score, keep)
        gm = got.instance_map.cpu()
        assert torch.equal(gm[~amb], imap[~amb].to(gm.dtype))
    else:
        g = torch.Generator().manual_seed(seed + 1)
        rows = torch.randperm(B * Q, generator=g)[:subset].sort().values
        v = F.interpolate(logits.flatten(0, 1)[rows].unsqueeze(0), (H, W), mode='bilinear', align_corners=False)[0]
        check_masks(got, v, rows)
        del v
        gm = got.instance_map.cpu()
        for y in range(0, H, 64):
            imap, amb = ref_map_rows(ref_rows(logits, y, min(H, y + 64), H, W), score, keep)
            assert torch.equal(gm[:, y:y + 64][~amb], imap[~amb].to(gm.dtype))
    return got


SHAPES = [(2, 7, 24, 20, 96, 80), (1, 5, 128, 128, 512, 512), (2, 9, 124, 108, 496, 432), (1, 3, 17, 13, 50, 41)]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('classes', [2, 4])
def test_extract_matches_restatement(device, shape, classes):
    B, Q, h, w, H, W = shape
    seed = sum(shape) * 10 + classes
    run_case(device, B, Q, h, w, H, W, classes, 0.0, torch.float32, seed)
    run_case(device, B, Q, h, w, H, W, classes, 0.6, torch.bfloat16, seed + 1)
    run_case(device, B, Q, h, w, H, W, classes, 0.55, torch.float16, seed + 2)
    # no kept query (every score is below 1.01): the map is all -1, the masks are still every query's
    got = run_case(device, B, Q, h, w, H, W, classes, 1.01, torch.float32, seed + 3)
    assert not got.keep.any() and (got.instance_map == -1).all()


def test_extract_waymo_scale(device):
    """256² logits on a 1024² grid — beyond K15's whole-map LDS tile.  Bits / areas / mask scores on 16 queries, the
    selection and the instance map on all 300."""
    got = run_case(device, 1, 300, 256, 256, 1024, 1024, 4, 0.4, torch.float32, 7, subset=16)
    assert got.keep.any()
    got = run_case(device, 1, 300, 256, 256, 1024, 1024, 2, 0.0, torch.bfloat16, 8, subset=16)


def test_extract_is_deterministic(device):
    from mask_bev_amd.predict import extract_instances
    cls, logits = make_inputs(2, 100, 128, 128, 4, 3)
    cls, logits = cls.to(device), logits.to(device)
    a = extract_instances(cls, logits, (512, 512), 0.3)
    b = extract_instances(cls, logits, (512, 512), 0.3)
    for name in ('labels', 'scores', 'keep', 'areas', 'mask_scores', 'instance_map'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.masks.words, b.masks.words)


def test_extract_memory_stays_far_below_dense(device):
    from mask_bev_amd.predict import extract_instances
    g = torch.Generator(device=device).manual_seed(0)
    cls = torch.randn(2, 300, 4, device=device, generator=g)
    logits = torch.randn(2, 300, 256, 256, device=device, generator=g)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = extract_instances(cls, logits, (1024, 1024))
    torch.cuda.synchronize()
    dense = 2 * 300 * 1024 * 1024 * 4
    assert torch.cuda.max_memory_allocated() - base < 0.1 * dense
    assert out.instance_map.shape == (2, 1024, 1024)


@pytest.mark.parametrize('B,Q', [(0, 5), (2, 0)])
def test_extract_empty(device, B, Q):
    from mask_bev_amd.predict import extract_instances
    out = extract_instances(torch.zeros(B, Q, 3, device=device), torch.zeros(B, Q, 8, 8, device=device), (32, 32))
    assert out.labels.shape == (B, Q) and out.keep.shape == (B, Q) and out.areas.shape == (B, Q)
    assert out.masks.words.shape[0] == 0 and out.instance_map.shape == (B, 32, 32)
    if B:
        assert (out.instance_map == -1).all()
