"""K42 (mbv_mask_self_overlap, mbv_mask_nms, mbv_overlap_filter; csrc/resolve.hip) through the C ABI, and what is built on it:
``ops.mask_self_overlap`` / ``mask_nms`` / ``overlap_filter``, ``extract_instances(..., resolve=)``, ``GraphedPredictStep`` and
the launcher's ``predict_resolve`` key.

Everything is integer arithmetic: every comparison is exact equality, against numpy popcounts for K42a and against the plain
loops of tests/resolve_ref.py for the rule; outputs are poisoned before every call."""
import numpy as np
import pytest
import torch

from tests import resolve_ref as R
from tests.util_cfg import random_scans, tiny_kwargs

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = -1, -3
POISON = 0x5a5a5a5a

# (H, W, Q, B): 37 x 29 = 1073 cells, 34 words (tail bits, no 16-byte path); 64 x 64 and 256 x 256 take the 16-byte paths; Q = 70
# and 300 cross the 64-lane ballots, the 32-row tiles and the 256-thread strides; 256 x 256 has 4 splits of the contraction
CASES = [(37, 29, 1, 1), (37, 29, 7, 3), (37, 29, 70, 1), (37, 29, 300, 3), (64, 64, 1, 3), (64, 64, 70, 3), (64, 64, 300, 1),
         (256, 256, 70, 3)]
KINDS = ('none', 'all', 'tied')


@pytest.fixture(scope='module')
def lib():
    from mask_bev_amd import _lib
    return _lib.load()


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def pack(lib, dense):
    """(N, H, W) bool → (N, words) int32 in mbv_pack_binary_masks' layout, tail bits zero."""
    n, h, w = dense.shape
    nwords = lib.mbv_packed_mask_words(h, w)
    flat = np.zeros((n, nwords * 32), dtype=bool)
    flat[:, :h * w] = dense.reshape(n, -1)
    return np.packbits(flat, axis=1, bitorder='little').view('<u4').astype(np.uint32).view(np.int32).reshape(n, nwords)


def make_frame(rng, h, w, q, kind):
    """One frame: random rectangles with forced duplicates and containments, an empty mask, and (Q >= 7, 'all') the strip cases
    of tests/test_resolve_cpu.py in rows 0 and 1 under the five best scores."""
    masks = np.zeros((q, h, w), dtype=bool)
    for i in range(q):
        if i > 0 and i % 5 == 3:
            masks[i] = masks[i - 1]                                          # a duplicate
            continue
        y0, x0 = int(rng.integers(0, h - 1)), int(rng.integers(0, w - 1))
        y1, x1 = int(rng.integers(y0 + 1, min(h, y0 + h // 2) + 1)), int(rng.integers(x0 + 1, min(w, x0 + w // 2) + 1))
        if i > 0 and i % 5 == 4:                                             # contained in its predecessor (or equal to it)
            ys, xs = np.nonzero(masks[i - 1].any(1))[0], np.nonzero(masks[i - 1].any(0))[0]
            if ys.size:
                masks[i, ys[0]:max(ys[0] + 1, (ys[0] + ys[-1] + 1) // 2 + 1), xs[0]:xs[-1] + 1] = True
                masks[i] &= masks[i - 1]
                continue
        masks[i, y0:y1, x0:x1] = True
    scores = (rng.random(q) * 0.85 + 0.05).astype(np.float32)
    labels = rng.integers(1, 3, q).astype(np.int32)
    keep = np.ones(q, dtype=bool) if kind == 'all' else np.zeros(q, dtype=bool) if kind == 'none' else rng.random(q) < 0.5
    if kind == 'tied':
        scores = (np.round(scores * 4) / 4 + 0.25).astype(np.float32)       # five values: ties everywhere
    if q >= 7:
        masks[q - 1] = False                                                 # an empty mask
        masks[:5] = False
        for i, (row, a, b) in enumerate(((0, 0, 8), (0, 2, 10), (0, 4, 12), (1, 0, 8), (1, 0, 4))):
            masks[i, row, a:b] = True
        masks[5:, :2] = False                                                # rows 0 and 1 belong to the strip cases
        labels[:5] = 1
        if kind == 'all':
            scores[:5] = np.array([0.99, 0.98, 0.97, 0.96, 0.95], np.float32)
    return masks, scores, labels, keep


def batches(h, w, q, b, seed):
    """Every kind of frame for every case: B = 3 holds one of each; B = 1 makes three batches."""
    rng = np.random.default_rng(seed)
    groups = [KINDS] if b == 3 else [(k,) for k in KINDS]
    for kinds in groups:
        frames = [make_frame(rng, h, w, q, k) for k in kinds]
        yield kinds, tuple(np.stack([f[i] for f in frames]) for i in range(4))


def np_inter(masks, keep):
    """(B, Q, H, W) bool, (B, Q) bool → (B, Q, Q) int32 popcounts, zero wherever either is not kept."""
    b, q = keep.shape
    flat = (masks & keep[:, :, None, None]).reshape(b, q, -1).astype(np.float64)
    return np.einsum('bik,bjk->bij', flat, flat).astype(np.int32)                     # f64 sums of 0 / 1 are exact to 2^53


def call_self_overlap(lib, device, words, keep, q, nwords):
    from mask_bev_amd.ops_core import _ptr, _stream
    b = keep.shape[0]
    d_words, d_keep = dev(words, device), dev(keep.astype(np.uint8), device)
    inter = torch.full((b, q, q), POISON, dtype=torch.int32, device=device)
    rc = lib.mbv_mask_self_overlap(_ptr(d_words), _ptr(d_keep), b, q, nwords, _ptr(inter), _stream())
    torch.cuda.synchronize()
    return rc, inter.cpu().numpy()


def call_nms(lib, device, inter, scores, labels, keep, num, den, same_label):
    from mask_bev_amd.ops_core import _ptr, _stream
    b, q = keep.shape
    d = [dev(inter, device), dev(scores, device), dev(labels, device), dev(keep.astype(np.uint8), device)]
    keep_out = torch.full((b, q), 0x5a, dtype=torch.uint8, device=device)
    by = torch.full((b, q), POISON, dtype=torch.int32, device=device)
    rc = lib.mbv_mask_nms(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), b, q, num, den, same_label, _ptr(keep_out), _ptr(by),
                          _stream())
    torch.cuda.synchronize()
    return rc, keep_out.cpu().numpy(), by.cpu().numpy()


def call_filter(lib, device, imap, areas, keep, num, den, min_cells):
    from mask_bev_amd.ops_core import _ptr, _stream
    b, h, w = imap.shape
    q = keep.shape[1]
    d_map, d_areas, d_keep = dev(imap, device), dev(areas, device), dev(keep.astype(np.uint8), device)
    keep_out = torch.full((b, q), 0x5a, dtype=torch.uint8, device=device)
    owned = torch.full((b, q), POISON, dtype=torch.int32, device=device)
    rc = lib.mbv_overlap_filter(_ptr(d_map), _ptr(d_areas), _ptr(d_keep), b, h, w, q, num, den, min_cells, _ptr(owned),
                                _ptr(keep_out), _stream())
    torch.cuda.synchronize()
    return rc, keep_out.cpu().numpy(), owned.cpu().numpy(), d_map.cpu().numpy()


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_k42a_self_overlap(lib, device, case):
    """All of inter against numpy: symmetric, the kept masks' areas on the diagonal, zeros for every row and column that is
    not kept — whatever garbage the words of those rows hold — into a poisoned table."""
    h, w, q, b = case
    nwords = lib.mbv_packed_mask_words(h, w)
    rng = np.random.default_rng(7)
    for kinds, (masks, _, _, keep) in batches(h, w, q, b, seed=h * 1000 + q):
        words = pack(lib, masks.reshape(-1, h, w))
        garbage = rng.integers(-2 ** 31, 2 ** 31, size=words.shape, dtype=np.int64).astype(np.int32)
        words = np.where(keep.reshape(-1)[:, None], words, garbage)
        rc, inter = call_self_overlap(lib, device, words, keep, q, nwords)
        want = np_inter(masks, keep)
        assert rc == 0 and inter.dtype == np.int32 and np.array_equal(inter, want), kinds
        assert np.array_equal(inter, inter.transpose(0, 2, 1))
        for f in range(len(kinds)):
            assert np.array_equal(np.diagonal(inter[f]), np.where(keep[f], masks[f].reshape(q, -1).sum(1), 0))
        if 'all' in kinds and q > 1:
            assert (inter[kinds.index('all')] > 0).sum() > q               # off-diagonal overlaps exist
        if 'none' in kinds:
            assert not inter[kinds.index('none')].any()


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_k42b_nms(lib, device, case):
    """keep_out and suppressed_by against the plain loops at 1/2 (the threshold-equality and non-transitive strips are in every
    'all' frame), 51/100, num == den, and without the label condition."""
    h, w, q, b = case
    for kinds, (masks, scores, labels, keep) in batches(h, w, q, b, seed=h * 1000 + q):
        inter = np_inter(masks, keep)
        seen = 0
        for num, den, same in ((1, 2, 1), (51, 100, 1), (1, 1, 1), (1, 3, 0)):
            rc, keep_out, by = call_nms(lib, device, inter, scores, labels, keep, num, den, same)
            assert rc == 0
            for f in range(len(kinds)):
                k1, sup = R.nms(inter[f].tolist(), scores[f], labels[f].tolist(), keep[f].tolist(), (num, den), bool(same))
                assert keep_out[f].tolist() == [int(v) for v in k1] and by[f].tolist() == sup, (kinds[f], num, den)
                seen += sum(1 for v in sup if v >= 0)
                if kinds[f] == 'all' and q >= 7 and same:
                    # A suppresses B at both thresholds (6 / 10), C survives; [0, 8) ~ [0, 4) is exactly 1 / 2
                    assert by[f][:5].tolist() == ([-1, 0, -1, -1, 3] if (num, den) == (1, 2) else
                                                  [-1, 0, -1, -1, -1] if (num, den) == (51, 100) else [-1] * 5)
                if kinds[f] == 'none':
                    assert not keep_out[f].any() and (by[f] == -1).all()
        assert seen > 0 or q == 1 or kinds == ('none',)                    # the duplicates are suppressed


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_k42c_overlap_filter(lib, device, case):
    """owned, keep_out and the rewritten map against the plain loops, on maps that also hold queries outside keep and values
    outside [0, Q)."""
    h, w, q, b = case
    rng = np.random.default_rng(11)
    for kinds, (masks, _, _, keep) in batches(h, w, q, b, seed=h * 1000 + q):
        f_num = len(kinds)
        prio = rng.random((f_num, q)).astype(np.float32)
        val = np.where(masks & keep[:, :, None, None], prio[:, :, None, None], -1.0)
        imap = np.where(val.max(1) >= 0, val.argmax(1), -1).astype(np.int32)
        stray = rng.random(imap.shape)
        imap = np.where(stray < 0.02, rng.integers(0, q, imap.shape), imap)          # any query, kept or not
        imap = np.where(stray > 0.99, rng.choice([q, q + 5, -7, 2 ** 31 - 1, -2 ** 31], imap.shape), imap).astype(np.int32)
        areas = masks.reshape(f_num, q, -1).sum(2).astype(np.int32)
        for ratio, min_cells in (((4, 5), 1), ((1, 1), 0), (None, 5), ((1, 3), 2)):
            num, den = (0, 1) if ratio is None else ratio
            rc, keep_out, owned, new = call_filter(lib, device, imap, areas, keep, num, den, min_cells)
            assert rc == 0
            for f in range(f_num):
                k2, own, want = R.overlap_filter(imap[f].tolist(), areas[f].tolist(), keep[f].tolist(), ratio, min_cells)
                assert keep_out[f].tolist() == [int(v) for v in k2] and owned[f].tolist() == own, (kinds[f], ratio)
                assert np.array_equal(new[f], np.asarray(want, dtype=np.int64).astype(np.int32)), (kinds[f], ratio)
                if kinds[f] == 'none':
                    assert not owned[f].any() and not ((new[f] >= 0) & (new[f] < q)).any()


def test_k42_abi_edges(lib, device):
    from mask_bev_amd.ops_core import _ptr, _stream
    s, null = _stream(), None
    t = torch.zeros(1024 * 1024, dtype=torch.int32, device=device)
    p = _ptr(t)
    # B * Q == 0: OK before any pointer is looked at
    for b, q in ((0, 5), (3, 0), (0, 0)):
        assert lib.mbv_mask_self_overlap(null, null, b, q, 34, null, s) == 0
        assert lib.mbv_mask_nms(null, null, null, null, b, q, 1, 2, 1, null, null, s) == 0
        assert lib.mbv_overlap_filter(null, null, null, b, 8, 8, q, 4, 5, 1, null, null, s) == 0
    # limits
    assert lib.mbv_mask_self_overlap(p, p, 1, 1025, 2, p, s) == UNSUPPORTED
    assert lib.mbv_mask_self_overlap(p, p, 65536, 1, 2, p, s) == UNSUPPORTED
    assert lib.mbv_mask_self_overlap(p, p, 1, 4, 32769, p, s) == UNSUPPORTED
    assert lib.mbv_mask_nms(p, p, p, p, 1, 1025, 1, 2, 1, p, p, s) == UNSUPPORTED
    assert lib.mbv_overlap_filter(p, p, p, 1, 8, 8, 1025, 4, 5, 1, p, p, s) == UNSUPPORTED
    assert lib.mbv_overlap_filter(p, p, p, 1, 1024, 1025, 4, 4, 5, 1, p, p, s) == UNSUPPORTED
    # null pointers, negative sizes, ratios
    assert lib.mbv_mask_self_overlap(null, p, 1, 4, 2, p, s) == BAD_ARG
    assert lib.mbv_mask_self_overlap(p, null, 1, 4, 2, p, s) == BAD_ARG
    assert lib.mbv_mask_self_overlap(p, p, 1, 4, 2, null, s) == BAD_ARG
    assert lib.mbv_mask_self_overlap(p, p, -1, 4, 2, p, s) == BAD_ARG
    assert lib.mbv_mask_self_overlap(p, p, 1, -4, 2, p, s) == BAD_ARG
    assert lib.mbv_mask_self_overlap(p, p, 1, 4, -2, p, s) == BAD_ARG
    for k in range(6):
        args = [p, p, p, p, 1, 4, 1, 2, 1, p, p]
        args[k if k < 4 else k + 5] = null
        assert lib.mbv_mask_nms(*args, s) == BAD_ARG, k
    assert lib.mbv_mask_nms(p, p, p, p, -1, 4, 1, 2, 1, p, p, s) == BAD_ARG
    for num, den in ((0, 2), (3, 2), (1, 65536), (-1, 2), (1, 0)):
        assert lib.mbv_mask_nms(p, p, p, p, 1, 4, num, den, 1, p, p, s) == BAD_ARG, (num, den)
    for k in (0, 1, 2, 10, 11):
        args = [p, p, p, 1, 8, 8, 4, 4, 5, 1, p, p]
        args[k] = null
        assert lib.mbv_overlap_filter(*args, s) == BAD_ARG, k
    for bad in (dict(b=-1), dict(h=0), dict(w=-3), dict(num=-1), dict(num=6), dict(den=65536), dict(den=0), dict(cells=-1)):
        a = dict(dict(b=1, h=8, w=8, num=4, den=5, cells=1), **bad)
        assert lib.mbv_overlap_filter(p, p, p, a['b'], a['h'], a['w'], 4, a['num'], a['den'], a['cells'], p, p, s) == BAD_ARG, bad
    torch.cuda.synchronize()
    assert not t.any()                                                      # a refused call writes nothing
    # Q = 1024 is accepted: 8 x 8 maps, half of them kept
    rng = np.random.default_rng(3)
    q, h, w = 1024, 8, 8
    masks = rng.random((1, q, h, w)) < 0.3
    masks[0, 1::2] = masks[0, 0::2]                                         # every odd query duplicates its predecessor
    keep = rng.random((1, q)) < 0.5
    scores = rng.random((1, q)).astype(np.float32)
    labels = np.ones((1, q), np.int32)
    rc, inter = call_self_overlap(lib, device, pack(lib, masks.reshape(-1, h, w)), keep, q, lib.mbv_packed_mask_words(h, w))
    assert rc == 0 and np.array_equal(inter, np_inter(masks, keep))
    rc, keep_out, by = call_nms(lib, device, inter, scores, labels, keep, 1, 2, 1)
    k1, sup = R.nms(inter[0].tolist(), scores[0], labels[0].tolist(), keep[0].tolist(), (1, 2), True)
    assert rc == 0 and keep_out[0].tolist() == [int(v) for v in k1] and by[0].tolist() == sup
    imap = rng.integers(-1, q, (1, h, w)).astype(np.int32)
    areas = masks.reshape(1, q, -1).sum(2).astype(np.int32)
    rc, keep_out, owned, new = call_filter(lib, device, imap, areas, np.asarray([k1]), 1, 20, 1)
    k2, own, want = R.overlap_filter(imap[0].tolist(), areas[0].tolist(), k1, (1, 20), 1)
    assert rc == 0 and keep_out[0].tolist() == [int(v) for v in k2] and owned[0].tolist() == own
    assert np.array_equal(new[0], np.asarray(want, dtype=np.int32))


def test_ops_wrappers_check_their_arguments(device):
    from mask_bev_amd import ops
    keep = torch.ones((2, 4), dtype=torch.bool, device=device)
    pm = ops.PackedMasks(torch.zeros((8, 2), dtype=torch.int32, device=device), 8, 8)
    inter = ops.mask_self_overlap(pm, keep)
    assert inter.shape == (2, 4, 4) and inter.dtype == torch.int32 and not inter.any()
    scores, labels = torch.rand((2, 4), device=device), torch.ones((2, 4), dtype=torch.int32, device=device)
    k1, by = ops.mask_nms(inter, scores, labels, keep)
    assert k1.dtype == torch.bool and k1.all() and (by == -1).all()
    imap = torch.zeros((2, 8, 8), dtype=torch.int32, device=device)
    k2, owned = ops.overlap_filter(imap, torch.full((2, 4), 64, dtype=torch.int32, device=device), k1, (4, 5), 1)
    assert k2.tolist() == [[True, False, False, False]] * 2 and owned.tolist() == [[64, 0, 0, 0]] * 2
    E = ops.MaskBevHipError
    for bad in (lambda: ops.mask_self_overlap(pm, keep[:, :3]), lambda: ops.mask_self_overlap(pm, keep.int()),
                lambda: ops.mask_self_overlap(ops.PackedMasks(pm.words, 9, 8), keep),
                lambda: ops.mask_nms(inter[:, :3], scores, labels, keep), lambda: ops.mask_nms(inter, scores.double(), labels, keep),
                lambda: ops.mask_nms(inter, scores, labels.long(), keep), lambda: ops.mask_nms(inter, scores, labels, keep, iou=(3, 2)),
                lambda: ops.mask_nms(inter, scores, labels, keep, iou=0.5), lambda: ops.mask_nms(inter.cpu(), scores, labels, keep),
                lambda: ops.overlap_filter(imap.long(), owned, k1), lambda: ops.overlap_filter(imap[:1], owned, k1),
                lambda: ops.overlap_filter(imap, owned, k1, (0, 1)), lambda: ops.overlap_filter(imap, owned, k1, (4, 5), -1),
                lambda: ops.overlap_filter(imap.permute(0, 2, 1)[:, :, ::2], owned, k1)):
        with pytest.raises(E):
            bad()


def _duplicated_inputs(b, q, h, w, seed):
    """Random decoder outputs with near-duplicates: query 3k + 1 repeats query 3k's map and class logits but for a little noise."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(b, q, 3, generator=g) * 2
    cls[..., 0] -= 1.5                                                       # most queries are kept
    logits = torch.randn(b, q, h, w, generator=g) * 3
    smooth = torch.nn.functional.interpolate(torch.randn(b, q, max(h // 4, 1), max(w // 4, 1), generator=g) * 4, (h, w),
                                             mode='bilinear', align_corners=False)
    logits = smooth + 0.3 * logits - 1.0
    for k in range(0, q - 1, 3):
        logits[:, k + 1] = logits[:, k] + 0.05 * torch.randn(b, h, w, generator=g)
        cls[:, k + 1] = cls[:, k] + 0.01 * torch.randn(b, 3, generator=g)
    return cls, logits


E2E = [(3, 7, 9, 7, 36, 28), (2, 70, 16, 16, 64, 64)]
SETTINGS = [dict(), dict(nms_iou=(3, 10), min_overlap=(1, 4), min_cells=2, same_label=False), dict(nms_iou=None, min_overlap=(1, 2)),
            dict(min_overlap=None, min_cells=3), dict(nms_iou=(1, 3), min_overlap=(1, 5), exclusive=True)]


@pytest.mark.parametrize('shape', E2E, ids=lambda c: 'x'.join(map(str, c)))
def test_extract_instances_resolve(device, shape):
    """End to end on random logits a quarter of the grid: K21's own outputs are taken as given; keep, suppressed_by, owned and
    the map equal the composition of the plain loops, fed the device's masks and the device's rebuilt map."""
    from mask_bev_amd import ops
    from mask_bev_amd.predict import ResolveSettings, extract_instances, unpack_bits
    b, q, h, w, H, W = shape
    cls, logits = _duplicated_inputs(b, q, h, w, seed=q)
    cls, logits = cls.to(device), logits.to(device)
    labels, scores, keep = ops.select_queries(cls, 0.0)
    base = ops.extract_masks(logits, scores, keep, (H, W))
    plain = extract_instances(cls, logits, (H, W))
    # resolve=None: today's outputs, bit for bit, and no new field
    assert plain.suppressed_by is None and plain.owned is None
    assert torch.equal(plain.keep, keep) and torch.equal(plain.masks.words, base['masks'].words)
    assert torch.equal(plain.instance_map, base['instance_map']) and torch.equal(plain.areas, base['areas'])
    assert plain.mask_scores.cpu().numpy().tobytes() == base['mask_scores'].cpu().numpy().tobytes()
    dense = unpack_bits(base['masks'].words, H, W).cpu().numpy().reshape(b, q, H, W)
    suppressed = dropped = 0
    for kw in SETTINGS:
        s = ResolveSettings(**kw)
        got = extract_instances(cls, logits, (H, W), resolve=s)
        assert got.keep.dtype == torch.bool and got.suppressed_by.dtype == torch.int32 and got.owned.dtype == torch.int32
        assert torch.equal(got.labels, labels) and torch.equal(got.scores, scores) and torch.equal(got.mask_scores, base['mask_scores'])
        for f in range(b):
            def rebuilt(keep1, f=f):
                k1 = torch.tensor([keep1], dtype=torch.bool, device=device)
                return ops.extract_masks(logits[f:f + 1], scores[f:f + 1], k1, (H, W), masks=False)['instance_map'][0].cpu().tolist()
            want = R.resolve(dense[f].tolist(), scores[f].cpu().numpy(), labels[f].tolist(), keep[f].tolist(), rebuilt, s.nms_iou,
                             s.min_overlap, s.min_cells, s.same_label)
            assert got.keep[f].tolist() == want['keep'] and got.suppressed_by[f].tolist() == want['suppressed_by'], (kw, f)
            assert got.owned[f].tolist() == want['owned'] and got.instance_map[f].cpu().tolist() == want['instance_map'], (kw, f)
            suppressed += sum(1 for v in want['suppressed_by'] if v >= 0)
            dropped += sum(1 for a, c in zip(want['keep1'], want['keep']) if a and not c)
        if not s.exclusive:
            assert torch.equal(got.masks.words, base['masks'].words) and torch.equal(got.areas, base['areas'])
            continue
        bits = unpack_bits(got.masks.words, H, W).reshape(b, q, H, W)
        assert int(bits.sum(1).max()) <= 1                                   # pairwise disjoint
        qs = torch.arange(q, device=device).view(1, q, 1, 1)
        assert torch.equal(bits, got.instance_map.unsqueeze(1) == qs)        # bit (y, x) of row q iff the map says q
        assert torch.equal(got.areas[got.keep], got.owned[got.keep]) and not got.areas[~got.keep].any()
    assert suppressed > 0 and dropped > 0                                    # both stages decided something
    for bad in (dict(masks=False), dict(instance_map=False)):
        with pytest.raises(ValueError):
            extract_instances(cls, logits, (H, W), resolve=ResolveSettings(), **bad)


def test_graphed_predict_with_resolve(device):
    """Every stage sits inside the captured graph: a replay equals eager predict on two different inputs."""
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.predict import GraphedPredictStep, ResolveSettings
    torch.manual_seed(0)
    kw = dict(tiny_kwargs(nx=96, ny=96, q=8), compute_dtype='fp32')
    m = MaskBevModule(**kw).to(device).train()
    m.log_scalars = False
    s = ResolveSettings(nms_iou=(1, 4), min_overlap=(1, 4), min_cells=2)
    batches_ = [[x.to(device) for x in random_scans(kw, sizes, seed=k)] for k, sizes in enumerate([[3000, 2500], [1200, 4100]])]
    g = GraphedPredictStep(m, batches_[0], resolve=s)
    plain = GraphedPredictStep(m, batches_[0])
    for scans in batches_[::-1]:
        got = g.step(scans).clone()
        want = m.predict(scans, resolve=s)
        for name in ('labels', 'keep', 'suppressed_by', 'owned', 'instance_map', 'areas'):
            assert torch.equal(getattr(got, name), getattr(want, name)), name
        assert torch.equal(got.masks.words, want.masks.words) and torch.allclose(got.scores, want.scores, rtol=1e-6, atol=0)
        old = plain.step(scans)
        assert old.suppressed_by is None and old.owned is None
        assert not (got.keep & ~old.keep).any()                              # resolving only ever removes
    g.close()
    plain.close()


def test_launcher_predict_resolve_keys(device, tmp_path, capsys, monkeypatch):
    """``predict_resolve: true`` on ``--test``: every prediction of the extra passes is made with the settings of the keys, and one
    ``resolved predictions: ..`` line says so; without the key ``predict`` is called as before and the line is absent."""
    import yaml
    import train_mask_bev_amd as launcher
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.predict import ResolveSettings
    from tests import track_ref as TR
    kw = tiny_kwargs()
    torch.manual_seed(0)
    model = MaskBevModule(**kw).to(device)
    model.log_scalars = False
    seq = tmp_path / 'data' / 'sequences' / '08'
    for sub in ('velodyne', 'mask_cache', 'labels'):
        (seq / sub).mkdir(parents=True)
    for i, sc in enumerate(random_scans(kw, [1500, 1201, 900, 700], seed=3)):
        sc.numpy().tofile(seq / 'velodyne' / f'{i:06d}.bin')
        imap = np.zeros((80, 80), dtype=np.int32)
        imap[10:22, 10:19], imap[40:52, 30:39] = 1, 2
        np.save(seq / 'mask_cache' / f'{i:06d}.npy', imap)
        words = np.full(sc.shape[0], (3 << 16) | 10, np.uint32)
        words[::4] = 40
        words.astype('<u4').tofile(seq / 'labels' / f'{i:06d}.label')
    tr = np.array([[0.0, -1.0, 0.0, 0.1], [0.0, 0.0, -1.0, -0.2], [1.0, 0.0, 0.0, 0.3], [0.0, 0.0, 0.0, 1.0]])
    cam = [tr @ TR.pose_2d(0.3 * k, 0.05 * k, 0.01 * k) @ np.linalg.inv(tr) for k in range(4)]
    np.savetxt(seq / 'poses.txt', np.stack([p[:3].reshape(-1) for p in cam]))
    (seq / 'calib.txt').write_text('P0: ' + ' '.join(['0'] * 12) + '\nTr: ' + ' '.join(repr(float(v)) for v in tr[:3].reshape(-1)) + '\n')
    base = dict(kw, dataset='semantic-kitti', batch_size=2, val_sequences=[8], train_sequences=[8], panoptic_min_points=1,
                track_instances=True, track_min_cells=2, track_max_tracks=32)
    base = {k: (list(v) if isinstance(v, tuple) else v) for k, v in base.items()}
    ck = tmp_path / 'ckpt' / 'tiny'
    ck.mkdir(parents=True)
    launcher.save_checkpoint(model, model.configure_optimizers()['optimizer'], ck / 'tiny-epoch=00-val_loss=1.000000.ckpt', 0,
                             'val_loss', 1.0)
    argv = ['--config', str(tmp_path / 'tiny.yml'), '--test', '--data-root', str(tmp_path / 'data'), '--checkpoint-root',
            str(tmp_path / 'ckpt'), '--render', str(tmp_path / 'frames')]
    calls = []
    real = MaskBevModule.predict

    def spy(self, *args, **kwargs):
        out = real(self, *args, **kwargs)
        calls.append((kwargs, out.suppressed_by is not None and out.owned is not None))
        return out

    monkeypatch.setattr(MaskBevModule, 'predict', spy)
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(base))
    assert launcher.main(argv) == 0
    out = capsys.readouterr().out
    assert len(calls) >= 6 and all(kwargs == {} and not resolved for kwargs, resolved in calls)     # 3 passes of 2 batches
    assert 'resolved predictions' not in out and 'point PQ' in out and 'point LSTQ' in out
    plain_calls, calls[:] = len(calls), []
    keys = dict(predict_resolve=True, predict_nms_iou=[1, 3], predict_min_overlap=[1, 2], predict_min_cells=2,
                predict_exclusive_masks=True)
    (tmp_path / 'tiny.yml').write_text(yaml.safe_dump(dict(base, **keys)))
    assert launcher.main(argv) == 0
    out = capsys.readouterr().out
    want = ResolveSettings(nms_iou=(1, 3), min_overlap=(1, 2), min_cells=2, exclusive=True)
    assert len(calls) == plain_calls and all(kwargs == dict(resolve=want) and resolved for kwargs, resolved in calls)
    assert out.count('resolved predictions: nms_iou 1/3, min_overlap 1/2, min_cells 2, exclusive masks') == 1
    assert 'point PQ' in out and 'point LSTQ' in out
