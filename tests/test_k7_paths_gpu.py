"""K7 (ops.mask_logits: the contraction on each of its three routes, the f32 output slot the decoder passes, and the
attention mask mbv_attn_mask_from_logits derives from the logits the op itself returns) against float64 on the CPU.

Every comparison prints ``max|got - ref64| / max|ref64|`` and its bar.  References are evaluated on the operands as the
dtype holds them; gradients by float64 autograd.  Bars:

* f32-accumulated logits stored in f32 (16-bit operands into an f32 slot; the f32 route; mbv_mask_logits_fwd with the
  f32 flag, the direct C-ABI test of k_mask_logits_f32): ``max(4e-6, 4 x e32)``, e32 the error of the same product
  evaluated in float32 on the CPU, per case and tensor.
* 16-bit stored logits and gradients (no slot; dE is an f32 product cast once, dF a 16-bit store of f32 sums): one
  rounding of the float64 value to the dtype, per element, plus the f32 bar — printed as the error beyond one rounding.
* The mask: expected = float64 restatement of upsample_bilinear2d(align_corners=False) of the RETURNED logits ->
  sigmoid < 0.5 -> rows that would block every key unblocked.  The source coordinates are the operator's float32 values
  (scale = H / h and scale * (o + 0.5) - 0.5 are float32 by the operator's definition; the product and the subtraction
  round once, as the kernel's fused multiply-add does); the complements, taps and sums are float64.  A pixel may
  disagree only where |v64| <= 8 * 2^-24 * max|its four taps|; the share of such pixels is asserted <= 1e-3.

Routes of _MaskLogits.forward are asserted with counters on the library's entry points and torch.bmm: mbv_gemm16_nn
(C % 8 == 0 and HW % 8 == 0), K7's own 16-bit kernel mbv_mask_logits_fwd (odd HW, C % 16 == 0), torch.bmm (f32).

Bars of the cases here — also in DESIGN.md §2: every f32 bar is 4e-6 (4 x e32 <= 3e-7: C <= 272); 16-bit stores add one
rounding (bf16 2^-8, fp16 2^-11 of the value).  The module has not run on an MI355X yet: the device's errors are not in this
table, and every line ``err … bar …`` the tests print is the measurement to copy here.
"""
import pytest
import torch

from tests.f64_bars import LO, NAME, check, err, err_beyond_one_rounding, f32_bar

MOD = 'k7-paths'
SENTINEL = 0x7FC12345           # a NaN payload: no kernel writes it, and no float compares equal to it
BAND = 8 * 2.0 ** -24
BAND_SHARE_CAP = 1e-3

# (B, Q, C, H, W): Q in {1, 31, 33, 130} around the 32-query blocks, HW in {8, 775, 128 k + 1} for the pixel tail,
# C in {16, 48, 256, 272} for the contraction tail (K7 stages 256 channels per pass; C = 272 leaves 16)
_GEMM16 = [(2, 1, 272, 2, 4), (2, 33, 48, 2, 4), (1, 130, 256, 16, 24), (2, 31, 16, 8, 9)]
_OWN = [(2, 1, 256, 5, 5), (2, 33, 48, 25, 31), (1, 130, 272, 3, 43), (2, 31, 16, 1, 257)]
_F32 = [(2, 33, 48, 25, 31), (1, 130, 272, 2, 4), (2, 1, 16, 3, 43)]


def _operands(shape, dt, seed):
    """embed / feature / d(logits) as ``dt`` holds them (float32 tensors on the CPU), with a zero query row."""
    B, Q, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    embed = torch.randn(B, Q, C, generator=g) / C ** 0.5
    feat = torch.randn(B, C, H, W, generator=g)
    go = torch.randn(B, Q, H, W, generator=g)
    embed[0, 0] = 0.0
    if dt != torch.float32:
        go = go.to(torch.bfloat16).float()  # exact in bf16 AND fp16: neither the slot's f32 gradient nor its 16-bit cast rounds
        go[go.abs() < 2.0 ** -14] = 0.0
    return tuple(t.to(dt).float() for t in (embed, feat, go))


_REF = {}


def _reference(shape, dt, seed):
    """float64 product and autograd gradients, and the float32 evaluation's error against them per tensor."""
    key = (shape, dt, seed)
    if key not in _REF:
        embed, feat, go = _operands(shape, dt, seed)
        res = {}
        for fdt in (torch.float64, torch.float32):
            # clone: .to(float32) of a float32 tensor is the tensor itself, and the cached operands must stay plain leaves
            e, f = embed.to(fdt).clone().requires_grad_(), feat.to(fdt).clone().requires_grad_()
            lg = torch.einsum('bqc,bchw->bqhw', e, f)
            lg.backward(go.to(fdt))
            res[fdt] = dict(logits=lg.detach(), d_embed=e.grad, d_feat=f.grad)
        r64, r32 = res[torch.float64], res[torch.float32]
        _REF[key] = (embed, feat, go, r64, {k: f32_bar(r32[k], r64[k]) for k in r64}, {k: err(r32[k], r64[k]) for k in r64})
    return _REF[key]


def test_cpu_references_have_an_error_of_their_own():
    """Every e32 the bars are built from is non-zero (the float32 evaluation is a different computation from float64) — but
    d(feature) of ONE query with 16-bit operands, which is one product of two 16-bit values per element: exact in float32."""
    for shape in _GEMM16 + _OWN + _F32:
        for dt in (torch.float32,) + LO:
            embed, feat, go, *_, e32 = _reference(shape, dt, 7)
            assert not (embed.requires_grad or feat.requires_grad or go.requires_grad)      # plain data: the device copies are leaves
            exact = {'d_feat'} if (shape[1] == 1 and dt != torch.float32) else set()
            assert all((v > 0.0) != (k in exact) for k, v in e32.items()), (shape, dt, e32)


class _Routes:
    """Counts the calls of the library's entry points (through the proxy's hook) and of torch.bmm."""

    def __init__(self, monkeypatch):
        from mask_bev_amd import _lib
        self.n = {}
        lib = _lib.load()

        def hook(name, fn, args):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*args)

        bmm = torch.bmm

        def counted_bmm(*a, **k):
            self.n['torch.bmm'] = self.n.get('torch.bmm', 0) + 1
            return bmm(*a, **k)

        monkeypatch.setattr(lib, 'hook', hook)
        monkeypatch.setattr(torch, 'bmm', counted_bmm)

    def forward_route(self):
        names = ('mbv_gemm16_nn', 'mbv_mask_logits_fwd', 'torch.bmm')
        return {k: self.n.get(k, 0) for k in names}


def _stack(device, shape, index=1, depth=3):
    B, Q, C, H, W = shape
    buf = torch.empty(depth, B, Q, H, W, dtype=torch.float32, device=device)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf, buf[index]


def _run(device, monkeypatch, capsys, shape, dt, slot, route):
    from mask_bev_amd import ops
    embed, feat, go, r64, bars, _ = _reference(shape, dt, 7)
    e_d = embed.to(device=device, dtype=dt).requires_grad_()
    f_d = feat.to(device=device, dtype=dt).requires_grad_()
    buf = out = None
    if slot:
        buf, out = _stack(device, shape)
    with monkeypatch.context() as patch:
        routes = _Routes(patch)
        logits, blocked = ops.mask_logits(e_d, f_d, (shape[3], shape[4]), out=out)
        ran = routes.forward_route()
    assert ran == {k: int(k == route) for k in ran}, ran
    logits.backward(go.to(device=device, dtype=logits.dtype))
    torch.cuda.synchronize()
    tag = f'{NAME[dt]} {shape} slot={int(slot)} {route}'
    bad = []
    if slot:
        assert logits.dtype == torch.float32 and logits.data_ptr() == out.data_ptr()
        raw = buf.view(torch.int32)
        assert bool((raw[0] == SENTINEL).all()) and bool((raw[2] == SENTINEL).all())      # the other slices are untouched
        assert bool(torch.isfinite(buf[1]).all())                                          # every element of the slot written
    else:
        assert logits.dtype == dt
    if logits.dtype == torch.float32:
        check(capsys, MOD, f'{tag} logits', err(logits, r64['logits']), bars['logits'], bad)
    else:
        check(capsys, MOD, f'{tag} logits (beyond one rounding)', err_beyond_one_rounding(logits, r64['logits'], dt),
              bars['logits'], bad)
    assert bool((logits[0, 0] == 0).all())                                                 # the zero query row
    for k, got in (('d_embed', e_d.grad), ('d_feat', f_d.grad)):
        assert got.dtype == dt
        if dt == torch.float32:
            check(capsys, MOD, f'{tag} {k}', err(got, r64[k]), bars[k], bad)
        else:
            check(capsys, MOD, f'{tag} {k} (beyond one rounding)', err_beyond_one_rounding(got, r64[k], dt), bars[k], bad)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('slot', [False, True])
@pytest.mark.parametrize('dt', LO)
@pytest.mark.parametrize('shape', _GEMM16)
def test_gemm16_route_against_float64(device, monkeypatch, capsys, shape, dt, slot):
    """C % 8 == 0 and HW % 8 == 0: the batched NN product of K17 (mbv_gemm16_nn), 16-bit store or the f32 store into the slot."""
    _run(device, monkeypatch, capsys, shape, dt, slot, 'mbv_gemm16_nn')


@pytest.mark.gpu
@pytest.mark.parametrize('slot', [False, True])
@pytest.mark.parametrize('dt', LO)
@pytest.mark.parametrize('shape', _OWN)
def test_own_kernel_route_against_float64(device, monkeypatch, capsys, shape, dt, slot):
    """Odd HW: K7's own 16-bit kernel (k_mask_logits_bf16<256, lo16_t> and its f32-store form <256, float>)."""
    _run(device, monkeypatch, capsys, shape, dt, slot, 'mbv_mask_logits_fwd')


@pytest.mark.gpu
@pytest.mark.parametrize('slot', [False, True])
@pytest.mark.parametrize('shape', _F32)
def test_f32_route_against_float64(device, monkeypatch, capsys, shape, slot):
    """f32 operands: torch.bmm, into a fresh tensor or into the slot."""
    _run(device, monkeypatch, capsys, shape, torch.float32, slot, 'torch.bmm')


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 33, 48, 25, 31), (1, 130, 272, 3, 43), (2, 31, 16, 1, 257), (2, 1, 256, 2, 4)])
def test_f32_kernel_c_abi_against_float64(device, capsys, shape):
    """k_mask_logits_f32 (v_mfma_f32_32x32x2_f32) is not reachable from ops.mask_logits any more (f32 goes to torch.bmm): called
    through mbv_mask_logits_fwd with the f32 flag, into a sentinel-filled buffer, at the Q / HW / C tails."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    B, Q, C, H, W = shape
    embed, feat, _, r64, bars, _ = _reference(shape, torch.float32, 7)
    e_d, f_d = embed.to(device), feat.to(device)
    buf, out = _stack(device, shape)
    ops.check(lib.mbv_mask_logits_fwd(ops._ptr(e_d), ops._ptr(f_d), 0, B, Q, C, H * W, ops._ptr(out), 1, ops._stream()),
              'mbv_mask_logits_fwd')
    torch.cuda.synchronize()
    raw = buf.view(torch.int32)
    assert bool((raw[0] == SENTINEL).all()) and bool((raw[2] == SENTINEL).all()) and bool(torch.isfinite(out).all())
    bad = []
    check(capsys, MOD, f'k_mask_logits_f32 {shape} logits', err(out, r64['logits']), bars['logits'], bad)
    assert not bad, bad


@pytest.mark.gpu
def test_slot_checks(device):
    """A slot of the wrong shape, the wrong dtype or a non-contiguous layout is refused (MaskBevHipError); nothing is written."""
    from mask_bev_amd import ops
    from mask_bev_amd._lib import MaskBevHipError
    B, Q, C, H, W = 2, 5, 16, 4, 6
    e = torch.randn(B, Q, C, device=device).bfloat16()
    f = torch.randn(B, C, H, W, device=device).bfloat16()
    good = torch.zeros(B, Q, H, W, device=device)
    wrong = {
        'shape': torch.zeros(B, Q, W, H, device=device),
        'rows': torch.zeros(B, Q + 1, H, W, device=device),
        'dtype': torch.zeros(B, Q, H, W, device=device, dtype=torch.bfloat16),
        'layout': torch.zeros(B, Q, W, H, device=device).transpose(2, 3),
        'strided': torch.zeros(B, Q, H, 2 * W, device=device)[..., ::2],
    }
    for name, slot in wrong.items():
        assert name in ('shape', 'rows') or slot.shape == good.shape
        with pytest.raises(MaskBevHipError):
            ops.mask_logits(e, f, (H, W), out=slot)
        torch.cuda.synchronize()
        assert bool((slot == 0).all()), name
    logits, _ = ops.mask_logits(e, f, (H, W), out=good)
    assert logits.data_ptr() == good.data_ptr()


# ------------------------------------------------------------------------------------------------------------------
# the attention mask
# ------------------------------------------------------------------------------------------------------------------
def _source(n_in, n_out):
    """(i0, i1, weight of i1) of upsample_bilinear2d(align_corners=False) along one axis: float32 scale and source
    coordinate (one rounding for scale * (o + 0.5) - 0.5), as float64 tensors."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    o = torch.arange(n_out, dtype=torch.float32) + 0.5
    src = (scale.double() * o.double() - 0.5).float().clamp_min(0.0)          # the double product is exact: rounds once
    i0 = src.floor().long()
    i1 = i0 + (i0 < n_in - 1).long()
    return i0, i1, (src - i0.float()).double()


def expected_mask(logits, size):
    """logits (R, H, W) of any dtype on the CPU -> (blocked (R, h*w) bool, band (R, h*w) bool) in float64."""
    v = logits.double()
    R, H, W = v.shape
    h, w = size
    y0, y1, ly = _source(H, h)
    x0, x1, lx = _source(W, w)
    ly, lx = ly.view(1, h, 1), lx.view(1, 1, w)
    t00, t01 = v[:, y0][:, :, x0], v[:, y0][:, :, x1]
    t10, t11 = v[:, y1][:, :, x0], v[:, y1][:, :, x1]
    r = (1 - ly) * ((1 - lx) * t00 + lx * t01) + ly * ((1 - lx) * t10 + lx * t11)
    blocked = (torch.sigmoid(r) < 0.5).flatten(1)
    blocked[blocked.all(-1)] = False
    taps = torch.stack([t00, t01, t10, t11]).abs().amax(0)
    band = (r.abs() <= BAND * taps).flatten(1)
    return blocked, band


# (B, Q, C, H, W, target): 4x down, identity, a non-integer ratio, up-sampling, 1 x 1; 63², 20 x 15 and 5 x 7 are no multiples
# of the kernel's 256 threads
_MASK_CASES = [(1, 33, 16, 32, 32, (8, 8)), (1, 6, 16, 16, 24, (16, 24)), (1, 5, 16, 125, 125, (63, 63)),
               (2, 7, 16, 8, 6, (20, 15)), (1, 4, 16, 8, 8, (1, 1)), (2, 3, 16, 16, 24, (5, 7))]
_MASK_SEED = 3


def test_cpu_mask_band_share_of_the_chosen_seed():
    """The band leaves out <= 1e-3 of the pixels of the float64 logits (as f32, bf16 and fp16 hold them) for the chosen seed."""
    for case in _MASK_CASES:
        for dt in (torch.float32,) + LO:
            *_, r64, _, _ = _reference(case[:5], dt, _MASK_SEED)
            for store in {torch.float32, dt}:
                lg = r64['logits'].to(store).flatten(0, 1)
                _, band = expected_mask(lg, case[5])
                nz = band & (lg.double().abs().amax((1, 2)) > 0).view(-1, 1)          # a zero row is all band, and exact
                assert float(nz.double().mean()) <= BAND_SHARE_CAP, (case, dt, store)


def _compare_mask(capsys, tag, blocked, logits, size, bad):
    exp, band = expected_mask(logits.detach().cpu().flatten(0, -3), size)
    got = blocked.cpu().view(exp.shape)
    zero_rows = (logits.detach().cpu().flatten(0, -3).double().abs().amax((1, 2)) == 0).view(-1, 1)
    band = band & ~zero_rows                                 # rows of exact zeros are exact: sigmoid(+-0) = 0.5, not blocked
    wrong = int(((got != exp) & ~band).sum())
    share = float(band.double().mean())
    check(capsys, MOD, f'{tag} mask: pixels that disagree outside the band', float(wrong), 0.0, bad)
    check(capsys, MOD, f'{tag} mask: share of pixels in the band', share, BAND_SHARE_CAP, bad)
    assert not bool(got.all(-1).any())


@pytest.mark.gpu
@pytest.mark.parametrize('slot', [False, True])
@pytest.mark.parametrize('dt', (torch.float32,) + LO)
def test_mask_from_the_returned_logits(device, capsys, dt, slot):
    """ops.mask_logits' mask against the float64 restatement applied to the logits the op returned (16-bit logits:
    k_attn_mask<lo16_t>; f32 logits and every slot: k_attn_mask<float>)."""
    from mask_bev_amd import ops
    bad = []
    for B, Q, C, H, W, size in _MASK_CASES:
        embed, feat, *_ = _reference((B, Q, C, H, W), dt, _MASK_SEED)
        out = _stack(device, (B, Q, C, H, W))[1] if slot else None
        logits, blocked = ops.mask_logits(embed.to(device=device, dtype=dt), feat.to(device=device, dtype=dt), size, out=out)
        torch.cuda.synchronize()
        assert blocked.shape == (B, 1, Q, size[0] * size[1]) and blocked.dtype == torch.bool
        assert logits.dtype == (torch.float32 if slot else dt)
        _compare_mask(capsys, f'{NAME[dt]} slot={int(slot)} {H}x{W}->{size[0]}x{size[1]}', blocked, logits, size, bad)
        assert not bool(blocked[0, 0, 0].any())              # the zero query: sigmoid(0) = 0.5 is not blocked
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('dt', (torch.float32,) + LO)
def test_mask_rows_with_a_rule(device, capsys, dt):
    """mbv_attn_mask_from_logits on logits with the rows the all-blocked rule and the 0.5 threshold decide: all negative (first
    row of the batch; comes out unblocked), all +0.0, all -0.0, one non-negative pixel (also the last row of the batch)."""
    from mask_bev_amd import _lib, ops
    lib = _lib.load()
    R, H, W = 9, 16, 24
    g = torch.Generator().manual_seed(11)
    lg = torch.randn(R, H, W, generator=g)
    neg = -(torch.rand(H, W, generator=g) + 0.125)
    lg[0] = neg
    lg[1] = 0.0
    lg[2] = -0.0
    lg[3] = neg
    lg[3, H - 1, W - 1] = 0.0                                 # exactly one non-negative pixel: the far corner, value +0.0
    lg[4] = neg
    lg[4, 5, 7] = 3.0
    lg[R - 1] = neg
    lg[R - 1, 0, 0] = 0.5
    lg = lg.to(dt)
    assert bool(torch.signbit(lg[2].float()).all()) and not bool(torch.signbit(lg[1].float()).any())
    l_d = lg.to(device)
    bad = []
    for size in ((H, W), (5, 7), (32, 48), (1, 1)):
        th, tw = size
        blocked = torch.ones(R, th * tw, dtype=torch.bool, device=device)
        ops.check(lib.mbv_attn_mask_from_logits(ops._ptr(l_d), ops._dt_flag(dt), R, H, W, th, tw, ops._ptr(blocked),
                                                ops._stream()), 'mbv_attn_mask_from_logits')
        torch.cuda.synchronize()
        _compare_mask(capsys, f'{NAME[dt]} rows {H}x{W}->{th}x{tw}', blocked, lg, size, bad)
        b = blocked.cpu()
        assert not bool(b[0].any()) and not bool(b[1].any()) and not bool(b[2].any())
        if size == (H, W):
            only = torch.ones(H, W, dtype=torch.bool)
            only[H - 1, W - 1] = False
            assert torch.equal(b[3].view(H, W), only)
            only = torch.ones(H, W, dtype=torch.bool)
            only[5, 7] = False
            assert torch.equal(b[4].view(H, W), only)
            only = torch.ones(H, W, dtype=torch.bool)
            only[0, 0] = False
            assert torch.equal(b[R - 1].view(H, W), only)
    assert not bad, bad
