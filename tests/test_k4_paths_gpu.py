"""K4 (ops.window_attention) in bf16 and fp16 against the float64 window attention on the CPU (ref_window_attention of
test_k4_window_attn_gpu.py in float64, autograd for the gradients), on the inputs as the dtype holds them.

Every comparison prints ``max|got - ref64| / max|ref64|`` per tensor — the output, d(qkv), d(qkv_bias), d(bias_table) —
and its bar, ``max(one output rounding, 2 x e_emul)``: e_emul is the error against float64 of the kernel emulated in
torch — the same function, float64 everywhere except at the points where csrc/window_attn.hip rounds to the dtype:

  forward (k_window_attn_fwd)
    * q, k, v of a real token are 16-bit operands (the input); a padded token's q, k, v are the f32 qkv bias ROUNDED to the
      dtype while staging (pad_pack / stage_part_swz) — its gradient passes through to the f32 bias;
    * the normalised probabilities P = exp2(s - m) / sum are rounded as the operand of O = P V (mma_acc_tr);
    * the output is stored in the dtype.
  backward (k_window_attn_bwd)
    * dO is a 16-bit operand (exact here: the test's dO is a 16-bit tensor), zero on padded tokens;
    * delta = sum_d dO O reads the STORED (rounded) output;
    * P = exp2(s + bias - lse) is rounded as the operand of dV = P^T dO;
    * dS scale = P (dP - delta) scale is rounded as the operand of dQ = dS K and dK = dS^T Q; the bias-table gradient adds
      the UNROUNDED dS (f64 in LDS, f32 atomics per table entry);
    * d(qkv) of a real token is stored in the dtype; a padded token's dQ, dK, dV rows are summed UNROUNDED (f32
      accumulators, f64 in LDS) into the f32 qkv-bias gradient.
  Scores, the relative-position bias and the shift mask, maxima and sums, lse and delta stay in f32 on the device and in
  float64 in the emulation.  The factor 2 covers summation order and f32 accumulation.  d(qkv_bias) and d(bias_table) get
  the same relative bar as the rest.

Bars of the cases here — also in DESIGN.md §2:
  bf16: out 7.2e-3 … 9.1e-3, d(qkv) 6.9e-3 … 8.4e-3, d(qkv_bias) 3.9e-3, d(bias_table) 3.9e-3 … 4.6e-3;
  fp16: out 9.2e-4 … 1.1e-3, d(qkv) 9.2e-4 … 9.8e-4, d(qkv_bias) 4.9e-4 … 5.9e-4, d(bias_table) 4.9e-4 … 8.2e-4;
  d(qkv_bias) of a map without padded tokens is zero throughout and must come out as exact zeros
  (the earlier bounds: 2e-2 on the output, 6e-2 absolute on d(qkv), 3e-2 of max(1, max|g|) on the parameter gradients).
The module has not run on an MI355X yet: the device's errors are not in this table, and every line ``err … bar …`` the
tests print is the measurement to copy here.
"""
import pytest
import torch

from oracle import maskbev_oracle as O
from tests.f64_bars import LO, NAME, ROUNDING, RoundGrad, RoundValue, check, err, rd
from tests.test_k4_window_attn_gpu import ref_window_attention

MOD = 'k4-paths'

# B, H, W, heads, D, ws, shift
CASES = [
    (1, 23, 30, 3, 32, 10, 5),      # the production class: 100-token windows, padding on both axes
    (2, 20, 20, 2, 64, 10, 0),
    (1, 13, 9, 3, 16, 4, 2),
    (1, 7, 7, 1, 32, 7, 3),
    (1, 4, 4, 2, 32, 10, 5),        # a map smaller than the window: the last stage of the 124 x 108 grid
]
KEYS = ('out', 'd_qkv', 'd_bias', 'd_table')


def _err(got, ref):
    """Relative max-norm error; a reference that is zero throughout (d(qkv_bias) of a map without padded tokens) asks for exact
    zeros: the error is then max|got| against a bar of 0."""
    if float(ref.abs().max()) == 0.0:
        return float(got.detach().double().abs().max())
    return err(got, ref)


class _EmuCore(torch.autograd.Function):
    """softmax(q k^T scale + add) v of every (window, head) with the kernel's roundings (module docstring)."""

    @staticmethod
    def forward(ctx, q, k, v, add, scale, dt):
        p = (q @ k.transpose(-2, -1) * scale + add).softmax(-1)
        out = rd(rd(p, dt) @ v, dt)
        ctx.save_for_backward(q, k, v, p, out)
        ctx.scale, ctx.dt = scale, dt
        return out

    @staticmethod
    def backward(ctx, go):
        q, k, v, p, out = ctx.saved_tensors
        delta = (go * out).sum(-1, keepdim=True)
        ds = p * (go @ v.transpose(-2, -1) - delta)
        dsr, pr = rd(ds * ctx.scale, ctx.dt), rd(p, ctx.dt)
        return dsr @ k, dsr.transpose(-2, -1) @ q, pr.transpose(-2, -1) @ go, ds, None, None


def emu_window_attention(qkv, qkv_bias, table, heads, ws, shift, dt):
    """ref_window_attention with the rounding points inserted."""
    b, h, w, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    pad_b, pad_r = (ws - h % ws) % ws, (ws - w % ws) % ws
    hp, wp = h + pad_b, w + pad_r
    full = RoundValue.apply(qkv_bias, dt).view(1, 1, 1, c3).expand(b, hp, wp, c3).clone()      # padded tokens: rounded bias
    full[:, :h, :w] = RoundGrad.apply(qkv, dt)                                                  # real tokens: d(qkv) is stored
    mask = None
    if shift:
        full = torch.roll(full, shifts=(-shift, -shift), dims=(1, 2))
        img = torch.zeros((1, hp, wp, 1))
        sl = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
        cnt = 0
        for a in sl:
            for bb in sl:
                img[:, a, bb, :] = cnt
                cnt += 1
        mw = O._window_partition(img, ws).view(-1, ws * ws)
        mask = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = mask.masked_fill(mask != 0, -100.0).masked_fill(mask == 0, 0.0).to(qkv.dtype)
    win = O._window_partition(full, ws).view(-1, ws * ws, 3, heads, d).permute(2, 0, 3, 1, 4)
    bias = table[O.rel_position_index(ws).view(-1)].view(ws * ws, ws * ws, heads).permute(2, 0, 1)
    add = bias.unsqueeze(0).expand(win.shape[1], heads, ws * ws, ws * ws)
    if mask is not None:
        nw = mask.shape[0]
        add = (add.reshape(b, nw, heads, ws * ws, ws * ws) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, ws * ws, ws * ws)
    out = _EmuCore.apply(win[0], win[1], win[2], add, d ** -0.5, dt).transpose(1, 2).reshape(-1, ws, ws, c)
    out = O._window_reverse(out, hp, wp, ws)
    if shift:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    return out[:, :h, :w].contiguous()


def _inputs(case, dt):
    B, H, W, heads, D, ws, shift = case
    g = torch.Generator().manual_seed(H * 31 + W + shift)
    C = heads * D
    qkv = torch.randn(B, H, W, 3 * C, generator=g)
    bias = torch.randn(3 * C, generator=g) * 0.5
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    go = torch.randn(B, H, W, C, generator=g)
    return qkv.to(dt).double(), bias.double(), table.double(), go.to(dt).double()      # parameters stay f32 values


def _evaluate(fn, qkv, bias, table, go):
    q, b, t = (x.clone().requires_grad_() for x in (qkv, bias, table))
    out = fn(q, b, t)
    out.backward(go)
    return dict(out=out.detach(), d_qkv=q.grad, d_bias=b.grad, d_table=t.grad)


_CACHE = {}


def _case(case, dt):
    key = (case, dt)
    if key not in _CACHE:
        heads, ws, shift = case[3], case[5], case[6]
        qkv, bias, table, go = _inputs(case, dt)
        ref = _evaluate(lambda q, b, t: ref_window_attention(q, b, t, heads, ws, shift), qkv, bias, table, go)
        emu = _evaluate(lambda q, b, t: emu_window_attention(q, b, t, heads, ws, shift, dt), qkv, bias, table, go)
        _CACHE[key] = (qkv, bias, table, go, ref, {k: _err(emu[k], ref[k]) for k in KEYS})
    return _CACHE[key]


def test_cpu_emulation_without_roundings_is_the_reference():
    """With float64 as the 'dtype' every rounding is the identity: the emulation (its hand-written backward included) must
    then equal float64 autograd of the reference."""
    for case in CASES:
        heads, ws, shift = case[3], case[5], case[6]
        qkv, bias, table, go = _inputs(case, torch.bfloat16)
        ref = _evaluate(lambda q, b, t: ref_window_attention(q, b, t, heads, ws, shift), qkv, bias, table, go)
        emu = _evaluate(lambda q, b, t: emu_window_attention(q, b, t, heads, ws, shift, torch.float64), qkv, bias, table, go)
        for k in KEYS:
            assert _err(emu[k], ref[k]) < 1e-12, (case, k, _err(emu[k], ref[k]))


@pytest.mark.parametrize('dt', LO)
def test_cpu_emulation_has_an_error_of_its_own(dt):
    for case in CASES:
        *_, ref, e_emul = _case(case, dt)
        padded = case[1] % case[5] != 0 or case[2] % case[5] != 0
        assert padded == (float(ref['d_bias'].abs().max()) > 0.0)
        for k, v in e_emul.items():
            assert (0.0 < v < 0.25) if (padded or k != 'd_bias') else v == 0.0, (case, dt, k, v)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', LO)
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(str(i) for i in c))
def test_window_attention_16bit_against_float64(device, capsys, case, dt):
    from mask_bev_amd import ops
    B, H, W, heads, D, ws, shift = case
    qkv, bias, table, go, ref, e_emul = _case(case, dt)
    q_d = qkv.to(device=device, dtype=dt).requires_grad_()
    b_d = bias.float().to(device).requires_grad_()
    t_d = table.float().to(device).requires_grad_()
    out = ops.window_attention(q_d, b_d, t_d, heads, ws, shift)
    assert out.dtype == dt and out.shape == (B, H, W, heads * D)
    out.backward(go.to(device=device, dtype=dt))
    torch.cuda.synchronize()
    got = dict(out=out, d_qkv=q_d.grad, d_bias=b_d.grad, d_table=t_d.grad)
    bad = []
    for k in KEYS:
        zero = float(ref[k].abs().max()) == 0.0                   # d(qkv_bias) without padded tokens: exact zeros
        bar = 0.0 if zero else max(ROUNDING[dt], 2.0 * e_emul[k])
        check(capsys, MOD, f'{NAME[dt]} {case} {k}', _err(got[k], ref[k]), bar, bad)
    assert not bad, bad
