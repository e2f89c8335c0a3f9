"""K6 (ops.attention) in bf16 and fp16 against float64 attention on the CPU (autograd for the gradients), on the inputs
as the dtype holds them.

Every comparison prints ``max|got - ref64| / max|ref64|`` per tensor and its bar,
``max(one output rounding, 2 x e_emul)``: e_emul is the error against float64 of the kernel emulated in torch — float64
everywhere except at the points where csrc/cross_attn.hip rounds to the dtype:

  forward (k_attn_fwd_split, k_attn_combine)
    * q, k, v are 16-bit operands of S = K Q^T (the inputs; nothing to round);
    * per 128-key split: P = exp2(s - m_split), un-normalised, relative to the SPLIT's running maximum, rounded as the
      operand of O_split = P V (mma_acc_tr: ``(lo16_t)x``); the split's sum l_split adds the unrounded P;
    * the output num / den (combine; o / l for a single split) is stored in the dtype.
  backward (k_attn_bwd)
    * dO is a 16-bit operand (the incoming gradient cast to the dtype — exact here, the test's dO is a 16-bit tensor);
    * delta = sum_d dO O reads the STORED (rounded) output;
    * P = exp2(s - lse) is rounded as the operand of dV = P^T dO;
    * dS = P (dP - delta) scale is rounded as the operand of dQ = dS K and dK = dS^T Q;
    * dQ, dK, dV leave the kernel in f32 and are cast to the dtype of q, k, v (ops_attention.py).
  Scores, running maxima and sums, lse, delta, the mask and the combine weights stay in f32 on the device and in float64
  in the emulation.  The factor 2 covers summation order and f32 accumulation.

Cases: the three production levels, the tile edges of Q and of the 128-key splits, the self-attention (no mask).  Every
masked case has a row with a single attendable key, a row whose whole first and whole last split are blocked (two
splits: the first; one split: the first key — blocking more would block the row) and a row with nothing blocked
(Q = 1, L = 129: batch 0 holds the single-key row, batch 1 the unblocked one — a blocked first split would leave one
key); keys are scaled per head up to logits of about +-40 (bf16) / +-20 (fp16); output gradients are scaled by 2^-8, 1 and 2^8.

dK of the key a single-key row attends to is a cancellation (dS = p (dP - delta) with p = 1 and dP = delta in exact
arithmetic: what is left is rounding noise of either side).  Those key rows are not dropped: there dK is compared with
the emulation's own value (same bar), everywhere else with float64.

Bars of the cases here (worst of the three dO scales) — also in DESIGN.md §2:
  bf16: out 3.9e-3 … 5.2e-3, dq 4.0e-3 … 1.6e-2, dk 4.7e-3 … 1.1e-2, dv 3.9e-3 … 7.5e-3;
  fp16: out 4.9e-4 … 7.5e-4, dq 8.6e-4 … 1.7e-3, dk 6.1e-4 … 1.9e-3, dv 4.9e-4 … 9.5e-4
  (the earlier bounds: 2e-2 absolute on outputs of magnitude 0.2 … 0.4, 6e-2 absolute on gradients).
The module has not run on an MI355X yet: the device's errors are not in this table, and every line ``err … bar …`` the
tests print is the measurement to copy here.
"""
import math

import pytest
import torch

from tests.f64_bars import LO, NAME, ROUNDING, check, err, rd
from tests.test_k6_attention_gpu import ref_attention

MOD = 'k6-paths'
SPLIT = 128
GSCALES = (2.0 ** -8, 1.0, 2.0 ** 8)

# B, Q, L, heads, D, masked
CASES = [(1, 100, 256, 8, 32, True), (1, 100, 1024, 8, 32, True), (1, 100, 4096, 8, 32, True),
         (2, 1, 129, 2, 64, True), (1, 129, 7, 4, 16, True), (2, 33, 300, 8, 32, True),
         (1, 100, 100, 8, 32, False)]
KMAX = {torch.bfloat16: 10.0, torch.float16: 5.0}


def _inputs(case, dt):
    B, Q, L, heads, D, masked = case
    g = torch.Generator().manual_seed(Q * 7 + L)
    E = heads * D
    q = torch.randn(B, Q, E, generator=g)
    k = torch.randn(B, L, E, generator=g) * torch.logspace(-2, math.log10(KMAX[dt]), heads).repeat_interleave(D)
    v = torch.randn(B, L, E, generator=g)
    go = torch.randn(B, Q, E, generator=g)
    blocked, single = None, []
    if masked:
        nsplit = (L + SPLIT - 1) // SPLIT
        blocked = torch.rand(B, Q, L, generator=g) < 0.7
        blocked[:, torch.arange(Q), torch.arange(Q) % L] = False          # no row is blocked as a whole
        # Q >= 3: rows 0, 1, 2 of every batch are the three kinds; Q = 1 (B = 2, L = 129): batch 0's only row is the single-key
        # row, batch 1's the unblocked one (a blocked first split would leave key 128 alone: the single-key row again)
        kinds = {(b, r): r for b in range(B) for r in range(3)} if Q >= 3 else {(b, 0): 2 * b for b in range(B)}
        for (b, r), kind in kinds.items():
            if kind == 0:                                                 # a single attendable key
                blocked[b, r] = True
                blocked[b, r, L // 2] = False
                single.append((b, L // 2))
            elif kind == 1:                                               # whole first and whole last split blocked
                if nsplit >= 3:
                    blocked[b, r, :SPLIT] = True
                    blocked[b, r, (nsplit - 1) * SPLIT:] = True
                    blocked[b, r, SPLIT + 5] = False
                elif nsplit == 2:
                    blocked[b, r, :SPLIT] = True
                    blocked[b, r, L - 1] = False
                else:
                    blocked[b, r, 0] = True
                    blocked[b, r, L - 1] = False
            else:                                                         # nothing blocked
                blocked[b, r] = False
        assert not bool(blocked.all(-1).any())
    q, k, v, go = (t.to(dt).double() for t in (q, k, v, go))              # as the dtype holds them
    return q, k, v, go, blocked, single


def emulate(q, k, v, go, blocked, heads, dt):
    """The kernels in float64 with their roundings to ``dt`` (module docstring) -> out, dq, dk, dv."""
    b, nq, e = q.shape
    nl = k.shape[1]
    d = e // heads
    scale = d ** -0.5
    qh, kh, vh, gh = (t.view(b, -1, heads, d).transpose(1, 2) for t in (q, k, v, go))
    s = qh @ kh.transpose(-1, -2) * scale
    if blocked is not None:
        s = s.masked_fill(blocked.view(b, 1, nq, nl), float('-inf'))
    nsplit = (nl + SPLIT - 1) // SPLIT
    pad = nsplit * SPLIT - nl
    sp = torch.nn.functional.pad(s, (0, pad), value=float('-inf')).view(b, heads, nq, nsplit, SPLIT)
    vp = torch.nn.functional.pad(vh, (0, 0, 0, pad)).view(b, heads, nsplit, SPLIT, d)
    m = sp.amax(-1)                                                       # (b, heads, nq, nsplit); -inf: split all blocked
    m_use = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(sp - m_use.unsqueeze(-1))
    l_s = p.sum(-1)
    o_s = torch.einsum('bhqsk,bhskd->bhqsd', rd(p, dt), vp)
    big = m.amax(-1, keepdim=True)
    w = torch.exp(m - big)                                                # exp(-inf) = 0 for a blocked split
    den = (w * l_s).sum(-1)
    out = rd((w.unsqueeze(-1) * o_s).sum(-2) / den.unsqueeze(-1), dt)     # (b, heads, nq, d), stored in the dtype
    lse = big.squeeze(-1) + torch.log(den)
    delta = (gh * out).sum(-1, keepdim=True)
    pn = torch.exp(s - lse.unsqueeze(-1))
    ds = pn * (gh @ vh.transpose(-1, -2) - delta) * scale
    dsr, pr = rd(ds, dt), rd(pn, dt)
    dq, dk, dv = dsr @ kh, dsr.transpose(-1, -2) @ qh, pr.transpose(-1, -2) @ gh

    def merge(t):
        return t.transpose(1, 2).reshape(b, -1, e)
    return merge(out), rd(merge(dq), dt), rd(merge(dk), dt), rd(merge(dv), dt)


_CACHE = {}


def _case(case, dt):
    """Inputs, the float64 reference (gradients for dO scale 1: a power-of-two scale multiplies them exactly), and per
    scale the emulation and its error against float64 per tensor."""
    key = (case, dt)
    if key not in _CACHE:
        heads = case[3]
        q, k, v, go, blocked, single = _inputs(case, dt)
        qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
        out = ref_attention(qr, kr, vr, blocked, heads)
        out.backward(go)
        ref = dict(out=out.detach(), dq=qr.grad, dk=kr.grad, dv=vr.grad)
        emu = {}
        for gs in GSCALES:
            o, dq, dk, dv = emulate(q, k, v, go * gs, blocked, heads, dt)
            emu[gs] = dict(out=o, dq=dq, dk=dk, dv=dv)
        _CACHE[key] = (q, k, v, go, blocked, single, ref, emu)
    return _CACHE[key]


def _ref_at(ref, name, gs):
    return ref[name] if name == 'out' else ref[name] * gs


def _dk_reference(ref, emu, single, gs):
    """float64 dK, but the emulation's own value on the key rows a single-key query attends to (a cancellation)."""
    r = (ref['dk'] * gs).clone()
    for b, key in single:
        r[b, key] = emu['dk'][b, key]
    return r


def test_cpu_emulation_without_roundings_is_the_reference():
    """With float64 as the 'dtype' every rounding is the identity: the emulation (split-wise forward, hand-written backward)
    must then equal float64 autograd of the reference."""
    for case in CASES:
        q, k, v, go, blocked, single, ref, _ = _case(case, torch.bfloat16)
        for name, t in zip(('out', 'dq', 'dk', 'dv'), emulate(q, k, v, go, blocked, case[3], torch.float64)):
            assert err(t, ref[name]) < 1e-12, (case, name, err(t, ref[name]))


@pytest.mark.parametrize('dt', LO)
def test_cpu_emulation_has_an_error_of_its_own(dt):
    """Every e_emul is non-zero and finite (no fp16 overflow at 2^8), the logits reach the magnitudes the docstring names."""
    for case in CASES:
        q, k, v, go, blocked, single, ref, emu = _case(case, dt)
        d = case[4]
        logit = (q.view(*q.shape[:2], case[3], d).transpose(1, 2) @ k.view(*k.shape[:2], case[3], d).transpose(1, 2)
                 .transpose(-1, -2)).abs().max() * d ** -0.5
        if case[2] >= 256:
            assert float(logit) >= 3.0 * KMAX[dt], (case, float(logit))
        for gs in GSCALES:
            for name in ('out', 'dq', 'dk', 'dv'):
                e = err(emu[gs][name], _ref_at(ref, name, gs))
                assert 0.0 < e < 0.25, (case, dt, gs, name, e)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', LO)
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(str(int(i)) for i in c))
def test_attention_16bit_against_float64(device, capsys, case, dt):
    from mask_bev_amd import ops
    heads = case[3]
    q, k, v, go, blocked, single, ref, emu = _case(case, dt)
    qd, kd, vd = (t.to(device=device, dtype=dt).requires_grad_() for t in (q, k, v))
    bd = None if blocked is None else blocked.to(device).unsqueeze(1)
    out = ops.attention(qd, kd, vd, bd, heads)
    assert out.dtype == dt
    bad = []
    tag = f'{NAME[dt]} {case[:5]}'
    for i, gs in enumerate(GSCALES):
        qd.grad = kd.grad = vd.grad = None
        out.backward((go * gs).to(device=device, dtype=dt), retain_graph=i + 1 < len(GSCALES))
        torch.cuda.synchronize()
        got = dict(out=out, dq=qd.grad, dk=kd.grad, dv=vd.grad)
        for name in ('out', 'dq', 'dk', 'dv'):
            if name == 'out' and i:
                continue
            r = _ref_at(ref, name, gs)
            bar = max(ROUNDING[dt], 2.0 * err(emu[gs][name], r))
            target = _dk_reference(ref, emu[gs], single, gs) if name == 'dk' else r
            assert got[name].dtype == dt
            check(capsys, MOD, f'{tag} dO x {gs:g} {name}', err(got[name], target), bar, bad)
    assert not bad, bad
