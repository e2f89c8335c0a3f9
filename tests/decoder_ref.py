"""The two nodes of the row-chain decoder (mask_bev_amd/decoder_fused.py: _DecA, _DecB) restated in plain torch on the CPU, the
backward by autograd.  tests/test_decoder_ref_cpu.py holds the restatement itself to torch's own modules; tests/test_k19_paths_gpu.py
holds the kernels to it.

Every function works in the dtype of its operands (float64: the reference; float32: the evaluation that gives each tensor its
bar) and takes a rounding dtype ``dt`` — bf16 / fp16: the value is rounded where the kernel rounds (the A operand of every GEMM
stage, the hidden image of the second FFN product, the weights, the 16-bit stores); None: nowhere.

A :class:`Tape` names the block boundaries (a 16-bit store's boundary holds the value BEFORE its rounding: the kernel's stored
value is held to one rounding of it).  ``tape.val[name]`` is what the reference computes there, ``tape.grad[name]`` the
gradient it computes there.  A tensor handed over in ``given`` REPLACES the reference's own value (or gradient) for everything
behind the boundary: that is "each block against float64 given the block before it" — a block is charged for its own arithmetic
only, not for a 16-bit rounding that falls the other way because its input differs in the last f32 bit, and not for the
attention kernels (K6) or the mask kernel (K7), whose results are inputs here."""
import math

import torch

from tests.f64_bars import RoundGrad, RoundValue, rd


class _Subst(torch.autograd.Function):
    """A named boundary: forward hands on ``value`` if there is one (else x), backward records the gradient under ``gname`` and
    hands on the given one if there is one."""

    @staticmethod
    def forward(ctx, x, value, tape, gname):
        ctx.tape, ctx.gname = tape, gname
        return x.view_as(x) if value is None else value.to(x.dtype).reshape(x.shape).clone()

    @staticmethod
    def backward(ctx, g):
        if ctx.gname is not None:
            ctx.tape.grad[ctx.gname] = g.detach().clone()
            sub = ctx.tape.given.get(ctx.gname)
            if sub is not None:
                g = sub.to(g.dtype).reshape(g.shape)
        return g, None, None, None


class Tape:
    def __init__(self, given=None):
        self.given = dict(given or {})
        self.val, self.grad = {}, {}

    def tap(self, name, x, grad=None):
        self.val[name] = x.detach()
        return _Subst.apply(x, self.given.get(name), self, grad)


def lin(x, w, b, dt):
    """A GEMM stage and its backward as the chains run them: y = rd(x) rd(w)^T + b, dx = rd(dy) rd(w), and the parameter
    gradients from the UNROUNDED pair, dw = dy^T x and db = sum dy.  The second term is zero in value and carries them."""
    if dt is None:
        return x @ w.t() + b
    data = RoundGrad.apply(RoundValue.apply(x, dt) @ rd(w.detach(), dt).t(), dt) + b.detach()
    par = x.detach() @ w.t() + b
    return data + (par - par.detach())


def store(x, dt):
    """A 16-bit store (the gradient passes)."""
    return x if dt is None else RoundValue.apply(x, dt)


def layer_norm(x, g, b, eps, tape=None, name=None):
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    xh = xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    if tape is not None:
        tape.val[name] = xh.detach()
        tape.val[name + '_stats'] = torch.cat([mean, 1 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)], -1).detach()
    return xh * g + b


def attention(q, k, v, batch, heads, blocked=None):
    """softmax(q k^T / sqrt(d) [blocked -> -inf]) v per head.  q (batch * Q, E); k, v (batch * N, E); blocked (batch, Q, N) bool."""
    e = q.shape[-1]
    d = e // heads
    qh, kh, vh = (t.reshape(batch, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(d)
    if blocked is not None:
        s = s.masked_fill(blocked.reshape(batch, 1, s.shape[2], s.shape[3]), float('-inf'))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(-1, e)


def pos_rows(pos, m):
    """positions of row r: pos[r mod Q]."""
    return pos[torch.arange(m) % pos.shape[0]]


def deca(x0, o1, pos, p, batch, heads, eps, dt, tape):
    """_DecA.  x0, o1 (m, E); pos (Q, E); p: wo, bo, g1, b1, w_in, b_in.  Returns (x1, o2).
    Boundaries: sum1 [ds1], x1 [g_ln1], posrows_a [dpos_a], t1, qkv [g_qkv], o2; tape.val['xh1'] is LN1's normalised input."""
    m, e = x0.shape
    o1 = tape.tap('o1', o1 if dt is None else RoundGrad.apply(o1, dt), 'g_o1')      # g_o1 is stored in the 16-bit type
    sum1 = tape.tap('sum1', x0 + lin(o1, p['wo'], p['bo'], dt), 'ds1')
    x1 = tape.tap('x1', layer_norm(sum1, p['g1'], p['b1'], eps, tape, 'xh1'), 'g_ln1')
    t1 = tape.tap('t1', x1 + tape.tap('posrows_a', pos_rows(pos, m), 'dpos_a'))
    w, b = p['w_in'], p['b_in']
    qkv = torch.stack([lin(t1, w[0:e], b[0:e], dt), lin(t1, w[e:2 * e], b[e:2 * e], dt), lin(x1, w[2 * e:], b[2 * e:], dt)])
    qkv = store(tape.tap('qkv', qkv, 'g_qkv'), dt)
    o2 = store(tape.tap('o2', attention(qkv[0], qkv[1], qkv[2], batch, heads)), dt)
    return x1, o2


def heads_of(x3, hd, dt, tape):
    """post-norm, class head, mask-embedding MLP (no gradient: the batched heads own it).  Boundaries: p, h1, h2."""
    x3 = x3.detach()
    pn = tape.tap('p', layer_norm(x3, hd['post_g'], hd['post_b'], hd['eps']))
    cls = lin(pn, hd['cls_w'], hd['cls_b'], dt)
    (w1, b1), (w2, b2), (w3, b3) = hd['mlp']
    h1 = tape.tap('h1', torch.relu(lin(pn, w1, b1, dt)))
    h2 = tape.tap('h2', torch.relu(lin(h1, w2, b2, dt)))
    me = lin(h2, w3, b3, dt)
    tape.val['cls'], tape.val['me'] = cls.detach(), me.detach()
    return cls.detach(), store(me, dt).detach()


def decb(x1, o2, pos, p, hd, nxt, batch, heads, eps, dt, tape):
    """_DecB.  x1, o2 (m, E); p: wo, bo, g2, b2, w1, bb1, w2, bb2, g3, b3 (+ nw_in, nb_in); hd: post_g, post_b, eps, cls_w,
    cls_b, mlp; nxt: None or dict k, v (batch * N, E), blocked (batch, Q, N).  Returns (x3, cls, me, o1n | None).
    Boundaries: sum2 [ds2], x2 [g_ln2], hpre [dh], hid, sum3 [ds3], x3 [g_ln3], posrows_b [dpos_b], t3, qc [g_qc], o1n."""
    m, e = x1.shape
    o2 = tape.tap('o2_in', o2 if dt is None else RoundGrad.apply(o2, dt), 'g_o2')   # g_o2 is stored in the 16-bit type
    sum2 = tape.tap('sum2', x1 + lin(o2, p['wo'], p['bo'], dt), 'ds2')
    x2 = tape.tap('x2', layer_norm(sum2, p['g2'], p['b2'], eps, tape, 'xh2'), 'g_ln2')
    hpre = tape.tap('hpre', lin(x2, p['w1'], p['bb1'], dt), 'dh')
    tape.val['hid'] = torch.relu(hpre).detach()
    # ReLU by the STORED activations' sign, as the backward kernel masks: (h > 0) of the given hidden image when there is one
    live = (tape.given['hid'].reshape(hpre.shape) if 'hid' in tape.given else hpre.detach()) > 0
    hid = _Subst.apply(hpre * live, tape.given.get('hid'), tape, None)
    sum3 = tape.tap('sum3', x2 + lin(hid, p['w2'], p['bb2'], dt), 'ds3')
    x3 = tape.tap('x3', layer_norm(sum3, p['g3'], p['b3'], eps, tape, 'xh3'), 'g_ln3')
    cls, me = heads_of(x3, hd, dt, tape)
    o1n = None
    if nxt is not None:
        t3 = tape.tap('t3', x3 + tape.tap('posrows_b', pos_rows(pos, m), 'dpos_b'))
        qc = store(tape.tap('qc', lin(t3, p['nw_in'][0:e], p['nb_in'][0:e], dt), 'g_qc'), dt)
        o1n = store(tape.tap('o1n', attention(qc, nxt['k'], nxt['v'], batch, heads, nxt['blocked'])), dt)
    return x3, cls, me, o1n
