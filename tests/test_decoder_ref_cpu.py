"""tests/decoder_ref.py (the float64 restatement of decoder_fused._DecA / _DecB) against torch's own modules: float64 on the
CPU, no rounding, forward and every gradient, bound 1e-12 of the largest entry."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import decoder_ref as D
from tests.f64_bars import err

B, Q, E, H, FF, OC, NK = 2, 5, 32, 2, 64, 24, 13
EPS = 1e-5
BOUND = 1e-12
F64 = torch.float64


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, dtype=F64) * scale


def _leaf(gen, *shape, scale=1.0):
    return _rand(gen, *shape, scale=scale).requires_grad_()


def _mha(gen, identity_kv):
    """nn.MultiheadAttention whose output projection is the identity (the nodes' attention ends before it); ``identity_kv``:
    the key / value projections too (the next layer's keys and values arrive projected)."""
    mha = nn.MultiheadAttention(E, H, batch_first=True, dtype=F64)
    with torch.no_grad():
        mha.in_proj_weight.copy_(_rand(gen, 3 * E, E, scale=E ** -0.5))
        mha.in_proj_bias.copy_(_rand(gen, 3 * E, scale=0.5))
        if identity_kv:
            mha.in_proj_weight[E:2 * E] = torch.eye(E, dtype=F64)
            mha.in_proj_weight[2 * E:] = torch.eye(E, dtype=F64)
            mha.in_proj_bias[E:] = 0
        mha.out_proj.weight.copy_(torch.eye(E, dtype=F64))
        mha.out_proj.bias.zero_()
    return mha


def _linear(gen, n, k):
    m = nn.Linear(k, n, dtype=F64)
    with torch.no_grad():
        m.weight.copy_(_rand(gen, n, k, scale=k ** -0.5))
        m.bias.copy_(_rand(gen, n, scale=0.5))
    return m


def _norm(gen):
    m = nn.LayerNorm(E, eps=EPS, dtype=F64)
    with torch.no_grad():
        m.weight.copy_(1 + _rand(gen, E, scale=0.3))
        m.bias.copy_(_rand(gen, E, scale=0.3))
    return m


def _twin(t):
    return t.detach().clone().requires_grad_()


def _same(tag, got, ref, bad):
    e = err(got, ref)
    if not e <= BOUND:
        bad.append(f'{tag}: {e:.3e}')


def test_deca_equals_torch_modules():
    gen = torch.Generator().manual_seed(1901)
    out_proj, ln1, mha = _linear(gen, E, E), _norm(gen), _mha(gen, False)
    x0, o1, pos = _leaf(gen, B, Q, E), _leaf(gen, B, Q, E), _leaf(gen, Q, E)
    g_x1, g_o2 = _rand(gen, B, Q, E), _rand(gen, B, Q, E)
    x1 = ln1(x0 + out_proj(o1))
    t1 = x1 + pos
    o2 = mha(t1, t1, x1, need_weights=False)[0]
    torch.autograd.backward([x1, o2], [g_x1, g_o2])

    p = dict(wo=_twin(out_proj.weight), bo=_twin(out_proj.bias), g1=_twin(ln1.weight), b1=_twin(ln1.bias),
             w_in=_twin(mha.in_proj_weight), b_in=_twin(mha.in_proj_bias))
    x0r, o1r, posr = _twin(x0), _twin(o1), _twin(pos)
    tape = D.Tape()
    x1r, o2r = D.deca(x0r.view(-1, E), o1r.view(-1, E), posr, p, B, H, EPS, None, tape)
    torch.autograd.backward([x1r, o2r], [g_x1.view(-1, E), g_o2.view(-1, E)])
    bad = []
    _same('x1', x1r.view(B, Q, E), x1, bad)
    _same('t1', tape.val['t1'].view(B, Q, E), t1, bad)
    _same('o2', o2r.view(B, Q, E), o2, bad)
    for tag, got, ref in (('d x0', x0r, x0), ('d o1', o1r, o1), ('d pos', posr, pos), ('d wo', p['wo'], out_proj.weight),
                          ('d bo', p['bo'], out_proj.bias), ('d g1', p['g1'], ln1.weight), ('d b1', p['b1'], ln1.bias),
                          ('d w_in', p['w_in'], mha.in_proj_weight), ('d b_in', p['b_in'], mha.in_proj_bias)):
        _same(tag, got.grad, ref.grad, bad)
    # the boundaries' gradients are what the kernels return: d(sum1) is d(x0), d(positions) per row folds to d(pos)
    _same('ds1', tape.grad['ds1'].view(B, Q, E), x0.grad, bad)
    _same('dpos rows', tape.grad['dpos_a'].view(B, Q, E).sum(0), pos.grad, bad)
    assert not bad, bad


def _decb_case(with_next):
    gen = torch.Generator().manual_seed(1902 + int(with_next))
    out_proj, ln2, fc1, fc2, ln3, post = _linear(gen, E, E), _norm(gen), _linear(gen, FF, E), _linear(gen, E, FF), _norm(gen), _norm(gen)
    cls_head = _linear(gen, 2, E)
    mlp = nn.Sequential(_linear(gen, E, E), nn.ReLU(), _linear(gen, E, E), nn.ReLU(), _linear(gen, OC, E))
    mha = _mha(gen, True)
    x1, o2, pos = _leaf(gen, B, Q, E), _leaf(gen, B, Q, E), _leaf(gen, Q, E)
    k, v = _rand(gen, B, NK, E), _rand(gen, B, NK, E)
    blocked = torch.rand(B, Q, NK, generator=gen) < 0.4
    blocked[:, :, 0] = False                                  # (no row blocks every key: K7 unblocks such rows)
    g_x3, g_o1n = _rand(gen, B, Q, E), _rand(gen, B, Q, E)
    x2 = ln2(x1 + out_proj(o2))
    hid = F.relu(fc1(x2))
    x3 = ln3(x2 + fc2(hid))
    pn = post(x3)
    cls, me = cls_head(pn), mlp(pn)
    outs, grads = [x3], [g_x3]
    if with_next:
        t3 = x3 + pos
        mask = blocked.view(B, 1, Q, NK).expand(B, H, Q, NK).reshape(B * H, Q, NK)
        o1n = mha(t3, k, v, attn_mask=mask, need_weights=False)[0]
        outs, grads = [x3, o1n], [g_x3, g_o1n]
    torch.autograd.backward(outs, grads)

    p = dict(wo=_twin(out_proj.weight), bo=_twin(out_proj.bias), g2=_twin(ln2.weight), b2=_twin(ln2.bias),
             w1=_twin(fc1.weight), bb1=_twin(fc1.bias), w2=_twin(fc2.weight), bb2=_twin(fc2.bias),
             g3=_twin(ln3.weight), b3=_twin(ln3.bias), nw_in=_twin(mha.in_proj_weight), nb_in=_twin(mha.in_proj_bias))
    hd = dict(post_g=post.weight.detach(), post_b=post.bias.detach(), eps=EPS, cls_w=cls_head.weight.detach(),
              cls_b=cls_head.bias.detach(), mlp=[(mlp[j].weight.detach(), mlp[j].bias.detach()) for j in (0, 2, 4)])
    nxt = dict(k=k.view(-1, E), v=v.view(-1, E), blocked=blocked) if with_next else None
    x1r, o2r, posr = _twin(x1), _twin(o2), _twin(pos)
    tape = D.Tape()
    x3r, clsr, mer, o1nr = D.decb(x1r.view(-1, E), o2r.view(-1, E), posr, p, hd, nxt, B, H, EPS, None, tape)
    if with_next:
        torch.autograd.backward([x3r, o1nr], [g_x3.view(-1, E), g_o1n.view(-1, E)])
    else:
        assert o1nr is None
        x3r.backward(g_x3.view(-1, E))
    bad = []
    for tag, got, ref in (('x2', tape.val['x2'], x2), ('hid', tape.val['hid'], hid), ('x3', x3r, x3), ('cls', clsr, cls),
                          ('me', mer, me), ('p', tape.val['p'], pn)):
        _same(tag, got.view(ref.shape), ref, bad)
    pairs = [('d x1', x1r, x1), ('d o2', o2r, o2), ('d wo', p['wo'], out_proj.weight), ('d bo', p['bo'], out_proj.bias),
             ('d g2', p['g2'], ln2.weight), ('d b2', p['b2'], ln2.bias), ('d w1', p['w1'], fc1.weight), ('d bb1', p['bb1'], fc1.bias),
             ('d w2', p['w2'], fc2.weight), ('d bb2', p['bb2'], fc2.bias), ('d g3', p['g3'], ln3.weight), ('d b3', p['b3'], ln3.bias)]
    for tag, got, ref in pairs:
        _same(tag, got.grad, ref.grad, bad)
    _same('ds2', tape.grad['ds2'].view(B, Q, E), x1.grad, bad)
    if with_next:
        _same('t3', tape.val['t3'].view(B, Q, E), t3, bad)
        _same('o1n', o1nr.view(B, Q, E), o1n, bad)
        _same('d pos', posr.grad, pos.grad, bad)
        _same('dpos rows', tape.grad['dpos_b'].view(B, Q, E).sum(0), pos.grad, bad)
        _same('d nw_in (query rows)', p['nw_in'].grad[:E], mha.in_proj_weight.grad[:E], bad)
        _same('d nb_in (query rows)', p['nb_in'].grad[:E], mha.in_proj_bias.grad[:E], bad)
        assert not p['nw_in'].grad[E:].any() and not p['nb_in'].grad[E:].any()
    else:
        assert posr.grad is None and p['nw_in'].grad is None and p['nb_in'].grad is None
    assert not bad, bad


def test_decb_with_next_layer_equals_torch_modules():
    _decb_case(True)


def test_decb_last_layer_equals_torch_modules():
    _decb_case(False)


def test_given_values_and_gradients_replace_the_references_own():
    """A boundary handed a value / a gradient uses it for everything behind it and still records its own."""
    gen = torch.Generator().manual_seed(1905)
    p = dict(wo=_leaf(gen, E, E, scale=E ** -0.5), bo=_leaf(gen, E), g1=_leaf(gen, E), b1=_leaf(gen, E),
             w_in=_leaf(gen, 3 * E, E, scale=E ** -0.5), b_in=_leaf(gen, 3 * E))
    x0, o1, pos = _leaf(gen, B * Q, E), _leaf(gen, B * Q, E), _leaf(gen, Q, E)
    t1, ds1 = _rand(gen, B * Q, E), _rand(gen, B * Q, E)
    tape = D.Tape(dict(t1=t1, ds1=ds1))
    x1, o2 = D.deca(x0, o1, pos, p, B, H, EPS, None, tape)
    torch.autograd.backward([x1, o2], [torch.ones_like(x1), torch.ones_like(o2)])
    assert torch.equal(tape.val['t1'], tape.val['x1'] + D.pos_rows(pos.detach(), B * Q))
    q = t1 @ p['w_in'][:E].t() + p['b_in'][:E]
    assert err(tape.val['qkv'][0], q) <= BOUND
    assert torch.equal(x0.grad, ds1) and not torch.equal(tape.grad['ds1'], ds1)
    assert err(o1.grad, ds1 @ p['wo']) <= BOUND and err(p['bo'].grad, ds1.sum(0)) <= BOUND
