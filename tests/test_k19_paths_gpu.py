"""K19 (csrc/rowchain.hip, driven by mask_bev_amd/decoder_fused.py) against float64 on the programs production builds.

``DF._DecA.apply`` / ``DF._DecB.apply`` are driven directly, set up as ``Mask2FormerHead._forward_decoder_fused`` sets them up:
plain f32 leaf parameters, ``WeightCopies.refresh`` with that function's entry list (transposed entries and the k-major flag
from ``ffn_split`` included), ``HeadPass(None)`` with ``gq = {}``, ``QueryPositions``, ``LayerCtx``, and for the next-layer branch
a ``SharedKV`` holder (two slots, the second one read) filled here.  The reference is tests/decoder_ref.py.

Each block is held to float64 GIVEN the block before it as the kernel returned it (decoder_ref.Tape): intermediates the nodes
keep are read from ``grad_fn.saved_tensors``; the ones they only allocate (``me``, ``ds3``, ``dh``, K6's ``g_qkv`` / ``g_qc``) are
caught where ``torch.empty`` makes them and where the C call receives them (_Capture); the heads' post-norm and hidden images,
which never leave LDS, are re-made from the returned ``x3`` by the same stage code (_head_images) — the kernel is deterministic —
and held to the bar themselves.  K6 (o2, g_qkv, o1n, g_qc) and K7 (mask_pred, blocked) are inputs, only called here.

Bars (tests/f64_bars.py, none of this module's own): f32 stores ``f32_bar(ref32, ref64)``; 16-bit stores the same bar on
``err_beyond_one_rounding``; column sums and LayerNorm parameter gradients the same bar, of max sum|.|.
Measured errors: DESIGN.md, "K19 against float64 on the programs production builds"."""
import pytest
import torch

from tests import decoder_ref as R
from tests.f64_bars import LO, NAME, check, err, err_beyond_one_rounding, f32_bar

pytestmark = pytest.mark.gpu

MOD = 'k19-paths'
F32, F64 = torch.float32, torch.float64
EPS = 1e-5
MASK_HW, TARGET, TARGET_ODD = (16, 12), (8, 6), (13, 10)

# ((B, Q, E, heads, F), oc, S = decoder_fused.ffn_split) — head dimension 32, class head 2 wide, MLP widths E, E, oc
C_RAGGED = ((3, 37, 64, 2, 512), 48, 2)           # 111 rows = 7 blocks, the last of 15; positions wrap inside a block
C_LANES = ((2, 20, 160, 5, 768), 160, 3)          # 40 rows, last block 8; E = 5 x 32: LayerNorm lanes with c >= n idle
C_ONE = ((1, 8, 128, 4, 256), 128, 1)             # less than one block; the unsplit B.fwd / B.bwd, one-workgroup FFN stage
C_FULL = ((4, 100, 256, 8, 2048), 256, 8)         # the 100-query configuration: 25 blocks, S = 8, RC_MAXC columns
C_F32_CHUNKS = ((3, 37, 64, 2, 320), 48, 1)       # fp32: the staged FFN form, chunks 256 + 64, row-major weights
C_F32_ONE = ((2, 20, 160, 5, 256), 160, 1)        # fp32: one chunk; exact-f32 MFMA at 5 lane groups
CASES = ([(dt, c) for c in (C_RAGGED, C_LANES, C_ONE) for dt in LO] + [(torch.bfloat16, C_FULL)]
         + [(F32, C_F32_CHUNKS), (F32, C_F32_ONE)])


def _cid(v):
    return NAME[v] if isinstance(v, torch.dtype) else 'x'.join(map(str, v[0]))


def _randn(seed, shape, scale=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale + mean


def _leaf(t, wd):
    return t.detach().clone().to(wd).requires_grad_()


class _Capture:
    """The library calls (through the proxy's hook) and the tensors ``torch.empty`` makes while it is active."""

    def __init__(self, patch):
        from mask_bev_amd import _lib
        self.calls, self.made = [], []
        real = torch.empty

        def hook(name, fn, args):
            self.calls.append((name, args))
            return fn(*args)

        def empty(*a, **k):
            t = real(*a, **k)
            self.made.append(t)
            return t

        patch.setattr(_lib.load(), 'hook', hook)
        patch.setattr(torch, 'empty', empty)

    def launches(self):
        return sum(name.startswith('mbv_rowchain_run') for name, _ in self.calls)

    def arg_tensor(self, name, index):
        """The tensor whose memory argument ``index`` of the one call of ``name`` points to."""
        hits = [a for n, a in self.calls if n == name]
        assert len(hits) == 1, (name, len(hits))
        ptr = hits[0][index].value
        return next(t for t in self.made if t.data_ptr() == ptr)

    def first(self, start, shape, dtype, known=()):
        """The first tensor of that shape and type made after position ``start`` that is none of ``known``."""
        ptrs = {t.data_ptr() for t in known if t is not None}
        return next(t for t in self.made[start:] if tuple(t.shape) == tuple(shape) and t.dtype == dtype
                    and t.data_ptr() not in ptrs)


class _Rig:
    """One decoder layer's operands on the CPU (f32; what enters in 16 bits already rounded) and the production set-up on the
    device."""

    def __init__(self, device, dt, case, seed):
        from mask_bev_amd import decoder_fused as DF
        from mask_bev_amd import ops
        from mask_bev_amd.mask2former_head import HeadPass
        (b, q, e, h, f), oc, split = case
        assert e // h == 32
        self.device, self.dt, self.shape, self.oc, self.seed = device, dt, (b, q, e, h, f), oc, seed
        self.m = b * q
        self.rdt = None if dt == F32 else dt
        assert DF.ffn_split(f, e, dt) == split, 'the split rule changed: this case no longer reaches what it states'
        self.split = split
        s = iter(range(seed, seed + 100))

        def w(n, k):
            return _randn(next(s), (n, k), k ** -0.5)

        def bias(n):
            return _randn(next(s), (n,), 0.5)

        def gamma():
            return _randn(next(s), (e,), 0.3, 1.0)

        def beta():
            return _randn(next(s), (e,), 0.3)

        self.pa = dict(wo=w(e, e), bo=bias(e), g1=gamma(), b1=beta(), w_in=w(3 * e, e), b_in=bias(3 * e))
        self.pb = dict(wo=w(e, e), bo=bias(e), g2=gamma(), b2=beta(), w1=w(f, e), bb1=bias(f), w2=w(e, f), bb2=bias(e),
                       g3=gamma(), b3=beta(), nw_in=w(3 * e, e), nb_in=bias(3 * e))
        self.hd = dict(post_g=gamma(), post_b=beta(), eps=EPS, cls_w=w(2, e), cls_b=bias(2),
                       mlp=[(w(e, e), bias(e)), (w(e, e), bias(e)), (w(oc, e), bias(oc))])
        self.pos = _randn(next(s), (q, e))
        self.mask_feature = _randn(next(s), (b, oc) + MASK_HW).to(dt)
        dev = lambda t: t.to(device).requires_grad_()                                   # noqa: E731
        self.da = {k: dev(v) for k, v in self.pa.items()}
        self.db = {k: dev(v) for k, v in self.pb.items()}
        self.dpos = dev(self.pos)
        d_cls_w, d_mlp = self.hd['cls_w'].to(device), [(a.to(device), c.to(device)) for a, c in self.hd['mlp']]
        # the entry list of Mask2FormerHead._forward_decoder_fused for this layer and the next one's query projection
        km = DF.ffn_split(f, e, dt) > 1
        A, B = self.da, self.db
        ents = [(d_cls_w, None, False)] + [(a, None, False) for a, _ in d_mlp]
        ents += [(A['wo'], None, False), (A['w_in'], None, False), (B['wo'], None, False), (B['w1'], None, False),
                 (B['w2'], None, False, km), (B['nw_in'], None, False)]
        ents += [(A['wo'], None, True), (A['w_in'], (0, e), True), (A['w_in'], (e, 2 * e), True), (A['w_in'], (2 * e, 3 * e), True),
                 (B['wo'], None, True), (B['w1'], None, True, km), (B['w2'], None, True), (B['nw_in'], (0, e), True)]
        self.tw = DF.WeightCopies()
        self.tw.refresh(ents, dt)
        self.hp = HeadPass(None)
        self.hp.gq = {}
        self.qpos = DF.QueryPositions.apply(self.dpos, self.hp)
        self.lc = DF.LayerCtx(b, q, e, h, f, EPS, dt, self.tw, self.hp, self.qpos)
        self.head = DF.HeadSpec(self.hd['post_g'].to(device), self.hd['post_b'].to(device), d_cls_w, self.hd['cls_b'].to(device),
                                d_mlp, self.mask_feature.to(device), None, index=1)
        self.DF, self.ops = DF, ops
        self.holders = {}

    def next_cross(self, target):
        """NextCross over a SharedKV holder of two slots filled with N(0, 1) in the compute type; slot 1 is the one read."""
        b, q, e, h, f = self.shape
        if target not in self.holders:
            n = target[0] * target[1]
            holder = self.ops.SharedKV()
            kc, vc = (_randn(self.seed + 200 + i + n, (b, n, 2 * e)).to(self.dt) for i in (0, 1))
            holder.k_cat, holder.v_cat, holder.n, holder.e = kc.to(self.device), vc.to(self.device), 2, e
            self.holders[target] = (holder, kc[:, :, e:].float().reshape(-1, e), vc[:, :, e:].float().reshape(-1, e))
        holder, k, v = self.holders[target]
        return self.DF.NextCross(self.db['nw_in'], self.db['nb_in'], holder, 1, target), k, v

    def clear_grads(self):
        for p in list(self.da.values()) + list(self.db.values()) + [self.dpos]:
            p.grad = None

    def _head_images(self, x3):
        """post-norm(x3) and the mask-embedding MLP's two hidden images, by the chain's own stages on the returned x3."""
        b, q, e, h, f = self.shape
        DF, lc, hs = self.DF, self.lc, self.head
        pn, h1, h2 = (torch.zeros((self.m, e), dtype=F32, device=self.device) for _ in range(3))
        (m1w, m1b), (m2w, m2b), _ = hs.mlp
        P = DF.Program(self.m, q, EPS, lc.wdt, 'test.heads')
        P.load(0, x3, e)
        P.ln(1, 0, -1, hs.post_g, hs.post_b, e)
        P.store(1, pn, e)
        P.gemm(2, 1, lc.w(m1w), e, e, bias=m1b, relu=True)
        P.store(2, h1, e)
        P.gemm(3, 2, lc.w(m2w), e, e, bias=m2b, relu=True)
        P.store(3, h2, e)
        P.run()
        return pn, h1, h2

    # ------------------------------------------------------------------------------------------------ the nodes
    def run_a(self, patch, x0, o1, g_x1, g_o2, fill):
        """_DecA forward and backward.  Returns what the kernels made (CPU) and the launch counts."""
        b, q, e, h, f = self.shape
        m, A, dev = self.m, self.da, self.device
        self.clear_grads()
        x0d, o1d = x0.to(dev).view(b, q, e).requires_grad_(), o1.to(dev).view(b, q, e).requires_grad_()
        with patch.context() as mp:
            cap = _Capture(mp)
            x1, o2 = self.DF._DecA.apply(self.lc, x0d, o1d, A['wo'], A['bo'], A['g1'], A['b1'], A['w_in'], A['b_in'])
            n_fwd = cap.launches()
            o1f, sum1, stats1, x1s, t1, qkv, o2s, lse = x1.grad_fn.saved_tensors
            assert x1s.data_ptr() == x1.data_ptr() and o2s.data_ptr() == o2.data_ptr()
            assert torch.equal(o1f, o1d.detach().view(m, e).float()), 'o1f: the f32 copy of o1'
            got = dict(sum1=sum1, stats1=stats1, x1=x1, t1=t1, qkv=qkv, o2=o2)
            got = {k: v.detach().cpu() for k, v in got.items()}
            self.hp.acc = fill.to(dev)
            outs = [(x1, g_x1), (o2, g_o2)]
            torch.autograd.backward([t for t, g in outs if g is not None],
                                    [g.to(dev).view(t.shape) for t, g in outs if g is not None])
            n_bwd = cap.launches() - n_fwd
            got['g_qkv'] = cap.arg_tensor('mbv_attn_bwd', 13).detach().cpu()
        torch.cuda.synchronize()
        assert tuple(got['g_qkv'].shape) == (3, m, e) and got['g_qkv'].dtype == F32
        got.update(ds1=x0d.grad.view(m, e).cpu(), g_o1=o1d.grad.view(m, e).cpu(), acc=self.hp.acc.cpu(),
                   **{'d ' + k: None if p.grad is None else p.grad.cpu() for k, p in A.items()})
        self.hp.acc = None
        return got, (n_fwd, n_bwd)

    def ref_a(self, wd, x0, o1, g_x1, g_o2, given):
        b, q, e, h, f = self.shape
        P = {k: _leaf(v, wd) for k, v in self.pa.items()}
        x0r, o1r = _leaf(x0, wd), _leaf(o1, wd)
        tape = R.Tape(given)
        x1, o2 = R.deca(x0r, o1r, _leaf(self.pos, wd), P, b, h, EPS, self.rdt, tape)
        zero = torch.zeros((self.m, e), dtype=wd)
        torch.autograd.backward([x1, o2], [zero if g is None else g.to(wd) for g in (g_x1, g_o2)])
        tape.param = {k: v.grad for k, v in P.items()}
        return tape

    def run_b(self, patch, x1, o2, target, g_x3, g_o1n, fill, g_heads=None, direct=False):
        """_DecB forward and backward; ``target``: the next layer's key grid, None: the last layer.  ``direct``: the backward
        is called with no gradient at all (autograd never does that: it would not call it)."""
        b, q, e, h, f = self.shape
        m, B, dev, oc = self.m, self.db, self.device, self.oc
        self.clear_grads()
        nxt = k = v = None
        if target is not None:
            nxt, k, v = self.next_cross(target)
        x1d, o2d = x1.to(dev).requires_grad_(), o2.to(dev).requires_grad_()
        with patch.context() as mp:
            cap = _Capture(mp)
            outs = self.DF._DecB.apply(self.lc, self.head, nxt, x1d, o2d, None, B['wo'], B['bo'], B['g2'], B['b2'], B['w1'], B['bb1'],
                                       B['w2'], B['bb2'], B['g3'], B['b3'], B['nw_in'] if nxt else None, B['nb_in'] if nxt else None)
            n_fwd = cap.launches()
            x3, cls = outs[0], outs[1]
            node = x3.grad_fn
            saved = node.saved_tensors
            o2f, sum2, stats2, x2, hid, sum3, stats3, t3, qc, mask, o1n, lse = saved
            assert torch.equal(o2f, o2d.detach().float()), 'o2f: the f32 copy of o2'
            me = cap.first(0, (m, oc), self.mask_feature.dtype, known=list(saved) + [x3])
            got = dict(sum2=sum2, stats2=stats2, x2=x2, hid=hid, sum3=sum3, stats3=stats3, x3=x3.view(m, e), cls=cls.view(m, -1), me=me)
            if nxt is not None:
                assert outs[3].data_ptr() == o1n.data_ptr()
                got.update(t3=t3, qc=qc, o1n=o1n, blocked=outs[4].view(b, q, -1))
            got = {k_: v_.detach().cpu() for k_, v_ in got.items()}
        pn, h1, h2 = self._head_images(x3.detach().view(m, e))
        got.update(p=pn.cpu(), h1=h1.cpu(), h2=h2.cpu())
        with patch.context() as mp:
            cap = _Capture(mp)
            self.hp.acc = fill.to(dev)
            if g_heads is not None:
                self.hp.gq[self.head.index] = g_heads.to(dev).view(b, q, e)
            if direct:
                ret = self.DF._DecB.backward(node, None, None, None, None, None)
                got['direct'] = [None if t is None else t.detach().cpu() for t in ret]
            else:
                pairs = [(x3, g_x3)] + ([(outs[3], g_o1n)] if nxt is not None else [])
                torch.autograd.backward([t for t, g in pairs if g is not None],
                                        [g.to(dev).view(t.shape) for t, g in pairs if g is not None])
            n_bwd = cap.launches()
            assert self.head.index not in self.hp.gq, 'the heads\' share of d(x3) was not taken'
            g_qc = None
            if nxt is not None and g_o1n is not None:
                g_qc = cap.arg_tensor('mbv_attn_bwd_ld', 14)
                assert tuple(g_qc.shape) == (m, e) and g_qc.dtype == F32
                got['g_qc'] = g_qc.detach().cpu()
            torch.cuda.synchronize()
            if not direct:
                ds2 = x1d.grad
                cands = [t for t in cap.made if tuple(t.shape) == (m, e) and t.dtype == F32
                         and (g_qc is None or t.data_ptr() != g_qc.data_ptr()) and not torch.equal(t, ds2)]
                got.update(ds3=cands[0].detach().cpu(), dh=cap.first(0, (m, f), F32).detach().cpu())
        if not direct:
            got.update(ds2=x1d.grad.cpu(), g_o2=o2d.grad.cpu(),
                       **{'d ' + k_: None if p.grad is None else p.grad.cpu() for k_, p in B.items()})
        got['acc'] = self.hp.acc.cpu()
        self.hp.acc = None
        return got, (n_fwd, n_bwd), (k, v)

    def ref_b(self, wd, x1, o2, kv, blocked, g_x3, g_o1n, given):
        b, q, e, h, f = self.shape
        P = {k: _leaf(v, wd) for k, v in self.pb.items()}
        hd = dict(self.hd, **{k: self.hd[k].to(wd) for k in ('post_g', 'post_b', 'cls_w', 'cls_b')})
        hd['mlp'] = [(a.to(wd), c.to(wd)) for a, c in self.hd['mlp']]
        nxt = None if blocked is None else dict(k=kv[0].to(wd), v=kv[1].to(wd), blocked=blocked)
        x1r, o2r = _leaf(x1, wd), _leaf(o2, wd)
        tape = R.Tape(given)
        x3, cls, me, o1n = R.decb(x1r, o2r, _leaf(self.pos, wd), P, hd, nxt, b, h, EPS, self.rdt, tape)
        zero = torch.zeros((self.m, e), dtype=wd)
        outs, grads = [x3], [zero if g_x3 is None else g_x3.to(wd)]
        if o1n is not None:
            outs, grads = outs + [o1n], grads + [zero if g_o1n is None else g_o1n.to(wd)]
        torch.autograd.backward(outs, grads)
        tape.param = {k: v.grad for k, v in P.items()}
        return tape


# ---- comparisons ----------------------------------------------------------------------------------------------------------
class _Cmp:
    def __init__(self, capsys, tag):
        self.capsys, self.tag, self.bad = capsys, tag, []

    def __call__(self, name, got, r64, r32, scale=None):
        """An f32 tensor at the f32 bar, a 16-bit one beyond one rounding; ``scale``: of that magnitude (max sum|.|)."""
        r64, r32 = r64.reshape(got.shape), r32.reshape(got.shape)
        tag = f'{self.tag} {name}'
        if scale is not None:           # the magnitude joins each side as one more entry: err and f32_bar then divide by it
            top = torch.tensor([scale], dtype=F64)
            got, r64, r32 = (torch.cat([t.reshape(-1).double(), top]) for t in (got, r64, r32.float()))
            check(self.capsys, MOD, f'{tag} (of max sum|.|)', err(got, r64), f32_bar(r32.float(), r64), self.bad)
            return
        bar = f32_bar(r32, r64)
        if got.dtype == F32:
            check(self.capsys, MOD, tag, err(got, r64), bar, self.bad)
        else:
            check(self.capsys, MOD, f'{tag} (beyond one rounding)', err_beyond_one_rounding(got, r64, got.dtype), bar, self.bad)

    def val(self, name, got, t64, t32, key=None):
        self(name, got[name], t64.val[key or name], t32.val[key or name])

    def grad(self, name, got, t64, t32, key=None):
        self(name, got[name], t64.grad[key or name], t32.grad[key or name])

    def colsum(self, name, got, terms64, terms32):
        """A column sum of the returned rows ``terms``."""
        self(name, got, terms64.sum(0), terms32.sum(0), scale=float(terms64.abs().sum(0).max()))


def _both(fn, given):
    return tuple(fn(wd, {k: v.to(wd) for k, v in given.items()}) for wd in (F64, F32))


def _check_a(cmp, rig, got, x0, o1, g_x1, g_o2, fill):
    e = rig.shape[2]
    given = {k: got[k] for k in ('sum1', 'x1', 't1', 'qkv', 'o2', 'g_qkv', 'ds1')}
    t64, t32 = _both(lambda wd, gv: rig.ref_a(wd, x0, o1, g_x1, g_o2, gv), given)
    for name in ('sum1', 'x1', 't1', 'qkv'):
        cmp.val(name, got, t64, t32)
    cmp.val('stats1', got, t64, t32, 'xh1_stats')
    cmp.grad('ds1', got, t64, t32)
    cmp.grad('g_o1', got, t64, t32)
    cmp('d(positions) accumulated', got['acc'], fill.double() + t64.grad['dpos_a'], fill + t32.grad['dpos_a'])
    cmp('d wo', got['d wo'], t64.param['wo'], t32.param['wo'])
    cmp.colsum('d bo', got['d bo'], got['ds1'].double(), got['ds1'])
    for nm, key, terms in (('d g1', 'g1', lambda t: t.grad['g_ln1'] * t.val['xh1']), ('d b1', 'b1', lambda t: t.grad['g_ln1'])):
        cmp(nm, got[nm], t64.param[key], t32.param[key], scale=float(terms(t64).abs().sum(0).max()))
    for j, third in enumerate(('q', 'k', 'v')):                 # per third: q and k pair with t1, v with x1
        rows = slice(j * e, (j + 1) * e)
        cmp(f'd w_in[{third}]', got['d w_in'][rows], t64.param['w_in'][rows], t32.param['w_in'][rows])
        cmp.colsum(f'd b_in[{third}]', got['d b_in'][rows], got['g_qkv'][j].double(), got['g_qkv'][j])


def _check_b(cmp, rig, got, kv, x1, o2, g_x3, g_o1n, fill, g_heads=None):
    e = rig.shape[2]
    nxt = 'o1n' in got
    qterm = nxt and g_o1n is not None
    keys = ['sum2', 'x2', 'hid', 'sum3', 'x3', 'p', 'h1', 'h2', 'ds2', 'dh', 'ds3'] + (['t3', 'qc', 'o1n'] if nxt else [])
    given = {k: got[k] for k in keys + (['g_qc'] if qterm else [])}
    up = g_x3 if g_heads is None else (g_heads if g_x3 is None else g_x3 + g_heads)
    t64, t32 = _both(lambda wd, gv: rig.ref_b(wd, x1, o2, kv, got.get('blocked'), up, g_o1n, gv), given)
    for name in ('sum2', 'x2', 'hid', 'sum3', 'x3', 'p', 'cls', 'h1', 'h2', 'me') + (('t3', 'qc') if nxt else ()):
        cmp.val(name, got, t64, t32)
    cmp.val('stats2', got, t64, t32, 'xh2_stats')
    cmp.val('stats3', got, t64, t32, 'xh3_stats')
    for name in ('ds3', 'dh', 'ds2', 'g_o2'):
        cmp.grad(name, got, t64, t32)
    if qterm:
        cmp('d(positions) accumulated', got['acc'], fill.double() + t64.grad['dpos_b'], fill + t32.grad['dpos_b'])
    else:
        assert torch.equal(got['acc'], fill), 'd(positions) changed without a query-projection term'
    for key in ('wo', 'w1', 'w2'):
        cmp(f'd {key}', got[f'd {key}'], t64.param[key], t32.param[key])
    cmp.colsum('d bo', got['d bo'], got['ds2'].double(), got['ds2'])
    cmp.colsum('d bb1', got['d bb1'], got['dh'].double(), got['dh'])
    cmp.colsum('d bb2', got['d bb2'], got['ds3'].double(), got['ds3'])
    for ln in ('2', '3'):
        for nm, key, terms in ((f'd g{ln}', f'g{ln}', lambda t: t.grad[f'g_ln{ln}'] * t.val[f'xh{ln}']),
                               (f'd b{ln}', f'b{ln}', lambda t: t.grad[f'g_ln{ln}'])):
            cmp(nm, got[nm], t64.param[key], t32.param[key], scale=float(terms(t64).abs().sum(0).max()))
    if qterm:
        cmp('d nw_in[q]', got['d nw_in'][:e], t64.param['nw_in'][:e], t32.param['nw_in'][:e])
        cmp.colsum('d nb_in[q]', got['d nb_in'][:e], got['g_qc'].double(), got['g_qc'])
        assert not got['d nw_in'][e:].any() and not got['d nb_in'][e:].any()
    else:
        assert got['d nw_in'] is None and got['d nb_in'] is None


def _inputs(rig, gscale=1.0):
    b, q, e, h, f = rig.shape
    s, m = rig.seed + 100, rig.m
    dt = rig.dt
    return dict(x0=_randn(s, (m, e)), o1=_randn(s + 1, (m, e), 0.5).to(dt), g_x1=_randn(s + 2, (m, e), gscale),
                g_o2=_randn(s + 3, (m, e), gscale).to(dt), g_x3=_randn(s + 4, (m, e), gscale),
                g_o1n=_randn(s + 5, (m, e), gscale).to(dt), fill_a=_randn(s + 6, (m, e), gscale),
                fill_b=_randn(s + 7, (m, e), gscale), g_heads=_randn(s + 8, (m, e), gscale))


def _launches(rig):
    return (1, 1), ((2, 2) if rig.split > 1 else (1, 1))


def _layer(device, monkeypatch, capsys, dt, case, gscale=1.0, targets=(TARGET,), last=True, tag=''):
    """Both nodes of one layer, forward and backward, every block against float64 given the one before it."""
    rig = _Rig(device, dt, case, 1900 + sum(case[0]))
    base = f'{NAME[dt]} {_cid(case)}{tag}'
    cmp = _Cmp(capsys, base + ' A')
    i = _inputs(rig, gscale)
    want_a, want_b = _launches(rig)
    got, n, = rig.run_a(monkeypatch, i['x0'], i['o1'], i['g_x1'], i['g_o2'], i['fill_a'])
    assert n == want_a, f'_DecA launches {n}'
    _check_a(cmp, rig, got, i['x0'], i['o1'], i['g_x1'], i['g_o2'], i['fill_a'])
    x1, o2 = got['x1'], got['o2']
    for target in targets:
        gb, n, kv = rig.run_b(monkeypatch, x1, o2, target, i['g_x3'], i['g_o1n'], i['fill_b'])
        assert n == want_b, f'_DecB launches {n}'
        cmp.tag = base + f' B(next {target[0]}x{target[1]})'
        _check_b(cmp, rig, gb, kv, x1, o2, i['g_x3'], i['g_o1n'], i['fill_b'])
    if last:
        gb, n, kv = rig.run_b(monkeypatch, x1, o2, None, i['g_x3'], None, i['fill_b'])
        assert n == want_b, f'_DecB (last layer) launches {n}'
        cmp.tag = base + ' B(last)'
        _check_b(cmp, rig, gb, kv, x1, o2, i['g_x3'], None, i['fill_b'])
    with capsys.disabled():
        print()
    assert not cmp.bad, cmp.bad


@pytest.mark.parametrize('dt,case', CASES, ids=_cid)
def test_production_nodes_against_float64(device, monkeypatch, capsys, dt, case):
    """_DecA and _DecB (with a next layer — on the first case also over 13 x 10 = 130 keys, no multiple of 16 — and as the last
    layer): forward, backward, every parameter gradient, d(positions) into a pre-filled accumulator, the launch counts."""
    targets = (TARGET, TARGET_ODD) if case is C_RAGGED else (TARGET,)
    _layer(device, monkeypatch, capsys, dt, case, targets=targets)


@pytest.mark.parametrize('dt', LO, ids=NAME.get)
def test_small_upstream_gradients_keep_the_relative_bars(device, monkeypatch, capsys, dt):
    """Every upstream gradient (and the accumulator's pre-fill) x 2^-12."""
    _layer(device, monkeypatch, capsys, dt, C_RAGGED, gscale=2.0 ** -12, last=False, tag=' grads x 2^-12')


@pytest.mark.parametrize('branch', ['gq', 'gq-no-g_x3', 'no-g_x1', 'no-g_o1n'])
def test_gradient_branches(device, monkeypatch, capsys, branch):
    """The heads' share of d(x3) from ``hp.gq`` (added and popped; alone when g_x3 is None), g_x1 = None, and g_o1n = None
    with a next layer (no query-projection term: d(positions) untouched, no gradient for the next in_proj)."""
    dt = torch.bfloat16
    rig = _Rig(device, dt, C_RAGGED, 1990)
    cmp = _Cmp(capsys, f'{NAME[dt]} {_cid(C_RAGGED)} {branch}')
    i = _inputs(rig)
    got, _ = rig.run_a(monkeypatch, i['x0'], i['o1'], None if branch == 'no-g_x1' else i['g_x1'], i['g_o2'], i['fill_a'])
    if branch == 'no-g_x1':
        _check_a(cmp, rig, got, i['x0'], i['o1'], None, i['g_o2'], i['fill_a'])
    else:
        x1, o2 = got['x1'], got['o2']
        g_x3 = None if branch == 'gq-no-g_x3' else i['g_x3']
        g_o1n = None if branch == 'no-g_o1n' else i['g_o1n']
        g_heads = i['g_heads'] if branch.startswith('gq') else None
        gb, _, kv = rig.run_b(monkeypatch, x1, o2, TARGET, g_x3, g_o1n, i['fill_b'], g_heads=g_heads)
        _check_b(cmp, rig, gb, kv, x1, o2, g_x3, g_o1n, i['fill_b'], g_heads=g_heads)
    with capsys.disabled():
        print()
    assert not cmp.bad, cmp.bad


def test_backward_without_any_gradient_gives_exact_zeros(device, monkeypatch):
    """g_x3 = None, nothing in ``hp.gq``, g_o1n = None: zeros go in, and LN3's parameter partials, d(b2) and d(x1) are exactly 0."""
    rig = _Rig(device, torch.bfloat16, C_RAGGED, 1991)
    i = _inputs(rig)
    got, _ = rig.run_a(monkeypatch, i['x0'], i['o1'], i['g_x1'], i['g_o2'], i['fill_a'])
    gb, _, _ = rig.run_b(monkeypatch, got['x1'], got['o2'], TARGET, None, None, i['fill_b'], direct=True)
    ret = gb['direct']
    # (lc, head, nxt, x1, o2, token, wo, bo, g2, b2, w1, bb1, w2, bb2, g3, b3, nw_in, nb_in)
    assert all(t is None for t in ret[:3] + [ret[5]] + ret[16:])
    for idx in (3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):
        assert ret[idx] is not None and not ret[idx].any(), f'gradient {idx} is not exactly zero'
    assert torch.equal(gb['acc'], i['fill_b'])


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16, F32], ids=NAME.get)
def test_hard_values_stay_finite(device, monkeypatch, dt):
    """A residual stream with rows at N(50, 1), rows of zeros, a constant row, rows x 2^-20 and x 2^10 (the value set of
    test_k12_paths_gpu.py: the chain's LayerNorm is its own f32 code): every output and gradient is finite."""
    case = C_RAGGED if dt != F32 else C_F32_CHUNKS
    rig = _Rig(device, dt, case, 1992)
    i = _inputs(rig)
    x = i['x0'].clone()
    m = rig.m
    x[0:m:5] += 50.0
    x[1:m:5] = 0.0
    x[2] = 3.25
    x[3:m:5] *= 2.0 ** -20
    x[4:m:5] *= 2.0 ** 10
    got, _ = rig.run_a(monkeypatch, x, i['o1'], i['g_x1'], i['g_o2'], i['fill_a'])
    gb, _, _ = rig.run_b(monkeypatch, x, got['o2'], TARGET, i['g_x3'], i['g_o1n'], i['fill_b'])
    for name, t in list(got.items()) + list(gb.items()):
        if torch.is_tensor(t) and t.is_floating_point():
            assert torch.isfinite(t).all(), f'{name} is not finite'
