"""In-place gradients of arena parameters: `arena_grad` tells one, `accumulate_wgrad` / `accumulate_colsum` / `_wgrad_into` add to
it outside autograd, `_fire_grad_hooks` announces it; `_PENDING` queues a pass's small ones for `flush_deferred_grads`' grouped launches."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib, switches
from ._lib import MaskBevHipError, check
from .ops_gemm_kernels import *          # noqa: F401,F403  (ops_core's and ops_records' names come along)


def arena_grad(p: Optional[torch.Tensor], rows: Optional[tuple] = None) -> Optional[torch.Tensor]:
    """The f32 gradient of arena parameter ``p`` that kernels accumulate into in place — rows ``rows=(r0, r1)`` of it, a
    view — or None: no parameter, not in a :class:`~mask_bev_amd.arena.ParameterArena`, no gradient, or not an f32 one."""
    g = p.grad if getattr(p, '_mbv_arena', False) else None
    if g is None or g.dtype != torch.float32:
        return None
    return g if rows is None else g[rows[0]:rows[1]]


def _compute_copy(p: Optional[torch.Tensor], dt: torch.dtype) -> Optional[torch.Tensor]:
    """The parameter in the compute dtype: the arena's bf16 shadow when there is one (arena.py), else a cast."""
    if p is None or p.dtype == dt:
        return p
    sh = getattr(p, '_mbv_shadow', None)
    if sh is not None and sh.dtype == dt:
        return sh
    return p.to(dt)


def _fire_grad_hooks(*params: torch.Tensor):
    """Gradients accumulated outside autograd still announce themselves to post-accumulate hooks (ddp.py), in argument order."""
    for p in params:
        hooks = getattr(p, '_post_accumulate_grad_hooks', None)
        if hooks:
            for h in list(hooks.values()):
                h(p)


def colsum_accum(g2: torch.Tensor, out: torch.Tensor, persistent: bool = False):
    """out (N,) f32 += column sums of g2 (T, N) (bf16 or f32) — the bias gradient, in one launch.
    ``persistent``: ``out`` is an arena gradient — inside a backward pass the sum joins the grouped launch at its end."""
    lib = _lib.load()
    _need_gpu(g2, out)
    if g2.dtype not in _ACT_DTYPES or out.dtype != torch.float32 or not out.is_contiguous():
        raise MaskBevHipError('colsum_accum: g2 must be f32, bf16 or fp16 and out contiguous f32')
    g2 = g2.contiguous()
    if persistent and _defer_colsum(g2, out, g2.shape[0], g2.shape[1], g2.shape[1]):
        return
    check(lib.mbv_colsum_accum(_ptr(g2), _dt_flag(g2.dtype), g2.shape[0], g2.shape[1], _ptr(out),
                               _stream()), 'mbv_colsum_accum')


# Parameter gradients are nobody's input.  During a backward pass the small ones — exact-f32 weight gradients of the
# decoder's few-row Linears, bias gradients (column sums), the per-block partial rows of K12's LayerNorm-parameter
# gradients — are collected and issued as a few grouped launches (mbv_wgrad_small_f32_group, mbv_colsum_accum_group)
# from an autograd-engine callback at the end of that pass: ≈ 140 launches of 5-12 us with the chip mostly idle become
# four that fill it.  Only accumulations into ARENA gradients are deferred (nothing reads those before the pass ends).
# `switches.wgrad_group = False` keeps the per-layer launches (A/B).
# One record per kind of deferred work (`stream`: its producer's) — an entry of mbv_wgrad_small_f32_group (bias_acc += column sums
# of g), of mbv_colsum_accum_group (the (rows, n) block of g that starts `offset` elements in, row stride ld), of mbv_gemm16_tn_group,
# of mbv_gemm32s_tn_group (absmax records; None: found at the flush) — and the four lists of a pass, each in arrival order.
_T, _OT = torch.Tensor, Optional[torch.Tensor]
SmallWgrad = NamedTuple('SmallWgrad', [('g', _T), ('x', _T), ('acc', _T), ('bias_acc', _OT), ('stream', object)])
ColSum = NamedTuple('ColSum', [('g', _T), ('out', _T), ('rows', int), ('n', int), ('ld', int), ('offset', int), ('stream', object)])
K17Wgrad = NamedTuple('K17Wgrad', [('g', _T), ('x', _T), ('acc', _T), ('stream', object)])
K20Wgrad = NamedTuple('K20Wgrad', [('g', _T), ('x', _T), ('acc', _T), ('amax_g', _OT), ('amax_x', _OT), ('stream', object)])
PendingPass = NamedTuple('PendingPass', [('small', list), ('colsum', list), ('tn', list), ('tn32', list)])
del NamedTuple, _T, _OT      # (every name left in this module is re-exported by `ops`)


def _small_as_k20(it: SmallWgrad) -> K20Wgrad:
    """fp32 compute: the product of a small-f32 entry as an entry of the grouped K20 launch (absmax found at the flush) ..."""
    return K20Wgrad(it.g, it.x, it.acc, None, None, it.stream)


def _small_bias_colsum(it: SmallWgrad) -> ColSum:
    """... and its bias column sums as an entry of the column-sum group."""
    return ColSum(it.g, it.bias_acc, it.g.shape[0], it.g.shape[1], it.g.stride(0), 0, it.stream)


_PENDING: dict = {}          # autograd graph-task id -> PendingPass of that backward pass; mutated, never rebound
_PENDING_MAX = 32            # entries kept at most: nesting depth of re-entrant passes + leftovers of passes that raised


def _pending_lists():
    """The pending lists of the running backward pass (creating them and arming the end-of-pass callback on first use),
    or None outside a pass / with the switch off.  Keyed by the engine's graph-task id: a re-entrant pass (the deferred
    heads re-evaluate a sub-graph inside the outer backward) flushes its own work, and what a pass that raised left
    behind is never mistaken for the next pass's work."""
    if not switches.get('wgrad_group'):
        return None
    tid = torch._C._current_graph_task_id()
    if tid < 0:
        return None
    lists = _PENDING.get(tid)
    if lists is None:
        try:        # the callback runs when this pass has executed every node
            torch.autograd.Variable._execution_engine.queue_callback(lambda: flush_deferred_grads(tid))
        except RuntimeError:
            return None
        # Leftovers of passes that raised before their callback ran hold (g, x) activations alive.  A live pass cannot be
        # told from a dead one by its id (an outer pass stays live while any number of inner passes come and go, each
        # with a higher id), but every pass that ENDS removes its entry, so the entries that exist are the nesting
        # depth plus the leaked ones: only when far more exist than passes can nest are the oldest dropped.
        if len(_PENDING) >= _PENDING_MAX:
            for old in sorted(_PENDING)[:len(_PENDING) - _PENDING_MAX + 1]:
                del _PENDING[old]
        lists = _PENDING[tid] = PendingPass([], [], [], [])
    return lists


def _defer_ok() -> bool:
    return _pending_lists() is not None


def _defer_small_wgrad(g2, x2, acc, bias_acc) -> bool:
    lists = _pending_lists()
    if lists is not None:
        lists.small.append(SmallWgrad(g2, x2, acc, bias_acc, torch.cuda.current_stream()))
    return lists is not None


def _defer_tn_wgrad(g2: torch.Tensor, x2: torch.Tensor, acc: torch.Tensor) -> bool:
    """`switches.tn_group`: ``1`` (default) — the K17 weight gradients of a backward pass are collected and issued as grouped
    launches at its end (mbv_gemm16_tn_group); ``all`` — every 16-bit arena weight gradient with at least 512 tokens joins
    the group, also those the per-layer policy leaves to the library (few tokens, wide inputs); ``0`` — per-layer launches."""
    lists = None if switches.get('tn_group') == '0' or not acc.is_contiguous() else _pending_lists()
    if lists is not None:
        lists.tn.append(K17Wgrad(g2, x2, acc, torch.cuda.current_stream()))
    return lists is not None


def _defer_tn32_wgrad(g2: torch.Tensor, x2: torch.Tensor, acc: torch.Tensor, amax) -> bool:
    """fp32 compute: a token-major K20 weight gradient joins the pass's grouped launch (``switches.tn32_group``)."""
    lists = _pending_lists() if switches.get('tn32_group') else None
    if lists is None:
        return False
    ag, ax = (None, None) if amax is None else (amax[0], amax[1])
    if switches.get('amax_hints'):      # resolved NOW: a hint lives as long as the tensor object it was left on, not until the flush
        ag = amax_hint_get(g2) if ag is None else ag
        ax = amax_hint_get(x2) if ax is None else ax
    lists.tn32.append(K20Wgrad(g2, x2, acc, ag, ax, torch.cuda.current_stream()))
    return True


def launch_tn_group(items) -> None:
    """The grouped launch(es) for a pass's products: deepest token sums first (their work items are the longest of a
    launch), one call per 16-bit dtype."""
    items = sorted(items, key=lambda it: -it[0].shape[0])
    # destinations an optimizer armed (FlatAdam.fuse_matrices): the launch applies their AdamW update in its epilogue.  An
    # armed destination takes ONE product per pass — a tied weight would be updated twice — so a second one raises.
    opt, blocks, seen = None, {}, set()
    for it in items:
        arm = _adam_arm(it[2])
        if arm is None or (opt is not None and arm is not opt):
            continue
        if it[2].data_ptr() in seen:
            raise MaskBevHipError('launch_tn_group: two products for one destination whose AdamW update is fused into its '
                                  'weight-gradient GEMM (a tied weight needs FlatAdam.fuse_matrices(None))')
        block = arm.claim_matrix(it[2])
        if block:
            opt = arm
            seen.add(it[2].data_ptr())
            blocks[it[2].data_ptr()] = block
    if opt is not None and not torch.cuda.is_current_stream_capturing():
        opt.write_adam_blocks()          # an eager pass: by value, right in front of the launch that reads them
    for dt in {it[0].dtype for it in items}:
        for wave in _distinct_destination_waves([it for it in items if it[0].dtype == dt]):
            fused = gemm16_tn_group(wave, [blocks.get(it[2].data_ptr(), 0) for it in wave], opt)
            if opt is not None:
                opt.note_matrices_applied([it[2] for it, f in zip(wave, fused) if f])


def _adam_arm(acc: torch.Tensor):
    """The optimizer that armed arena gradient ``acc`` for the fused update (a weak reference on the tensor object), or None."""
    ref = getattr(acc, '_mbv_adam', None)
    return None if ref is None or not switches.get('adam_in_wgrad') else ref()


def _distinct_destination_waves(items):
    """Split ``(g, x, acc)`` products into successive launches whose ``acc`` ranges are pairwise disjoint.  Inside one
    grouped launch a destination is read-modified-written without atomics (single-range entries add their tile in
    place, multi-range entries are folded in by ``k_add_parts_group``), so a weight used twice in one backward pass —
    tied weights, one Linear applied twice — must not meet itself in a launch: its second product goes to the next
    one, which the stream orders behind the first."""
    waves = []                       # [(items, [(lo, hi) byte ranges])]
    for it in items:
        lo = it[2].data_ptr()
        hi = lo + it[2].numel() * it[2].element_size()
        for w_items, w_ranges in waves:
            if all(hi <= a or lo >= b for a, b in w_ranges):
                w_items.append(it)
                w_ranges.append((lo, hi))
                break
        else:
            waves.append(([it], [(lo, hi)]))
    return [w for w, _ in waves]


def _defer_colsum(g2: torch.Tensor, out: torch.Tensor, rows: int, n: int, ld: int, offset: int = 0) -> bool:
    """out (n,) f32 += column sums of the (rows, n) block of ``g2`` that starts ``offset`` elements in, row stride ld."""
    ok = g2.is_cuda and g2.dtype in _ACT_DTYPES and out.dtype == torch.float32 and out.is_contiguous()
    lists = _pending_lists() if ok else None
    if lists is not None:
        lists.colsum.append(ColSum(g2, out, int(rows), int(n), int(ld), int(offset), torch.cuda.current_stream()))
    return lists is not None


def _colsum_now(g2: torch.Tensor, out: torch.Tensor, rows: int, n: int, ld: int, offset: int = 0) -> None:
    """The immediate form of :func:`_defer_colsum` (the kernel that produced ``g2`` was told its reduction comes later,
    so when the queue refuses it the reduction has to happen here — dropping it would lose the gradient silently)."""
    if g2.dtype not in _ACT_DTYPES or out.dtype != torch.float32:
        raise MaskBevHipError('column-sum accumulate: g2 must be f32, bf16 or fp16 and out f32')
    if not out.is_contiguous():
        tmp = torch.zeros(n, dtype=torch.float32, device=out.device)
        _colsum_now(g2, tmp, rows, n, ld, offset)
        out.add_(tmp)
        return
    lib = _lib.load()
    PA, IA, LA = ctypes.c_void_p * 1, ctypes.c_int32 * 1, ctypes.c_int64 * 1
    check(lib.mbv_colsum_accum_group(PA(g2.data_ptr() + offset * g2.element_size()), IA(_dt_flag(g2.dtype)),
                                     LA(int(rows)), IA(int(n)), LA(int(ld)), PA(out.data_ptr()), 1, _stream()),
          'mbv_colsum_accum_group')


def accumulate_colsum(g2: torch.Tensor, out: torch.Tensor, rows: int, n: int, ld: int, offset: int = 0) -> None:
    """:func:`_defer_colsum` when the running backward pass's queue takes the work, else :func:`_colsum_now`."""
    if not _defer_colsum(g2, out, rows, n, ld, offset):
        _colsum_now(g2, out, rows, n, ld, offset)


def flush_deferred_grads(task_id: Optional[int] = None) -> None:
    """Issue the parameter-gradient work collected by backward pass ``task_id`` (default: by every pass that has some
    pending — callable directly; a no-op when nothing is pending)."""
    tids = [task_id] if task_id is not None else list(_PENDING)
    if task_id is not None:          # passes nested INSIDE this one have ended: what they left (they raised) is dropped
        for t in [t for t in _PENDING if t > task_id]:
            del _PENDING[t]
    passes = [_PENDING.pop(t) for t in tids if t in _PENDING]
    wg, cs = [it for p in passes for it in p.small], [it for p in passes for it in p.colsum]
    tn, tn32 = [it for p in passes for it in p.tn], [it for p in passes for it in p.tn32]
    if not wg and not cs and not tn and not tn32:
        return
    lib = _lib.load()
    cur = torch.cuda.current_stream()
    wg_all = list(wg)
    for st in {it.stream for it in wg + cs + tn + tn32}:
        if st != cur:
            cur.wait_stream(st)
    if tn:
        launch_tn_group([(it.g, it.x, it.acc) for it in tn])
    if wg and switches.get('gemm32s') and switches.get('tn32_group'):
        # fp32 compute: the few-row products K20 takes (n, k multiples of 8, aligned rows) leave the exact-f32 MFMA group
        # for ONE grouped K20 launch (+ one absmax launch per 32 products); their bias column sums join the column-sum group
        k20 = [it for it in wg if (it.g.dtype == torch.float32 and it.x.dtype == torch.float32 and it.g.shape[0] <= 8192
                                   and _gemm32s_ok(it.g, it.x) and it.acc.dtype == torch.float32 and it.acc.is_contiguous()
                                   and it.acc.data_ptr() % 16 == 0
                                   and (it.bias_acc is None or (it.bias_acc.dtype == torch.float32
                                                                and it.bias_acc.is_contiguous())))]
        if k20:
            ids = {id(it) for it in k20}
            wg = [it for it in wg if id(it) not in ids]
            tn32 = tn32 + [_small_as_k20(it) for it in k20]
            cs += [_small_bias_colsum(it) for it in k20 if it.bias_acc is not None]
    if tn32:
        # deepest token sums first (their work items are the longest of a launch); a weight used twice meets itself in the next launch
        for wave in _distinct_destination_waves(sorted(tn32, key=lambda it: -it.g.shape[0])):
            gemm32s_tn_group([(it.g, it.x, it.acc, it.amax_g, it.amax_x) for it in wave])
    if wg:
        n = len(wg)
        PA, IA = ctypes.c_void_p * n, ctypes.c_int32 * n
        check(lib.mbv_wgrad_small_f32_group(
            PA(*[it.g.data_ptr() for it in wg]), PA(*[it.x.data_ptr() for it in wg]),
            PA(*[it.acc.data_ptr() for it in wg]), PA(*[(it.bias_acc.data_ptr() if it.bias_acc is not None else 0) for it in wg]),
            IA(*[it.g.shape[0] for it in wg]), IA(*[it.g.shape[1] for it in wg]), IA(*[it.x.shape[1] for it in wg]),
            n, _stream()), 'mbv_wgrad_small_f32_group')
    if cs:
        n = len(cs)
        PA, IA, LA = ctypes.c_void_p * n, ctypes.c_int32 * n, ctypes.c_int64 * n
        check(lib.mbv_colsum_accum_group(
            PA(*[it.g.data_ptr() + it.offset * it.g.element_size() for it in cs]), IA(*[_dt_flag(it.g.dtype) for it in cs]),
            LA(*[it.rows for it in cs]), IA(*[it.n for it in cs]), LA(*[it.ld for it in cs]),
            PA(*[it.out.data_ptr() for it in cs]), n, _stream()), 'mbv_colsum_accum_group')
    for it in wg_all + tn + tn32:     # the producers' memory may be reused by later work on their own streams
        if it.stream != cur:
            it.g.record_stream(cur)
            it.x.record_stream(cur)
    for it in cs:
        if it.stream != cur:
            it.g.record_stream(cur)


def _wgrad_splits(tokens: int) -> int:
    """The weight gradient dW = dY^T X has tiny M x N (channels) and K = tokens (up to 65 536): one library GEMM
    under-fills the chip (measured 290 us vs 47 us at T = 65 536, 192 -> 576, MI355X).  Split K into chunks
    solved as one batched GEMM and reduce the partials in f32."""
    for s, t in ((128, 131072), (32, 32768), (8, 8192)):
        if tokens >= t:
            return s
    return 1


def _wgrad_into(acc: torch.Tensor, g2: torch.Tensor, x2: torch.Tensor, bias_acc: Optional[torch.Tensor] = None,
                persistent: bool = False, amax=None) -> bool:
    """acc (out, in) f32 += g2^T x2, f32 accumulation inside the GEMM (no bf16 round trip, no separate add).
    Returns True when ``bias_acc`` (out,) f32 += column sums of g2 was done by the same launch.
    ``persistent``: ``acc`` / ``bias_acc`` are arena gradients nobody reads before the backward pass ends — the
    small-token form may then be deferred to the grouped launch at the end of the pass."""
    t = g2.shape[0]
    if ((amax is not None or (g2.dtype == torch.float32 and x2.dtype == torch.float32 and g2.is_cuda and gemm32s_wants(t)))
            and acc.dtype == torch.float32 and acc.is_contiguous() and acc.data_ptr() % 16 == 0 and _gemm32s_ok(g2, x2)):
        # fp32 compute: K20, token sum in parts, owner adds (the absmax words come from the layer's forward when it has them);
        # an arena gradient joins the pass's grouped launch
        if persistent and _defer_tn32_wgrad(g2, x2, acc, amax):
            return False
        gemm32s_tn_acc(acc, g2, x2, None if amax is None else amax[0], None if amax is None else amax[1])
        return False
    if (g2.dtype in _GEMM16_DT and x2.dtype == g2.dtype and acc.stride(-1) == 1 and acc.data_ptr() % 16 == 0
            and gemm16_policy() != 'none' and _gemm16_ok(g2, x2)):
        per_layer = _k17_wants('wgrad', t) and (x2.shape[1] <= switches.get('tn_max_in') or gemm16_policy() == 'all')   # 2048-wide patch rows: the library wins (77 vs 95 us)
        # few-token 16-bit products (the decoder's 400-row output projections: a 256 x 256 result over 400 rows) are a
        # handful of work items of the grouped launch; alone, the library ran them as ONE 256 x 256 tile — 30 us each
        few = t <= 512 and gemm16_policy() == 'auto'       # (1024-token layers stay with the library unless `armed`: measured)
        # a destination whose AdamW update the grouped launch performs (FlatAdam.fuse_matrices) joins it whenever its token sum
        # is one work item deep, also where the GEMM alone is the library's (Swin stage 4's 1024 tokens, 3072-wide fc2 rows):
        # the comparison is now GEMM + 34 B per parameter of optimizer pass against a GEMM with a 26-byte epilogue
        armed = (switches.get('adam_wgrad_min_tokens') <= t <= 4096 and gemm16_policy() == 'auto'
                 and acc.is_contiguous() and _adam_arm(acc) is not None)
        if (persistent and (per_layer or few or armed or (switches.get('tn_group') == 'all' and t >= 512))
                and _defer_tn_wgrad(g2, x2, acc)):
            return False                         # K17, grouped with the pass's other weight gradients at its end
        if per_layer:
            gemm16_tn_acc(acc, g2, x2)           # K17: split over the tokens, parts added into the arena
            return False
    if (g2.dtype == torch.float32 and x2.dtype == torch.float32 and t <= _SMALL_F32_ROWS and g2.is_cuda
            and acc.is_contiguous()):
        lib = _lib.load()
        g2, x2 = g2.contiguous(), x2.contiguous()
        fuse = bias_acc is not None and bias_acc.is_contiguous() and bias_acc.dtype == torch.float32
        if persistent and _defer_small_wgrad(g2, x2, acc, bias_acc if fuse else None):
            return fuse
        check(lib.mbv_wgrad_small_f32(_ptr(g2), _ptr(x2), t, g2.shape[1], x2.shape[1], _ptr(acc),
                                      _ptr(bias_acc) if fuse else ctypes.c_void_p(0), _stream()),
              'mbv_wgrad_small_f32')
        return fuse
    s = _wgrad_splits(t)
    od = {} if g2.dtype == torch.float32 else dict(out_dtype=torch.float32)
    if s == 1:
        torch.addmm(acc, g2.t(), x2, out=acc, **od)
        return False
    c = t // s
    part = torch.bmm(g2[:s * c].view(s, c, -1).transpose(1, 2), x2[:s * c].view(s, c, -1), **od)
    if s * c < t:
        torch.addmm(acc, g2[s * c:].t(), x2[s * c:], out=acc, **od)
    if acc.is_contiguous() and part.is_cuda:
        colsum_accum(part.view(s, -1), acc.view(-1))         # Σ over the K-chunks, added in the same launch
    else:
        acc.add_(part.sum(0))
    return False


def accumulate_wgrad(p: torch.Tensor, g2: torch.Tensor, x2: torch.Tensor, rows: Optional[tuple] = None, amax=None) -> None:
    """Arena parameter ``p``'s gradient (its row range ``rows``) += g2^T x2 through :func:`_wgrad_into`, then announced."""
    _wgrad_into(arena_grad(p, rows), g2, x2, None, persistent=True, amax=amax)
    _fire_grad_hooks(p)


# every name of this module — the underscore helpers included — is part of the package-internal surface `ops` re-exports
__all__ = [_n for _n in list(globals()) if not _n.startswith('__')]
