"""What launches a GEMM and what decides who takes one: K17 (16-bit MFMA, csrc/gemm.hip), K20 (f32 products from IEEE-half pairs,
csrc/gemm_f32s.hip), the library-or-K20 f32 products.  The bottom layer: no autograd node and no queue (ops_pgrad, ops_gemm build on it)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib, switches
from ._lib import MaskBevHipError, check
from .ops_records import *          # noqa: F401,F403  (ops_core's names come along)


_GEMM16_DT = {torch.bfloat16: 0, torch.float16: 1}
_ACT = {None: 0, 'none': 0, 'relu': 1, 'gelu': 2}


def gemm16_enabled() -> bool:
    """A/B switch: `switches.gemm16 = '0'` sends every Linear back to the library GEMM."""
    return switches.get('gemm16') != '0'


def gemm16_policy() -> str:
    """Which Linear work runs on K17 (csrc/gemm.hip) instead of the library GEMM.  `switches.gemm16` =
    ``auto`` (default): the fused forms — FFN input layer + activation, FFN output layer's data gradient + activation
    backward + bias gradient — and the arena-accumulating weight gradient, for token counts where K17 measured at or
    above the library (scratch/bench_gemm.py, profiles/r02); ``all``: every eligible Linear, forward and backward;
    ``0``: none (the round-1 path)."""
    v = switches.get('gemm16')
    return {'1': 'auto', '0': 'none'}.get(v, v)


# below these token counts the 128 x 128 tiles under-fill the chip and the library's split / stream-K kernels win
# (scratch/bench_gemm.py on the bench shapes, profiles/r02/c_gemm_shapes.txt).  The fused FFN forms pay down to 4096
# tokens (Swin stage 3): the K17 GEMM alone is slower there than the library's, but it replaces GEMM + GELU forward and
# GEMM + activation-backward/column-sum pass backward — step A/B 8192 / 4096 / 1024: 29.19 / 28.92 / 30.51 ms
def _k17_min_tokens(kind: str) -> Optional[int]:
    return {'fused': switches.get('k17_fused_min'), 'wgrad': 4096}.get(kind)


def _k17_wants(kind: str, tokens: int) -> bool:
    pol = gemm16_policy()
    if pol == 'none':
        return False
    if pol == 'all':
        return True
    floor = _k17_min_tokens(kind)
    return floor is not None and tokens >= floor


def _gemm16_ok(*ts: torch.Tensor) -> bool:
    dt = ts[0].dtype
    return (dt in _GEMM16_DT and all(t.is_cuda and t.dtype == dt and t.dim() == 2 and t.stride(1) == 1
                                     and t.stride(0) % 8 == 0 and t.shape[1] % 8 == 0 and t.data_ptr() % 16 == 0
                                     and t.shape[0] * t.stride(0) * 2 < 0x7fff0000 for t in ts))


def gemm16_nt(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
              out_dtype: Optional[torch.dtype] = None, want_pre: bool = False):
    """``act(x (M, K) @ w (N, K)^T + bias)`` on K17 (bf16 / fp16 inputs, f32 accumulation).  Returns ``out`` or
    ``(out, pre_activation)`` with ``want_pre``.  ``bias`` f32 (N,).  Raises MaskBevHipError for shapes K17 does not take
    (check with :func:`gemm16_nt_ok`)."""
    lib = _lib.load()
    if not _gemm16_ok(x, w) or x.shape[1] != w.shape[1]:
        raise MaskBevHipError('gemm16_nt: unsupported operands')
    m, k = x.shape
    n = w.shape[0]
    od = out_dtype or x.dtype
    if od not in (x.dtype, torch.float32):
        raise MaskBevHipError('gemm16_nt: out dtype must be the input dtype or f32')
    out = torch.empty((m, n), dtype=od, device=x.device)
    pre = torch.empty((m, n), dtype=od, device=x.device) if (want_pre and _ACT[act]) else None
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.data_ptr() % 16):
        raise MaskBevHipError('gemm16_nt: bias must be contiguous f32, 16-byte aligned')
    check(lib.mbv_gemm16_nt(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(pre), m, n, k, x.stride(0), w.stride(0), n,
                            _GEMM16_DT[x.dtype], int(od == torch.float32), _ACT[act], 1, 0, 0, 0, _stream()),
          'mbv_gemm16_nt')
    return (out, pre) if want_pre else out


def gemm16_nn(g: torch.Tensor, w: torch.Tensor, act: Optional[str] = None, aux: Optional[torch.Tensor] = None,
              colsum: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None, colsum_sink=None) -> torch.Tensor:
    """``act'(aux) * (g (M, N) @ w (N, K))`` on K17: the data gradient of a Linear, optionally multiplied by the
    derivative of the activation in front of it (``aux``: ReLU output / GELU pre-activation, (M, K)) with the column
    sums of the result added to ``colsum`` (K,) f32.  ``colsum_sink`` (ops_pgrad.accumulate_colsum): the launch leaves
    its per-wave-row partial sums as rows of a tensor and hands ``(parts, colsum, rows, K, K)`` to it instead."""
    lib = _lib.load()
    if not _gemm16_ok(g, w) or g.shape[1] != w.shape[0]:
        raise MaskBevHipError('gemm16_nn: unsupported operands')
    m, n = g.shape
    k = w.shape[1]
    a = _ACT[act]
    if a and (aux is None or not _gemm16_ok(aux) or aux.dtype != g.dtype or tuple(aux.shape) != (m, k)):
        raise MaskBevHipError('gemm16_nn: aux must be a (M, K) tensor of the input dtype')
    od = out_dtype or g.dtype
    out = torch.empty((m, k), dtype=od, device=g.device)
    if colsum is not None and (colsum.dtype != torch.float32 or not colsum.is_contiguous()):
        raise MaskBevHipError('gemm16_nn: colsum must be contiguous f32')
    if colsum is not None and colsum_sink is not None:
        # inside a backward pass the per-wave-row partial sums join the pass's grouped column-sum launch (one small
        # reduction launch per fused data gradient less: 16 per step); the rows live in a tensor of their own until then
        rows = int(lib.mbv_gemm16_nn_part_rows(m, k, 1))
        parts = torch.empty(int(lib.mbv_gemm16_nn_workspace_bytes(m, k, 1)) // 4, dtype=torch.float32, device=g.device)
        check(lib.mbv_gemm16_nn_parts(_ptr(g), _ptr(w), _ptr(out), _ptr(aux if a else None), _ptr(parts), parts.numel() * 4,
                                      m, n, k, g.stride(0), w.stride(0), k, aux.stride(0) if a else 0,
                                      _GEMM16_DT[g.dtype], int(od == torch.float32), a, 1, 0, 0, 0, _stream()),
              'mbv_gemm16_nn_parts')
        colsum_sink(parts, colsum, rows, k, k)
        return out
    ws = _workspace(lib.mbv_gemm16_nn_workspace_bytes(m, k, 1), g.device) if colsum is not None else None
    check(lib.mbv_gemm16_nn(_ptr(g), _ptr(w), _ptr(out), _ptr(aux if a else None), _ptr(colsum), m, n, k, g.stride(0),
                            w.stride(0), k, aux.stride(0) if a else 0, _GEMM16_DT[g.dtype],
                            int(od == torch.float32), a, 1, 0, 0, 0, _ptr(ws), 0 if ws is None else ws.numel(),
                            _stream()), 'mbv_gemm16_nn')
    return out


def gemm16_tn_acc(acc: torch.Tensor, g: torch.Tensor, x: torch.Tensor, splits: int = 0) -> None:
    """``acc (N, K) f32 += g (M, N)^T @ x (M, K)`` on K17 (split over M, f32 atomic adds): the weight gradient of a
    Linear accumulated straight into the arena."""
    lib = _lib.load()
    if (not _gemm16_ok(g, x) or g.shape[0] != x.shape[0] or acc.dtype != torch.float32 or acc.stride(1) != 1
            or tuple(acc.shape) != (g.shape[1], x.shape[1]) or acc.data_ptr() % 16):
        raise MaskBevHipError('gemm16_tn_acc: unsupported operands')
    m, n = g.shape
    k = x.shape[1]
    ws = None
    if acc.is_contiguous():               # partial results + owner-adds instead of atomics
        ws = _workspace(lib.mbv_gemm16_tn_workspace_bytes(m, n, k), g.device)
    check(lib.mbv_gemm16_tn(_ptr(g), _ptr(x), _ptr(acc), m, n, k, g.stride(0), x.stride(0), acc.stride(0),
                            _GEMM16_DT[g.dtype], 1, 1, int(splits), 1, 0, 0, 0, _ptr(ws),
                            0 if ws is None else ws.numel(), _stream()), 'mbv_gemm16_tn')


def gemm16_nt_acc(x: torch.Tensor, w: torch.Tensor, splits: int = 0) -> torch.Tensor:
    """``x (B, M, K) @ w (B, N, K)^T`` → (B, M, N) f32 on K17 with the contraction split over workgroups (f32 atomic
    adds into a zeroed result): few rows, long K."""
    lib = _lib.load()
    if x.dim() != 3 or w.dim() != 3 or x.shape[0] != w.shape[0] or x.shape[2] != w.shape[2]:
        raise MaskBevHipError('gemm16_nt_acc: (B, M, K) and (B, N, K) operands')
    x, w = x.contiguous(), w.contiguous()
    if not _gemm16_ok(x[0], w[0]):
        raise MaskBevHipError('gemm16_nt_acc: unsupported operands')
    b, m, k = x.shape
    n = w.shape[1]
    out = torch.zeros((b, m, n), dtype=torch.float32, device=x.device)
    check(lib.mbv_gemm16_nt_acc(_ptr(x), _ptr(w), _ptr(out), m, n, k, k, k, n, _GEMM16_DT[x.dtype], int(splits), b,
                                m * k, n * k, m * n, _stream()), 'mbv_gemm16_nt_acc')
    return out


def mask_logits_backward(dl: torch.Tensor, embed: torch.Tensor, feature: torch.Tensor):
    """Backward of ``einsum('bqc,bcp->bqp', embed, feature)`` (/root/reference: mask_bev/models/networks/
    mask2former_head/mask2former_head.py:459) for dl (B, R, P), embed (B, R, C), feature (B, C, P):
    ``d_embed = dl . feature^T`` (B, R, C) f32 and ``d_feature = embed^T . dl`` (B, C, P) in the operands' dtype.  16-bit
    operands run on K17 (split-K NT with f32 atomics; batched TN stored once); anything else on the library GEMM."""
    if (dl.is_cuda and dl.dtype in _GEMM16_DT and embed.dtype == dl.dtype and feature.dtype == dl.dtype
            and gemm16_policy() != 'none' and dl.shape[2] % 8 == 0 and embed.shape[2] % 8 == 0):
        dl, embed, feature = dl.contiguous(), embed.contiguous(), feature.contiguous()
        if _gemm16_ok(dl[0], embed[0], feature[0]):
            return gemm16_nt_acc(dl, feature), gemm16_tn(embed, dl)
    return torch.bmm(dl, feature.transpose(1, 2)), torch.bmm(embed.transpose(1, 2), dl)


def gemm16_tn(g: torch.Tensor, x: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``g (B, M, N)^T @ x (B, M, K)`` → (B, N, K), stored once per tile (no split over M)."""
    lib = _lib.load()
    if g.dim() != 3 or x.dim() != 3 or g.shape[:2] != x.shape[:2] or not g.is_contiguous() or not x.is_contiguous():
        raise MaskBevHipError('gemm16_tn: (B, M, N) and (B, M, K) contiguous operands')
    if not _gemm16_ok(g[0], x[0]):
        raise MaskBevHipError('gemm16_tn: unsupported operands')
    b, m, n = g.shape
    k = x.shape[2]
    od = out_dtype or g.dtype
    out = torch.empty((b, n, k), dtype=od, device=g.device)
    check(lib.mbv_gemm16_tn(_ptr(g), _ptr(x), _ptr(out), m, n, k, n, k, k, _GEMM16_DT[g.dtype], 0,
                            int(od == torch.float32), 1, b, m * n, m * k, n * k, None, 0, _stream()), 'mbv_gemm16_tn')
    return out


def gemm16_tn_group(items, adam=None, optimizer=None):
    """``acc (N, K) f32 += g (M, N)^T @ x (M, K)`` for every ``(g, x, acc)`` of ``items`` in one K17 launch per 48 (all of
    one 16-bit dtype, contiguous ``acc``).

    ``adam`` (with ``optimizer``, a :class:`~mask_bev_amd.arena.FlatAdam`): per item the device address of the hyper-parameter
    block of its parameter group, or 0 — an item with a block whose token sum is one work item deep takes the AdamW update
    of its weight in the product's epilogue instead of adding to ``acc`` (mbv_gemm16_tn_group_adam).  Returns one flag per
    item: whether the launch applied its update."""
    if not items:
        return []
    lib = _lib.load()
    n = len(items)
    dt = items[0][0].dtype
    for g, x, acc in items:
        if (g.dtype != dt or not _gemm16_ok(g, x) or g.shape[0] != x.shape[0] or acc.dtype != torch.float32
                or not acc.is_contiguous() or tuple(acc.shape) != (g.shape[1], x.shape[1]) or acc.data_ptr() % 16):
            raise MaskBevHipError('gemm16_tn_group: unsupported operands')
    PA, LA = ctypes.c_void_p * n, ctypes.c_int64 * n
    m, nn, k = LA(*[g.shape[0] for g, _, _ in items]), LA(*[g.shape[1] for g, _, _ in items]), \
        LA(*[x.shape[1] for _, x, _ in items])
    nbytes = lib.mbv_gemm16_tn_group_workspace_bytes(m, nn, k, n)
    ws = _workspace(nbytes, items[0][0].device) if nbytes else None
    ptrs = (PA(*[g.data_ptr() for g, _, _ in items]), PA(*[x.data_ptr() for _, x, _ in items]),
            PA(*[a.data_ptr() for _, _, a in items]), m, nn, k,
            LA(*[g.stride(0) for g, _, _ in items]), LA(*[x.stride(0) for _, x, _ in items]),
            n, _GEMM16_DT[dt], _ptr(ws), int(nbytes))
    if adam is None or optimizer is None or not any(adam):
        check(lib.mbv_gemm16_tn_group(*ptrs, _stream()), 'mbv_gemm16_tn_group')
        return [False] * n
    ar = optimizer.arena
    fused = (ctypes.c_int32 * n)()
    check(lib.mbv_gemm16_tn_group_adam(*ptrs, PA(*[int(b or 0) for b in adam]), ar.grad.data_ptr(), ar.param.data_ptr(),
                                       optimizer.exp_avg.data_ptr(), optimizer.exp_avg_sq.data_ptr(), _ptr(ar.shadow),
                                       ar.numel, fused, _stream()), 'mbv_gemm16_tn_group_adam')
    return [bool(f) for f in fused]


def _gemm32s_ok(*ts: torch.Tensor) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0
               and t.shape[1] % 8 == 0 and t.data_ptr() % 16 == 0 and t.shape[0] * t.stride(0) * 4 < 0x7fff0000 for t in ts)


def _amax_ptr(amax, i: int):
    """Pointer to record i of ``amax``: an (n, 64) tensor of records, or a tuple of one-record tensors."""
    if amax is None:
        return ctypes.c_void_p(0)
    if isinstance(amax, (tuple, list)):
        return ctypes.c_void_p(0 if amax[i] is None else amax[i].data_ptr())
    return ctypes.c_void_p(amax.data_ptr() + 4 * AMAX_SLOTS * i)


def gemm32s_nt(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
               amax: Optional[torch.Tensor] = None, want_pre: bool = False, hint_out: bool = False):
    """``act(x (M, K) @ w (N, K)^T + bias)`` in f32 on K20.  ``amax`` = ``f32_absmax([x, w])`` (computed here when None).
    ``hint_out``: the epilogue max-combines |out| into an absmax record left as a hint for the next K20 product."""
    lib = _lib.load()
    if not _gemm32s_ok(x, w) or x.shape[1] != w.shape[1] or w.shape[0] % 8:
        raise MaskBevHipError('gemm32s_nt: unsupported operands')
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.data_ptr() % 16):
        raise MaskBevHipError('gemm32s_nt: bias must be contiguous f32, 16-byte aligned')
    if amax is None:
        amax = tuple(operand_amax([x, w], (True, False)))
    m, k = x.shape
    n = w.shape[0]
    out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    pre = torch.empty((m, n), dtype=torch.float32, device=x.device) if (want_pre and _ACT[act]) else None
    rec = amax_record(x.device) if hint_out else None
    AMAX_VERIFY.check(x, amax[0], 'gemm32s_nt x')
    AMAX_VERIFY.check(w, amax[1], 'gemm32s_nt w')
    check(lib.mbv_gemm32s_nt(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(pre), m, n, k, x.stride(0), w.stride(0), n,
                             _amax_ptr(amax, 0), _amax_ptr(amax, 1), _ptr(rec), _ACT[act], 1, 0, 0, 0, _stream()),
          'mbv_gemm32s_nt')
    amax_hint_set(out, rec)
    return (out, pre) if want_pre else out


def gemm32s_nn(g: torch.Tensor, w: torch.Tensor, amax_g: Optional[torch.Tensor] = None,
               amax_w: Optional[torch.Tensor] = None, hint_out: bool = False) -> torch.Tensor:
    """``g (M, N) @ w (N, K)`` in f32 on K20 (the data gradient of a Linear); amax_* = one-word tensors."""
    lib = _lib.load()
    if not _gemm32s_ok(g, w) or g.shape[1] != w.shape[0]:
        raise MaskBevHipError('gemm32s_nn: unsupported operands')
    if amax_g is None or amax_w is None:
        both = operand_amax([g, w], (True, False))
        amax_g = both[0] if amax_g is None else amax_g
        amax_w = both[1] if amax_w is None else amax_w
    m, n = g.shape
    k = w.shape[1]
    out = torch.empty((m, k), dtype=torch.float32, device=g.device)
    rec = amax_record(g.device) if hint_out else None
    AMAX_VERIFY.check(g, amax_g, 'gemm32s_nn g')
    AMAX_VERIFY.check(w, amax_w, 'gemm32s_nn w')
    check(lib.mbv_gemm32s_nn(_ptr(g), _ptr(w), _ptr(out), m, n, k, g.stride(0), w.stride(0), k, _amax_ptr(amax_g, 0),
                             _amax_ptr(amax_w, 0), _ptr(rec), 1, 0, 0, 0, _stream()), 'mbv_gemm32s_nn')
    amax_hint_set(out, rec)
    return out


def gemm32s_tn_acc(acc: torch.Tensor, g: torch.Tensor, x: torch.Tensor, amax_g: Optional[torch.Tensor] = None,
                   amax_x: Optional[torch.Tensor] = None) -> None:
    """``acc (N, K) f32 += g (M, N)^T @ x (M, K)`` on K20 (the weight gradient; token sum in parts, owner adds)."""
    lib = _lib.load()
    if (not _gemm32s_ok(g, x) or g.shape[0] != x.shape[0] or acc.dtype != torch.float32 or not acc.is_contiguous()
            or tuple(acc.shape) != (g.shape[1], x.shape[1]) or acc.data_ptr() % 16):
        raise MaskBevHipError('gemm32s_tn_acc: unsupported operands')
    if amax_g is None or amax_x is None:
        both = operand_amax([g, x])
        amax_g = both[0] if amax_g is None else amax_g
        amax_x = both[1] if amax_x is None else amax_x
    m, n = g.shape
    k = x.shape[1]
    nbytes = lib.mbv_gemm32s_tn_workspace_bytes(m, n, k)
    ws = _workspace(nbytes, g.device) if nbytes else None
    AMAX_VERIFY.check(g, amax_g, 'gemm32s_tn_acc g')
    AMAX_VERIFY.check(x, amax_x, 'gemm32s_tn_acc x')
    check(lib.mbv_gemm32s_tn_acc(_ptr(g), _ptr(x), _ptr(acc), m, n, k, g.stride(0), x.stride(0), _amax_ptr(amax_g, 0),
                                 _amax_ptr(amax_x, 0), _ptr(ws), int(nbytes), _stream()), 'mbv_gemm32s_tn_acc')


def gemm32s_tn_group(items) -> None:
    """``acc (N, K) f32 += g (M, N)^T @ x (M, K)`` for every ``(g, x, acc[, amax_g, amax_x])`` of ``items`` (f32, pairwise
    disjoint ``acc``) in one K20 launch (+ one parts-add launch) per 48; the operands that come without an absmax record get
    theirs from one absmax launch per 64 of them."""
    if not items:
        return
    lib = _lib.load()
    n = len(items)
    items = [tuple(it) + (None, None) if len(it) == 3 else tuple(it) for it in items]
    for g, x, acc, _, _ in items:
        if (not _gemm32s_ok(g, x) or g.shape[0] != x.shape[0] or acc.dtype != torch.float32
                or not acc.is_contiguous() or tuple(acc.shape) != (g.shape[1], x.shape[1]) or acc.data_ptr() % 16):
            raise MaskBevHipError('gemm32s_tn_group: unsupported operands')
    need = [(i, j) for i, it in enumerate(items) for j in (0, 1) if it[3 + j] is None]
    recs = {}
    if switches.get('amax_hints'):                       # an earlier product of the pass read the same tensor
        for key in list(need):
            r = amax_hint_get(items[key[0]][key[1]])
            if r is not None:
                recs[key] = r
                need.remove(key)
    for c in range(0, len(need), 64):
        chunk = need[c:c + 64]
        r = f32_absmax([items[i][j] for i, j in chunk])
        for q, key in enumerate(chunk):
            recs[key] = r[q:q + 1]
    amax = [[it[3 + j] if it[3 + j] is not None else recs[(i, j)] for j in (0, 1)] for i, it in enumerate(items)]
    if switches.get('amax_verify'):
        for i, it in enumerate(items):
            AMAX_VERIFY.check(it[0], amax[i][0], 'gemm32s_tn_group g')
            AMAX_VERIFY.check(it[1], amax[i][1], 'gemm32s_tn_group x')
    PA, LA = ctypes.c_void_p * n, ctypes.c_int64 * n
    m, nn, k = LA(*[it[0].shape[0] for it in items]), LA(*[it[0].shape[1] for it in items]), LA(*[it[1].shape[1] for it in items])
    nbytes = lib.mbv_gemm32s_tn_group_workspace_bytes(m, nn, k, n)
    ws = _workspace(nbytes, items[0][0].device) if nbytes else None
    check(lib.mbv_gemm32s_tn_group(PA(*[it[0].data_ptr() for it in items]), PA(*[it[1].data_ptr() for it in items]),
                                   PA(*[it[2].data_ptr() for it in items]), m, nn, k,
                                   LA(*[it[0].stride(0) for it in items]), LA(*[it[1].stride(0) for it in items]),
                                   PA(*[_amax_ptr(a[0], 0).value for a in amax]), PA(*[_amax_ptr(a[1], 0).value for a in amax]),
                                   n, _ptr(ws), int(nbytes), _stream()), 'mbv_gemm32s_tn_group')


def mm32_nt(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x (M, K) @ w (N, K)^T (+ bias)`` for f32 operands: K20 when the product is large enough and its operands fit
    (``switches.gemm32s``), else the library's f32 GEMM — the fp32 compute mode's stand-in for ``torch.mm`` / ``addmm``."""
    if (x.dtype == torch.float32 and w.dtype == torch.float32 and x.is_cuda and x.dim() == 2 and gemm32s_wants(x.shape[0])
            and _gemm32s_ok(x, w) and w.shape[0] % 8 == 0
            and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.data_ptr() % 16 == 0))):
        return gemm32s_nt(x, w, bias)
    return torch.mm(x, w.t()) if bias is None else torch.addmm(bias, x, w.t())


def mm32_nn(g: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``g (M, N) @ w (N, K)`` for f32 operands: K20 or the library (see :func:`mm32_nt`)."""
    if (g.dtype == torch.float32 and w.dtype == torch.float32 and g.is_cuda and g.dim() == 2 and gemm32s_wants(g.shape[0])
            and _gemm32s_ok(g, w)):
        return gemm32s_nn(g, w)
    return torch.mm(g, w)


# Under autocast, f32 activations with at most this many rows (the decoder's B*Q query tokens) are multiplied in
# f32: the GEMM is microseconds either way, and the five cast kernels per layer and direction are not.
_SMALL_F32_ROWS = 2048
_SMALL_F32_MACS = 1 << 30          # … and only while the f32 GEMM itself stays in the microseconds


# every name of this module — the underscore helpers included — is part of the package-internal surface `ops` re-exports
__all__ = [_n for _n in list(globals()) if not _n.startswith('__')]
