"""The autograd nodes of the GEMM-shaped work and their entry points: the 4 x 4 patch projection and the 3 x 3 convolution on
K20 / K17, the Linear (library GEMM, K17 or K20) and the fused FFN pairs.  The launches are ops_gemm_kernels', the direct /
deferred / grouped parameter gradients ops_pgrad's; every name of both is a name of this module too."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, switches
from ._lib import MaskBevHipError, check
from .ops_gemm_kernels import *          # noqa: F401,F403  (ops_core's and ops_records' names come along)
from .ops_pgrad import *          # noqa: F401,F403


class _PatchEmbed32(torch.autograd.Function):
    """The backbone's 4 x 4 patch projection on the f32 NCHW pseudo-image as K20 products that gather / scatter the image
    directly (csrc/gemm_f32s.hip, GATHER modes): (B, C, H, W) -> tokens (B, H/4, W/4, E)."""

    @staticmethod
    def forward(ctx, image, weight, bias):
        lib = _lib.load()
        b, c, h, w = image.shape
        e = weight.shape[0]
        image = image.contiguous()
        w2 = weight.reshape(e, -1)
        amax = tuple(operand_amax([image.view(b * c * h, w), w2], (True, False)))      # (K3 leaves the image's record)
        out = torch.empty((b, h // 4, w // 4, e), dtype=torch.float32, device=image.device)
        AMAX_VERIFY.check(image, amax[0], 'patch_embed32 image')
        AMAX_VERIFY.check(w2, amax[1], 'patch_embed32 weight')
        check(lib.mbv_patch_embed32_fwd(_ptr(image), _ptr(w2), _ptr(bias), _ptr(out), b, c, h, w, e, _amax_ptr(amax, 0),
                                        _amax_ptr(amax, 1), _stream()), 'mbv_patch_embed32_fwd')
        ctx.save_for_backward(image, weight)
        ctx.amax, ctx.bias = amax, bias
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        image, weight = ctx.saved_tensors
        bias = ctx.bias
        b, c, h, w = image.shape
        e = weight.shape[0]
        g = g.contiguous()
        g2 = g.view(-1, e)
        amax_g = f32_absmax([g2])
        w2 = weight.reshape(e, -1)
        gi = gw = gb = None
        AMAX_VERIFY.check(g2, amax_g, 'patch_embed32_bwd g')
        AMAX_VERIFY.check(image, ctx.amax[0], 'patch_embed32_bwd image')
        AMAX_VERIFY.check(w2, ctx.amax[1], 'patch_embed32_bwd weight')
        if ctx.needs_input_grad[0]:
            gi = torch.empty_like(image)
            check(lib.mbv_patch_embed32_bwd_image(_ptr(g2), _ptr(w2), _ptr(gi), b, c, h, w, e, _amax_ptr(amax_g, 0),
                                                  _amax_ptr(ctx.amax, 1), _stream()), 'mbv_patch_embed32_bwd_image')
        if ctx.needs_input_grad[1]:
            direct = arena_grad(weight) is not None and weight.grad.is_contiguous()
            acc = weight.grad if direct else torch.zeros_like(weight)
            nbytes = lib.mbv_patch_embed32_bwd_weight_workspace_bytes(b, c, h, w, e)
            ws = _workspace(nbytes, g.device) if nbytes else None
            check(lib.mbv_patch_embed32_bwd_weight(_ptr(g2), _ptr(image), _ptr(acc), b, c, h, w, e, _amax_ptr(amax_g, 0),
                                                   _amax_ptr(ctx.amax, 0), _ptr(ws), int(nbytes), _stream()),
                  'mbv_patch_embed32_bwd_weight')
            if direct:
                _fire_grad_hooks(weight)
            else:
                gw = acc
        if bias is not None and ctx.needs_input_grad[2]:
            if arena_grad(bias) is not None:
                colsum_accum(g2, bias.grad, persistent=True)
                _fire_grad_hooks(bias)
            else:
                gb = g2.sum(0)
        return gi, gw, gb


def patch_embed32_ok(image: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> bool:
    """fp32 compute, a 4 x 4 stride-4 projection, shapes K20's gather modes take (include/maskbev_hip.h)."""
    if not (switches.get('gemm32s') and image.is_cuda and image.dtype == torch.float32 and weight.dtype == torch.float32
            and image.dim() == 4 and weight.dim() == 4 and tuple(weight.shape[2:]) == (4, 4)
            and weight.shape[1] == image.shape[1] and not torch.is_autocast_enabled('cuda')):
        return False
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.data_ptr() % 16):
        return False
    b, c, h, w = image.shape
    return bool(weight.is_contiguous() and weight.data_ptr() % 16 == 0
                and _lib.load().mbv_patch_embed32_supported(b, c, h, w, weight.shape[0]))


def patch_embed32(image: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    return _PatchEmbed32.apply(image, weight, bias)


class _Conv3x3K20(torch.autograd.Function):
    """``conv2d(x, weight, padding=1)`` for a 3 x 3 kernel on an f32 (B, C, H, W) map as K20 products on a zero-bordered
    channels-last ROWS copy of the map (csrc/conv_pad.hip, mbv_conv3x3_gemm32s): forward and data gradient are one product
    over k = (tap, channel) each, the weight gradient nine entries of the grouped TN launch — no im2col, no MIOpen."""

    @staticmethod
    def forward(ctx, x, weight):
        lib = _lib.load()
        b, c, h, w = x.shape
        cout = weight.shape[0]
        x = x.contiguous()
        rows = int(lib.mbv_conv_rows(b, h, w))
        xp = torch.zeros((rows, c), dtype=torch.float32, device=x.device)
        check(lib.mbv_conv_pad_rows(_ptr(x), _ptr(xp), b, c, h, w, 4, _stream()), 'mbv_conv_pad_rows')
        wm = weight.detach().permute(0, 2, 3, 1).reshape(cout, 9 * c).contiguous()
        rec = f32_absmax([xp, wm])
        outp = torch.empty((rows, cout), dtype=torch.float32, device=x.device)
        AMAX_VERIFY.check(xp, rec[0:1], 'conv3x3_gemm32s x')
        AMAX_VERIFY.check(wm, rec[1:2], 'conv3x3_gemm32s w')
        check(lib.mbv_conv3x3_gemm32s(_ptr(xp), _ptr(wm), _ptr(outp), b, h, w, c, cout, _amax_ptr(rec, 0), _amax_ptr(rec, 1),
                                      None, _stream()), 'mbv_conv3x3_gemm32s')
        y = torch.empty((b, cout, h, w), dtype=torch.float32, device=x.device)
        check(lib.mbv_conv_unpad_rows(_ptr(outp), _ptr(y), b, cout, h, w, 4, _stream()), 'mbv_conv_unpad_rows')
        ctx.save_for_backward(xp, weight)
        ctx.rec_x, ctx.dims = rec[0:1], (b, c, h, w, cout)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        xp, weight = ctx.saved_tensors
        b, c, h, w, cout = ctx.dims
        rows = xp.shape[0]
        guard, mp = w + 3, b * (h + 2) * (w + 2)
        gy = gy.contiguous()
        gyp = torch.zeros((rows, cout), dtype=torch.float32, device=gy.device)
        check(lib.mbv_conv_pad_rows(_ptr(gy), _ptr(gyp), b, cout, h, w, 4, _stream()), 'mbv_conv_pad_rows')
        gx = gw = None
        wd = weight.detach()
        if ctx.needs_input_grad[0]:
            wflip = wd.flip(2, 3).permute(1, 2, 3, 0).reshape(c, 9 * cout).contiguous()
            rec = f32_absmax([gyp, wflip])
            rec_g = rec[0:1]
            gxp = torch.empty((rows, c), dtype=torch.float32, device=gy.device)
            check(lib.mbv_conv3x3_gemm32s(_ptr(gyp), _ptr(wflip), _ptr(gxp), b, h, w, cout, c, _amax_ptr(rec, 0),
                                          _amax_ptr(rec, 1), None, _stream()), 'mbv_conv3x3_gemm32s')
            gx = torch.empty((b, c, h, w), dtype=torch.float32, device=gy.device)
            check(lib.mbv_conv_unpad_rows(_ptr(gxp), _ptr(gx), b, c, h, w, 4, _stream()), 'mbv_conv_unpad_rows')
        else:
            rec_g = f32_absmax([gyp])
        if ctx.needs_input_grad[1]:
            # d weight[co][ci][dy][dx] = sum_m gyp[m][co] xp[m + shift_t][ci]: nine token-major products of the grouped launch
            dwm = torch.zeros((9, cout, c), dtype=torch.float32, device=gy.device)
            g2 = gyp[guard:guard + mp]
            items = []
            for t in range(9):
                sh = guard + (t // 3 - 1) * (w + 2) + (t % 3 - 1)
                items.append((g2, xp[sh:sh + mp], dwm[t], rec_g, ctx.rec_x))
            gemm32s_tn_group(items)
            gw = dwm.permute(1, 2, 0).reshape(cout, c, 3, 3)
            if arena_grad(weight) is not None:
                weight.grad.add_(gw)
                _fire_grad_hooks(weight)
                gw = None
        return gx, gw


class _Conv3x3K17(torch.autograd.Function):
    """The same convolution for the 16-bit compute modes: 16-bit rows, K17 products (mbv_conv3x3_gemm16; the weight gradient
    nine entries of mbv_gemm16_tn_group, f32).  ``x`` f32 or 16-bit (cast to ``dt``), the result and d x in ``dt``."""

    @staticmethod
    def forward(ctx, x, weight, dt):
        lib = _lib.load()
        b, c, h, w = x.shape
        cout = weight.shape[0]
        ctx.x_dtype = x.dtype
        x = x.to(dt).contiguous()
        rows = int(lib.mbv_conv_rows(b, h, w))
        xp = torch.zeros((rows, c), dtype=dt, device=x.device)
        check(lib.mbv_conv_pad_rows(_ptr(x), _ptr(xp), b, c, h, w, 2, _stream()), 'mbv_conv_pad_rows')
        wm = _compute_copy(weight, dt).detach().permute(0, 2, 3, 1).reshape(cout, 9 * c).contiguous()
        outp = torch.empty((rows, cout), dtype=dt, device=x.device)
        check(lib.mbv_conv3x3_gemm16(_ptr(xp), _ptr(wm), _ptr(outp), b, h, w, c, cout, _GEMM16_DT[dt], 0, _stream()),
              'mbv_conv3x3_gemm16')
        y = torch.empty((b, cout, h, w), dtype=dt, device=x.device)
        check(lib.mbv_conv_unpad_rows(_ptr(outp), _ptr(y), b, cout, h, w, 2, _stream()), 'mbv_conv_unpad_rows')
        ctx.save_for_backward(xp, weight)
        ctx.dims, ctx.dt = (b, c, h, w, cout), dt
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        xp, weight = ctx.saved_tensors
        b, c, h, w, cout = ctx.dims
        dt = ctx.dt
        rows = xp.shape[0]
        guard, mp = w + 3, b * (h + 2) * (w + 2)
        gy = gy.to(dt).contiguous()
        gyp = torch.zeros((rows, cout), dtype=dt, device=gy.device)
        check(lib.mbv_conv_pad_rows(_ptr(gy), _ptr(gyp), b, cout, h, w, 2, _stream()), 'mbv_conv_pad_rows')
        gx = gw = None
        if ctx.needs_input_grad[0]:
            wflip = _compute_copy(weight, dt).detach().flip(2, 3).permute(1, 2, 3, 0).reshape(c, 9 * cout).contiguous()
            gxp = torch.empty((rows, c), dtype=dt, device=gy.device)
            check(lib.mbv_conv3x3_gemm16(_ptr(gyp), _ptr(wflip), _ptr(gxp), b, h, w, cout, c, _GEMM16_DT[dt], 0, _stream()),
                  'mbv_conv3x3_gemm16')
            gx = torch.empty((b, c, h, w), dtype=dt, device=gy.device)
            check(lib.mbv_conv_unpad_rows(_ptr(gxp), _ptr(gx), b, c, h, w, 2, _stream()), 'mbv_conv_unpad_rows')
            gx = gx.to(ctx.x_dtype)
        if ctx.needs_input_grad[1]:
            dwm = torch.zeros((9, cout, c), dtype=torch.float32, device=gy.device)
            g2 = gyp[guard:guard + mp]
            items = []
            for t in range(9):
                sh = guard + (t // 3 - 1) * (w + 2) + (t % 3 - 1)
                items.append((g2, xp[sh:sh + mp], dwm[t]))
            gemm16_tn_group(items)
            gw = dwm.permute(1, 2, 0).reshape(cout, c, 3, 3)
            if arena_grad(weight) is not None:
                weight.grad.add_(gw)
                _fire_grad_hooks(weight)
                gw = None
            else:
                gw = gw.to(weight.dtype)
        return gx, gw, None


def conv3x3_16_ok(x: torch.Tensor, conv) -> bool:
    """A 16-bit compute mode (autocast to bf16 / fp16, or 16-bit tensors), a 3 x 3 stride-1 padding-1 convolution without bias
    whose channel counts K17 takes."""
    if not (gemm16_enabled() and x.is_cuda and x.dim() == 4):
        return False
    dt = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled('cuda') else x.dtype
    return bool(dt in _GEMM16_DT and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
                and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.padding_mode == 'zeros'
                and x.shape[1] % 32 == 0 and conv.weight.shape[0] % 32 == 0 and x.shape[0] * x.shape[2] * x.shape[3] >= 1024)


def conv3x3_16(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    dt = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled('cuda') else x.dtype
    with torch.autocast('cuda', enabled=False):
        return _Conv3x3K17.apply(x, weight, dt)


def conv3x3_32_ok(x: torch.Tensor, conv) -> bool:
    """fp32 compute, a 3 x 3 stride-1 padding-1 convolution without bias whose channel counts K20 takes."""
    return bool(switches.get('conv3x3_k20') and switches.get('gemm32s') and x.is_cuda and x.dtype == torch.float32
                and x.dim() == 4 and conv.weight.dtype == torch.float32 and not torch.is_autocast_enabled('cuda')
                and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
                and conv.groups == 1 and conv.bias is None and conv.padding_mode == 'zeros'
                and x.shape[1] % 32 == 0 and conv.weight.shape[0] % 32 == 0
                and gemm32s_wants(x.shape[0] * x.shape[2] * x.shape[3]))


def conv3x3_32(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    return _Conv3x3K20.apply(x, weight)


def _wgrad(g2: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    """dW (out, in) = g2^T x2 for token-major g2 (T, out), x2 (T, in); f32 result, split-K for large T."""
    t = g2.shape[0]
    s = _wgrad_splits(t)
    if s == 1:
        return g2.t().mm(x2).float()
    c = t // s                          # rows per chunk; the ragged tail (< s rows) is one more small GEMM
    gw = torch.bmm(g2[:s * c].view(s, c, -1).transpose(1, 2), x2[:s * c].view(s, c, -1)).sum(0, dtype=torch.float32)
    if s * c < t:                       # (the tail's product accumulates through the GEMM's beta = 1: no add launch)
        if g2.dtype == torch.float32:
            gw = torch.addmm(gw, g2[s * c:].t(), x2[s * c:])
        else:
            gw = gw + g2[s * c:].t().mm(x2[s * c:]).float()
    return gw


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, rows, f32_out=False, skip_bias_grad=False):
        if torch.is_autocast_enabled('cuda') and not (
                x.dtype == torch.float32 and weight.dtype == torch.float32
                and x.numel() <= _SMALL_F32_ROWS * x.shape[-1] and x.numel() * weight.shape[0] <= _SMALL_F32_MACS):
            dt = torch.get_autocast_dtype('cuda')
            ctx.gx_f32 = x.dtype == torch.float32 and dt in _LO_DTYPES and x.is_cuda    # the caller's tensor is f32
            x, w, b = x.to(dt), _compute_copy(weight, dt), _compute_copy(bias, dt)
        else:
            ctx.gx_f32 = False
            w, b = weight, bias
        if rows is not None:
            w = w[rows[0]:rows[1]]
            b = None if b is None else b[rows[0]:rows[1]]
        x2k = x.reshape(-1, x.shape[-1]) if x.is_cuda and x.dtype in _GEMM16_DT else None
        ctx.amax = None
        x32 = None
        if x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32 and x.dim() >= 2:
            x32 = x.reshape(-1, x.shape[-1])
            if not (gemm32s_wants(x32.shape[0]) and _gemm32s_ok(x32, w) and w.shape[0] % 8 == 0
                    and (b is None or (b.dtype == torch.float32 and b.is_contiguous() and b.data_ptr() % 16 == 0))):
                x32 = None
        with torch.autocast('cuda', enabled=False):
            if x32 is not None:
                # fp32 compute: K20 — f32 products from IEEE-half pairs on the 16-bit matrix pipe (csrc/gemm_f32s.hip).  The
                # operand scales: x's absmax record from its producer when it left one (K12, K20), else one pass over x;
                # the weight's once per parameter update
                hints = bool(switches.get('amax_hints'))
                hx = amax_hint_get(x32) if hints else None
                if hx is not None:
                    ctx.amax = (hx, weight_amax(w))
                else:
                    both = f32_absmax([x32, w])
                    ctx.amax = (both[0:1], both[1:2])
                y2 = gemm32s_nt(x32, w, b, amax=ctx.amax, hint_out=hints)
                y = y2.view(x.shape[:-1] + (w.shape[0],))       # (reads y2's record through its _base)
            elif (x2k is not None and gemm16_policy() == 'all' and _gemm16_ok(x2k, w)
                    and (bias is None or bias.dtype == torch.float32)):
                bf = None if bias is None else (bias if rows is None else bias[rows[0]:rows[1]])
                y = gemm16_nt(x2k, w, bf, out_dtype=torch.float32 if f32_out else None)
                y = y.view(x.shape[:-1] + (w.shape[0],))
            elif f32_out and x.dtype in _LO_DTYPES and x.is_cuda:
                # 16-bit GEMM with the f32 accumulators stored as f32 (the consumer wants f32: no cast pass)
                x2 = x.reshape(-1, x.shape[-1])
                if bias is not None:
                    bf = bias if rows is None else bias[rows[0]:rows[1]]
                    y = torch.addmm(bf.float(), x2, w.t(), out_dtype=torch.float32)
                else:
                    y = torch.mm(x2, w.t(), out_dtype=torch.float32)
                y = y.view(x.shape[:-1] + (w.shape[0],))
            else:
                y = torch.nn.functional.linear(x, w, b)
        ctx.save_for_backward(x, w)
        ctx.weight, ctx.bias, ctx.rows = weight, bias, rows
        ctx.skip_bias_grad = skip_bias_grad
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        weight, bias, rows = ctx.weight, ctx.bias, ctx.rows
        gy = gy.to(x.dtype)
        g2 = gy.reshape(-1, gy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        gx = gw = gb = None
        amax_g = None
        if ctx.amax is not None:
            if not g2.is_contiguous():
                g2 = g2.contiguous()
            if _gemm32s_ok(g2, w) and _gemm32s_ok(x2):
                amax_g = amax_hint_get(g2) if switches.get('amax_hints') else None
                if amax_g is None:
                    amax_g = f32_absmax([g2])
        if ctx.needs_input_grad[0]:
            if amax_g is not None:
                gx = gemm32s_nn(g2, w, amax_g, ctx.amax[1], hint_out=bool(switches.get('amax_hints')))
                gx = gx.view(x.shape)        # (a view reads the record gemm32s_nn left on gx through its _base)
            elif gemm16_policy() == 'all' and g2.is_cuda and _gemm16_ok(g2, w):
                gx = gemm16_nn(g2, w).view_as(x)
            elif ctx.gx_f32:         # an f32 input was cast for the GEMM: its gradient leaves the GEMM as f32 (no cast pass)
                gx = torch.mm(g2, w, out_dtype=torch.float32).view_as(x)
            else:
                gx = g2.mm(w).view_as(x)
        bias_done = ctx.skip_bias_grad        # the consumer of this layer's output accumulates db (K12 / activation op)
        bias_direct = bias is not None and ctx.needs_input_grad[2] and not bias_done and arena_grad(bias) is not None
        if ctx.needs_input_grad[1]:
            acc = arena_grad(weight, rows)
            if acc is not None:
                bacc = arena_grad(bias, rows) if bias_direct else None
                bias_done = _wgrad_into(acc, g2, x2, bacc, persistent=True,                  # straight into the arena
                                        amax=None if amax_g is None else (amax_g, ctx.amax[0])) or bias_done
                _fire_grad_hooks(weight)
                if bias_done:
                    _fire_grad_hooks(bias)
            elif amax_g is not None and weight.dtype == torch.float32 and weight.is_contiguous():
                gw = torch.zeros_like(weight)
                gemm32s_tn_acc(gw if rows is None else gw[rows[0]:rows[1]], g2, x2, amax_g, ctx.amax[0])
            elif rows is None:
                gw = _wgrad(g2, x2).to(weight.dtype)
            else:
                gw = torch.zeros_like(weight)
                gw[rows[0]:rows[1]] = _wgrad(g2, x2)
        if bias is not None and ctx.needs_input_grad[2] and not bias_done:
            if bias_direct:
                colsum_accum(g2, arena_grad(bias, rows), persistent=True)
                _fire_grad_hooks(bias)
            elif rows is None:
                gb = g2.sum(0, dtype=torch.float32).to(bias.dtype)
            else:
                gb = torch.zeros_like(bias)
                gb[rows[0]:rows[1]] = g2.sum(0, dtype=torch.float32)
        return gx, gw, gb, None, None, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
           rows: Optional[tuple] = None, f32_out: bool = False, skip_bias_grad: bool = False) -> torch.Tensor:
    """y = x W^T + b on the library GEMM (hipBLASLt) honouring autocast, with the split-K weight gradient.
    ``rows=(r0, r1)`` uses rows r0:r1 of the parameters (the q / k / v blocks of a packed ``in_proj_weight``)
    without materialising slices or zero-padded slice gradients.  Parameters that live in a
    :class:`~mask_bev_amd.arena.ParameterArena` are read through their bf16 shadow and receive their gradient by
    direct f32 accumulation (the autograd gradient returned for them is ``None``)."""
    return _Linear.apply(x, weight, bias, rows, f32_out, skip_bias_grad)


class _FFN(torch.autograd.Function):
    """``fc2(act(fc1(x)))`` of an mmcv FFN (/root/reference: mask_bev/models/networks/swin/swin.py:347-377) with the
    element-wise work folded into K17's epilogues: forward, fc1 + bias + activation in one launch (stores the
    pre-activation for GELU); backward, the data gradient of fc2 times the activation derivative with the column sums
    of the result (= d bias of fc1) in one launch, the two weight gradients accumulated straight into the arena, and no
    separate activation / bias kernels.  Parameters must live in a parameter arena (bf16 shadow, f32 gradients)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, kind, defer_out_bias):
        dt = torch.get_autocast_dtype('cuda')
        x2 = x.reshape(-1, x.shape[-1])
        if x2.dtype != dt:
            x2 = x2.to(dt)
        w1c, w2c = _compute_copy(w1, dt), _compute_copy(w2, dt)
        if kind == 'gelu':
            a, h = gemm16_nt(x2, w1c, b1, act='gelu', want_pre=True)
        else:
            a, h = gemm16_nt(x2, w1c, b1, act='relu'), None
        if gemm16_policy() == 'all':
            out = gemm16_nt(a, w2c, b2)
        else:
            out = torch.nn.functional.linear(a, w2c, _compute_copy(b2, dt))
        ctx.save_for_backward(x2, a if h is None else h, a, w1c, w2c)
        ctx.params = (w1, b1, w2, b2)
        ctx.kind, ctx.defer_out_bias, ctx.xshape = kind, defer_out_bias, x.shape
        ctx.x_f32 = x.dtype == torch.float32
        return out.view(x.shape[:-1] + (w2.shape[0],))

    @staticmethod
    def backward(ctx, gout):
        x2, aux, a, w1c, w2c = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        g2 = gout.reshape(-1, gout.shape[-1])
        if g2.dtype != x2.dtype:
            g2 = g2.to(x2.dtype)
        g2 = g2.contiguous()
        # d hidden = (g . W2) * act'(.), column sums -> d b1
        dh = gemm16_nn(g2, w2c, act=ctx.kind, aux=aux, colsum=b1.grad,
                       colsum_sink=accumulate_colsum if switches.get('nn_colsum_defer') and _defer_ok() else None)
        _fire_grad_hooks(b1)
        accumulate_wgrad(w2, g2, a)
        if not ctx.defer_out_bias:
            colsum_accum(g2, b2.grad)
            _fire_grad_hooks(b2)
        accumulate_wgrad(w1, dh, x2)
        gx = None
        if ctx.needs_input_grad[0]:
            if gemm16_policy() == 'all':
                gx = gemm16_nn(dh, w1c)
            elif ctx.x_f32:        # an f32 input (post-LN residual stream) takes its gradient in f32: no 16-bit round trip + cast
                gx = torch.mm(dh, w1c, out_dtype=torch.float32)
            else:
                gx = dh.mm(w1c)
            gx = gx.view(ctx.xshape)
        return gx, None, None, None, None, None, None


class _FFN32(torch.autograd.Function):
    """``fc2(act(fc1(x)))`` of an mmcv FFN in fp32 compute on K20 (csrc/gemm_f32s.hip): forward, fc1 + bias + activation in one
    launch (stores the activation and the pre-activation, leaves the activation's absmax record for fc2); backward, the data
    gradient of fc2 times the activation's derivative with the partial column sums of the result (= d bias of fc1) in one
    launch — no activation kernels, no pass over the hidden gradient — then the two weight gradients and fc1's data gradient.
    /root/reference: mask_bev/models/networks/swin/swin.py:347-355."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, kind, defer_out_bias):
        x2 = x.reshape(-1, x.shape[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        hx = amax_hint_get(x2) if switches.get('amax_hints') else None
        if hx is None:
            both = f32_absmax([x2, w1])
            ax, aw1 = both[0:1], both[1:2]
        else:
            ax, aw1 = hx, weight_amax(w1)
        a, h = gemm32s_nt(x2, w1, b1, act=kind, amax=(ax, aw1), want_pre=True, hint_out=True)
        aa = amax_hint_get(a)
        aw2 = weight_amax(w2)
        out = gemm32s_nt(a, w2, b2, amax=(aa, aw2), hint_out=bool(switches.get('amax_hints')))
        ctx.save_for_backward(x2, h, a)
        ctx.params = (w1, b1, w2, b2)
        ctx.amax = (ax, aw1, aa, aw2)
        ctx.kind, ctx.defer_out_bias, ctx.xshape = kind, defer_out_bias, x.shape
        return out.view(x.shape[:-1] + (w2.shape[0],))           # (reads out's record through its _base)

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        x2, h, a = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        ax, aw1, aa, aw2 = ctx.amax
        g2 = gout.reshape(-1, gout.shape[-1])
        if g2.dtype != torch.float32:
            g2 = g2.float()
        if not g2.is_contiguous():
            g2 = g2.contiguous()
        ag = amax_hint_get(g2) if switches.get('amax_hints') else None
        if ag is None:
            ag = f32_absmax([g2])
        t, f = h.shape
        # d hidden = (g . W2) * act'(pre), its partial column sums -> d b1, its absmax record for the products below
        dh = torch.empty_like(h)
        rows = lib.mbv_gemm32s_nn_part_rows(t, 1)
        parts = torch.empty((rows, f), dtype=torch.float32, device=h.device)
        adh = amax_record(h.device)
        AMAX_VERIFY.check(g2, ag, 'gemm32s_nn_act g')
        AMAX_VERIFY.check(w2, aw2, 'gemm32s_nn_act w2')
        check(lib.mbv_gemm32s_nn_act(_ptr(g2), _ptr(w2), _ptr(dh), _ptr(h), _ptr(parts), parts.numel() * 4, t, w2.shape[0], f,
                                     g2.stride(0), w2.stride(0), f, f, _ptr(ag), _ptr(aw2), _ptr(adh), _ACT[ctx.kind],
                                     _stream()), 'mbv_gemm32s_nn_act')
        accumulate_colsum(parts, b1.grad, rows, f, f)
        _fire_grad_hooks(b1)
        accumulate_wgrad(w2, g2, a, amax=(ag, aa))
        if not ctx.defer_out_bias:
            colsum_accum(g2, b2.grad, persistent=True)
            _fire_grad_hooks(b2)
        accumulate_wgrad(w1, dh, x2, amax=(adh, ax))
        gx = None
        if ctx.needs_input_grad[0]:
            gx2 = gemm32s_nn(dh, w1, adh, aw1, hint_out=bool(switches.get('amax_hints')))
            gx = gx2.view(ctx.xshape)
        return gx, None, None, None, None, None, None


def ffn32_ok(x: torch.Tensor, fc1_w, fc1_b, fc2_w, fc2_b) -> bool:
    """The K20 FFN applies: fp32 compute (no autocast) on the device, arena-resident f32 parameters with f32 gradients, a token
    count K20 takes, shapes in 8-element chunks."""
    if not (x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled('cuda') and torch.is_grad_enabled()
            and switches.get('gemm32s') and switches.get('ffn32')):
        return False
    rows = x.numel() // max(1, x.shape[-1])
    if not gemm32s_wants(rows) or x.shape[-1] % 8:
        return False
    for p in (fc1_w, fc1_b, fc2_w, fc2_b):
        if (arena_grad(p) is None or p.dtype != torch.float32 or not p.is_contiguous() or p.data_ptr() % 16
                or not p.grad.is_contiguous()):
            return False
    return fc1_w.shape[0] % 8 == 0 and fc1_w.shape[1] % 8 == 0 and fc2_w.shape[0] % 8 == 0


def ffn32(x: torch.Tensor, fc1_w, fc1_b, fc2_w, fc2_b, kind: str, defer_out_bias: bool = False) -> torch.Tensor:
    return _FFN32.apply(x, fc1_w, fc1_b, fc2_w, fc2_b, kind, defer_out_bias)


def ffn_fused_ok(x: torch.Tensor, fc1_w, fc1_b, fc2_w, fc2_b) -> bool:
    """The fused FFN (K17 epilogues) applies: 16-bit autocast on a ROCm device, arena-resident parameters with f32
    gradients, token count in K17's range, 16-byte-chunk shapes."""
    if not (x.is_cuda and torch.is_autocast_enabled('cuda') and torch.is_grad_enabled()):
        return False
    dt = torch.get_autocast_dtype('cuda')
    rows = x.numel() // max(1, x.shape[-1])
    if dt not in _GEMM16_DT or not _k17_wants('fused', rows):
        return False
    for p in (fc1_w, fc1_b, fc2_w, fc2_b):
        if arena_grad(p) is None:
            return False
        sh = getattr(p, '_mbv_shadow', None)
        if p.dim() == 2 and (sh is None or sh.dtype != dt):
            return False
    return fc1_w.shape[0] % 8 == 0 and fc1_w.shape[1] % 8 == 0 and fc2_w.shape[0] % 8 == 0


def ffn(x: torch.Tensor, fc1_w, fc1_b, fc2_w, fc2_b, kind: str, defer_out_bias: bool = False) -> torch.Tensor:
    """``fc2(act(fc1(x)))`` through :class:`_FFN` (check :func:`ffn_fused_ok` first).  ``defer_out_bias``: the
    consumer of the result (K12 with ``branch_bias``) accumulates d b2."""
    return _FFN.apply(x, fc1_w, fc1_b, fc2_w, fc2_b, kind, defer_out_bias)


# every name of this module — the underscore helpers included — is part of the package-internal surface `ops` re-exports
__all__ = [_n for _n in list(globals()) if not _n.startswith('__')]
