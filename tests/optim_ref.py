"""K40 restated: one LAMB step and one (Nesterov) SGD step of ONE tensor, plain torch at the dtype of the tensors handed in —
the yardstick of tests/test_optim_cpu.py and tests/test_k40_optim_gpu.py.  Written from the rule as the K40 block of
include/maskbev_hip.h words it (torch_optimizer 0.3.0 Lamb.step; torch/optim/sgd.py's single-tensor order), not from
csrc/optim_flat.hip or mask_bev_amd/optimizers.py.  Python scalars stay Python floats (float64) until they meet a tensor.
The two ``*_unfused`` functions restate one AdamW / SGD step in f32 with one rounding per operation, for exact comparisons."""
import math

import torch


def lamb_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, clamp_value=10.0, debias=False):
    """One LAMB step of a tensor, ``t`` the 1-based step count.  Returns (p, m, v, trust, u) — new tensors, inputs untouched;
    ``trust`` is a Python float."""
    b1, b2 = betas
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = m / (v.sqrt() + eps)
    if weight_decay != 0:
        u = u + weight_decay * p
    wn = min(float(p.square().sum().sqrt()), clamp_value)
    un = float(u.square().sum().sqrt())
    trust = 1.0 if wn == 0 or un == 0 else wn / un
    bias_correction = math.sqrt(1 - b2 ** t) / (1 - b1 ** t) if debias else 1.0
    p = p - (lr * bias_correction * trust) * u
    return p, m, v, trust, u


def sgd_step(p, g, buf, lr, momentum=0.99, dampening=0.0, weight_decay=0.0, nesterov=True):
    """One SGD step of a tensor; ``buf`` None = torch's first step (the buffer becomes the gradient).  Returns (p, buf)."""
    # `x.add(y, alpha=a)` is the operation torch.optim.SGD itself issues for x + a * y: ATen's CPU kernel may fuse the multiply
    # and the add, so spelling the update any other way differs from torch in the last bit
    if weight_decay != 0:
        g = g.add(p, alpha=weight_decay)
    if momentum != 0:
        buf = g.clone() if buf is None else buf.mul(momentum).add(g, alpha=1 - dampening)
        g = g.add(buf, alpha=momentum) if nesterov else buf
    return p.add(g, alpha=-lr), buf


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def adamw_step_unfused(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, decoupled=True):
    """One Adam / AdamW step of an f32 tensor with ONE ROUNDING PER OPERATION in the order mbv_adamw_step's block of
    include/maskbev_hip.h words it: every multiply and add is its own torch call on f32 tensors (no ``alpha=``, no
    ``addcmul``, which a backend may fuse), the hyper-parameters are rounded to f32 first, and the bias corrections are taken
    in float64 from the f32 betas and rounded once.  IEEE multiply / add / divide / sqrt are correctly rounded on the CPU and
    on the device, so a kernel that keeps this order is equal to it bit for bit.  Returns (p, m, v)."""
    lr, b1, b2, eps, wd, gs, one = (_f32(x) for x in (lr, betas[0], betas[1], eps, weight_decay, grad_scale, 1.0))
    bc1 = _f32(1.0 - float(b1) ** t)
    bc2_sqrt = _f32(math.sqrt(1.0 - float(b2) ** t))
    g = g * gs
    if decoupled:
        p = p * (one - lr * wd)
    elif weight_decay != 0:
        g = g + wd * p
    m = m + (g - m) * (one - b1)
    v = v * b2 + ((one - b2) * g) * g
    denom = v.sqrt() / bc2_sqrt + eps
    return p - (lr / bc1) * (m / denom), m, v


def sgd_step_unfused(p, g, buf, lr, momentum=0.99, dampening=0.0, weight_decay=0.0, nesterov=True, grad_scale=1.0):
    """``sgd_step`` for f32 tensors with one rounding per operation (see ``adamw_step_unfused``) and a buffer that starts at
    zero, as mbv_sgd_step's does.  Returns (p, buf)."""
    lr, mom, wd, gs = (_f32(x) for x in (lr, momentum, weight_decay, grad_scale))
    g = g * gs
    if weight_decay != 0:
        g = g + wd * p
    buf = buf * mom + (_f32(1.0) - _f32(dampening)) * g
    g = g + mom * buf if nesterov else buf
    return p - lr * g, buf
