"""K40 restated: one LAMB step and one (Nesterov) SGD step of ONE tensor, plain torch at the dtype of the tensors handed in —
the yardstick of tests/test_optim_cpu.py and tests/test_k40_optim_gpu.py.  Written from the rule as the K40 block of
include/maskbev_hip.h words it (torch_optimizer 0.3.0 Lamb.step; torch/optim/sgd.py's single-tensor order), not from
csrc/optim_flat.hip or mask_bev_amd/optimizers.py.  Python scalars stay Python floats (float64) until they meet a tensor."""
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
