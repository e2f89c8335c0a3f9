"""Per-tensor optimizers the reference takes from packages outside torch.

``Lamb`` restates ``torch_optimizer.Lamb`` (0.3.0), which ``optimiser_type: lamb`` names (mask_bev/mask_bev_module.py:148-151):
plain torch, any device.  It is what ``MaskBevModule.configure_optimizers`` returns for a module without a parameter arena;
with an arena the same rule runs as three flat launches (``arena.FlatLamb``, K40).

``clip_gradients`` is the launcher's one call for gradient clipping by global norm whatever the optimizer; ``ClipStats`` keeps
an epoch's sums of what a clipping flat optimizer reports, on the device."""
from __future__ import annotations

import math

from typing import Optional

import torch


class Lamb(torch.optim.Optimizer):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning"), per parameter tensor::

        m = b1 m + (1 - b1) g          v = b2 v + (1 - b2) g g
        u = m / (sqrt(v) + eps) + weight_decay p            (the term only if weight_decay != 0)
        wn = min(||p||, clamp_value)   un = ||u||           trust = 1 if wn == 0 or un == 0 else wn / un
        p -= lr * bias_correction * trust * u               (bias_correction = sqrt(1 - b2^t) / (1 - b1^t) with debias, else 1)

    State keys ``step``, ``exp_avg``, ``exp_avg_sq``."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.0,
                 clamp_value: float = 10.0, debias: bool = False):
        if lr <= 0.0 or eps < 0.0 or weight_decay < 0.0 or clamp_value < 0.0:
            raise ValueError('Lamb: lr must be positive; eps, weight_decay and clamp_value non-negative')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f'Lamb: betas {betas} outside [0, 1)')
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.clamp_value = float(clamp_value)
        self.debias = bool(debias)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group['betas']
            for p in group['params']:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError('Lamb does not support sparse gradients')
                state = self.state[p]
                if not state:
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p)
                    state['exp_avg_sq'] = torch.zeros_like(p)
                m, v = state['exp_avg'], state['exp_avg_sq']
                state['step'] += 1
                m.mul_(b1).add_(g, alpha=1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                step_size = group['lr']
                if self.debias:
                    step_size *= math.sqrt(1 - b2 ** state['step']) / (1 - b1 ** state['step'])
                u = m / v.sqrt().add_(group['eps'])
                if group['weight_decay'] != 0:
                    u.add_(p, alpha=group['weight_decay'])
                wn = torch.linalg.vector_norm(p).clamp(0, self.clamp_value)
                un = torch.linalg.vector_norm(u)
                # (0-dim tensors: no host round trip per parameter)
                trust = torch.where((wn == 0) | (un == 0), torch.ones_like(wn), wn / un)
                p.sub_(u * (step_size * trust))
        return loss


def clip_gradients(optimizer, parameters, max_norm: Optional[float]) -> Optional[torch.Tensor]:
    """Clip the global 2-norm of the gradients of ``parameters`` at ``max_norm`` before ``optimizer.step()``.  ``None`` for
    ``max_norm is None`` (nothing to do) and for a flat optimizer (``arena.FlatOptimizer``), which clips inside its own
    ``step()`` when built with ``max_grad_norm`` (K41) — the loss scale and ``grad_scale`` it folds in are unknown here.
    Otherwise ``torch.nn.utils.clip_grad_norm_`` scales the gradients in place and its total norm is returned."""
    from .arena import FlatOptimizer
    if max_norm is None or isinstance(optimizer, FlatOptimizer):
        return None
    return torch.nn.utils.clip_grad_norm_(parameters, float(max_norm))


class ClipStats:
    """An epoch's sums of a clipping flat optimizer's ``grad_norm`` / ``clip_coef`` (0-d device tensors that the next step
    overwrites), kept on the device and read once.  A step whose norm is not finite — an overflowed fp16 step, which the
    optimizer skipped — enters neither the mean nor the clipped count: it is counted as skipped."""

    def __init__(self):
        self.sums = None                 # [sum of the finite norms, steps with a finite norm, of those: coefficient < 1]

    def add(self, grad_norm: torch.Tensor, clip_coef: torch.Tensor) -> None:
        finite = torch.isfinite(grad_norm)
        row = torch.stack([torch.where(finite, grad_norm, torch.zeros_like(grad_norm)).double(), finite.double(),
                           (finite & (clip_coef < 1)).double()])
        self.sums = row if self.sums is None else self.sums + row

    def summary(self, n_steps: int):
        """(mean of the finite norms, clipped steps, applied steps, skipped steps); the one host read."""
        total, applied, clipped = (0.0, 0.0, 0.0) if self.sums is None else self.sums.tolist()
        return total / max(1.0, applied), int(clipped), int(applied), n_steps - int(applied)

    def line(self, n_steps: int) -> str:
        mean, clipped, applied, skipped = self.summary(n_steps)
        return f'grad_norm {mean:.4g} clipped {clipped}/{applied}' + (f' skipped {skipped}' if skipped else '')
