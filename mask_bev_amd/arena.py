"""Parameter arena: every parameter, gradient and optimizer moment of a ``MaskBevModule`` laid out in four flat
HBM buffers (288 GB of HBM3E makes the extra bf16 shadow free), so that the per-step bookkeeping of ≈ 700 tensors
collapses into a handful of launches (K11 and K40, csrc/optim_flat.hip):

* ``param``   f32 — ``p.data`` of every parameter is a view into it (checkpoint keys and shapes unchanged);
* ``grad``    f32 — ``p.grad`` is a view; the Linear layers accumulate their weight / bias gradients straight into
                    it (``ops.linear``), autograd adds the rest in place; one fill clears it, and the gradient
                    all-reduce runs over contiguous chunks of it with no bucket copies;
* ``shadow``  bf16 — the copy of the weights the bf16 GEMMs read, written by the optimizer kernel itself instead
                    of ≈ 450 per-layer cast kernels per step;
* ``exp_avg``, ``exp_avg_sq`` f32 — Adam moments (owned by :class:`FlatAdam`; :class:`FlatLamb` owns the same pair,
                    :class:`FlatSGD` one momentum buffer).

The arena is laid out in the reference's differential-lr groups — encoder, backbone, head
(mask_bev/mask_bev_module.py:131-139) — each a contiguous segment, so an optimizer step is one
``mbv_adamw_step`` launch per group (one launch in total when the groups share a learning rate).

The three optimizers are :class:`FlatOptimizer` subclasses: the base owns the ``step()`` frame, ``zero_grad`` and the
checkpoint format; a subclass names its state (``KIND`` / ``STATE`` / ``HYPER``) and issues its launches in ``_launch``.

:class:`WeightAverage` (K43) keeps one more flat f32 buffer beside them: an exponential moving average or running mean of
``param``, updated in one streaming pass behind the optimizer step and exchanged with ``param`` for evaluation.

Build it after the module is on its GPU (``module.to(device)`` re-allocates parameters and would detach the views).
"""
from __future__ import annotations

import contextlib
import ctypes
import weakref
from typing import Dict, Iterable, List, Optional, Tuple

import torch
from torch import nn

from . import _lib, ops
from ._lib import check

_ALIGN = 64          # elements: every parameter starts on a 256-byte boundary
_SHORT_RUN = 1 << 23  # elements: an optimizer run shorter than this shares a launch with its like (FlatAdam._launch)
CLIP_RANGES = 8       # element ranges one mbv_grad_norm_partials call sums (kNormRanges of csrc/optim_flat.hip)


def _round_up(n: int, a: int) -> int:
    return (n + a - 1) // a * a


class ParameterArena:
    def __init__(self, segments: Iterable[Tuple[str, nn.Module]], shadow_dtype: Optional[torch.dtype] = torch.bfloat16):
        segments = list(segments)
        seen = set()
        self.layout: List[Tuple[nn.Parameter, int]] = []          # (parameter, offset)
        self.segments: Dict[str, Tuple[int, int]] = {}
        off = 0
        device = None
        for name, mod in segments:
            start = off
            for p in mod.parameters():
                if id(p) in seen:
                    continue
                seen.add(id(p))
                if p.dtype != torch.float32:
                    raise TypeError('the arena holds f32 master parameters')
                device = device or p.device
                if p.device != device:
                    raise ValueError('all parameters must live on one device')
                self.layout.append((p, off))
                off += _round_up(p.numel(), _ALIGN)
            self.segments[name] = (start, off)
        if device is None:
            raise ValueError('no parameters')
        self.numel = off
        self.device = device
        self.param = torch.zeros(off, dtype=torch.float32, device=device)
        self.grad = torch.zeros(off, dtype=torch.float32, device=device)
        self.shadow = None
        if shadow_dtype is not None:
            if shadow_dtype not in (torch.bfloat16, torch.float16):
                raise TypeError('the shadow copy is bf16 or fp16')
            self.shadow = torch.zeros(off, dtype=shadow_dtype, device=device)
        with torch.no_grad():
            for p, o in self.layout:
                n = p.numel()
                view = self.param[o:o + n].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self.grad[o:o + n].view(p.shape)
                p._mbv_arena = True                         # ops.linear accumulates dW / db into p.grad directly
                if self.shadow is not None:
                    p._mbv_shadow = self.shadow[o:o + n].view(p.shape)
        self.refresh_shadow()

    # -- views ------------------------------------------------------------------------------------------
    def segment(self, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        a, b = self.segments[name]
        return self.param[a:b], self.grad[a:b]

    def span(self, names: Iterable[str]) -> Tuple[int, int]:
        """Smallest contiguous range covering the named segments."""
        ab = [self.segments[n] for n in names]
        return min(a for a, _ in ab), max(b for _, b in ab)

    def range_of(self, module_or_params) -> Tuple[int, int]:
        """Arena range [lo, hi) holding exactly the parameters of a sub-module (they are laid out in registration
        order, so a sub-module's parameters are contiguous); raises if other parameters are interleaved."""
        params = list(module_or_params.parameters()) if isinstance(module_or_params, nn.Module) else list(module_or_params)
        ids = {id(p) for p in params}
        inside = [(o, o + _round_up(p.numel(), _ALIGN)) for p, o in self.layout if id(p) in ids]
        if len(inside) != len(ids):
            raise ValueError('parameters outside the arena')
        lo, hi = min(a for a, _ in inside), max(b for _, b in inside)
        if any(lo <= o < hi and id(p) not in ids for p, o in self.layout):
            raise ValueError('the parameters are not contiguous in the arena')
        return lo, hi

    # -- maintenance ------------------------------------------------------------------------------------
    @property
    def shadow_flag(self) -> int:
        """MBV_DT_BF16 / MBV_DT_F16 (maskbev_hip.h); 0 without a shadow."""
        return 0 if self.shadow is None else (2 if self.shadow.dtype == torch.float16 else 1)

    def refresh_shadow(self):
        """Re-derive the 16-bit shadow from the f32 parameters (after load_state_dict / broadcast / manual edits)."""
        ops.note_parameters_changed()
        if self.shadow is None or self.numel == 0:
            return
        if self.device.type != 'cuda':
            self.shadow.copy_(self.param)
            return
        lib = _lib.load()
        check(lib.mbv_refresh_shadow(self.param.data_ptr(), self.shadow.data_ptr(), self.shadow_flag, self.numel,
                                     torch.cuda.current_stream(self.device).cuda_stream), 'mbv_refresh_shadow')

    def zero_grad(self, names: Optional[Iterable[str]] = None):
        if names is None:
            self.grad.zero_()
        else:
            a, b = self.span(names)
            self.grad[a:b].zero_()

    def rebind(self):
        """Re-attach ``p.grad`` views (an ``optimizer.zero_grad(set_to_none=True)`` drops them)."""
        for p, o in self.layout:
            p.grad = self.grad[o:o + p.numel()].view(p.shape)

    def intact(self) -> bool:
        base = self.param.untyped_storage().data_ptr()
        return all(p.data.untyped_storage().data_ptr() == base for p, _ in self.layout)


class LossScaler:
    """Dynamic loss scaling for fp16 compute with ``torch.amp.GradScaler``'s rules (start at 2**16, halve on a
    non-finite gradient and skip that update, double after ``growth_interval`` clean steps) — but with the scale, the
    overflow flag and the clean-step count held on the device and read / updated by kernels (K11:
    ``mbv_grad_nonfinite``, ``mbv_adamw_step(loss_scale, skip_flag)``, ``mbv_loss_scale_update``), so that a step
    neither synchronises with the host nor changes shape: ``scale_loss`` is captured in the HIP graph like any other
    multiply.  Gradients are left scaled in the arena; the optimizer kernel divides on the fly."""

    def __init__(self, device, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        self.device = torch.device(device)
        self.scale = torch.full((1,), float(init_scale), dtype=torch.float32, device=self.device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.clean_steps = torch.zeros(1, dtype=torch.int32, device=self.device)
        # updates actually APPLIED (an overflowed step is skipped): Adam's bias-correction count, read by k_adamw
        self.applied_steps = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)

    def scale_loss(self, loss: torch.Tensor) -> torch.Tensor:
        return loss * self.scale.view(())

    def check(self, grad: torch.Tensor):
        """flag |= any non-finite element of ``grad`` (the all-reduced arena gradient)."""
        lib = _lib.load()
        check(lib.mbv_grad_nonfinite(grad.data_ptr(), grad.numel(), self.flag.data_ptr(),
                                     torch.cuda.current_stream(self.device).cuda_stream), 'mbv_grad_nonfinite')

    def update(self):
        lib = _lib.load()
        check(lib.mbv_loss_scale_update(self.scale.data_ptr(), self.clean_steps.data_ptr(), self.flag.data_ptr(),
                                        self.growth_factor, self.backoff_factor, self.growth_interval,
                                        self.applied_steps.data_ptr(),
                                        torch.cuda.current_stream(self.device).cuda_stream), 'mbv_loss_scale_update')

    def get_scale(self) -> float:
        return float(self.scale.item())

    def state_dict(self):
        return dict(scale=self.get_scale(), clean_steps=int(self.clean_steps.item()),
                    applied_steps=int(self.applied_steps.item()),
                    growth_factor=self.growth_factor, backoff_factor=self.backoff_factor,
                    growth_interval=self.growth_interval)

    def load_state_dict(self, sd):
        self.scale.fill_(float(sd['scale']))
        self.clean_steps.fill_(int(sd.get('clean_steps', 0)))
        if 'applied_steps' in sd:
            self.applied_steps.fill_(int(sd['applied_steps']))
        self.growth_factor = float(sd.get('growth_factor', self.growth_factor))
        self.backoff_factor = float(sd.get('backoff_factor', self.backoff_factor))
        self.growth_interval = int(sd.get('growth_interval', self.growth_interval))


def _refuse_frozen(arena: ParameterArena, who: str):
    frozen = [tuple(p.shape) for p, _ in arena.layout if not p.requires_grad]
    if frozen:          # the single launch updates (and decays) every element of a segment; torch skips frozen ones
        raise ValueError(f'{who} updates whole arena segments: {len(frozen)} frozen parameter(s) in the arena '
                         f'(first shape {frozen[0]}); keep frozen parameters out of the arena')


def _segment_groups(arena: ParameterArena, groups: List[dict]) -> List[dict]:
    """torch ``param_groups`` over arena segments: one flat parameter per group, the segment's name kept."""
    pgs = []
    for g in groups:
        a, b = arena.segments[g['segment']]
        flat = nn.Parameter(arena.param[a:b], requires_grad=True)
        flat.grad = arena.grad[a:b]
        pg = {k: v for k, v in g.items() if k != 'segment'}
        pg['params'] = [flat]
        pg['segment'] = g['segment']
        pgs.append(pg)
    return pgs


def _merged_runs(arena: ParameterArena, param_groups: List[dict], hyper) -> List[list]:
    """[[a, b, hp], ...]: adjacent groups whose ``hyper(pg)`` tuples are equal share one launch over [a, b)."""
    runs: List[list] = []
    for pg in param_groups:
        a, b = arena.segments[pg['segment']]
        hp = hyper(pg)
        if runs and runs[-1][2] == hp and runs[-1][1] == a:
            runs[-1][1] = b
        else:
            runs.append([a, b, hp])
    return runs


def _load_per_parameter_state(arena: ParameterArena, state: dict, fields: Dict[str, torch.Tensor], what: str) -> int:
    """Map a per-parameter torch optimizer state (numbered in module.parameters() order = the order of the arena layout)
    onto flat buffers: ``fields`` = {state key: flat destination}.  Returns the largest ``step`` found (0 without one)."""
    if len(state) != len(arena.layout):
        raise ValueError(f'optimizer state has {len(state)} parameters, the arena {len(arena.layout)}: '
                         f'cannot map a per-parameter {what} state onto the arena')
    steps = 0
    with torch.no_grad():
        for idx, (p, o) in enumerate(arena.layout):
            st = state[idx] if idx in state else state[str(idx)]
            n = p.numel()
            for key, flat in fields.items():
                if tuple(st[key].shape) != tuple(p.shape):
                    raise ValueError(f'optimizer state {idx} has shape {tuple(st[key].shape)}, '
                                     f'parameter {tuple(p.shape)}')
                flat[o:o + n].copy_(st[key].reshape(-1))
            if 'step' in st:
                steps = max(steps, int(st['step']))
    return steps


class FlatOptimizer(torch.optim.Optimizer):
    """What the flat optimizers share: the frame of ``step()`` (closure, cached-record invalidation, step count, the
    :class:`LossScaler` check before and update after the launches of ``_launch``), ``zero_grad`` and the checkpoint format.

    ``state_dict()['flat_state']`` holds the flat buffers named in ``STATE``, ``kind`` = ``KIND`` and — for the classes that
    count steps — ``steps``, the number of APPLIED updates (with a scaler that count lives on the device,
    ``LossScaler.applied_steps``).  ``load_state_dict`` takes that format (a ``kind`` other than the class's own is refused;
    a state without one, from before the key existed, is accepted), or a per-parameter torch state mapped through the arena
    layout, and restores the ``HYPER`` keys of the param groups.

    **Gradient clipping by global norm (K41).**  ``max_grad_norm`` (``None`` = off: nothing is allocated and every launch is
    what it was; a positive float or ``float('inf')`` = on, fixed for the optimizer's lifetime) makes ``step()`` measure the
    2-norm of the gradient the optimizer is about to apply — ``grad * grad_scale / loss scale``, so the fp16 loss scale and
    the data-parallel ``1 / world`` are accounted for — over the arena's segments in two launches (``mbv_grad_norm_partials``,
    ``mbv_grad_clip_coef``) with ``torch.nn.utils.clip_grad_norm_``'s rule ``coef = min(1, max_norm / (norm + 1e-6))``.
    They leave one device float, ``loss scale / coef``, which the update kernels take in place of the loss scale:

    * the gradient buffer is never scaled in place — with ``zero_grad=False``, ``p.grad`` after ``step()`` holds the
      UN-clipped gradient, where torch's utility scales ``p.grad`` itself;
    * ``float('inf')`` measures and never clips: the update is bit for bit the one without clipping;
    * the threshold crosses the C ABI as an f32: 0.01 is applied as float32(0.01), 2e-8 relative from the double torch's
      utility would use, while the ``max_grad_norm`` property returns the value as given;
    * an overflowed fp16 step is skipped as before; it reports ``grad_norm = inf`` and the loss-scale protocol is untouched;
    * a non-finite norm WITHOUT a scaler poisons the parameters, as ``clip_grad_norm_(error_if_nonfinite=False)`` followed
      by ``step()`` does.

    ``grad_norm``, ``clip_coef`` and ``grad_norms()`` are views of the device record of the last step: reading them costs no
    host synchronisation until the caller asks for a value."""

    KIND = ''                   # 'adam' | 'lamb' | 'sgd'
    STATE: Tuple[str, ...] = ()  # the flat state buffers, each the size of the arena
    HYPER: Tuple[str, ...] = ()  # param-group keys a checkpoint restores
    COUNTS_STEPS = True         # keeps ``steps``
    ENTRY = ''                  # the native entry point named when a CPU arena is refused

    def __init__(self, arena: ParameterArena, param_groups, defaults: dict, scaler: Optional[LossScaler],
                 zero_grad: bool = True, max_grad_norm: Optional[float] = None):
        self.arena = arena
        self.scaler = scaler
        self.zero_grad_in_step = zero_grad
        self.grad_scale = 1.0
        _refuse_frozen(arena, type(self).__name__)
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:
                raise ValueError(f'max_grad_norm must be positive (inf measures without clipping), got {max_grad_norm}')
            if len(arena.segments) > CLIP_RANGES:
                raise ValueError(f'gradient clipping sums at most {CLIP_RANGES} arena segments, the arena has '
                                 f'{len(arena.segments)}')
        self._max_grad_norm = max_grad_norm
        super().__init__(param_groups, defaults)
        for name in self.STATE:
            setattr(self, name, torch.zeros_like(arena.param))
        if self.COUNTS_STEPS:
            self.steps = 0
        if max_grad_norm is not None:
            # K41: the segments as element ranges, their chunk boundaries in the partial slab, and the 16-float device record
            spans = list(arena.segments.values())
            bounds = [0]
            for a, b in spans:
                bounds.append(bounds[-1] + (b - a + LAMB_CHUNK - 1) // LAMB_CHUNK)
            self._clip_start = (ctypes.c_int64 * len(spans))(*[a for a, _ in spans])
            self._clip_len = (ctypes.c_int64 * len(spans))(*[b - a for a, b in spans])
            self._clip_bounds = (ctypes.c_int32 * len(bounds))(*bounds)
            self._clip_partials = torch.zeros(max(1, bounds[-1]), dtype=torch.float64, device=arena.device)
            self._clip_rec = torch.zeros(16, dtype=torch.float32, device=arena.device)
            self._clip_rec[2] = 1.0             # before the first step: norm 0, coefficient 1

    def _require_cuda(self):
        if self.arena.device.type != 'cuda':
            raise _lib.MaskBevHipError(f'{type(self).__name__} runs on the MI355X only ({self.ENTRY})')

    # -- K41: clipping by global norm ----------------------------------------------------------------------------------
    @property
    def max_grad_norm(self) -> Optional[float]:
        """The clipping threshold given at construction (``None``: no clipping, no norm)."""
        return self._max_grad_norm

    def _clip_record(self) -> torch.Tensor:
        if self._max_grad_norm is None:
            raise _lib.MaskBevHipError(f'{type(self).__name__} was built without max_grad_norm: no gradient norm is measured')
        return self._clip_rec

    @property
    def grad_norm(self) -> torch.Tensor:
        """0-d device tensor: the last step's total norm of the gradient as applied (un-scaled, data-parallel mean)."""
        return self._clip_record()[1]

    @property
    def clip_coef(self) -> torch.Tensor:
        """0-d device tensor: the last step's coefficient ``min(1, max_grad_norm / (grad_norm + 1e-6))``."""
        return self._clip_record()[2]

    def grad_norms(self) -> Dict[str, torch.Tensor]:
        """Segment name -> 0-d device tensor: the last step's gradient norm of each arena segment."""
        rec = self._clip_record()
        return {name: rec[3 + i] for i, name in enumerate(self.arena.segments)}

    def _measure_norm(self, lib, stream: int):
        """The two K41 launches over the arena's segments: the record's divisor is what ``_scaler_ptrs`` hands on."""
        ar, sc = self.arena, self.scaler
        n_partials = self._clip_bounds[len(self._clip_bounds) - 1]
        with ops.TIMER.span('k_grad_norm_partials'):
            check(lib.mbv_grad_norm_partials(ar.grad.data_ptr(), ar.numel, self._clip_start, self._clip_len,
                                             len(self._clip_start), self._clip_partials.data_ptr(), n_partials, stream),
                  'mbv_grad_norm_partials')
        with ops.TIMER.span('k_grad_clip_coef'):
            check(lib.mbv_grad_clip_coef(self._clip_partials.data_ptr(), n_partials, self._clip_bounds, len(self._clip_start),
                                         self._max_grad_norm, float(self.grad_scale),
                                         0 if sc is None else sc.scale.data_ptr(), self._clip_rec.data_ptr(), stream),
                  'mbv_grad_clip_coef')

    def _scaler_ptrs(self) -> Tuple[int, int, int]:
        """(loss scale, overflow flag, applied-step count) device addresses; zeros without a scaler.  With clipping the
        first is the record's divisor ``loss scale / clip coefficient``, which the kernels divide by where they divided by
        the loss scale."""
        sc = self.scaler
        flag, applied = (0, 0) if sc is None else (sc.flag.data_ptr(), sc.applied_steps.data_ptr())
        if self._max_grad_norm is not None:
            return self._clip_rec.data_ptr(), flag, applied
        return (0 if sc is None else sc.scale.data_ptr()), flag, applied

    def _launch(self, lib, stream: int):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._require_cuda()
        ops.note_parameters_changed()          # cached per-weight records (K20's absmax words) die with this update
        if self.COUNTS_STEPS:
            self.steps += 1
        sc = self.scaler
        if sc is not None:
            sc.check(self.arena.grad)
        lib, stream = _lib.load(), torch.cuda.current_stream(self.arena.device).cuda_stream
        if self._max_grad_norm is not None:
            self._measure_norm(lib, stream)
        self._launch(lib, stream)
        if sc is not None:
            sc.update()
        return loss

    def zero_grad(self, set_to_none: bool = False):
        """Gradients live in the arena: clear in place (``step()`` already did when ``zero_grad_in_step``)."""
        if not self.zero_grad_in_step:
            self.arena.zero_grad()

    def state_dict(self):
        sd = super().state_dict()
        flat = {name: getattr(self, name) for name in self.STATE}
        if self.COUNTS_STEPS:
            flat['steps'] = self.steps if self.scaler is None else int(self.scaler.applied_steps.item())
        flat['kind'] = self.KIND
        sd['flat_state'] = flat
        if self.scaler is not None:
            sd['loss_scaler'] = self.scaler.state_dict()
        return sd

    def load_state_dict(self, sd):
        if self.scaler is not None and sd.get('loss_scaler') is not None:
            self.scaler.load_state_dict(sd['loss_scaler'])
        flat, steps = sd.get('flat_state'), None
        if flat is not None:
            if flat.get('kind', self.KIND) != self.KIND:
                raise ValueError(f"flat optimizer state of kind {flat.get('kind')!r} cannot be loaded into "
                                 f"{type(self).__name__}")
            for name in self.STATE:
                getattr(self, name).copy_(flat[name])
            if self.COUNTS_STEPS:
                steps = int(flat['steps'])
        elif sd.get('state'):
            # a per-parameter state_dict (torch.optim.Adam / AdamW / SGD, optimizers.Lamb / torch_optimizer.Lamb: the
            # reference's checkpoints, or a run saved without the arena): its parameters are numbered in
            # module.parameters() order = the order of the arena layout
            steps = _load_per_parameter_state(self.arena, sd['state'], {name: getattr(self, name) for name in self.STATE},
                                              type(self).__name__[len('Flat'):])
        if self.COUNTS_STEPS and steps is not None:
            self.steps = steps
            if self.scaler is not None:
                self.scaler.applied_steps.fill_(steps)
        for pg, saved in zip(self.param_groups, sd.get('param_groups', [])):
            for k in self.HYPER:
                if k in saved:
                    pg[k] = saved[k]


class FlatAdam(FlatOptimizer):
    """Adam / AdamW over a :class:`ParameterArena`: one ``mbv_adamw_step`` launch per parameter group.

    ``param_groups`` carry ``lr`` / ``weight_decay`` / ``betas`` / ``eps`` like torch's optimizers, so the
    reference's schedulers (ReduceLROnPlateau, CosineAnnealingLR — mask_bev_module.py:153-159) drive it unchanged.
    Adjacent groups with identical hyper-parameters are fused into one launch.  ``step()`` also refreshes the 16-bit
    shadow and clears the gradient in the same pass (``zero_grad=True``).  With a :class:`LossScaler` (fp16 compute) the
    gradient is checked for inf / nan first, un-scaled inside the update kernel, and an overflowed step leaves
    parameters and moments untouched, and Adam's bias-correction count does not advance either: with a scaler the count
    of APPLIED updates lives on the device (``LossScaler.applied_steps``, incremented by ``mbv_loss_scale_update``), as
    ``torch.amp.GradScaler`` skipping ``optimizer.step()`` would leave torch's.  ``state_dict()['flat_state']['steps']``
    is that count."""

    KIND, STATE, HYPER = 'adam', ('exp_avg', 'exp_avg_sq'), ('lr', 'betas', 'eps', 'weight_decay')
    ENTRY = 'mbv_adamw_step'

    def __init__(self, arena: ParameterArena, groups: List[dict], lr: float = 1e-3, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 1e-2, decoupled: bool = True, zero_grad: bool = True,
                 scaler: Optional[LossScaler] = None, max_grad_norm: Optional[float] = None):
        self.decoupled = decoupled
        super().__init__(arena, _segment_groups(arena, groups), dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay),
                         scaler, zero_grad, max_grad_norm)
        self._k3 = None              # (weight, bias, offset_w, offset_b) of a LayerNorm whose update K3's backward performs
        self._k3_applied = False
        self._mx: Dict[int, nn.Parameter] = {}     # arena offset -> weight whose update its weight-gradient GEMM performs
        self._mx_applied: set = set()              # offsets of those a pass has updated since the last step()
        self._adam_dev = None        # (param groups, 16) words: one mbv_adam_dev block per group, read by those GEMMs

    # -- K3 backward + AdamW of the (C, ny, nx) LayerNorm affine in one launch (csrc/scatter_layernorm.hip, ADAM) ------------
    def fuse_layernorm_affine(self, weight: Optional[nn.Parameter], bias: Optional[nn.Parameter] = None) -> bool:
        """Ask K3's backward to perform the AdamW update of ``weight`` / ``bias`` (the encoder's (C, ny, nx) LayerNorm affine,
        a third of the model's parameters) itself: their gradients are complete in that kernel's registers, so they never
        reach the arena — 16 B per parameter of gradient traffic less per step.  The CALLER guarantees one backward pass
        per ``step()`` (the graph step does); a second pass before ``step()`` raises.  Not with a loss scaler (an overflowed
        step must skip EVERY update, and the verdict is only known after the whole backward) and not with a gradient
        all-reduce (``grad_scale`` != 1: the reduced gradient does not exist inside the kernel), and for the same reason not
        with ``max_grad_norm``: the clip coefficient needs the norm of the WHOLE gradient, which exists only after the
        backward, and a gradient consumed here never reaches the arena to be measured.  ``None`` disarms.
        The arm is a weak reference on the weight (``weight._mbv_k3_adam``), where K3's backward finds it: several optimizers
        can be armed at once, each for its own parameters, and a dropped optimizer disarms itself.
        Returns whether the fusion is armed."""
        if self._k3 is not None and self.k3_armed(self._k3[0]):
            del self._k3[0]._mbv_k3_adam
        self._k3, self._k3_applied = None, False
        if (weight is None or bias is None or self.scaler is not None or not self.zero_grad_in_step
                or self._max_grad_norm is not None):
            return False
        off = {id(p): o for p, o in self.arena.layout}
        if id(weight) not in off or id(bias) not in off or weight.shape != bias.shape:
            return False
        self._k3 = (weight, bias, off[id(weight)], off[id(bias)])
        # the two ranges are cut out of k_adamw from now on: nothing would apply or clear what their gradient holds
        for o in self._k3[2:]:
            self.arena.grad[o:o + _round_up(weight.numel(), _ALIGN)].zero_()
        weight._mbv_k3_adam = weakref.ref(self)
        return True

    def k3_armed(self, weight) -> bool:
        """This optimizer is the live arm of ``weight``: K3's backward hands it the update of that LayerNorm affine."""
        ref = getattr(weight, '_mbv_k3_adam', None)
        return ref is not None and ref() is self

    def claim(self, weight, bias):
        """Called by K3's backward: the optimizer state of (weight, bias) for the fused update, or None (not the armed
        parameters / a data-parallel step).  Marks the update as applied for the coming ``step()``."""
        k3 = self._k3
        if k3 is None or weight is not k3[0] or bias is not k3[1] or float(self.grad_scale) != 1.0:
            return None
        if self._k3_applied:
            raise _lib.MaskBevHipError('FlatAdam: K3 backward ran twice before step() with the fused LayerNorm-affine update '
                                       'armed (gradient accumulation needs fuse_layernorm_affine(None))')
        _, _, ow, ob = k3
        pg = self._group_of(ow)
        n = weight.numel()
        if self._group_of(ob + n - 1) is not pg:
            return None
        ar = self.arena
        self._k3_applied = True
        return dict(m_w=self.exp_avg.data_ptr() + 4 * ow, v_w=self.exp_avg_sq.data_ptr() + 4 * ow,
                    m_b=self.exp_avg.data_ptr() + 4 * ob, v_b=self.exp_avg_sq.data_ptr() + 4 * ob,
                    sh_w=0 if ar.shadow is None else ar.shadow.data_ptr() + 2 * ow,
                    sh_b=0 if ar.shadow is None else ar.shadow.data_ptr() + 2 * ob, shadow_flag=ar.shadow_flag,
                    lr=float(pg['lr']), beta1=float(pg['betas'][0]), beta2=float(pg['betas'][1]), eps=float(pg['eps']),
                    weight_decay=float(pg['weight_decay']), step=self.steps + 1, decoupled=1 if self.decoupled else 0)

    # -- AdamW of Linear weights in the epilogue of their weight-gradient product (csrc/gemm.hip, k_gemm16_tn_group) --------------
    def fuse_matrices(self, params: Optional[Iterable[nn.Parameter]]) -> bool:
        """Ask the grouped K17 weight-gradient launch (``ops.launch_tn_group``) to perform the AdamW update of these 2-D
        weights itself: a product whose token sum is one work item deep holds the complete gradient of its tile in registers,
        so the gradient never reaches the arena — 16 B per parameter of gradient traffic less per step.  Only weights used
        ONCE per pass qualify (a second product for an armed weight raises), and the CALLER guarantees one backward pass per
        ``step()``; a second pass before ``step()`` raises.  Refused with a loss scaler, with ``grad_scale`` != 1 and without
        ``zero_grad_in_step``, as :meth:`fuse_layernorm_affine` and for its reasons, and with ``max_grad_norm`` (the update
        would run before the norm of the whole gradient exists, on a gradient the norm never sees).  ``None`` disarms.  The arm is a weak
        reference on the weight's gradient view (``p.grad._mbv_adam``), where the launcher finds it.  A product that does not
        qualify when it runs (deeper token sum, another kernel) leaves its weight to ``mbv_adamw_step`` as ever: what is cut
        out of that pass is what a launch REPORTED applied.  Returns whether anything is armed."""
        for p in self._mx.values():
            g = p.grad
            ref = getattr(g, '_mbv_adam', None) if g is not None else None
            if ref is not None and ref() is self:
                del g._mbv_adam
        self._mx, self._mx_applied = {}, set()
        params = list(params or [])
        if (not params or self.scaler is not None or float(self.grad_scale) != 1.0 or not self.zero_grad_in_step
                or self._max_grad_norm is not None or self.arena.device.type != 'cuda'):
            return False
        off = {id(p): o for p, o in self.arena.layout}
        for p in params:
            o = off.get(id(p))
            g = p.grad
            if (o is None or p.dim() != 2 or p.numel() % 8 or g is None
                    or g.data_ptr() != self.arena.grad.data_ptr() + 4 * o or self._group_of(o) is None):
                continue
            self._mx[o] = p
            # the range is cut out of k_adamw whenever a launch applied it: nothing would clear what its gradient holds
            self.arena.grad[o:o + _round_up(p.numel(), _ALIGN)].zero_()
            g._mbv_adam = weakref.ref(self)
        if self._mx and self._adam_dev is None:
            self._adam_dev = torch.zeros(len(self.param_groups), 16, dtype=torch.float32, device=self.arena.device)
        return bool(self._mx)

    @property
    def matrices_armed(self) -> bool:
        return bool(self._mx)

    def _matrix_offset(self, acc: torch.Tensor) -> Optional[int]:
        o = (acc.data_ptr() - self.arena.grad.data_ptr()) // 4
        p = self._mx.get(o)
        return o if p is not None and acc.numel() == p.numel() else None

    def claim_matrix(self, acc: torch.Tensor) -> int:
        """Called by the launcher for a destination ``acc``: the device address of the hyper-parameter block the fused update
        of that weight reads, or 0 (not armed / a data-parallel step)."""
        o = self._matrix_offset(acc)
        if o is None or float(self.grad_scale) != 1.0:
            return 0
        if o in self._mx_applied:
            raise _lib.MaskBevHipError('FlatAdam: a second weight-gradient product before step() for a weight whose update '
                                       'is fused into that product (gradient accumulation needs fuse_matrices(None))')
        pg = self._group_of(o)
        return self._adam_dev.data_ptr() + 64 * next(i for i, q in enumerate(self.param_groups) if q is pg)

    def write_adam_blocks(self):
        """The hyper-parameters of the COMING update (``steps + 1``) into every group's device block, on the current stream:
        before each replay of a graph that holds fused launches, or right in front of an eager one."""
        if not self._mx:
            return
        lib, stream = _lib.load(), torch.cuda.current_stream(self.arena.device).cuda_stream
        for i, pg in enumerate(self.param_groups):
            check(lib.mbv_adam_args_write(self._adam_dev.data_ptr() + 64 * i, float(pg['lr']), float(pg['betas'][0]),
                                          float(pg['betas'][1]), float(pg['eps']), float(pg['weight_decay']), self.steps + 1,
                                          1 if self.decoupled else 0, self.arena.shadow_flag, stream), 'mbv_adam_args_write')

    def note_matrices_applied(self, accs) -> None:
        """These destinations' updates were applied by a launch (or by the replay of one): the coming ``step()`` skips them."""
        for acc in accs:
            o = acc if isinstance(acc, int) else self._matrix_offset(acc)
            if o is not None and o in self._mx:
                self._mx_applied.add(o)

    def take_matrices_applied(self) -> List[int]:
        """Offsets marked applied, unmarking them: what a graph CAPTURE recorded (nothing ran) and each replay re-announces."""
        done, self._mx_applied = sorted(self._mx_applied), set()
        return done

    def _group_of(self, offset: int):
        for pg in self.param_groups:
            a, b = self.arena.segments[pg['segment']]
            if a <= offset < b:
                return pg
        return None

    @staticmethod
    def _cut(runs: List[list], ranges) -> List[list]:
        """``runs`` without the element ranges ``[(lo, hi), ...]``: what a fused kernel already updated."""
        for lo, hi in sorted(ranges, reverse=True):
            cut = []
            for a, b, hp in runs:
                if lo >= b or hi <= a:
                    cut.append([a, b, hp])
                else:
                    if a < lo:
                        cut.append([a, lo, hp])
                    if hi < b:
                        cut.append([hi, b, hp])
            runs = cut
        return runs

    def _launch(self, lib, stream):
        ar = self.arena
        # fuse adjacent groups with the same hyper-parameters into one launch
        runs = _merged_runs(ar, self.param_groups, lambda pg: (float(pg['lr']), float(pg['betas'][0]), float(pg['betas'][1]),
                                                               float(pg['eps']), float(pg['weight_decay'])))
        if self._k3_applied:
            # K3's backward already updated these two parameters (and left their gradient range untouched: zero): cut their
            # element ranges out of the launches
            self._k3_applied = False
            w, bp, ow, ob = self._k3
            runs = self._cut(runs, [(o, o + _round_up(w.numel(), _ALIGN)) for o in (ow, ob)])
        if self._mx_applied:
            # ... and the weight-gradient launches these matrices
            runs = self._cut(runs, [(o, o + _round_up(self._mx[o].numel(), _ALIGN)) for o in self.take_matrices_applied()])
        scale, flag, applied = self._scaler_ptrs()
        runs = [r for r in runs if r[1] > r[0]]
        # what the cuts leave between the matrices of a block — biases, LayerNorm affines, position tables — is dozens of short
        # ranges: those of one hyper-parameter set share a launch (mbv_adamw_step_ranges) instead of taking one each
        short: Dict[tuple, list] = {}
        for a, b, hp in runs:
            if b - a < _SHORT_RUN:
                short.setdefault(hp, []).append((a, b))
        for hp, rs in short.items():
            if len(rs) < 2:
                continue
            runs = [r for r in runs if r[2] != hp or (r[0], r[1]) not in rs]
            lr, b1, b2, eps, wd = hp
            LA = ctypes.c_int64 * len(rs)
            with ops.TIMER.span('k_adamw'):
                check(lib.mbv_adamw_step_ranges(ar.param.data_ptr(), ar.grad.data_ptr(), self.exp_avg.data_ptr(),
                                                self.exp_avg_sq.data_ptr(), 0 if ar.shadow is None else ar.shadow.data_ptr(),
                                                ar.shadow_flag, ar.numel, LA(*[a for a, _ in rs]), LA(*[b - a for a, b in rs]),
                                                len(rs), lr, b1, b2, eps, wd, self.steps, float(self.grad_scale),
                                                1 if self.decoupled else 0, 1 if self.zero_grad_in_step else 0, scale, flag,
                                                applied, stream), 'mbv_adamw_step_ranges')
        for a, b, (lr, b1, b2, eps, wd) in runs:
            sh = 0 if ar.shadow is None else ar.shadow.data_ptr() + 2 * a
            with ops.TIMER.span('k_adamw'):
                check(lib.mbv_adamw_step(ar.param.data_ptr() + 4 * a, ar.grad.data_ptr() + 4 * a,
                                         self.exp_avg.data_ptr() + 4 * a, self.exp_avg_sq.data_ptr() + 4 * a, sh,
                                         ar.shadow_flag, b - a, lr, b1, b2, eps, wd, self.steps,
                                         float(self.grad_scale), 1 if self.decoupled else 0,
                                         1 if self.zero_grad_in_step else 0, scale, flag, applied, stream),
                      'mbv_adamw_step')


LAMB_CHUNK = 4096    # elements per chunk of the LAMB chunk table (kChunk of csrc/optim_flat.hip)


class FlatLamb(FlatOptimizer):
    """LAMB over a :class:`ParameterArena` (K40, csrc/optim_flat.hip): the rule of ``torch_optimizer.Lamb`` — the Adam
    direction ``u = m / (sqrt(v) + eps) + weight_decay * p`` scaled per parameter TENSOR by the trust ratio
    ``min(||p||, clamp_value) / ||u||`` — in three kinds of launch whatever the number of tensors: ``mbv_lamb_moments``
    (moments, ``u`` and per-chunk partial sums of ``p²`` and ``u²``), ``mbv_lamb_trust`` (one ratio per tensor) and
    ``mbv_lamb_apply`` (update, 16-bit shadow, gradient clear).  The per-tensor norms come from a chunk table built here
    once (every parameter's padded range cut into chunks of ``LAMB_CHUNK`` elements) and a partial slab; no float atomics,
    so a step is bit-reproducible and replays from a graph.

    Same ``param_groups`` contract as :class:`FlatAdam` (the schedulers drive ``lr``; adjacent groups with equal
    hyper-parameters share a launch), same :class:`LossScaler` and ``grad_scale`` conventions.  ``zero_grad_in_step`` is
    always true: the moments pass stashes ``u`` in the gradient buffer and the apply pass clears it, so the gradient does
    not survive a step.  There is no ``fuse_layernorm_affine``: the trust ratio needs the whole tensor's norm, which K3's
    backward does not have.  ``trust_ratio`` holds the last step's ratio of every arena parameter, in layout order."""

    KIND, STATE, HYPER = 'lamb', ('exp_avg', 'exp_avg_sq'), ('lr', 'betas', 'eps', 'weight_decay')
    ENTRY = 'mbv_lamb_moments'

    def __init__(self, arena: ParameterArena, groups: List[dict], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.0, clamp_value: float = 10.0, debias: bool = False,
                 scaler: Optional[LossScaler] = None, max_grad_norm: Optional[float] = None):
        self.arena = arena
        self._require_cuda()
        self.clamp_value = float(clamp_value)
        self.debias = bool(debias)
        super().__init__(arena, _segment_groups(arena, groups), dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay),
                         scaler, max_grad_norm=max_grad_norm)
        # chunk table: (start, len | param << 32) per chunk = mbv_lamb_chunk; [chunk_begin, chunk_end) per parameter
        import numpy as np
        recs, ranges = [], []
        self._chunk_at: Dict[int, int] = {}            # arena offset of a parameter (or the arena's end) -> its first chunk
        for i, (p, o) in enumerate(arena.layout):
            self._chunk_at[o] = len(recs)
            end = o + _round_up(p.numel(), _ALIGN)
            begin = len(recs)
            for s in range(o, end, LAMB_CHUNK):
                recs.append((s, min(LAMB_CHUNK, end - s), i))
            ranges.append((begin, len(recs)))
        self._chunk_at[arena.numel] = len(recs)
        table = np.zeros(len(recs), dtype=np.dtype([('start', '<i8'), ('len', '<i4'), ('param', '<i4')]))
        for k, name in enumerate(('start', 'len', 'param')):
            table[name] = [r[k] for r in recs]
        self.n_chunks, self.n_params = len(recs), len(ranges)
        self._chunks = torch.from_numpy(table.view(np.int64).reshape(-1, 2).copy()).to(arena.device)
        self._param_chunks = torch.tensor(ranges, dtype=torch.int32).reshape(-1, 2).to(arena.device)
        self._partials = torch.zeros(2, max(1, self.n_chunks), dtype=torch.float32, device=arena.device)
        self.trust_ratio = torch.ones(self.n_params, dtype=torch.float32, device=arena.device)

    def _chunk_range(self, a: int, b: int) -> Tuple[int, int]:
        """Chunks of the element range [a, b), whose ends are parameter boundaries (segments are)."""
        return self._chunk_at[a], self._chunk_at[b]

    def _launch(self, lib, stream):
        ar = self.arena
        scale, flag, applied = self._scaler_ptrs()
        hint = _lib.WORK_HINT.setdefault('lamb_elems', {})
        # the learning rate only enters the apply pass: the moments passes merge over it
        for a, b, (b1, b2, eps, wd) in _merged_runs(ar, self.param_groups, lambda pg: (
                float(pg['betas'][0]), float(pg['betas'][1]), float(pg['eps']), float(pg['weight_decay']))):
            c0, c1 = self._chunk_range(a, b)
            hint[(c0, c1)] = b - a
            with ops.TIMER.span('k_lamb_moments'):
                check(lib.mbv_lamb_moments(ar.param.data_ptr(), ar.grad.data_ptr(), self.exp_avg.data_ptr(),
                                           self.exp_avg_sq.data_ptr(), ar.numel, self._chunks.data_ptr(), self.n_chunks,
                                           c0, c1, self._partials.data_ptr(), b1, b2, eps, wd, float(self.grad_scale),
                                           scale, flag, stream), 'mbv_lamb_moments')
        with ops.TIMER.span('k_lamb_trust'):
            check(lib.mbv_lamb_trust(self._partials.data_ptr(), self.n_chunks, self._param_chunks.data_ptr(), self.n_params,
                                     self.clamp_value, self.trust_ratio.data_ptr(), stream), 'mbv_lamb_trust')
        sh = 0 if ar.shadow is None else ar.shadow.data_ptr()
        for a, b, (lr, b1, b2) in _merged_runs(ar, self.param_groups, lambda pg: (
                float(pg['lr']), float(pg['betas'][0]), float(pg['betas'][1]))):
            c0, c1 = self._chunk_range(a, b)
            hint[(c0, c1)] = b - a
            with ops.TIMER.span('k_lamb_apply'):
                check(lib.mbv_lamb_apply(ar.param.data_ptr(), ar.grad.data_ptr(), sh, ar.shadow_flag, ar.numel,
                                         self._chunks.data_ptr(), self.n_chunks, c0, c1, self.trust_ratio.data_ptr(),
                                         self.n_params, lr, b1, b2, 1 if self.debias else 0, self.steps, applied, flag,
                                         stream), 'mbv_lamb_apply')


class FlatSGD(FlatOptimizer):
    """SGD with (Nesterov) momentum over a :class:`ParameterArena` (K40): one ``mbv_sgd_step`` launch over the whole arena
    in ``torch.optim.SGD``'s single-tensor order, with the 16-bit shadow refresh and the gradient clear folded in and the
    :class:`LossScaler` / ``grad_scale`` conventions of :class:`FlatAdam`.

    ONE group over the whole arena: the reference builds its SGD from ``self.parameters()`` and so ignores
    ``differential_lr`` (mask_bev_module.py:145-147); that quirk is kept.  One moment buffer, zero-initialised — equal to
    torch's first-step ``buf = grad`` exactly when ``dampening`` is 0; with a non-zero ``dampening`` the first step's
    buffer is ``(1 - dampening) * grad``."""

    KIND, STATE, HYPER = 'sgd', ('momentum_buffer',), ('lr', 'momentum', 'dampening', 'weight_decay', 'nesterov')
    COUNTS_STEPS = False
    ENTRY = 'mbv_sgd_step'

    def __init__(self, arena: ParameterArena, lr: float = 1e-3, momentum: float = 0.99, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = True, zero_grad: bool = True,
                 scaler: Optional[LossScaler] = None, max_grad_norm: Optional[float] = None):
        self.arena = arena
        self._require_cuda()
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        flat = nn.Parameter(arena.param, requires_grad=True)
        flat.grad = arena.grad
        super().__init__(arena, [flat], dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                             nesterov=nesterov), scaler, zero_grad, max_grad_norm)

    def _launch(self, lib, stream):
        ar = self.arena
        scale, flag, _ = self._scaler_ptrs()
        pg = self.param_groups[0]
        with ops.TIMER.span('k_sgd'):
            check(lib.mbv_sgd_step(ar.param.data_ptr(), ar.grad.data_ptr(), self.momentum_buffer.data_ptr(),
                                   0 if ar.shadow is None else ar.shadow.data_ptr(), ar.shadow_flag, ar.numel,
                                   float(pg['lr']), float(pg['momentum']), float(pg['dampening']),
                                   float(pg['weight_decay']), 1 if pg['nesterov'] else 0, float(self.grad_scale),
                                   1 if self.zero_grad_in_step else 0, scale, flag, stream), 'mbv_sgd_step')


AVERAGE_MODES = {'ema': 0, 'mean': 1}     # MBV_AVERAGE_EMA / MBV_AVERAGE_MEAN (maskbev_hip.h)


class WeightAverage:
    """An averaged copy of a :class:`ParameterArena`'s parameters (K43, csrc/optim_flat.hip): the exponential moving average
    the Mask2Former family is evaluated and checkpointed on (mmengine's ``EMAHook``, timm's ``ModelEmaV2``) or SWA's
    equal-weight running mean.  ``avg`` is ONE more flat f32 buffer, initialised to a copy of ``arena.param``; an update is one
    C call (two launches) whatever the number of tensors, with no host synchronisation, and can be captured in a graph: the
    counters and the blend weight live in a 16-byte device record that the update itself advances.

    The rule of one ``update()`` (call it after ``optimizer.step()``), in f32 with one rounding per operation, for
    ``u`` = updates applied and ``c`` = applied optimizer steps seen so far:

    * with a :class:`LossScaler` the step counts only if the scaler's ``applied_steps`` moved since the last call — an
      overflowed fp16 step, which the optimizer skipped, leaves ``avg`` and both counters alone;
    * ``c += 1``; unless ``c % every == 0`` nothing else happens (the pass returns at once: launch latency only);
    * ``mode='mean'``: ``w = 1 / (u + 1)``;  ``mode='ema'``: ``w = 1 - d``, ``d = decay``, or with ``warmup``
      ``d = min(decay, (1 + u) / (10 + u))`` (timm's / ``torch.optim.swa_utils.get_ema_multi_avg_fn``'s warm-up);
    * ``avg = avg + w * (param - avg)`` (``avg = param`` exactly when ``w == 1``); ``u += 1``.

    ``decay`` crosses the C ABI as an f32: 0.9999 is applied as float32(0.9999), 2e-9 from the double, and ``w`` is
    ``1.0f - float32(decay)``; the ``decay`` attribute returns the value as given.  An f32 average with a small ``w`` stops
    moving once ``|param - avg|`` falls below about ``2**-24 / w`` of ``|avg|`` (``w = 1e-4``: 6e-4 relative) — true of every
    f32 EMA; compensated summation is not attempted.

    ``swap()`` exchanges ``param`` and ``avg`` in one pass that also rewrites the 16-bit shadow, and drops the cached
    per-weight records (``ops.note_parameters_changed``): the module then computes with the averaged weights, and a second
    ``swap()`` restores everything bit for bit.  ``applied()`` is the context manager for that.  While the average is swapped
    in, ``update()`` and ``state_dict()`` raise — ``param`` does not hold the live weights then.

    Module BUFFERS are not averaged (the PFN BatchNorm's running statistics, < 2 KB, not in the arena): evaluation under the
    average reads the live ones — mmengine's ``update_buffers=False`` default.

    A CPU arena is served by plain torch f32 operations, one per rounding (``swap`` = three copies and ``refresh_shadow``)."""

    KIND = 'weight_average'

    def __init__(self, arena: ParameterArena, mode: str = 'ema', decay: float = 0.9999, warmup: bool = True, every: int = 1,
                 scaler: Optional[LossScaler] = None):
        if mode not in AVERAGE_MODES:
            raise ValueError(f"weight average mode must be 'ema' or 'mean', got {mode!r}")
        self.arena = arena
        self.scaler = scaler
        self._set_hyper(mode, decay, warmup, every)
        self.avg = arena.param.detach().clone()
        # (updates, calls, seen, weight as f32 bits) = mbv_weight_average_state
        self._rec = torch.zeros(4, dtype=torch.int32, device=arena.device)
        self.is_applied = False
        self.reset()

    def _set_hyper(self, mode, decay, warmup, every):
        decay, every = float(decay), int(every)
        d32 = float(torch.tensor(decay, dtype=torch.float32))
        if not 0.0 <= d32 < 1.0:
            raise ValueError(f'weight average decay must lie in [0, 1) as a float32, got {decay}')
        if every < 1:
            raise ValueError(f'weight average every must be at least 1, got {every}')
        if mode not in AVERAGE_MODES:
            raise ValueError(f"weight average mode must be 'ema' or 'mean', got {mode!r}")
        self.mode, self.decay, self.warmup, self.every = mode, decay, bool(warmup), every

    # -- the record -----------------------------------------------------------------------------------------------------
    @property
    def num_updates(self) -> torch.Tensor:
        """0-d device tensor (int32): averaging updates applied so far."""
        return self._rec[0]

    @property
    def last_weight(self) -> torch.Tensor:
        """0-d device tensor (f32): the blend weight of the last ``update()``; 0 = it did nothing."""
        return self._rec.view(torch.float32)[3]

    @torch.no_grad()
    def reset(self):
        """``avg = param``, no updates and no calls so far; with a scaler, steps applied before now are not counted."""
        self._refuse_applied('reset()')
        self.avg.copy_(self.arena.param)
        self._rec.zero_()
        if self.scaler is not None:
            self._rec[2:3].copy_(self.scaler.applied_steps)        # device to device: no host synchronisation

    def _refuse_applied(self, what: str):
        if self.is_applied:
            raise _lib.MaskBevHipError(f'WeightAverage.{what} while the average is swapped in: arena.param holds the averaged '
                                       f'weights, not the live ones (swap() back first)')

    # -- update ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self):
        self._refuse_applied('update()')
        ar, sc = self.arena, self.scaler
        if ar.device.type != 'cuda':
            return self._update_torch()
        lib = _lib.load()
        with ops.TIMER.span('k_average_blend'):
            check(lib.mbv_weight_average_update(ar.param.data_ptr(), self.avg.data_ptr(), ar.numel, self._rec.data_ptr(),
                                                0 if sc is None else sc.applied_steps.data_ptr(), AVERAGE_MODES[self.mode],
                                                self.decay, 1 if self.warmup else 0, self.every,
                                                torch.cuda.current_stream(ar.device).cuda_stream),
                  'mbv_weight_average_update')

    def _update_torch(self):
        """The rule on a CPU arena: torch f32 scalars and tensors, one operation per rounding."""
        f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
        u, c, seen = (int(v) for v in self._rec[:3])
        applied = True
        if self.scaler is not None:
            now = int(self.scaler.applied_steps)
            applied, seen = now != seen, now
        w = f32(0.0)
        if applied:
            c += 1
            if c % self.every == 0:
                if self.mode == 'mean':
                    w = f32(1.0) / f32(u + 1)
                else:
                    d = f32(self.decay)
                    if self.warmup:
                        d = torch.minimum(d, f32(1 + u) / f32(10 + u))
                    w = f32(1.0) - d
                u += 1
        self._rec[0], self._rec[1], self._rec[2] = u, c, seen
        self._rec.view(torch.float32)[3] = w
        w = float(w)
        if w == 1.0:
            self.avg.copy_(self.arena.param)
        elif w != 0.0:
            self.avg.add_((self.arena.param - self.avg).mul_(w))

    # -- evaluation under the average -----------------------------------------------------------------------------------
    @torch.no_grad()
    def swap(self):
        """Exchange ``arena.param`` and ``avg`` (and rewrite the 16-bit shadow); flips ``is_applied``."""
        ar = self.arena
        if ar.device.type != 'cuda':
            live = ar.param.clone()
            ar.param.copy_(self.avg)
            self.avg.copy_(live)
            ar.refresh_shadow()
        elif ar.numel:
            lib = _lib.load()
            with ops.TIMER.span('k_average_swap'):
                check(lib.mbv_weight_average_swap(ar.param.data_ptr(), self.avg.data_ptr(),
                                                  0 if ar.shadow is None else ar.shadow.data_ptr(), ar.shadow_flag, ar.numel,
                                                  torch.cuda.current_stream(ar.device).cuda_stream),
                      'mbv_weight_average_swap')
            ops.note_parameters_changed()
        self.is_applied = not self.is_applied

    @contextlib.contextmanager
    def applied(self):
        """``with average.applied():`` — the module computes with the averaged weights inside, with the live ones after, also
        when the body raises."""
        self._refuse_applied('applied()')
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # -- checkpoint -----------------------------------------------------------------------------------------------------
    def state_dict(self):
        self._refuse_applied('state_dict()')
        u, c, seen = (int(v) for v in self._rec[:3].tolist())
        return dict(kind=self.KIND, avg=self.avg, updates=u, calls=c, seen=seen, mode=self.mode, decay=self.decay,
                    warmup=self.warmup, every=self.every)

    @torch.no_grad()
    def load_state_dict(self, sd):
        self._refuse_applied('load_state_dict()')
        if sd.get('kind') != self.KIND:
            raise ValueError(f"state of kind {sd.get('kind')!r} cannot be loaded into {type(self).__name__}")
        if tuple(sd['avg'].shape) != tuple(self.avg.shape):
            raise ValueError(f"averaged weights of {tuple(sd['avg'].shape)} elements, the arena has {tuple(self.avg.shape)}")
        self._set_hyper(sd.get('mode', self.mode), sd.get('decay', self.decay), sd.get('warmup', self.warmup),
                        sd.get('every', self.every))
        self.avg.copy_(sd['avg'])
        self._rec.copy_(torch.tensor([int(sd['updates']), int(sd['calls']), int(sd['seen']), 0], dtype=torch.int32))
