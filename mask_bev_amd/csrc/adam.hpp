// Optimizer arithmetic.  AdamW: shared by K11's optimizer pass (optim_flat.hip) and K3's backward with the update of the (C, ny, nx)
// LayerNorm affine fused into it (scatter_layernorm.hip): ONE definition, so the two paths are bit-identical.
// Follows torch/optim/adamw.py's single-tensor update order (mask_bev/mask_bev_module.py:131-166 configures it).
#pragma once
#include "common.hpp"

struct AdamArgs {
  float lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2_sqrt, grad_scale;
  int decoupled, zero_grad;
  int shadow_kind;                 // MBV_DT_BF16 / MBV_DT_F16: storage of the weight shadow
  const float* loss_scale;         // device scalar (nullable): gradients arrive multiplied by it (fp16 loss scaling)
  const int* skip;                 // device flag (nullable): non-zero = the gradient held inf / nan, skip the update
  const int* applied;              // device count of updates APPLIED so far (nullable): the bias corrections then use
                                   //   t = *applied + 1 — torch.amp.GradScaler skips optimizer.step() on an overflow, so
                                   //   Adam's step count must not advance there (a host count would)
};

// The hyper-parameters of one parameter group in DEVICE memory (= mbv_adam_dev, maskbev_hip.h): what an update that is
// captured in a graph reads at replay time — the learning rate and the bias corrections change from step to step, kernel
// arguments do not.  Written by mbv_adam_args_write (optim_flat.hip), read by K17's grouped weight-gradient epilogue.
struct AdamDev {
  float lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2_sqrt;
  int decoupled, shadow_kind;
  int pad[7];
};
static_assert(sizeof(AdamDev) == 64, "one block per 64 bytes");

__device__ __forceinline__ AdamArgs adam_args_from(const AdamDev& d) {
  AdamArgs a;
  a.lr = d.lr; a.beta1 = d.beta1; a.beta2 = d.beta2; a.eps = d.eps; a.weight_decay = d.weight_decay;
  a.bias_correction1 = d.bias_correction1; a.bias_correction2_sqrt = d.bias_correction2_sqrt;
  a.grad_scale = 1.0f; a.decoupled = d.decoupled; a.zero_grad = 0; a.shadow_kind = d.shadow_kind;
  a.loss_scale = nullptr; a.skip = nullptr; a.applied = nullptr;
  return a;
}

__device__ __forceinline__ unsigned short shadow_bits(float p, int kind) {
  return kind == MBV_DT_F16 ? __builtin_bit_cast(unsigned short, (_Float16)p) : f32_to_bf16_rne(p);
}

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a) {
  // contraction pinned OFF here, not by a unit's build flags: the update must not depend on which unit runs it or how that
  // unit is built; unfused multiply / add is also what torch's single-tensor AdamW computes
#pragma clang fp contract(off)
  g *= a.grad_scale;
  if (a.decoupled) {
    p *= 1.0f - a.lr * a.weight_decay;            // param.mul_(1 - lr * wd)
  } else if (a.weight_decay != 0.0f) {
    g += a.weight_decay * p;                      // Adam: L2 term folded into the gradient
  }
  m += (g - m) * (1.0f - a.beta1);                // exp_avg.lerp_(grad, 1 - beta1)
  v = v * a.beta2 + (1.0f - a.beta2) * g * g;     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  const float denom = sqrtf(v) / a.bias_correction2_sqrt + a.eps;
  p -= (a.lr / a.bias_correction1) * (m / denom);
}

// ---- K40: LAMB and (Nesterov) SGD over the arena (optim_flat.hip) ------------------------------------------------------
// LAMB as torch_optimizer 0.3.0's Lamb.step states it, cut where the per-tensor norms are needed: the moments pass leaves
// u = m / (sqrt(v) + eps) + wd * p, the apply pass takes p -= (step_size * trust) * u.  Contraction pinned off as above.
struct LambArgs {
  // 1 - beta is taken in f64 from the f64 betas of the entry point and rounded once, as torch rounds the Python scalar:
  // 1.0f - 0.999f is 0.99998713e-3, 1.3e-5 away from the 0.001 the rule means
  float beta1, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay, grad_scale;
  const float* loss_scale;         // as AdamArgs
  const int* skip;
};

__device__ __forceinline__ float lamb_moments_one(float p, float g, float& m, float& v, const LambArgs& a) {
#pragma clang fp contract(off)
  g *= a.grad_scale;
  m = m * a.beta1 + a.one_minus_beta1 * g;        // exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
  v = v * a.beta2 + a.one_minus_beta2 * g * g;    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  float u = m / (sqrtf(v) + a.eps);               // exp_avg / exp_avg_sq.sqrt().add(eps)
  if (a.weight_decay != 0.0f) u += a.weight_decay * p;
  return u;
}

__device__ __forceinline__ float lamb_apply_one(float p, float u, float scaled_step) {
#pragma clang fp contract(off)
  return p - scaled_step * u;                     // p.add_(adam_step, alpha=-step_size * trust_ratio)
}

// torch/optim/sgd.py's single-tensor order; the momentum buffer starts at zero, which gives torch's first-step `buf = grad`
// exactly when dampening is 0 (momentum * 0 + grad == grad)
struct SgdArgs {
  float lr, momentum, one_minus_dampening, weight_decay, grad_scale;
  int nesterov, zero_grad, shadow_kind;
  const float* loss_scale;
  const int* skip;
};

__device__ __forceinline__ void sgd_one(float& p, float g, float& buf, const SgdArgs& a) {
#pragma clang fp contract(off)
  g *= a.grad_scale;
  if (a.weight_decay != 0.0f) g += a.weight_decay * p;      // grad.add(param, alpha=weight_decay)
  buf = buf * a.momentum + a.one_minus_dampening * g;       // buf.mul_(momentum).add_(grad, alpha=1 - dampening)
  g = a.nesterov ? g + a.momentum * buf : buf;              // grad.add(buf, alpha=momentum) / grad = buf
  p -= a.lr * g;                                            // param.add_(grad, alpha=-lr)
}

// ---- K43: weight averaging over the arena (optim_flat.hip) ---------------------------------------------------------------
// The device record of a WeightAverage (= mbv_weight_average_state, maskbev_hip.h): the counters a captured update advances
// itself, and the blend weight its tick leaves for the streaming pass that follows it on the stream.
struct AverageRec {
  int updates;                     // u: averaging updates applied so far
  int calls;                       // c: applied optimizer steps seen
  int seen;                        // the LossScaler's applied_steps at the last call
  float weight;                    // w of this call; 0 = nothing to do
};
static_assert(sizeof(AverageRec) == 16, "the record is four words");

// avg.lerp_(p, w) written out: three roundings, and w == 1 takes p itself (avg + (p - avg) need not be p)
__device__ __forceinline__ float average_one(float avg, float p, float w) {
#pragma clang fp contract(off)
  if (w == 1.0f) return p;
  const float d = p - avg;
  return avg + w * d;
}
