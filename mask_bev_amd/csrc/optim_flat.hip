// K11 / K40 — the optimizer passes over the flat parameter arena (HBM-bound, no MFMA).
//
//   mbv_adamw_step      one pass of Adam / AdamW: reads param, grad, exp_avg, exp_avg_sq (16 B/elem), writes param, exp_avg,
//                       exp_avg_sq (12 B/elem), optionally the 16-bit shadow the GEMMs read (2 B/elem) and the zeroed gradient
//                       (4 B/elem).
//   mbv_refresh_shadow  f32 -> 16-bit shadow of an arena; mbv_grad_nonfinite / mbv_loss_scale_update: fp16 loss scaling.
//   mbv_lamb_moments    reads param, grad, exp_avg, exp_avg_sq (16 B/elem), writes exp_avg, exp_avg_sq and the un-scaled update
//                       u over grad (12 B/elem); per chunk the block-reduced sums of p^2 and u^2 go to a partial slab.
//   mbv_lamb_trust      per parameter: the partials summed in a fixed order in f64 -> trust ratio (f32).
//   mbv_lamb_apply      reads param, u (8 B/elem), writes param, the 16-bit shadow and the zeroed gradient (10 B/elem).
//   mbv_sgd_step        one pass: reads param, grad, momentum buffer (12 B), writes param, buffer, shadow, zeroed grad (14 B).
//
//   mbv_grad_norm_partials   K41: reads grad (4 B/elem); per chunk the block-reduced f64 sum of g^2 goes to a partial slab (8 B).
//   mbv_grad_clip_coef       K41: the partials summed in a fixed order in f64 -> a 16-float record: the divisor
//                            loss_scale / clip_coefficient the passes above take in place of the loss scale, the total norm,
//                            the coefficient and the norm of every range.  The gradient itself is never rewritten.
//
//   mbv_weight_average_update   K43: two launches.  One thread decides from a 16-byte device record whether this call blends
//                               and with what weight (EMA with optional decay warm-up, or the equal-weight running mean; an
//                               overflowed fp16 step, read off K11's applied-step count, and the steps between `every` do
//                               not); then one pass reads param and avg (8 B/elem) and writes avg (4 B/elem), or returns at
//                               once on weight 0.  param, grad and the shadow are not touched.
//   mbv_weight_average_swap     K43: param <-> avg in one pass (16 B/elem) that also rewrites the shadow (2 B/elem).
//
// A LAMB step is 28 + 18 = 46 B/elem against k_adamw's 34; SGD is 26; clipping adds 4; averaging adds 12.  The per-tensor norms of LAMB come from a CHUNK TABLE
// built once by the host: every parameter's padded arena range is cut into chunks of kChunk = 4096 elements (a chunk never
// straddles two parameters; the last chunk of a parameter is shorter, a multiple of 64).  One block works on one chunk at a
// time, so a chunk's two sums are taken in one fixed order whatever the grid — no float atomics, bit-reproducible, replayable.
//
// The unit is built with -ffp-contract=off (K40's updates are compared with per-tensor torch restatements).  That flag
// cannot change a bit of k_adamw, which used to be built with hipcc's default: its float multiply-adds all sit inside
// adam_one, which pins contraction off itself, and what remains in the kernel is one division and f64 pow / sqrt.
//
// Reference: torch.optim.AdamW / Adam (single-tensor update order of torch/optim/adamw.py), torch_optimizer 0.3.0 Lamb.step
// and torch/optim/sgd.py `_single_tensor_sgd`, as configured at mask_bev/mask_bev_module.py:131-166; the arithmetic itself is
// in adam.hpp, the frame the streaming kernels share in arena_stream.hpp.
#include "common.hpp"
#include "arena_stream.hpp"

namespace {

// 4 elements per thread per iteration (float4 loads: 16 B/lane, fully coalesced), grid-stride.
__global__ void __launch_bounds__(256) k_adamw(float* __restrict__ param, float* __restrict__ grad,
                                               float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                               unsigned short* __restrict__ shadow, long n, AdamArgs a) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  if (a.loss_scale) a.grad_scale /= *a.loss_scale;
  if (a.skip && *a.skip) {         // overflowed step: parameters, moments and the shadow stay; the gradient is dropped
    if (a.zero_grad) clear_grad(grad, n);
    return;
  }
  if (a.applied) {                 // bias corrections from the device-side count of applied updates
    const double t = (double)(*a.applied + 1);
    a.bias_correction1 = (float)(1.0 - pow((double)a.beta1, t));
    a.bias_correction2_sqrt = (float)sqrt(1.0 - pow((double)a.beta2, t));
  }
  // Streaming accesses: every array is read once and written once per step and is far larger than the caches (6.8 GB at the
  // bench size), so loads and stores carry the non-temporal hint — 1.33 -> 1.25 ms measured; a second row per thread in
  // flight was slower (1.37 ms).
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f4 p = __builtin_nontemporal_load(reinterpret_cast<const f4*>(param) + i);
    const f4 g = __builtin_nontemporal_load(reinterpret_cast<const f4*>(grad) + i);
    f4 m = __builtin_nontemporal_load(reinterpret_cast<const f4*>(exp_avg) + i);
    f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(exp_avg_sq) + i);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float pc = p[c], mc = m[c], vc = v[c];
      adam_one(pc, g[c], mc, vc, a);
      p[c] = pc; m[c] = mc; v[c] = vc;
    }
    __builtin_nontemporal_store(p, reinterpret_cast<f4*>(param) + i);
    __builtin_nontemporal_store(m, reinterpret_cast<f4*>(exp_avg) + i);
    __builtin_nontemporal_store(v, reinterpret_cast<f4*>(exp_avg_sq) + i);
    if (shadow) store_shadow4(shadow, i, p, a.shadow_kind);
    if (a.zero_grad) __builtin_nontemporal_store(f4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f4*>(grad) + i);
  }
  // ragged tail (< 4 elements)
  const long t = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    float p = param[t], m = exp_avg[t], v = exp_avg_sq[t];
    adam_one(p, grad[t], m, v, a);
    param[t] = p; exp_avg[t] = m; exp_avg_sq[t] = v;
    if (shadow) shadow[t] = shadow_bits(p, a.shadow_kind);
    if (a.zero_grad) grad[t] = 0.f;
  }
}

// k_adamw over up to kAdamRanges SHORT element ranges of the arena in one launch: what is left of a segment between the
// weights that took their update elsewhere (K3's backward, K17's grouped weight gradient) is dozens of ranges of a few hundred
// to a few hundred thousand elements — biases, LayerNorm affines, position tables — and one launch each is 3 us of kernel
// behind 8 us of launch.  Block b works on chunk (b - block_begin[i]) of range i, kRangeChunk4 float4 items; starts and
// lengths are multiples of 4 elements (arena parameters start on 64-element boundaries), so there is no ragged tail.
constexpr int kAdamRanges = 64;
constexpr int kRangeChunk4 = 1024;      // float4 items per block: 4 per thread
struct AdamRanges {
  long start4[kAdamRanges];             // first float4 item
  int len4[kAdamRanges];                // float4 items
  int block_begin[kAdamRanges];
  int n;
};

__global__ void __launch_bounds__(256) k_adamw_ranges(float* __restrict__ param, float* __restrict__ grad,
                                                      float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                      unsigned short* __restrict__ shadow, const AdamRanges r, AdamArgs a) {
  int i = 0;
  while (i + 1 < r.n && (int)blockIdx.x >= r.block_begin[i + 1]) ++i;       // block-uniform
  const long base = r.start4[i];
  const int c0 = ((int)blockIdx.x - r.block_begin[i]) * kRangeChunk4;
  const int c1 = c0 + kRangeChunk4 < r.len4[i] ? c0 + kRangeChunk4 : r.len4[i];
  if (a.loss_scale) a.grad_scale /= *a.loss_scale;
  if (a.skip && *a.skip) {         // overflowed step, as k_adamw: only the gradient clear is honoured
    if (a.zero_grad)
      for (int j = c0 + threadIdx.x; j < c1; j += 256)
        __builtin_nontemporal_store(f4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f4*>(grad) + base + j);
    return;
  }
  if (a.applied) {
    const double t = (double)(*a.applied + 1);
    a.bias_correction1 = (float)(1.0 - pow((double)a.beta1, t));
    a.bias_correction2_sqrt = (float)sqrt(1.0 - pow((double)a.beta2, t));
  }
  for (int j = c0 + threadIdx.x; j < c1; j += 256) {
    const long idx = base + j;
    f4 p = __builtin_nontemporal_load(reinterpret_cast<const f4*>(param) + idx);
    const f4 g = __builtin_nontemporal_load(reinterpret_cast<const f4*>(grad) + idx);
    f4 m = __builtin_nontemporal_load(reinterpret_cast<const f4*>(exp_avg) + idx);
    f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(exp_avg_sq) + idx);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float pc = p[c], mc = m[c], vc = v[c];
      adam_one(pc, g[c], mc, vc, a);
      p[c] = pc; m[c] = mc; v[c] = vc;
    }
    __builtin_nontemporal_store(p, reinterpret_cast<f4*>(param) + idx);
    __builtin_nontemporal_store(m, reinterpret_cast<f4*>(exp_avg) + idx);
    __builtin_nontemporal_store(v, reinterpret_cast<f4*>(exp_avg_sq) + idx);
    if (shadow) store_shadow4(shadow, idx, p, a.shadow_kind);
    if (a.zero_grad) __builtin_nontemporal_store(f4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f4*>(grad) + idx);
  }
}

// f32 -> 16-bit shadow refresh of an arena (after load_state_dict / parameter broadcast).
__global__ void __launch_bounds__(256) k_shadow(const float* __restrict__ param, unsigned short* __restrict__ shadow,
                                                long n, int kind) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) shadow[i] = shadow_bits(param[i], kind);
}

// ---- fp16 loss scaling, all on the device (no host synchronisation, replayable) ---------------------------------
// flag |= "some gradient element is inf or nan" (what torch.amp.GradScaler's unscale_ reports as found_inf)
__global__ void __launch_bounds__(256) k_grad_nonfinite(const float* __restrict__ grad, long n, int* __restrict__ flag) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const uint4 u = reinterpret_cast<const uint4*>(grad)[i];
    bad |= ((u.x & 0x7f800000u) == 0x7f800000u) | ((u.y & 0x7f800000u) == 0x7f800000u) |
           ((u.z & 0x7f800000u) == 0x7f800000u) | ((u.w & 0x7f800000u) == 0x7f800000u);
  }
  const long t = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) bad |= (__float_as_uint(grad[t]) & 0x7f800000u) == 0x7f800000u;
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// GradScaler.update(): overflow -> scale *= backoff, streak = 0; else streak += 1 and every `interval` clean steps
// scale *= growth.  Clears the flag for the next step.
__global__ void k_loss_scale_update(float* __restrict__ scale, int* __restrict__ streak, int* __restrict__ flag,
                                    float growth, float backoff, int interval, int* __restrict__ applied) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (*flag) {
    *scale = fmaxf(*scale * backoff, 1.f);
    *streak = 0;
  } else {
    if (applied) ++*applied;       // this step's update was applied: Adam's step count advances
    if (++*streak >= interval) {
      const float s = *scale * growth;
      if (s <= 3.0e38f && s == s) *scale = s;
      *streak = 0;
    }
  }
  *flag = 0;
}

// ---- K40: LAMB --------------------------------------------------------------------------------------------------------
constexpr int kChunk = 4096;            // elements per chunk: 4 float4 per lane of a 256-thread block

struct ChunkRec {                       // = mbv_lamb_chunk (maskbev_hip.h)
  long start;                           // first arena element, a multiple of 4
  int len;                              // elements, a multiple of 4, 0 < len <= kChunk
  int param;                            // index of the parameter the chunk belongs to
};
static_assert(sizeof(ChunkRec) == 16, "chunk records are 16 bytes");

// a record that would reach outside the arena (a corrupted table) is skipped, never followed
__device__ __forceinline__ bool chunk_ok(const ChunkRec& r, long n) {
  return r.start >= 0 && r.len > 0 && r.len <= kChunk && ((r.start | r.len) & 3) == 0 && r.start + r.len <= n;
}

// sums of (a, b) over the 256 threads of the block in one fixed order: xor-butterfly inside a wave, then the four waves
__device__ __forceinline__ float2 block_sum2(float a, float b, float2* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  __syncthreads();                      // the previous chunk's readers are done with lds
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = make_float2(a, b);
  __syncthreads();
  return make_float2((lds[0].x + lds[1].x) + (lds[2].x + lds[3].x), (lds[0].y + lds[1].y) + (lds[2].y + lds[3].y));
}

__global__ void __launch_bounds__(256) k_lamb_moments(const float* __restrict__ param, float* __restrict__ grad,
                                                      float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, long n,
                                                      const ChunkRec* __restrict__ chunks, int n_chunks, int c0, int c1,
                                                      float* __restrict__ partials, LambArgs a) {
  __shared__ float2 lds[4];
  if (a.skip && *a.skip) return;        // overflowed step: moments stay, grad keeps the raw gradient (the apply pass drops it)
  if (a.loss_scale) a.grad_scale /= *a.loss_scale;
  for (int c = c0 + blockIdx.x; c < c1; c += gridDim.x) {
    const ChunkRec r = chunks[c];
    float sp = 0.f, su = 0.f;
    if (chunk_ok(r, n)) {
      const long base = r.start >> 2;
      const int n4 = r.len >> 2;
      // every array is touched once per step and is far larger than the caches: non-temporal, as k_adamw
      for (int i = threadIdx.x; i < n4; i += 256) {
        const f4 p = __builtin_nontemporal_load(reinterpret_cast<const f4*>(param) + base + i);
        f4 g = __builtin_nontemporal_load(reinterpret_cast<const f4*>(grad) + base + i);
        f4 m = __builtin_nontemporal_load(reinterpret_cast<const f4*>(exp_avg) + base + i);
        f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(exp_avg_sq) + base + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float mc = m[k], vc = v[k];
          const float u = lamb_moments_one(p[k], g[k], mc, vc, a);
          m[k] = mc; v[k] = vc; g[k] = u;
          sp += p[k] * p[k];
          su += u * u;
        }
        __builtin_nontemporal_store(m, reinterpret_cast<f4*>(exp_avg) + base + i);
        __builtin_nontemporal_store(v, reinterpret_cast<f4*>(exp_avg_sq) + base + i);
        __builtin_nontemporal_store(g, reinterpret_cast<f4*>(grad) + base + i);      // u: read once more, by the apply pass
      }
    }
    const float2 s = block_sum2(sp, su, lds);
    if (threadIdx.x == 0) {
      partials[c] = s.x;
      partials[(long)n_chunks + c] = s.y;
    }
  }
}

// one block per parameter: its chunks' partials in f64, thread t takes chunks t, t + 256, ...; then a fixed tree
__global__ void __launch_bounds__(256) k_lamb_trust(const float* __restrict__ partials, int n_chunks,
                                                    const int2* __restrict__ param_chunks, float clamp_value,
                                                    float* __restrict__ trust) {
  __shared__ double lp[256], lu[256];
  const int2 range = param_chunks[blockIdx.x];
  const int cb = range.x < 0 ? 0 : range.x, ce = range.y > n_chunks ? n_chunks : range.y;
  double sp = 0.0, su = 0.0;
  for (int c = cb + threadIdx.x; c < ce; c += 256) {
    sp += (double)partials[c];
    su += (double)partials[(long)n_chunks + c];
  }
  lp[threadIdx.x] = sp; lu[threadIdx.x] = su;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) { lp[threadIdx.x] += lp[threadIdx.x + w]; lu[threadIdx.x] += lu[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double wn = fmin(sqrt(lp[0]), (double)clamp_value), un = sqrt(lu[0]);
    trust[blockIdx.x] = (wn == 0.0 || un == 0.0) ? 1.f : (float)(wn / un);
  }
}

__global__ void __launch_bounds__(256) k_lamb_apply(float* __restrict__ param, float* __restrict__ grad,
                                                    unsigned short* __restrict__ shadow, int shadow_kind, long n,
                                                    const ChunkRec* __restrict__ chunks, int c0, int c1,
                                                    const float* __restrict__ trust, int n_params, float step_size,
                                                    float lr, double beta1, double beta2, const int* __restrict__ applied,
                                                    const int* __restrict__ skip) {
  const bool skipped = skip && *skip;
  if (applied) {                        // debias from the device-side count of applied updates (as k_adamw)
    const double t = (double)(*applied + 1);
    step_size = (float)((double)lr * sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t)));
  }
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int c = c0 + blockIdx.x; c < c1; c += gridDim.x) {
    const ChunkRec r = chunks[c];
    if (!chunk_ok(r, n) || r.param < 0 || r.param >= n_params) continue;
    const long base = r.start >> 2;
    const int n4 = r.len >> 2;
    if (skipped) {                      // overflowed step: parameters and shadow stay, the gradient is dropped
      for (int i = threadIdx.x; i < n4; i += 256) __builtin_nontemporal_store(zero, reinterpret_cast<f4*>(grad) + base + i);
      continue;
    }
    const float scaled = step_size * trust[r.param];
    for (int i = threadIdx.x; i < n4; i += 256) {
      f4 p = __builtin_nontemporal_load(reinterpret_cast<const f4*>(param) + base + i);
      const f4 u = __builtin_nontemporal_load(reinterpret_cast<const f4*>(grad) + base + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] = lamb_apply_one(p[k], u[k], scaled);
      __builtin_nontemporal_store(p, reinterpret_cast<f4*>(param) + base + i);
      if (shadow) store_shadow4(shadow, base + i, p, shadow_kind);
      __builtin_nontemporal_store(zero, reinterpret_cast<f4*>(grad) + base + i);
    }
  }
}

// ---- K40: (Nesterov) SGD ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sgd(float* __restrict__ param, float* __restrict__ grad, float* __restrict__ buf,
                                             unsigned short* __restrict__ shadow, long n, SgdArgs a) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (a.loss_scale) a.grad_scale /= *a.loss_scale;
  if (a.skip && *a.skip) {              // overflowed step: parameters, buffer and shadow stay; the gradient is dropped
    if (a.zero_grad) clear_grad(grad, n);
    return;
  }
  for (long i = first; i < n4; i += stride) {
    f4 p = __builtin_nontemporal_load(reinterpret_cast<const f4*>(param) + i);
    const f4 g = __builtin_nontemporal_load(reinterpret_cast<const f4*>(grad) + i);
    f4 b = __builtin_nontemporal_load(reinterpret_cast<const f4*>(buf) + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pc = p[k], bc = b[k];
      sgd_one(pc, g[k], bc, a);
      p[k] = pc; b[k] = bc;
    }
    __builtin_nontemporal_store(p, reinterpret_cast<f4*>(param) + i);
    __builtin_nontemporal_store(b, reinterpret_cast<f4*>(buf) + i);
    if (shadow) store_shadow4(shadow, i, p, a.shadow_kind);
    if (a.zero_grad) __builtin_nontemporal_store(f4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f4*>(grad) + i);
  }
  const long t = (n4 << 2) + first;     // ragged tail (< 4 elements)
  if (t < n) {
    float p = param[t], b = buf[t];
    sgd_one(p, grad[t], b, a);
    param[t] = p; buf[t] = b;
    if (shadow) shadow[t] = shadow_bits(p, a.shadow_kind);
    if (a.zero_grad) grad[t] = 0.f;
  }
}

// ---- K41: gradient clipping by global norm ------------------------------------------------------------------------------
constexpr int kNormRanges = 8;
struct NormRanges {
  long start4[kNormRanges];             // first float4 item of the range
  long len4[kNormRanges];               // float4 items
  int chunk_begin[kNormRanges + 1];     // first chunk of the range in `partials`; [n] = all chunks
  int n;
};

// sum of a over the 256 threads of the block in f64, in block_sum2's fixed order: xor-butterfly inside a wave, then the four waves
__device__ __forceinline__ double block_sum_f64(double a, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
  __syncthreads();                      // the previous chunk's readers are done with lds
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = a;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// partials[c] = sum of (double)g * (double)g over chunk c; one block per chunk at a time, so the sum's order is the chunk's own
// whatever the grid.  The four float4 of a lane are loaded before any is used (plain loads: k_adamw reads the gradient next).
__global__ void __launch_bounds__(256) k_grad_norm_partials(const float* __restrict__ grad, const NormRanges r,
                                                            double* __restrict__ partials) {
  __shared__ double lds[4];
  const int total = r.chunk_begin[r.n];
  for (int c = blockIdx.x; c < total; c += gridDim.x) {
    int i = 0;
    while (i + 1 < r.n && c >= r.chunk_begin[i + 1]) ++i;                    // block-uniform
    const long first = (long)(c - r.chunk_begin[i]) * (kChunk / 4);         // float4 items into the range
    const long left = r.len4[i] - first;
    const int n4 = left < kChunk / 4 ? (int)left : kChunk / 4;
    const f4* src = reinterpret_cast<const f4*>(grad) + r.start4[i] + first;
    f4 g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = (int)threadIdx.x + 256 * k;
      g[k] = j < n4 ? src[j] : f4{0.f, 0.f, 0.f, 0.f};
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = (double)g[k][e];
        s += d * d;
      }
    s = block_sum_f64(s, lds);
    if (threadIdx.x == 0) partials[c] = s;
  }
}

struct ClipRanges {
  int chunk[kNormRanges + 1];           // chunk boundaries of the ranges in `partials`
  int n;
};

// partials[c0, c1) summed by the one block: thread t takes chunks t, t + 256, ..., then a fixed tree (as k_lamb_trust)
__device__ __forceinline__ double tree_sum_f64(const double* __restrict__ partials, int c0, int c1, double* lds) {
  double s = 0.0;
  for (int c = c0 + (int)threadIdx.x; c < c1; c += 256) s += partials[c];
  __syncthreads();                      // the previous sum's readers are done with lds
  lds[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
    __syncthreads();
  }
  return lds[0];
}

// rec (16 f32) = { L / coef, total norm, coef, norm of range 0 .. 7, 0 ... } with torch.nn.utils.clip_grad_norm_'s rule on the
// gradient the optimizer applies (g * grad_scale / L); every norm in f64, rounded to f32 once
__global__ void __launch_bounds__(256) k_grad_clip_coef(const double* __restrict__ partials, const ClipRanges r,
                                                        double max_norm, double grad_scale,
                                                        const float* __restrict__ loss_scale, float* __restrict__ rec) {
  __shared__ double lds[256];
  const double L = loss_scale ? (double)*loss_scale : 1.0;
  const double unit = grad_scale / L;
  double norms[kNormRanges];
#pragma unroll
  for (int i = 0; i < kNormRanges; ++i)
    norms[i] = i < r.n ? sqrt(tree_sum_f64(partials, r.chunk[i], r.chunk[i + 1], lds)) * unit : 0.0;
  const double sum = r.n > 0 ? tree_sum_f64(partials, r.chunk[0], r.chunk[r.n], lds) : 0.0;
  if (threadIdx.x != 0) return;
  const double total = sqrt(sum) * unit;
  double coef = 1.0;                    // max_norm = +inf measures and never clips: rec[0] is L bit for bit
  if (max_norm <= 1.7976931348623157e308) {
    coef = max_norm / (total + 1e-6);
    if (coef > 1.0) coef = 1.0;         // a NaN norm stays a NaN coefficient, as torch's clamp leaves it
  }
  rec[0] = (float)(L / coef);
  rec[1] = (float)total;
  rec[2] = (float)coef;
#pragma unroll
  for (int i = 0; i < kNormRanges; ++i) rec[3 + i] = (float)norms[i];
#pragma unroll
  for (int i = 3 + kNormRanges; i < 16; ++i) rec[i] = 0.f;
}

// ---- K43: EMA / running mean of the parameters -----------------------------------------------------------------------------
enum { kAverageEma = 0, kAverageMean = 1 };                // = MBV_AVERAGE_EMA / MBV_AVERAGE_MEAN

// The grid cap of K43's two streams: 256 blocks per CU, not kMaxBlocks' 16.  Measured at the bench arena (200.8 M elements,
// profiles/k43, scratch/ubench/k43_blend_grid.hip): the blend under the 4096-block cap runs 48 grid-stride trips per thread
// and reaches 4.6 - 4.7 TB/s of model bytes, 0.76 of k_sgd in the same run; the same kernel under a 65536-block cap (3 trips)
// reaches 6.3 TB/s, and with one float4 per thread 6.4.  More loads per thread in flight (2 or 4 float4 rows) and plain
// instead of non-temporal accesses changed nothing under the low cap.  The older kernels keep kMaxBlocks: their launches
// are not this change's to alter.
constexpr long kAverageMaxBlocks = 256 * 256;

// The decision of one update, by one thread, in a launch of its own: the streaming pass behind it on the stream reads the
// weight this leaves (one kernel in which a block advances the counters while others still read them would race).  With
// K11's applied-step count the step counts only if the count moved since the last call: k_loss_scale_update has cleared the
// overflow flag by now, but it does not advance the count on an overflow.
__global__ void k_average_tick(AverageRec* __restrict__ rec, const int* __restrict__ applied_steps, int mode, float decay,
                               int warmup, int every) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  AverageRec r = *rec;
  bool applied = true;
  if (applied_steps) {
    const int a = *applied_steps;
    applied = a != r.seen;
    r.seen = a;
  }
  r.weight = 0.f;
  if (applied) {
    r.calls += 1;
    if (r.calls % every == 0) {
      if (mode == kAverageMean) {
        r.weight = 1.0f / (float)(r.updates + 1);
      } else {
        float d = decay;
        if (warmup) d = fminf(decay, (float)(1 + r.updates) / (float)(10 + r.updates));
        r.weight = 1.0f - d;
      }
      r.updates += 1;
    }
  }
  *rec = r;
}

// avg = avg + w (p - avg) over n elements, k_sgd's frame; reads param and avg, writes avg (12 B/elem); w == 0 costs the launch only
__global__ void __launch_bounds__(256) k_average_blend(const float* __restrict__ param, float* __restrict__ avg, long n,
                                                       const AverageRec* __restrict__ rec) {
  const float w = rec->weight;          // uniform: one scalar load
  if (w == 0.f) return;
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long i = first; i < n4; i += stride) {
    const f4 p = __builtin_nontemporal_load(reinterpret_cast<const f4*>(param) + i);
    f4 a = __builtin_nontemporal_load(reinterpret_cast<const f4*>(avg) + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = average_one(a[k], p[k], w);
    __builtin_nontemporal_store(a, reinterpret_cast<f4*>(avg) + i);
  }
  const long t = (n4 << 2) + first;     // ragged tail (< 4 elements)
  if (t < n) avg[t] = average_one(avg[t], param[t], w);
}

// param <-> avg, and the 16-bit shadow of what param now holds: 16 B/elem (+ 2 B); bits are moved, so twice is the identity
__global__ void __launch_bounds__(256) k_average_swap(float* __restrict__ param, float* __restrict__ avg,
                                                      unsigned short* __restrict__ shadow, int shadow_kind, long n) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long i = first; i < n4; i += stride) {
    const f4 p = __builtin_nontemporal_load(reinterpret_cast<const f4*>(param) + i);
    const f4 a = __builtin_nontemporal_load(reinterpret_cast<const f4*>(avg) + i);
    __builtin_nontemporal_store(a, reinterpret_cast<f4*>(param) + i);
    __builtin_nontemporal_store(p, reinterpret_cast<f4*>(avg) + i);
    if (shadow) store_shadow4(shadow, i, a, shadow_kind);
  }
  const long t = (n4 << 2) + first;     // ragged tail (< 4 elements)
  if (t < n) {
    const float p = param[t], a = avg[t];
    param[t] = a; avg[t] = p;
    if (shadow) shadow[t] = shadow_bits(a, shadow_kind);
  }
}

// one thread fills a parameter group's hyper-parameter block (plain stores): stream-ordered in front of the launches that read it
__global__ void k_adam_args_write(AdamDev* __restrict__ dst, AdamDev v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v;
}

// Adam's bias corrections of update `step` (1-based), in f64 on the host and rounded once: the ONE place they are computed for
// kernels that take them by value (k_adamw) and for the device block (mbv_adam_args_write), so the two are equal bit for bit
inline void adam_bias_corrections(float beta1, float beta2, int64_t step, float& bc1, float& bc2_sqrt) {
  bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
}

inline unsigned chunk_grid(int c0, int c1) { return (unsigned)(c1 - c0 < kMaxBlocks ? c1 - c0 : kMaxBlocks); }

inline bool bad_shadow(const void* shadow, int32_t shadow_dtype) {       // 8-byte aligned, bf16 or fp16
  return shadow && ((reinterpret_cast<size_t>(shadow) & 7) || (shadow_dtype != MBV_DT_BF16 && shadow_dtype != MBV_DT_F16));
}

}  // namespace

extern "C" int mbv_adamw_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                              int32_t shadow_dtype, int64_t n, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int64_t step, float grad_scale, int32_t decoupled, int32_t zero_grad,
                              const float* loss_scale, const int32_t* skip_flag, const int32_t* applied_steps,
                              void* stream) {
  if (n < 0 || step < 1 || !param || !grad || !exp_avg || !exp_avg_sq) return MBV_ERR_BAD_ARG;
  if (n == 0) return MBV_OK;
  if (misaligned16(param, grad, exp_avg, exp_avg_sq) || bad_shadow(shadow_bf16, shadow_dtype)) return MBV_ERR_BAD_ARG;
  AdamArgs a;
  a.shadow_kind = shadow_dtype; a.loss_scale = loss_scale; a.skip = skip_flag; a.applied = applied_steps;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay;
  adam_bias_corrections(beta1, beta2, step, a.bias_correction1, a.bias_correction2_sqrt);
  a.grad_scale = grad_scale; a.decoupled = decoupled; a.zero_grad = zero_grad;
  hipLaunchKernelGGL(k_adamw, dim3(stream_blocks(n >> 2)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, reinterpret_cast<unsigned short*>(shadow_bf16), (long)n, a);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

// mbv_adamw_step over `count` element ranges [start[i], start[i] + len[i]) of arenas of n elements (HOST arrays; starts and
// lengths multiples of 4, ranges inside the arena), one launch per 64 ranges: for the many short ranges a step leaves between
// weights updated elsewhere.  Same arithmetic, same loss-scaling protocol.
extern "C" int mbv_adamw_step_ranges(float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                                     int32_t shadow_dtype, int64_t n, const int64_t* start, const int64_t* len, int32_t count,
                                     float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                                     float grad_scale, int32_t decoupled, int32_t zero_grad, const float* loss_scale,
                                     const int32_t* skip_flag, const int32_t* applied_steps, void* stream) {
  if (n < 0 || count < 0 || step < 1 || !param || !grad || !exp_avg || !exp_avg_sq) return MBV_ERR_BAD_ARG;
  if (count > 0 && (!start || !len)) return MBV_ERR_BAD_ARG;
  if (misaligned16(param, grad, exp_avg, exp_avg_sq) || bad_shadow(shadow_bf16, shadow_dtype)) return MBV_ERR_BAD_ARG;
  for (int i = 0; i < count; ++i)
    if (start[i] < 0 || len[i] < 0 || ((start[i] | len[i]) & 3) || start[i] + len[i] > n || len[i] > 0x7fffffffLL)
      return MBV_ERR_BAD_ARG;
  AdamArgs a;
  a.shadow_kind = shadow_dtype; a.loss_scale = loss_scale; a.skip = skip_flag; a.applied = applied_steps;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay;
  adam_bias_corrections(beta1, beta2, step, a.bias_correction1, a.bias_correction2_sqrt);
  a.grad_scale = grad_scale; a.decoupled = decoupled; a.zero_grad = zero_grad;
  for (int base = 0; base < count; base += kAdamRanges) {
    AdamRanges r;
    r.n = 0;
    long blocks = 0;
    for (int i = base; i < count && i < base + kAdamRanges; ++i) {
      if (len[i] == 0) continue;
      r.start4[r.n] = start[i] >> 2; r.len4[r.n] = (int)(len[i] >> 2); r.block_begin[r.n] = (int)blocks;
      blocks += ((len[i] >> 2) + kRangeChunk4 - 1) / kRangeChunk4;
      ++r.n;
    }
    if (r.n == 0) continue;
    if (blocks > 0x7fffffffLL) return MBV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_adamw_ranges, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, reinterpret_cast<unsigned short*>(shadow_bf16), r, a);
    MBV_CHECK_LAUNCH();
  }
  return MBV_OK;
}

// The hyper-parameters of update `step` into a 64-byte device block (mbv_adam_dev) that mbv_gemm16_tn_group_adam's fused
// entries read when they RUN: called eagerly before each replay of a graph that holds such a launch.
extern "C" int mbv_adam_args_write(void* dev_block, float lr, float beta1, float beta2, float eps, float weight_decay,
                                   int64_t step, int32_t decoupled, int32_t shadow_kind, void* stream) {
  if (!dev_block || step < 1 || (reinterpret_cast<size_t>(dev_block) & 3)) return MBV_ERR_BAD_ARG;
  if (shadow_kind != 0 && shadow_kind != MBV_DT_BF16 && shadow_kind != MBV_DT_F16) return MBV_ERR_BAD_ARG;
  AdamDev v = {};
  v.lr = lr; v.beta1 = beta1; v.beta2 = beta2; v.eps = eps; v.weight_decay = weight_decay;
  adam_bias_corrections(beta1, beta2, step, v.bias_correction1, v.bias_correction2_sqrt);
  v.decoupled = decoupled; v.shadow_kind = shadow_kind;
  hipLaunchKernelGGL(k_adam_args_write, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<AdamDev*>(dev_block), v);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_grad_nonfinite(const float* grad, int64_t n, int32_t* flag, void* stream) {
  if (n < 0 || !grad || !flag || misaligned16(grad)) return MBV_ERR_BAD_ARG;
  if (n == 0) return MBV_OK;
  hipLaunchKernelGGL(k_grad_nonfinite, dim3(stream_blocks(n >> 2)), dim3(256), 0, (hipStream_t)stream, grad, (long)n, flag);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_loss_scale_update(float* loss_scale, int32_t* clean_steps, int32_t* flag, float growth, float backoff,
                                     int32_t growth_interval, int32_t* applied_steps, void* stream) {
  if (!loss_scale || !clean_steps || !flag || growth < 1.f || backoff <= 0.f || backoff > 1.f || growth_interval < 1)
    return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_loss_scale_update, dim3(1), dim3(64), 0, (hipStream_t)stream, loss_scale, clean_steps, flag,
                     growth, backoff, growth_interval, applied_steps);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_refresh_shadow(const float* param, void* shadow_bf16, int32_t shadow_dtype, int64_t n, void* stream) {
  if (n < 0 || !param || !shadow_bf16) return MBV_ERR_BAD_ARG;
  if (shadow_dtype != MBV_DT_BF16 && shadow_dtype != MBV_DT_F16) return MBV_ERR_BAD_ARG;
  if (n == 0) return MBV_OK;
  hipLaunchKernelGGL(k_shadow, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, param,
                     reinterpret_cast<unsigned short*>(shadow_bf16), (long)n, shadow_dtype);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_lamb_moments(const float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                const mbv_lamb_chunk* chunks, int32_t n_chunks, int32_t c0, int32_t c1, float* partials,
                                double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                                const float* loss_scale, const int32_t* skip_flag, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !chunks || !partials || n < 0 || n_chunks < 0) return MBV_ERR_BAD_ARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return MBV_ERR_BAD_ARG;
  if (c0 < 0 || c1 < c0 || c1 > n_chunks) return MBV_ERR_BAD_ARG;
  if (misaligned16(param, grad, exp_avg, exp_avg_sq) || misaligned16(chunks) || (reinterpret_cast<size_t>(partials) & 3))
    return MBV_ERR_BAD_ARG;
  if (c1 == c0) return MBV_OK;
  LambArgs a;
  a.beta1 = (float)beta1; a.beta2 = (float)beta2;
  a.one_minus_beta1 = (float)(1.0 - beta1); a.one_minus_beta2 = (float)(1.0 - beta2); a.eps = eps; a.weight_decay = weight_decay; a.grad_scale = grad_scale;
  a.loss_scale = loss_scale; a.skip = skip_flag;
  hipLaunchKernelGGL(k_lamb_moments, dim3(chunk_grid(c0, c1)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, (long)n, reinterpret_cast<const ChunkRec*>(chunks), n_chunks, c0, c1, partials, a);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_lamb_trust(const float* partials, int32_t n_chunks, const int32_t* param_chunks, int32_t n_params,
                              float clamp_value, float* trust, void* stream) {
  if (!partials || !param_chunks || !trust || n_chunks < 0 || n_params < 0) return MBV_ERR_BAD_ARG;
  if ((reinterpret_cast<size_t>(partials) & 3) || (reinterpret_cast<size_t>(param_chunks) & 7) ||
      (reinterpret_cast<size_t>(trust) & 3))
    return MBV_ERR_BAD_ARG;
  if (n_params == 0) return MBV_OK;
  hipLaunchKernelGGL(k_lamb_trust, dim3((unsigned)n_params), dim3(256), 0, (hipStream_t)stream, partials, n_chunks,
                     reinterpret_cast<const int2*>(param_chunks), clamp_value, trust);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_lamb_apply(float* param, float* grad, void* shadow, int32_t shadow_dtype, int64_t n,
                              const mbv_lamb_chunk* chunks, int32_t n_chunks, int32_t c0, int32_t c1, const float* trust,
                              int32_t n_params, float lr, double beta1, double beta2, int32_t debias, int64_t step,
                              const int32_t* applied_steps, const int32_t* skip_flag, void* stream) {
  if (!param || !grad || !chunks || !trust || n < 0 || n_chunks < 0 || n_params < 0 || step < 1) return MBV_ERR_BAD_ARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return MBV_ERR_BAD_ARG;
  if (c0 < 0 || c1 < c0 || c1 > n_chunks) return MBV_ERR_BAD_ARG;
  if (misaligned16(param, grad, chunks) || (reinterpret_cast<size_t>(trust) & 3)) return MBV_ERR_BAD_ARG;
  if (bad_shadow(shadow, shadow_dtype)) return MBV_ERR_BAD_ARG;
  if (c1 == c0) return MBV_OK;
  float step_size = lr;
  if (debias)
    step_size = (float)((double)lr * sqrt(1.0 - pow(beta2, (double)step)) / (1.0 - pow(beta1, (double)step)));
  hipLaunchKernelGGL(k_lamb_apply, dim3(chunk_grid(c0, c1)), dim3(256), 0, (hipStream_t)stream, param, grad,
                     reinterpret_cast<unsigned short*>(shadow), shadow_dtype, (long)n,
                     reinterpret_cast<const ChunkRec*>(chunks), c0, c1, trust, n_params, step_size, lr, beta1, beta2,
                     debias ? applied_steps : nullptr, skip_flag);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

// K41: per-chunk sums of squares of `count` <= 8 element ranges of the gradient (HOST arrays, as mbv_adamw_step_ranges)
extern "C" int mbv_grad_norm_partials(const float* grad, int64_t n, const int64_t* start, const int64_t* len, int32_t count,
                                      double* partials, int32_t n_partials, void* stream) {
  if (n < 0 || count < 0 || n_partials < 0 || !grad || misaligned16(grad)) return MBV_ERR_BAD_ARG;
  if (count > kNormRanges) return MBV_ERR_UNSUPPORTED;
  if (count > 0 && (!start || !len)) return MBV_ERR_BAD_ARG;
  NormRanges r;
  r.n = 0;
  long chunks = 0;
  for (int i = 0; i < count; ++i) {
    if (start[i] < 0 || len[i] < 0 || ((start[i] | len[i]) & 3) || start[i] > n || len[i] > n - start[i]) return MBV_ERR_BAD_ARG;
    if (len[i] == 0) continue;
    r.start4[r.n] = start[i] >> 2; r.len4[r.n] = len[i] >> 2; r.chunk_begin[r.n] = (int)chunks;
    chunks += (len[i] + kChunk - 1) / kChunk;
    if (chunks > 0x7fffffffLL) return MBV_ERR_UNSUPPORTED;
    ++r.n;
  }
  r.chunk_begin[r.n] = (int)chunks;
  if (chunks != n_partials) return MBV_ERR_BAD_ARG;
  if (chunks == 0) return MBV_OK;
  if (!partials || (reinterpret_cast<size_t>(partials) & 7)) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_grad_norm_partials, dim3(chunk_grid(0, (int)chunks)), dim3(256), 0, (hipStream_t)stream, grad, r,
                     partials);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

// K41: the partials of mbv_grad_norm_partials -> the 16-float record the optimizer kernels take in place of the loss scale
extern "C" int mbv_grad_clip_coef(const double* partials, int32_t n_partials, const int32_t* range_chunks, int32_t count,
                                  float max_norm, float grad_scale, const float* loss_scale, float* rec, void* stream) {
  if (n_partials < 0 || count < 0 || !rec || (reinterpret_cast<size_t>(rec) & 3)) return MBV_ERR_BAD_ARG;
  if (!(max_norm > 0.f)) return MBV_ERR_BAD_ARG;                             // <= 0 or NaN
  if (count > kNormRanges) return MBV_ERR_UNSUPPORTED;
  if (loss_scale && (reinterpret_cast<size_t>(loss_scale) & 3)) return MBV_ERR_BAD_ARG;
  ClipRanges r = {};
  if (count > 0) {
    if (!range_chunks || range_chunks[0] != 0 || range_chunks[count] != n_partials) return MBV_ERR_BAD_ARG;
    for (int i = 0; i < count; ++i)
      if (range_chunks[i + 1] < range_chunks[i]) return MBV_ERR_BAD_ARG;
    for (int i = 0; i <= count; ++i) r.chunk[i] = range_chunks[i];
    r.n = count;
  }
  if (r.n > 0 && n_partials > 0 && (!partials || (reinterpret_cast<size_t>(partials) & 7))) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_grad_clip_coef, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, r, (double)max_norm,
                     (double)grad_scale, loss_scale, rec);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

// K43: one averaging update = the tick and the streaming pass, in that order on the stream
extern "C" int mbv_weight_average_update(const float* param, float* avg, int64_t n, mbv_weight_average_state* state,
                                         const int32_t* applied_steps, int32_t mode, float decay, int32_t warmup,
                                         int32_t every, void* stream) {
  if (n < 0 || !param || !avg || !state || param == avg) return MBV_ERR_BAD_ARG;
  if (mode != kAverageEma && mode != kAverageMean) return MBV_ERR_BAD_ARG;
  if (!(decay >= 0.f && decay < 1.f) || every < 1) return MBV_ERR_BAD_ARG;                 // NaN included
  if ((reinterpret_cast<size_t>(state) & 3) || (reinterpret_cast<size_t>(applied_steps) & 3)) return MBV_ERR_BAD_ARG;
  if (n == 0) return MBV_OK;
  if (misaligned16(param, avg)) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_average_tick, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<AverageRec*>(state),
                     applied_steps, mode, decay, warmup, every);
  MBV_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_average_blend, dim3(stream_blocks(n >> 2, kAverageMaxBlocks)), dim3(256), 0, (hipStream_t)stream, param, avg, (long)n,
                     reinterpret_cast<const AverageRec*>(state));
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_weight_average_swap(float* param, float* avg, void* shadow, int32_t shadow_dtype, int64_t n,
                                       void* stream) {
  if (n < 0 || !param || !avg || param == avg) return MBV_ERR_BAD_ARG;
  if (n == 0) return MBV_OK;
  if (misaligned16(param, avg) || bad_shadow(shadow, shadow_dtype)) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_average_swap, dim3(stream_blocks(n >> 2, kAverageMaxBlocks)), dim3(256), 0, (hipStream_t)stream, param, avg,
                     reinterpret_cast<unsigned short*>(shadow), shadow_dtype, (long)n);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_sgd_step(float* param, float* grad, float* momentum_buf, void* shadow, int32_t shadow_dtype, int64_t n,
                            float lr, float momentum, float dampening, float weight_decay, int32_t nesterov,
                            float grad_scale, int32_t zero_grad, const float* loss_scale, const int32_t* skip_flag,
                            void* stream) {
  if (n < 0 || !param || !grad || !momentum_buf) return MBV_ERR_BAD_ARG;
  if (n == 0) return MBV_OK;
  if (misaligned16(param, grad, momentum_buf) || bad_shadow(shadow, shadow_dtype)) return MBV_ERR_BAD_ARG;
  SgdArgs a;
  a.lr = lr; a.momentum = momentum; a.one_minus_dampening = 1.0f - dampening; a.weight_decay = weight_decay;
  a.grad_scale = grad_scale; a.nesterov = nesterov; a.zero_grad = zero_grad; a.shadow_kind = shadow_dtype;
  a.loss_scale = loss_scale; a.skip = skip_flag;
  hipLaunchKernelGGL(k_sgd, dim3(stream_blocks(n >> 2)), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf,
                     reinterpret_cast<unsigned short*>(shadow), (long)n, a);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
