// The frame the flat-arena streaming kernels of optim_flat.hip share (k_adamw, k_sgd, k_lamb_*, k_grad_nonfinite): 16-byte
// vector types, the four-lane shadow store, the gradient clear of an overflowed step, and the host-side alignment test and
// grid size.  The update rules themselves are in adam.hpp; the per-element loops stay written out in each kernel.
#pragma once
#include "adam.hpp"

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned short us4 __attribute__((ext_vector_type(4)));

constexpr int kMaxBlocks = 256 * 16;    // 16 blocks per CU, grid-stride beyond

// 16-bit shadow of four updated parameters, vector index i (read again by the next forward: a normal store)
__device__ __forceinline__ void store_shadow4(unsigned short* __restrict__ shadow, long i, f4 p, int kind) {
  us4 s;
  s.x = shadow_bits(p.x, kind); s.y = shadow_bits(p.y, kind);
  s.z = shadow_bits(p.z, kind); s.w = shadow_bits(p.w, kind);
  reinterpret_cast<us4*>(shadow)[i] = s;
}

// grad[0, n) = 0 by the whole grid, ragged tail (< 4 elements) included: all an overflowed step does
__device__ __forceinline__ void clear_grad(float* __restrict__ grad, long n) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long i = first; i < n4; i += stride) __builtin_nontemporal_store(f4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f4*>(grad) + i);
  const long t = (n4 << 2) + first;
  if (t < n) grad[t] = 0.f;
}

static inline bool misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return ((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b) | reinterpret_cast<size_t>(c) |
           reinterpret_cast<size_t>(d)) & 15) != 0;
}

// blocks of 256 threads for n4 items of one thread-iteration each: capped at `cap` (kMaxBlocks unless a kernel has measured
// another), at least one (the ragged tail)
static inline unsigned stream_blocks(long n4, long cap = kMaxBlocks) {
  long blocks = (n4 + 255) / 256;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}
