// The counter hash of the device-side random draws (K10's point sampling, K23's augmentations).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

// PCG output function on a 32-bit state (Jarzynski & Olano, "Hash Functions for GPU Rendering", JCGT 2020)
__host__ __device__ __forceinline__ uint32_t pcg_hash(uint32_t v) {
  const uint32_t s = v * 747796405u + 2891336453u;
  const uint32_t w = ((s >> ((s >> 28u) + 4u)) ^ s) * 277803737u;
  return (w >> 22u) ^ w;
}
