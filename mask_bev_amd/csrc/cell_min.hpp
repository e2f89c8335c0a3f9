// The lowest return of every BEV cell on K31's order-preserving u32 encoding of an f32: the one copy of that pass, launched
// by K35a (point_lift.hip) and K38a (visibility.hip).  A file that includes this must be compiled with -ffp-contract=off
// (point_cell.hpp).
#pragma once
#include "common.hpp"
#include "point_cell.hpp"

namespace {

constexpr int kCellMinThreads = 256;
constexpr uint32_t kEncInf = 0xff800000u;                       // encode_ordered(+inf)

// f32 → u32 with the order of the floats (negative numbers: all bits flipped; others: the sign bit set) and back
__device__ __forceinline__ uint32_t encode_ordered(float z) {
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float decode_ordered(uint32_t e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

__global__ void __launch_bounds__(kCellMinThreads) k_ground_init(int64_t cells, uint32_t* __restrict__ enc) {
  const int64_t stride = (int64_t)gridDim.x * kCellMinThreads;
  for (int64_t i = (int64_t)blockIdx.x * kCellMinThreads + threadIdx.x; i < cells; i += stride) enc[i] = kEncInf;
}

// one thread per point (blocks of 256, grid.y = scan): the cell's minimum takes the point's z when the point takes part
__global__ void __launch_bounds__(kCellMinThreads) k_ground_points(const float* __restrict__ points, int dim,
                                                                   int64_t total_points,
                                                                   const int32_t* __restrict__ scan_offsets, LiftGeom g,
                                                                   int prefilter, float z_floor, uint32_t* __restrict__ enc) {
  const int b = blockIdx.y;
  int64_t begin = scan_offsets[b], end = scan_offsets[b + 1];
  begin = begin < 0 ? 0 : begin;                                   // offsets that point outside the table read nothing
  end = end > total_points ? total_points : end;
  const int64_t i = begin + (int64_t)blockIdx.x * kCellMinThreads + threadIdx.x;
  if (i >= end) return;
  int64_t cx, cy;
  float z;
  // A plain atomic per point.  The cells near the sensor take hundreds of returns each and their few cache lines bound this
  // launch; a device-scope read in front of the atomic (skip when the stored value is already lower) was measured SLOWER,
  // 57 us against 34 us at 4 x 120 k points: it doubles the requests to those same lines.
  if (point_cell(points + i * dim, g, prefilter, cx, cy, z) && z >= z_floor)
    atomicMin(&enc[((int64_t)b * g.gy + cy) * g.gx + cx], encode_ordered(z));
}

}  // namespace
