// K1's cell rule for one point, shared by every kernel that asks "which BEV cell did the voxeliser put this point in":
// K31 / K35 (point_lift.hip) and K36a (render.hip).  A file that includes this must be compiled with -ffp-contract=off.
#pragma once
#include "common.hpp"

struct LiftGeom {          // VoxelGeom of voxelize.hip
  float x_min, y_min, z_min, x_max, y_max, z_max;
  float vx, vy, vz;
  int gx, gy, gz;
};

// K1's cell rule for the point at p: true iff the voxeliser keeps the point, then (cx, cy) is its BEV cell.  The one copy:
// K31, K35a, K35b and K36a all decide with it.
__device__ __forceinline__ bool point_cell(const float* __restrict__ p, const LiftGeom& g, int prefilter, int64_t& cx,
                                           int64_t& cy, float& z_out) {
  const float x = p[0], y = p[1], z = p[2];
  bool ok = true;
  if (prefilter) {
    ok = (g.x_min < x) && (x < g.x_max) && (g.y_min < y) && (y < g.y_max) && (g.z_min < z) && (z < g.z_max);
  }
  const float qx = floorf((x - g.x_min) / g.vx);
  const float qy = floorf((y - g.y_min) / g.vy);
  const float qz = floorf((z - g.z_min) / g.vz);
  ok = ok && (qx >= 0.f) && (qx < (float)g.gx) && (qy >= 0.f) && (qy < (float)g.gy) && (qz >= 0.f) &&
       (qz < (float)g.gz);  // NaN fails every compare
  cx = ok ? (int64_t)qx : 0;
  cy = ok ? (int64_t)qy : 0;
  z_out = z;
  return ok;
}
