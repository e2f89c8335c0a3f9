// K38a — mbv_visibility_map: which BEV cells a scan could observe at the height one asks about.  The rule is in
// include/maskbev_hip.h (K38a); this file restates nothing, it implements it.
//
// Four launches on the caller's stream, no host synchronisation:
//   1. init    the encoded cell minima to +inf, vis to 0.
//   2. points  K35a's pass with no floor (cell_min.hpp, the one copy): one thread per point, integer atomicMin on K31's
//              order-preserving encoding.  A point the cell rule accepts has a finite z (an infinite or NaN z fails the rule
//              on the z axis), so a cell is a target iff its minimum is not the encoding of +inf.
//   3. rays    a block of 256 threads owns 256 consecutive cells of one scan's plane.  Every thread reads its cell; a target
//              puts its ray (dx, dy, n, the two f32 terms of the height test that do not depend on k) into LDS, and an
//              inclusive scan of n over the block numbers the block's samples 0 .. total.  The threads then walk the samples
//              with a stride of 256: a binary search of the scan (8 LDS reads) finds the sample's ray, the rest is the line
//              and the compare.  Chosen over a wavefront per target with lanes over k: ray lengths run from 0 to ~700 cells,
//              so a wavefront per ray idles most lanes on the short rays near the sensor and one launch would need a
//              compaction of the targets in front of it; here consecutive lanes take consecutive k of one ray whatever its
//              length, a block without a target leaves after the scan, and no list is built.  The line is taken in 32-bit
//              integers where n <= 16384 (|2 k d + n| < 2^30, the same quotients) and in 64-bit integers beyond.
//              A certified cell gets the byte 1 with a plain store: every writer of a byte writes the same value, so the
//              result does not depend on the order of the rays, and the cells next to the sensor, which every ray crosses,
//              see plain stores, not atomics.
//   4. hit     one thread per cell: a target's byte gets bit 1 (the only writer of the byte in this launch).
// total_points == 0: vis is zeroed with one fill.  Integer atomics and idempotent stores only: bit-deterministic.
#include "common.hpp"
#include "point_cell.hpp"   // LiftGeom, point_cell: K1's cell rule, the one copy
#include "cell_min.hpp"     // the cell minima on the encoding: K35a's pass

namespace {

constexpr int kThreads = 256;
constexpr int kOriginLimit = 1 << 20, kNarrow = 16384;
constexpr uint8_t kPassed = 1, kHit = 2;

__global__ void __launch_bounds__(kThreads) k_vis_init(int64_t cells, uint32_t* __restrict__ enc, uint8_t* __restrict__ vis) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < cells; i += stride) {
    enc[i] = kEncInf;
    vis[i] = 0;
  }
}

template <typename T>
__device__ __forceinline__ T floor_div(T a, T d) {                // d > 0
  T q = a / d;
  return (a - q * d < 0) ? q - 1 : q;
}

__global__ void __launch_bounds__(kThreads) k_vis_rays(const uint32_t* __restrict__ enc, int gx, int gy, int origin_cx,
                                                       int origin_cy, float origin_z, float z_top,
                                                       uint8_t* __restrict__ vis) {
  __shared__ int32_t s_end[kThreads];                              // the inclusive scan of n
  __shared__ int32_t s_n[kThreads], s_dx[kThreads], s_dy[kThreads];
  __shared__ float s_rise[kThreads], s_rhs[kThreads];
  const int t = threadIdx.x;
  const int64_t plane = (int64_t)gy * gx;
  const int64_t cell = (int64_t)blockIdx.x * kThreads + t;
  const uint32_t* enc_b = enc + (int64_t)blockIdx.y * plane;
  int32_t n = 0;
  if (cell < plane) {
    const uint32_t e = enc_b[cell];
    if (e != kEncInf) {
      const int ty = (int)(cell / gx), tx = (int)(cell - (int64_t)ty * gx);
      const int dx = tx - origin_cx, dy = ty - origin_cy;          // |d| <= 65536 + 2^20
      const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
      n = ax > ay ? ax : ay;
      s_dx[t] = dx;
      s_dy[t] = dy;
      s_rise[t] = decode_ordered(e) - origin_z;
      s_rhs[t] = (z_top - origin_z) * (float)n;
    }
  }
  s_n[t] = n;
  s_end[t] = n;                                                    // a block's sum is below 256 * 2^21
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {
    const int32_t v = t >= o ? s_end[t - o] : 0;
    __syncthreads();
    s_end[t] += v;
    __syncthreads();
  }
  const int32_t total = s_end[kThreads - 1];
  uint8_t* vis_b = vis + (int64_t)blockIdx.y * plane;
  for (int32_t s = t; s < total; s += kThreads) {
    int lo = 0, hi = kThreads - 1;                                 // the first ray whose scan value exceeds s
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_end[mid] > s) hi = mid;
      else lo = mid + 1;
    }
    const int32_t nr = s_n[lo];
    const int32_t k = s - (s_end[lo] - nr);                        // in [0, nr)
    const int dx = s_dx[lo], dy = s_dy[lo];
    int64_t cx, cy;
    if (nr <= kNarrow) {
      cx = origin_cx + floor_div<int32_t>(2 * k * dx + nr, 2 * nr);
      cy = origin_cy + floor_div<int32_t>(2 * k * dy + nr, 2 * nr);
    } else {
      cx = origin_cx + floor_div<int64_t>(2 * (int64_t)k * dx + nr, 2 * (int64_t)nr);
      cy = origin_cy + floor_div<int64_t>(2 * (int64_t)k * dy + nr, 2 * (int64_t)nr);
    }
    if (cx < 0 || cx >= gx || cy < 0 || cy >= gy) continue;
    if (s_rise[lo] * (float)k <= s_rhs[lo]) vis_b[cy * gx + cx] = kPassed;   // NaN fails
  }
}

__global__ void __launch_bounds__(kThreads) k_vis_hit(int64_t cells, const uint32_t* __restrict__ enc,
                                                      uint8_t* __restrict__ vis) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < cells; i += stride)
    if (enc[i] != kEncInf) vis[i] |= kHit;
}

bool vis_sizes_ok(int32_t batch, int32_t gx, int32_t gy) {
  return !(batch < 0 || batch > 65535 || gx <= 0 || gy <= 0 || gx > 65536 || gy > 65536);
}

}  // namespace

extern "C" size_t mbv_visibility_map_workspace_bytes(int32_t batch, int32_t gx, int32_t gy) {
  if (!vis_sizes_ok(batch, gx, gy)) return 0;
  MbvCarver c(nullptr);
  c.take<uint32_t>((int64_t)batch * gy * gx);
  return c.off;
}

extern "C" int mbv_visibility_map(const float* points, int32_t point_dim, int64_t total_points, const int32_t* scan_offsets,
                                  int32_t batch, float x_min, float y_min, float z_min, float x_max, float y_max, float z_max,
                                  float vx, float vy, float vz, int32_t gx, int32_t gy, int32_t gz, int32_t prefilter,
                                  int32_t origin_cx, int32_t origin_cy, float origin_z, float z_top, uint8_t* vis,
                                  void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (batch < 0 || total_points < 0 || (point_dim != 3 && point_dim != 4) || gx <= 0 || gy <= 0 || gz <= 0 ||
      origin_cx < -kOriginLimit || origin_cx > kOriginLimit || origin_cy < -kOriginLimit || origin_cy > kOriginLimit)
    return MBV_ERR_BAD_ARG;
  if (batch > 65535 || total_points >= 0x7FFFFFFFll || gx > 65536 || gy > 65536) return MBV_ERR_UNSUPPORTED;
  if (batch == 0) return MBV_OK;
  if (!vis || (total_points > 0 && (!points || !scan_offsets))) return MBV_ERR_BAD_ARG;
  const int64_t plane = (int64_t)gy * gx, cells = (int64_t)batch * plane;
  if (total_points == 0) {
    MBV_CHECK_HIP(mbv_fill_async(vis, 0, (size_t)cells, stream));
    return MBV_OK;
  }
  MbvCarver c(workspace);
  uint32_t* enc = c.take<uint32_t>(cells);
  if (!workspace || workspace_bytes < c.off) return MBV_ERR_WORKSPACE;

  int64_t init_blocks = (cells + kThreads - 1) / kThreads;
  init_blocks = init_blocks > 4096 ? 4096 : init_blocks;
  hipLaunchKernelGGL(k_vis_init, dim3((unsigned)init_blocks), dim3(kThreads), 0, stream, cells, enc, vis);
  MBV_CHECK_LAUNCH();
  const LiftGeom g{x_min, y_min, z_min, x_max, y_max, z_max, vx, vy, vz, gx, gy, gz};
  hipLaunchKernelGGL(k_ground_points, dim3((unsigned)((total_points + kCellMinThreads - 1) / kCellMinThreads), batch),
                     dim3(kCellMinThreads), 0, stream, points, (int)point_dim, total_points, scan_offsets, g, (int)prefilter,
                     -INFINITY, enc);
  MBV_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_vis_rays, dim3((unsigned)((plane + kThreads - 1) / kThreads), batch), dim3(kThreads), 0, stream, enc,
                     (int)gx, (int)gy, (int)origin_cx, (int)origin_cy, origin_z, z_top, vis);
  MBV_CHECK_LAUNCH();
  int64_t hit_blocks = (cells + kThreads - 1) / kThreads;
  hit_blocks = hit_blocks > (1 << 20) ? (1 << 20) : hit_blocks;
  hipLaunchKernelGGL(k_vis_hit, dim3((unsigned)hit_blocks), dim3(kThreads), 0, stream, cells, enc, vis);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
