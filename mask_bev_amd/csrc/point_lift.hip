// K31 — lift predicted BEV instances to the points of the scan: per-point query labels, points per query and the
// z-extent of every query's points.
//
// The scan that made the pseudo-image has a z for every point, K1's cell rule says which BEV cell a point fell into and
// K21's instance map says which query owns that cell.  One thread per point (blocks of 256, grid.y = scan):
//   1. the cell, EXACTLY as k_point_keys (voxelize.hip) computes it: c = floorf((p - min) / vs) with the subtraction and the
//      division as separate IEEE f32 operations (compiled with -ffp-contract=off), rejected when c < 0 or c >= grid on any of
//      the three axes (NaN fails every compare), and under `prefilter` the strict min < p < max on all three axes first.  A
//      point K1 would drop gets -1.
//   2. q = instance_map[b][cy][cx] (row = y-cell, column = x-cell); a value outside [0, num_queries) counts as -1 and is
//      never used as an index.
//   3. per block, an LDS table (count, min, max per query; 12 KB at 1024 queries) takes integer atomics on an
//      order-preserving integer encoding of the f32 z; each query a block touched is flushed once with integer global
//      atomics (add / min / max).  The z histogram, (batch, num_queries, z_bins) in the workspace, takes plain global integer
//      atomics: points inside instances are a small share of a scan.
// Integer atomics only: the result does not depend on the order of the points' arrival, hence bit-deterministic.
//
// A small launch in front initialises every output and the workspace (nothing has to be pre-set by the caller), a small
// launch behind decodes the extremes and walks the histograms.
//
// The histogram arithmetic (f32 and integers only; tests/point_lift_ref.py restates it operation by operation):
//   bw      = (z_max - z_min) / (float)z_bins                              the geometry's z range in z_bins equal bins
//   bin(z)  = clamp((int)floorf((z - z_min) / bw), 0, z_bins - 1)
//   rank(q) = clamp((int64)floorf(q * (float)(n - 1)), 0, n - 1)           n = the query's points, ranks ascend with z
//   k(r)    = the first bin whose cumulative count exceeds r              the bin that holds the point of rank r
//   z_lo    = z_min + (float)k(rank(q_lo)) * bw                            that bin's lower edge
//   z_hi    = z_min + (float)(k(rank(q_hi)) + 1) * bw                      that bin's upper edge
// both then clamped into [z_min, z_max] of the query's own points: fminf(fmaxf(edge, zmin), zmax).
#include "common.hpp"

namespace {

constexpr int kThreads = 256, kMaxQueries = 1024, kMaxBins = 256;

struct LiftGeom {          // VoxelGeom of voxelize.hip
  float x_min, y_min, z_min, x_max, y_max, z_max;
  float vx, vy, vz;
  int gx, gy, gz;
};

// f32 → u32 with the order of the floats (negative numbers: all bits flipped; others: the sign bit set) and back
__device__ __forceinline__ uint32_t encode_ordered(float z) {
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float decode_ordered(uint32_t e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

__global__ void __launch_bounds__(kThreads) k_lift_init(int64_t total_points, int64_t bq, int64_t hist_elems,
                                                        int32_t* __restrict__ point_query, int32_t* __restrict__ counts,
                                                        uint32_t* __restrict__ enc_min, uint32_t* __restrict__ enc_max,
                                                        int32_t* __restrict__ hist) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  for (int64_t i = t; i < total_points; i += stride) point_query[i] = -1;
  for (int64_t i = t; i < bq; i += stride) {
    counts[i] = 0;
    enc_min[i] = 0xffffffffu;
    enc_max[i] = 0u;
  }
  for (int64_t i = t; i < hist_elems; i += stride) hist[i] = 0;
}

__global__ void __launch_bounds__(kThreads) k_lift_points(const float* __restrict__ points, int dim, int64_t total_points,
                                                          const int32_t* __restrict__ scan_offsets, LiftGeom g,
                                                          int prefilter, const int32_t* __restrict__ instance_map,
                                                          int num_queries, int z_bins, int32_t* __restrict__ point_query,
                                                          int32_t* __restrict__ counts, uint32_t* __restrict__ enc_min,
                                                          uint32_t* __restrict__ enc_max, int32_t* __restrict__ hist) {
  __shared__ int32_t s_cnt[kMaxQueries];
  __shared__ uint32_t s_min[kMaxQueries], s_max[kMaxQueries];
  const int b = blockIdx.y;
  int64_t begin = scan_offsets[b], end = scan_offsets[b + 1];
  begin = begin < 0 ? 0 : begin;                                   // offsets that point outside the table read nothing
  end = end > total_points ? total_points : end;
  const int64_t first = begin + (int64_t)blockIdx.x * kThreads;
  if (first >= end) return;                                        // the whole block: no barrier has been reached
  for (int q = threadIdx.x; q < num_queries; q += kThreads) {
    s_cnt[q] = 0;
    s_min[q] = 0xffffffffu;
    s_max[q] = 0u;
  }
  __syncthreads();
  const int64_t i = first + threadIdx.x;
  if (i < end) {
    const float* p = points + i * dim;
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
    int32_t q = -1;
    if (ok) {
      const int64_t cx = (int64_t)qx, cy = (int64_t)qy;
      const int32_t v = instance_map[((int64_t)b * g.gy + cy) * g.gx + cx];
      if (v >= 0 && v < num_queries) q = v;
    }
    point_query[i] = q;
    if (q >= 0) {
      const uint32_t e = encode_ordered(z);
      atomicAdd(&s_cnt[q], 1);
      atomicMin(&s_min[q], e);
      atomicMax(&s_max[q], e);
      const float bw = (g.z_max - g.z_min) / (float)z_bins;
      const float fb = floorf((z - g.z_min) / bw);
      int bin = fb >= (float)z_bins ? z_bins - 1 : (fb >= 0.f ? (int)fb : 0);   // (a NaN quotient, bw == 0: bin 0)
      atomicAdd(&hist[((int64_t)b * num_queries + q) * z_bins + bin], 1);
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < num_queries; q += kThreads) {
    const int32_t c = s_cnt[q];
    if (c > 0) {
      const int64_t o = (int64_t)b * num_queries + q;
      atomicAdd(&counts[o], c);
      atomicMin(&enc_min[o], s_min[q]);
      atomicMax(&enc_max[o], s_max[q]);
    }
  }
}

__device__ __forceinline__ int64_t rank_of(float quantile, int32_t n) {
  int64_t r = (int64_t)floorf(quantile * (float)(n - 1));
  r = r < 0 ? 0 : r;
  return r > (int64_t)n - 1 ? (int64_t)n - 1 : r;
}

__global__ void __launch_bounds__(kThreads) k_lift_finalize(int64_t bq, int z_bins, float z_lo_geom, float z_hi_geom,
                                                            float q_lo, float q_hi, const int32_t* __restrict__ counts,
                                                            const uint32_t* __restrict__ enc_min,
                                                            const uint32_t* __restrict__ enc_max,
                                                            const int32_t* __restrict__ hist, float* __restrict__ z_extent) {
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= bq) return;
  const int32_t n = counts[o];
  float zmin = 0.f, zmax = 0.f, zlo = 0.f, zhi = 0.f;
  if (n > 0) {
    zmin = decode_ordered(enc_min[o]);
    zmax = decode_ordered(enc_max[o]);
    const int64_t r_lo = rank_of(q_lo, n), r_hi = rank_of(q_hi, n);
    const int32_t* h = hist + o * z_bins;
    int k_lo = z_bins - 1, k_hi = z_bins - 1;
    bool have_lo = false, have_hi = false;
    int64_t cum = 0;
    for (int k = 0; k < z_bins; ++k) {
      cum += h[k];
      if (!have_lo && cum > r_lo) { k_lo = k; have_lo = true; }
      if (!have_hi && cum > r_hi) { k_hi = k; have_hi = true; }
    }
    const float bw = (z_hi_geom - z_lo_geom) / (float)z_bins;
    const float lo_edge = z_lo_geom + (float)k_lo * bw;
    const float hi_edge = z_lo_geom + (float)(k_hi + 1) * bw;
    zlo = fminf(fmaxf(lo_edge, zmin), zmax);
    zhi = fminf(fmaxf(hi_edge, zmin), zmax);
  }
  z_extent[o * 4 + 0] = zmin;
  z_extent[o * 4 + 1] = zmax;
  z_extent[o * 4 + 2] = zlo;
  z_extent[o * 4 + 3] = zhi;
}

struct LiftWorkspace {
  uint32_t *enc_min, *enc_max;
  int32_t* hist;
  size_t bytes;
};

LiftWorkspace carve_lift(void* ws, int64_t bq, int z_bins) {
  MbvCarver c(ws);
  LiftWorkspace w;
  w.enc_min = c.take<uint32_t>(bq);
  w.enc_max = c.take<uint32_t>(bq);
  w.hist = c.take<int32_t>(bq * z_bins);
  w.bytes = c.off;
  return w;
}

}  // namespace

extern "C" size_t mbv_lift_instances_workspace_bytes(int32_t batch, int32_t num_queries, int32_t z_bins) {
  if (batch < 0 || num_queries < 0 || num_queries > kMaxQueries || z_bins < 1 || z_bins > kMaxBins) return 0;
  return carve_lift(nullptr, (int64_t)batch * num_queries, z_bins).bytes;
}

extern "C" int mbv_lift_instances(const float* points, int32_t point_dim, int64_t total_points,
                                  const int32_t* scan_offsets, int32_t batch, float x_min, float y_min, float z_min,
                                  float x_max, float y_max, float z_max, float vx, float vy, float vz, int32_t gx,
                                  int32_t gy, int32_t gz, int32_t prefilter, const int32_t* instance_map,
                                  int32_t num_queries, int32_t z_bins, float q_lo, float q_hi, int32_t* point_query,
                                  int32_t* counts, float* z_extent, void* workspace, size_t workspace_bytes,
                                  void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (batch < 0 || total_points < 0 || num_queries < 0 || (point_dim != 3 && point_dim != 4) || gx <= 0 || gy <= 0 ||
      gz <= 0 || z_bins < 1 || z_bins > kMaxBins || !(0.f <= q_lo && q_lo <= q_hi && q_hi <= 1.f))
    return MBV_ERR_BAD_ARG;
  if (num_queries > kMaxQueries || total_points >= 0x7FFFFFFFll || batch > 65535) return MBV_ERR_UNSUPPORTED;
  const int64_t bq = (int64_t)batch * num_queries;
  if (bq == 0) {                                   // no query to own a point: every point is unlabelled
    if (point_query) MBV_CHECK_HIP(mbv_fill_async(point_query, 0xff, sizeof(int32_t) * total_points, stream));
    return MBV_OK;
  }
  if (total_points == 0) {
    if (counts) MBV_CHECK_HIP(mbv_fill_async(counts, 0, sizeof(int32_t) * bq, stream));
    if (z_extent) MBV_CHECK_HIP(mbv_fill_async(z_extent, 0, sizeof(float) * 4 * bq, stream));
    return MBV_OK;
  }
  if (!points || !scan_offsets || !instance_map || !point_query || !counts || !z_extent) return MBV_ERR_BAD_ARG;
  LiftWorkspace w = carve_lift(workspace, bq, z_bins);
  if (!workspace || workspace_bytes < w.bytes) return MBV_ERR_WORKSPACE;

  const int64_t hist_elems = bq * z_bins;
  const int64_t most = total_points > hist_elems ? total_points : hist_elems;
  int64_t init_blocks = (most + kThreads - 1) / kThreads;
  init_blocks = init_blocks > 4096 ? 4096 : init_blocks;
  hipLaunchKernelGGL(k_lift_init, dim3((unsigned)init_blocks), dim3(kThreads), 0, stream, total_points, bq, hist_elems,
                     point_query, counts, w.enc_min, w.enc_max, w.hist);
  MBV_CHECK_LAUNCH();
  // the y dimension of the grid walks the scans; x covers the longest scan (blocks past a scan's end exit at once)
  LiftGeom g{x_min, y_min, z_min, x_max, y_max, z_max, vx, vy, vz, gx, gy, gz};
  const unsigned bx = (unsigned)((total_points + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(k_lift_points, dim3(bx, batch), dim3(kThreads), 0, stream, points, (int)point_dim, total_points,
                     scan_offsets, g, (int)prefilter, instance_map, (int)num_queries, (int)z_bins, point_query, counts,
                     w.enc_min, w.enc_max, w.hist);
  MBV_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_lift_finalize, dim3((unsigned)((bq + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, bq,
                     (int)z_bins, z_min, z_max, q_lo, q_hi, counts, w.enc_min, w.enc_max, w.hist, z_extent);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
