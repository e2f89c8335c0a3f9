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
//
// K35 — the same lift above a ground estimate made from the scan itself (include/maskbev_hip.h, K35; tests/ground_ref.py).
//   K35a  mbv_ground_map: per BEV cell the lowest z of the points the cell rule accepts (integer atomicMin on the encoding
//         below), then the minimum of that over a (2 radius + 1)^2 window of cells as two separable passes, along x and along
//         y.  Each pass stages a tile and its halo of `radius` cells in LDS (cells outside the grid: +inf) and takes the
//         minima from there; the minima are unsigned-integer minima on the encoding, so -0.0 < +0.0 holds through all passes.
//   K35b  mbv_lift_instances_ground: k_lift_points<true> reads g = ground[b][cy][cx] and keeps the query only where
//         z > g + clearance and z <= g + max_height (one rounded add each: this file is compiled without contraction); a
//         fourth table takes the minimum of g per query.  K31 is k_lift_points<false> of the same body.
#include "common.hpp"
#include "point_cell.hpp"   // LiftGeom, point_cell: K1's cell rule, the one copy
#include "cell_min.hpp"     // encode_ordered / decode_ordered, kEncInf and the cell-minimum pass, the one copy

namespace {

constexpr int kThreads = 256, kMaxQueries = 1024, kMaxBins = 256;
constexpr int kTile = 64, kRowTileRows = 16, kMaxRadius = 32;   // K35a: tiles of the window passes, the largest halo

__global__ void __launch_bounds__(kThreads) k_lift_init(int64_t total_points, int64_t bq, int64_t hist_elems,
                                                        int32_t* __restrict__ point_query, int32_t* __restrict__ counts,
                                                        uint32_t* __restrict__ enc_min, uint32_t* __restrict__ enc_max,
                                                        int32_t* __restrict__ hist, uint32_t* __restrict__ enc_gnd) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  for (int64_t i = t; i < total_points; i += stride) point_query[i] = -1;
  for (int64_t i = t; i < bq; i += stride) {
    counts[i] = 0;
    enc_min[i] = 0xffffffffu;
    enc_max[i] = 0u;
    if (enc_gnd) enc_gnd[i] = 0xffffffffu;                         // K35b only
  }
  for (int64_t i = t; i < hist_elems; i += stride) hist[i] = 0;
}

// GROUND = false: K31.  GROUND = true: K35b, the label rule above `ground` and the per-query minimum of the ground height.
template <bool GROUND>
__global__ void __launch_bounds__(kThreads) k_lift_points(const float* __restrict__ points, int dim, int64_t total_points,
                                                          const int32_t* __restrict__ scan_offsets, LiftGeom g,
                                                          int prefilter, const int32_t* __restrict__ instance_map,
                                                          int num_queries, int z_bins, const float* __restrict__ ground,
                                                          float clearance, float max_height,
                                                          int32_t* __restrict__ point_query, int32_t* __restrict__ counts,
                                                          uint32_t* __restrict__ enc_min, uint32_t* __restrict__ enc_max,
                                                          int32_t* __restrict__ hist, uint32_t* __restrict__ enc_gnd) {
  __shared__ int32_t s_cnt[kMaxQueries];
  __shared__ uint32_t s_min[kMaxQueries], s_max[kMaxQueries];
  __shared__ uint32_t s_gnd[GROUND ? kMaxQueries : 1];
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
    if (GROUND) s_gnd[q] = 0xffffffffu;
  }
  __syncthreads();
  const int64_t i = first + threadIdx.x;
  if (i < end) {
    int64_t cx, cy;
    float z;
    const bool ok = point_cell(points + i * dim, g, prefilter, cx, cy, z);
    int32_t q = -1;
    float gnd = 0.f;
    if (ok) {
      const int64_t cell = ((int64_t)b * g.gy + cy) * g.gx + cx;
      const int32_t v = instance_map[cell];
      if (v >= 0 && v < num_queries) q = v;
      if (GROUND && q >= 0) {
        gnd = ground[cell];
        if (!((z > gnd + clearance) && (z <= gnd + max_height))) q = -1;   // +inf (an empty window) and NaN fail
      }
    }
    point_query[i] = q;
    if (q >= 0) {
      const uint32_t e = encode_ordered(z);
      atomicAdd(&s_cnt[q], 1);
      atomicMin(&s_min[q], e);
      atomicMax(&s_max[q], e);
      if (GROUND) atomicMin(&s_gnd[q], encode_ordered(gnd));
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
      if (GROUND) atomicMin(&enc_gnd[o], s_gnd[q]);
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
                                                            const int32_t* __restrict__ hist, float* __restrict__ z_extent,
                                                            const uint32_t* __restrict__ enc_gnd,
                                                            float* __restrict__ z_ground) {
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
  if (z_ground) z_ground[o] = n > 0 ? decode_ordered(enc_gnd[o]) : 0.f;   // K35b only
}


// ---- K35a: the elevation grid ---------------------------------------------------------------------------------------------

// k_ground_init and k_ground_points, the cell minima on the encoding, are in cell_min.hpp: K38a launches them too

// Four cells of a row starting at column x (any sign), +inf outside [0, gx).  VEC: gx is a multiple of 4, x too, and the
// row is 16-byte aligned, so a quad lies wholly inside or wholly outside.
template <bool VEC>
__device__ __forceinline__ uint4 load_quad(const uint32_t* __restrict__ row, int x, int gx) {
  uint4 v = make_uint4(kEncInf, kEncInf, kEncInf, kEncInf);
  if (VEC) {
    if (x >= 0 && x < gx) v = *reinterpret_cast<const uint4*>(row + x);
  } else {
    if (x >= 0 && x < gx) v.x = row[x];
    if (x + 1 >= 0 && x + 1 < gx) v.y = row[x + 1];
    if (x + 2 >= 0 && x + 2 < gx) v.z = row[x + 2];
    if (x + 3 >= 0 && x + 3 < gx) v.w = row[x + 3];
  }
  return v;
}

template <bool VEC, typename T4, typename T>
__device__ __forceinline__ void store_quad(T* __restrict__ row, int x, int gx, T a, T b, T c, T d) {
  if (VEC) {
    T4 v;
    v.x = a; v.y = b; v.z = c; v.w = d;
    *reinterpret_cast<T4*>(row + x) = v;                           // x < gx and gx % 4 == 0: x + 3 < gx
  } else {
    row[x] = a;
    if (x + 1 < gx) row[x + 1] = b;
    if (x + 2 < gx) row[x + 2] = c;
    if (x + 3 < gx) row[x + 3] = d;
  }
}

__device__ __forceinline__ uint4 umin4(uint4 a, uint4 b) {
  return make_uint4(a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y, a.z < b.z ? a.z : b.z, a.w < b.w ? a.w : b.w);
}

// The window minimum along x, and cell_min decoded on the way.  A block owns kTile columns of kRowTileRows rows; its LDS
// tile holds those and `hr` = radius rounded up to 4 columns either side.  A thread owns four consecutive columns of one
// row: it walks the quads that cover its four windows once, every element taking part in the windows it lies in (the
// conditions are the same in every lane).
template <bool VEC>
__global__ void __launch_bounds__(kThreads) k_ground_rows(const uint32_t* __restrict__ enc, int gx, int gy, int radius,
                                                          float* __restrict__ cell_min, uint32_t* __restrict__ row_enc) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[kRowTileRows][kTile + 2 * kMaxRadius];
  const int hr = (radius + 3) & ~3;
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kRowTileRows;
  const int64_t plane = (int64_t)blockIdx.z * gy * gx;
  const int wq = (kTile + 2 * hr) >> 2;                            // quads of a tile row in use
  for (int i = threadIdx.x; i < wq * kRowTileRows; i += kThreads) {
    const int r = i / wq, qd = i - r * wq;
    uint4 v = make_uint4(kEncInf, kEncInf, kEncInf, kEncInf);
    if (y0 + r < gy) v = load_quad<VEC>(enc + plane + (int64_t)(y0 + r) * gx, x0 - hr + 4 * qd, gx);
    *reinterpret_cast<uint4*>(&tile[r][4 * qd]) = v;
  }
  __syncthreads();
  const int cq = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int x = x0 + 4 * cq, y = y0 + r;
  if (x >= gx || y >= gy) return;
  // output k = column x + k sits at tile column 4 cq + k + hr; its window starts `off` + k elements into quad cq
  const int off = hr - radius, span = 2 * radius;
  const uint4* row4 = reinterpret_cast<const uint4*>(tile[r]);
  uint32_t m[4] = {kEncInf, kEncInf, kEncInf, kEncInf};
  const int nblk = ((off + span + 3) >> 2) + 1;
  for (int t = 0; t < nblk; ++t) {
    const uint4 v = row4[cq + t];
    const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = 4 * t + u - off;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j >= k && j <= k + span) m[k] = e[u] < m[k] ? e[u] : m[k];
    }
  }
  const uint4 c = row4[cq + (hr >> 2)];
  const int64_t o = plane + (int64_t)y * gx;
  store_quad<VEC, uint4>(row_enc + o, x, gx, m[0], m[1], m[2], m[3]);
  store_quad<VEC, float4>(cell_min + o, x, gx, decode_ordered(c.x), decode_ordered(c.y), decode_ordered(c.z),
                          decode_ordered(c.w));
}

// The window minimum along y of the row minima: a block owns kTile x kTile cells and stages them with `radius` rows above
// and below.  A thread owns four columns of four consecutive rows and walks the 2 radius + 4 rows its windows cover once.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) k_ground_cols(const uint32_t* __restrict__ row_enc, int gx, int gy, int radius,
                                                          float* __restrict__ ground) {
  __shared__ __attribute__((aligned(16))) uint4 tile[(kTile + 2 * kMaxRadius) * (kTile / 4)];
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const int64_t plane = (int64_t)blockIdx.z * gy * gx;
  const int rows = kTile + 2 * radius;
  for (int i = threadIdx.x; i < rows * (kTile / 4); i += kThreads) {
    const int r = i >> 4, qd = i & 15;
    const int y = y0 - radius + r;
    uint4 v = make_uint4(kEncInf, kEncInf, kEncInf, kEncInf);
    if (y >= 0 && y < gy) v = load_quad<VEC>(row_enc + plane + (int64_t)y * gx, x0 + 4 * qd, gx);
    tile[i] = v;
  }
  __syncthreads();
  const int cq = threadIdx.x & 15, o0 = (threadIdx.x >> 4) * 4;
  const int x = x0 + 4 * cq;
  if (x >= gx || y0 + o0 >= gy) return;
  const int span = 2 * radius;
  const uint4 inf4 = make_uint4(kEncInf, kEncInf, kEncInf, kEncInf);
  uint4 m[4] = {inf4, inf4, inf4, inf4};
  for (int j = 0; j < span + 4; ++j) {                             // tile row o0 + j is grid row y0 + o0 + j - radius
    const uint4 v = tile[(o0 + j) * (kTile / 4) + cq];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j >= k && j <= k + span) m[k] = umin4(m[k], v);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + o0 + k;
    if (y < gy)
      store_quad<VEC, float4>(ground + plane + (int64_t)y * gx, x, gx, decode_ordered(m[k].x), decode_ordered(m[k].y),
                              decode_ordered(m[k].z), decode_ordered(m[k].w));
  }
}

struct GroundWorkspace {
  uint32_t *enc, *row_enc;
  size_t bytes;
};

GroundWorkspace carve_ground(void* ws, int64_t cells) {
  MbvCarver c(ws);
  GroundWorkspace w;
  w.enc = c.take<uint32_t>(cells);
  w.row_enc = c.take<uint32_t>(cells);
  w.bytes = c.off;
  return w;
}

struct LiftWorkspace {
  uint32_t *enc_min, *enc_max, *enc_gnd;
  int32_t* hist;
  size_t bytes;
};

LiftWorkspace carve_lift(void* ws, int64_t bq, int z_bins, bool with_ground) {
  MbvCarver c(ws);
  LiftWorkspace w;
  w.enc_min = c.take<uint32_t>(bq);
  w.enc_max = c.take<uint32_t>(bq);
  w.hist = c.take<int32_t>(bq * z_bins);
  w.enc_gnd = with_ground ? c.take<uint32_t>(bq) : nullptr;
  w.bytes = c.off;
  return w;
}

// K31 (ground == nullptr) and K35b behind one set of checks and launches
int lift_instances(const float* points, int32_t point_dim, int64_t total_points, const int32_t* scan_offsets, int32_t batch,
                   const LiftGeom& g, int32_t prefilter, const int32_t* instance_map, int32_t num_queries, int32_t z_bins,
                   float q_lo, float q_hi, bool with_ground, const float* ground, float clearance, float max_height,
                   int32_t* point_query, int32_t* counts, float* z_extent, float* z_ground, void* workspace,
                   size_t workspace_bytes, hipStream_t stream) {
  if (batch < 0 || total_points < 0 || num_queries < 0 || (point_dim != 3 && point_dim != 4) || g.gx <= 0 || g.gy <= 0 ||
      g.gz <= 0 || z_bins < 1 || z_bins > kMaxBins || !(0.f <= q_lo && q_lo <= q_hi && q_hi <= 1.f))
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
    if (z_ground) MBV_CHECK_HIP(mbv_fill_async(z_ground, 0, sizeof(float) * bq, stream));
    return MBV_OK;
  }
  if (!points || !scan_offsets || !instance_map || !point_query || !counts || !z_extent) return MBV_ERR_BAD_ARG;
  if (with_ground && (!ground || !z_ground)) return MBV_ERR_BAD_ARG;
  LiftWorkspace w = carve_lift(workspace, bq, z_bins, with_ground);
  if (!workspace || workspace_bytes < w.bytes) return MBV_ERR_WORKSPACE;

  const int64_t hist_elems = bq * z_bins;
  const int64_t most = total_points > hist_elems ? total_points : hist_elems;
  int64_t init_blocks = (most + kThreads - 1) / kThreads;
  init_blocks = init_blocks > 4096 ? 4096 : init_blocks;
  hipLaunchKernelGGL(k_lift_init, dim3((unsigned)init_blocks), dim3(kThreads), 0, stream, total_points, bq, hist_elems,
                     point_query, counts, w.enc_min, w.enc_max, w.hist, w.enc_gnd);
  MBV_CHECK_LAUNCH();
  // the y dimension of the grid walks the scans; x covers the longest scan (blocks past a scan's end exit at once)
  const dim3 grid((unsigned)((total_points + kThreads - 1) / kThreads), batch);
  if (with_ground)
    hipLaunchKernelGGL(k_lift_points<true>, grid, dim3(kThreads), 0, stream, points, (int)point_dim, total_points,
                       scan_offsets, g, (int)prefilter, instance_map, (int)num_queries, (int)z_bins, ground, clearance,
                       max_height, point_query, counts, w.enc_min, w.enc_max, w.hist, w.enc_gnd);
  else
    hipLaunchKernelGGL(k_lift_points<false>, grid, dim3(kThreads), 0, stream, points, (int)point_dim, total_points,
                       scan_offsets, g, (int)prefilter, instance_map, (int)num_queries, (int)z_bins,
                       (const float*)nullptr, 0.f, 0.f, point_query, counts, w.enc_min, w.enc_max, w.hist,
                       (uint32_t*)nullptr);
  MBV_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_lift_finalize, dim3((unsigned)((bq + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, bq,
                     (int)z_bins, g.z_min, g.z_max, q_lo, q_hi, counts, w.enc_min, w.enc_max, w.hist, z_extent, w.enc_gnd,
                     with_ground ? z_ground : (float*)nullptr);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

bool lift_sizes_ok(int32_t batch, int32_t num_queries, int32_t z_bins) {
  return !(batch < 0 || num_queries < 0 || num_queries > kMaxQueries || z_bins < 1 || z_bins > kMaxBins);
}

}  // namespace

extern "C" size_t mbv_lift_instances_workspace_bytes(int32_t batch, int32_t num_queries, int32_t z_bins) {
  if (!lift_sizes_ok(batch, num_queries, z_bins)) return 0;
  return carve_lift(nullptr, (int64_t)batch * num_queries, z_bins, false).bytes;
}

extern "C" int mbv_lift_instances(const float* points, int32_t point_dim, int64_t total_points,
                                  const int32_t* scan_offsets, int32_t batch, float x_min, float y_min, float z_min,
                                  float x_max, float y_max, float z_max, float vx, float vy, float vz, int32_t gx,
                                  int32_t gy, int32_t gz, int32_t prefilter, const int32_t* instance_map,
                                  int32_t num_queries, int32_t z_bins, float q_lo, float q_hi, int32_t* point_query,
                                  int32_t* counts, float* z_extent, void* workspace, size_t workspace_bytes,
                                  void* stream_) {
  const LiftGeom g{x_min, y_min, z_min, x_max, y_max, z_max, vx, vy, vz, gx, gy, gz};
  return lift_instances(points, point_dim, total_points, scan_offsets, batch, g, prefilter, instance_map, num_queries,
                        z_bins, q_lo, q_hi, false, nullptr, 0.f, 0.f, point_query, counts, z_extent, nullptr, workspace,
                        workspace_bytes, reinterpret_cast<hipStream_t>(stream_));
}

extern "C" size_t mbv_lift_instances_ground_workspace_bytes(int32_t batch, int32_t num_queries, int32_t z_bins) {
  if (!lift_sizes_ok(batch, num_queries, z_bins)) return 0;
  return carve_lift(nullptr, (int64_t)batch * num_queries, z_bins, true).bytes;
}

extern "C" int mbv_lift_instances_ground(const float* points, int32_t point_dim, int64_t total_points,
                                         const int32_t* scan_offsets, int32_t batch, float x_min, float y_min, float z_min,
                                         float x_max, float y_max, float z_max, float vx, float vy, float vz, int32_t gx,
                                         int32_t gy, int32_t gz, int32_t prefilter, const int32_t* instance_map,
                                         int32_t num_queries, int32_t z_bins, float q_lo, float q_hi, const float* ground,
                                         float clearance, float max_height, int32_t* point_query, int32_t* counts,
                                         float* z_extent, float* z_ground, void* workspace, size_t workspace_bytes,
                                         void* stream_) {
  const LiftGeom g{x_min, y_min, z_min, x_max, y_max, z_max, vx, vy, vz, gx, gy, gz};
  return lift_instances(points, point_dim, total_points, scan_offsets, batch, g, prefilter, instance_map, num_queries,
                        z_bins, q_lo, q_hi, true, ground, clearance, max_height, point_query, counts, z_extent, z_ground,
                        workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream_));
}

extern "C" size_t mbv_ground_map_workspace_bytes(int32_t batch, int32_t gx, int32_t gy) {
  if (batch < 0 || batch > 65535 || gx <= 0 || gy <= 0 || gx > 65536 || gy > 65536) return 0;
  return carve_ground(nullptr, (int64_t)batch * gy * gx).bytes;
}

extern "C" int mbv_ground_map(const float* points, int32_t point_dim, int64_t total_points, const int32_t* scan_offsets,
                              int32_t batch, float x_min, float y_min, float z_min, float x_max, float y_max, float z_max,
                              float vx, float vy, float vz, int32_t gx, int32_t gy, int32_t gz, int32_t prefilter,
                              int32_t radius, float z_floor, float* cell_min, float* ground, void* workspace,
                              size_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (batch < 0 || total_points < 0 || radius < 0 || (point_dim != 3 && point_dim != 4) || gx <= 0 || gy <= 0 || gz <= 0)
    return MBV_ERR_BAD_ARG;
  if (radius > kMaxRadius || batch > 65535 || total_points >= 0x7FFFFFFFll || gx > 65536 || gy > 65536)
    return MBV_ERR_UNSUPPORTED;
  if (batch == 0) return MBV_OK;
  if (!cell_min || !ground || (total_points > 0 && (!points || !scan_offsets))) return MBV_ERR_BAD_ARG;
  const int64_t cells = (int64_t)batch * gy * gx;
  GroundWorkspace w = carve_ground(workspace, cells);
  if (!workspace || workspace_bytes < w.bytes) return MBV_ERR_WORKSPACE;

  int64_t init_blocks = (cells + kThreads - 1) / kThreads;
  init_blocks = init_blocks > 4096 ? 4096 : init_blocks;
  hipLaunchKernelGGL(k_ground_init, dim3((unsigned)init_blocks), dim3(kThreads), 0, stream, cells, w.enc);
  MBV_CHECK_LAUNCH();
  if (total_points > 0) {
    const LiftGeom g{x_min, y_min, z_min, x_max, y_max, z_max, vx, vy, vz, gx, gy, gz};
    hipLaunchKernelGGL(k_ground_points, dim3((unsigned)((total_points + kThreads - 1) / kThreads), batch), dim3(kThreads), 0,
                       stream, points, (int)point_dim, total_points, scan_offsets, g, (int)prefilter, z_floor, w.enc);
    MBV_CHECK_LAUNCH();
  }
  // one condition for the 16-byte paths of both passes: whole quads per row, every plane 16-byte aligned
  const bool vec = (gx & 3) == 0 && ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(cell_min) |
                                      reinterpret_cast<uintptr_t>(ground)) & 15) == 0;
  const unsigned tx = (unsigned)((gx + kTile - 1) / kTile);
  const dim3 row_grid(tx, (unsigned)((gy + kRowTileRows - 1) / kRowTileRows), batch);
  const dim3 col_grid(tx, (unsigned)((gy + kTile - 1) / kTile), batch);
  if (vec) {
    hipLaunchKernelGGL(k_ground_rows<true>, row_grid, dim3(kThreads), 0, stream, w.enc, (int)gx, (int)gy, (int)radius,
                       cell_min, w.row_enc);
    MBV_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ground_cols<true>, col_grid, dim3(kThreads), 0, stream, w.row_enc, (int)gx, (int)gy, (int)radius,
                       ground);
  } else {
    hipLaunchKernelGGL(k_ground_rows<false>, row_grid, dim3(kThreads), 0, stream, w.enc, (int)gx, (int)gy, (int)radius,
                       cell_min, w.row_enc);
    MBV_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ground_cols<false>, col_grid, dim3(kThreads), 0, stream, w.row_enc, (int)gx, (int)gy, (int)radius,
                       ground);
  }
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
