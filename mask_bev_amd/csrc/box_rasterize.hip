// K24 — KITTI / Waymo box tables → instance-id maps, the input of K14.
//
// Replaces the paint loop of KittiRasterizer.get_mask / WaymoRasterizer.get_mask (mask_bev/datasets/kitti/kitti_rasterizer.py
// :45-56, mask_bev/datasets/waymo/waymo_rasterizer.py:38-45: one uint8 image and one cv2.drawContours(..., -1) per box on the
// host).  The box corners are made on the host in f64 with the reference's expressions (rasterize.box_vertices); the kernel
// sees integer vertices only and all its arithmetic is integer, so the map is a pure function of the table: the fill rule of
// include/maskbev_hip.h (K24), restated in numpy by tests/box_rasterize_ref.py.
//
// One launch for a batch.  A workgroup owns a 16 x 64 tile of one frame's map (64 cells along y, the contiguous axis: a
// wave stores 256 contiguous bytes per row) and every thread four cells of it.  The frame's table is staged in LDS in chunks
// of 256 boxes, LAST chunk first: thread t loads box t, computes its bounding box, and a wave ballot of "the bounding box
// meets this tile" gives one 64-bit mask per wave.  The threads then walk the set bits from the highest down — a wave-uniform
// loop over the boxes that can touch the tile — and a cell takes the id of the first box that holds it: the last one in
// table order, which is what the reference's overwrite leaves.  Every cell of every map is written, 0 where no box claims it.
// At 800 x 800 x 4 the 10 MB store and the launch are the cost; no MFMA, 13 KB of LDS.
#include "common.hpp"

namespace {

constexpr int kTileX = 16, kTileY = 64, kThreads = 256, kCellsPerThread = kTileX / (kThreads / kTileY);
constexpr int kChunk = kThreads;                 // boxes staged per pass: one per thread
constexpr int kCoordLimit = 1 << 20;             // |vertex coordinate| <= 2^20: differences fit 22 bits, 2 i d + n fits 46

struct StagedBoxes {
  int32_t v[kChunk][8];                          // x0 y0 x1 y1 x2 y2 x3 y3
  int32_t bb[kChunk][4];                         // inclusive xmin, ymin, xmax, ymax of the vertices: I and L lie inside
  int32_t id[kChunk];
  unsigned long long hit[kChunk / 64];           // per staging wave: boxes whose bounding box meets the tile
};

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {      // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// (px, py) on the line a → b of the rule: along the major axis the line advances one cell per step, so the step index
// follows from the major coordinate and the minor coordinate is checked.
__device__ __forceinline__ bool on_line(int ax, int ay, int bx, int by, int px, int py) {
  const int dx = bx - ax, dy = by - ay;
  const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const int n = adx > ady ? adx : ady;
  if (n == 0) return px == ax && py == ay;
  if (adx >= ady) {
    const int i = dx < 0 ? ax - px : px - ax;
    if (i < 0 || i > n) return false;
    return py == ay + (int)floor_div(2 * (int64_t)i * dy + n, 2 * (int64_t)n);
  }
  const int i = dy < 0 ? ay - py : py - ay;
  if (i < 0 || i > n) return false;
  return px == ax + (int)floor_div(2 * (int64_t)i * dx + n, 2 * (int64_t)n);
}

__device__ __forceinline__ bool in_box(const int32_t* __restrict__ v, int px, int py) {
  bool on = false, odd = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ax = v[2 * e], ay = v[2 * e + 1], bx = v[(2 * e + 2) & 7], by = v[(2 * e + 3) & 7];
    const int dx = bx - ax, dy = by - ay;
    const int64_t cross = (int64_t)dx * (py - ay) - (int64_t)dy * (px - ax);
    const int xlo = ax < bx ? ax : bx, xhi = ax < bx ? bx : ax, ylo = ay < by ? ay : by, yhi = ay < by ? by : ay;
    on = on || (cross == 0 && px >= xlo && px <= xhi && py >= ylo && py <= yhi);
    const bool straddles = (ay > py) != (by > py);
    odd = odd != (straddles && (dy > 0 ? cross > 0 : cross < 0));
    on = on || on_line(ax, ay, bx, by, px, py);
  }
  return on || odd;
}

__global__ void __launch_bounds__(kThreads) k_rasterize_boxes(const int32_t* __restrict__ vertices,
                                                              const int32_t* __restrict__ ids,
                                                              const int32_t* __restrict__ frame_offsets, int batch, int nx,
                                                              int ny, int32_t* __restrict__ maps) {
  __shared__ StagedBoxes s;
  const int b = blockIdx.z, t = threadIdx.x;
  const int x0 = blockIdx.y * kTileX, y0 = blockIdx.x * kTileY;
  const int x1 = (x0 + kTileX < nx ? x0 + kTileX : nx) - 1, y1 = (y0 + kTileY < ny ? y0 + kTileY : ny) - 1;   // inclusive
  // the frame's rows of the table, never outside what the offsets declare as its length
  const int64_t total = frame_offsets[batch] > 0 ? frame_offsets[batch] : 0;
  int64_t begin = frame_offsets[b], end = frame_offsets[b + 1];
  begin = begin < 0 ? 0 : (begin > total ? total : begin);
  end = end < begin ? begin : (end > total ? total : end);

  const int py = y0 + (t & (kTileY - 1)), pxb = x0 + (t >> 6);         // cells (pxb + 4 k, py), k = 0 .. 3
  int32_t val[kCellsPerThread];
#pragma unroll
  for (int k = 0; k < kCellsPerThread; ++k) val[k] = 0;
  unsigned claimed = 0;                                                // bit k: cell k has its box, or lies outside the grid
#pragma unroll
  for (int k = 0; k < kCellsPerThread; ++k) claimed |= (py > y1 || pxb + 4 * k > x1) ? 1u << k : 0u;
  constexpr unsigned kAllClaimed = (1u << kCellsPerThread) - 1;

  for (int64_t hi = end; hi > begin; hi -= kChunk) {                   // chunks from the end of the table
    const int64_t lo = hi - kChunk > begin ? hi - kChunk : begin;
    const int count = (int)(hi - lo);
    __syncthreads();                                                   // the previous chunk has been read
    bool hit = false;
    if (t < count) {
      const int4* src = reinterpret_cast<const int4*>(vertices + (lo + t) * 8);
      const int4 p = src[0], q = src[1];
      const int32_t v[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
      int xmin = v[0], xmax = v[0], ymin = v[1], ymax = v[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s.v[t][2 * e] = v[2 * e];
        s.v[t][2 * e + 1] = v[2 * e + 1];
        xmin = v[2 * e] < xmin ? v[2 * e] : xmin;
        xmax = v[2 * e] > xmax ? v[2 * e] : xmax;
        ymin = v[2 * e + 1] < ymin ? v[2 * e + 1] : ymin;
        ymax = v[2 * e + 1] > ymax ? v[2 * e + 1] : ymax;
      }
      s.bb[t][0] = xmin; s.bb[t][1] = ymin; s.bb[t][2] = xmax; s.bb[t][3] = ymax;
      s.id[t] = ids[lo + t];
      // a vertex beyond ±2^20 cells (rasterize.box_vertices refuses it) paints nothing: the products below stay in 64 bits
      const bool sane = xmin >= -kCoordLimit && ymin >= -kCoordLimit && xmax <= kCoordLimit && ymax <= kCoordLimit;
      hit = sane && xmax >= x0 && xmin <= x1 && ymax >= y0 && ymin <= y1;
    }
    const unsigned long long m = __ballot(hit);
    if ((t & 63) == 0) s.hit[t >> 6] = m;
    __syncthreads();
    for (int w = (count - 1) >> 6; w >= 0; --w) {
      unsigned long long bits = s.hit[w];                              // the same in every lane: a uniform loop
      while (bits) {
        const int j = 63 - __clzll((long long)bits);
        bits &= ~(1ull << j);
        const int box = w * 64 + j;
        if (claimed == kAllClaimed) continue;
        const int bx0 = s.bb[box][0], by0 = s.bb[box][1], bx1 = s.bb[box][2], by1 = s.bb[box][3];
        if (py < by0 || py > by1) continue;
#pragma unroll
        for (int k = 0; k < kCellsPerThread; ++k) {
          const int px = pxb + 4 * k;
          if (!(claimed & (1u << k)) && px >= bx0 && px <= bx1 && in_box(s.v[box], px, py)) {
            val[k] = s.id[box];
            claimed |= 1u << k;
          }
        }
      }
    }
  }
  if (py <= y1) {
    int32_t* __restrict__ out = maps + (int64_t)b * nx * ny;
#pragma unroll
    for (int k = 0; k < kCellsPerThread; ++k) {
      const int px = pxb + 4 * k;
      if (px <= x1) out[(int64_t)px * ny + py] = val[k];
    }
  }
}

}  // namespace

extern "C" int mbv_rasterize_boxes(const int32_t* vertices, const int32_t* ids, const int32_t* frame_offsets, int32_t batch,
                                   int32_t nx, int32_t ny, int32_t* maps, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (batch < 1 || batch > 65535 || nx < 1 || ny < 1 || (int64_t)nx * ny > ((int64_t)1 << 26)) return MBV_ERR_BAD_ARG;
  if ((nx + kTileX - 1) / kTileX > 65535) return MBV_ERR_BAD_ARG;      // the grid's y dimension
  if (!vertices || !ids || !frame_offsets || !maps) return MBV_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(vertices) & 15) return MBV_ERR_BAD_ARG;
  const dim3 grid((unsigned)((ny + kTileY - 1) / kTileY), (unsigned)((nx + kTileX - 1) / kTileX), (unsigned)batch);
  hipLaunchKernelGGL(k_rasterize_boxes, grid, dim3(kThreads), 0, stream, vertices, ids, frame_offsets, (int)batch, (int)nx,
                     (int)ny, maps);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
