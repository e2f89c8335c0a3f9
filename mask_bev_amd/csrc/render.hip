// K36 — BEV frames of scans, instances, tracks and boxes, composed on the device (include/maskbev_hip.h, K36;
// tests/render_ref.py restates both kernels as plain loops).
//
//   K36a  mbv_cell_counts: returns per BEV cell.  A launch zeroes the (B, gy, gx) table, then one thread per point (blocks of
//         256, grid.y = scan) decides with K1's cell rule — point_cell of point_cell.hpp, the copy K31 and K35 use — and adds
//         one with an integer atomic: the result does not depend on the order of the points.
//   K36b  mbv_render_bev: the (B, H, W, 3) uint8 image, H = gy * s, W = gx * s.  All layer arithmetic is integer.
//
// How K36b stores.  The image is one flat run of B * H * W pixels of three bytes; four consecutive pixels are twelve bytes,
// three whole dwords, whatever the row length is.  So the unit of work is a QUAD of four consecutive flat pixels, one per
// lane, stored as three dwords.  A quad belongs to the image row it STARTS in; when W is no multiple of 4 the last quad of a
// row runs into the next row (or the next scan), and each of its pixels is shaded at its own (scan, row, column).  Only the
// very last quad of the whole image can be short: that one lane stores bytes.  No row has a scalar head or tail.
//
// A workgroup of 256 lanes owns 32 quads of 8 consecutive output rows of one scan.  Boxes: the scan's table is walked in
// chunks of kBoxChunk rows; wave 0 loads a chunk into LDS, one box per lane, marks the boxes out of the coordinate bound and
// rejects those whose bounding box, grown by `line`, misses the tile's pixels; the ballot of the survivors is the list every
// lane then walks in row order (later rows win).  A pixel of a quad that ran out of the tile's rows is not covered by that
// rejection: its lane walks the pixel's scan's table from memory instead (at most one lane per row, and none when W % 4 == 0).
// The workgroup of tile (0, 0) of a scan sees every row of the table once and writes the scan's `skipped`.
#include "common.hpp"
#include "point_cell.hpp"   // LiftGeom, point_cell: K1's cell rule, the one copy

namespace {

constexpr int kThreads = 256;
constexpr int kBoxChunk = 64;                  // boxes staged in LDS at a time: one per lane of wave 0
constexpr int kTileQuads = 32, kTileRows = 8;  // a workgroup's tile: 32 quads (128 pixels) of 8 rows
constexpr int kMaxSide = 4096, kMaxScale = 8, kMaxLine = 32;
constexpr int kCornerBound = 16384;            // half-pixel units; keeps cross(u, v)^2 below 2^62
static_assert(kBoxChunk == MBV_WAVE, "the chunk's survivors are one ballot of wave 0");
static_assert(kTileQuads * kTileRows == kThreads, "one quad per lane");

__global__ void __launch_bounds__(kThreads) k_counts_zero(int64_t cells, int32_t* __restrict__ counts) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < cells; i += stride) counts[i] = 0;
}

__global__ void __launch_bounds__(kThreads) k_count_points(const float* __restrict__ points, int dim, int64_t total_points,
                                                           const int32_t* __restrict__ scan_offsets, LiftGeom g,
                                                           int prefilter, int32_t* __restrict__ counts) {
  const int b = blockIdx.y;
  int64_t begin = scan_offsets[b], end = scan_offsets[b + 1];
  begin = begin < 0 ? 0 : begin;                                   // offsets that point outside the table read nothing
  end = end > total_points ? total_points : end;
  const int64_t i = begin + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= end) return;
  int64_t cx, cy;
  float z;
  if (point_cell(points + i * dim, g, prefilter, cx, cy, z)) atomicAdd(&counts[((int64_t)b * g.gy + cy) * g.gx + cx], 1);
}

struct RenderArgs {
  const int32_t* counts;
  const uint8_t* density_lut;
  const int32_t* instance_map;
  const int32_t* id_table;
  const uint8_t* palette;
  const int32_t* gt_map;
  const int32_t* box_corners;
  const uint8_t* box_rgb;
  const int32_t* box_offsets;
  uint8_t* image;
  int32_t* skipped;
  int64_t num_boxes, total_pixels;
  int batch, gx, gy, scale, H, W;
  int num_queries, palette_size, alpha;
  int gt_background, line, flip;
  uint32_t untracked_rgb, gt_rgb;                                  // r | g << 8 | b << 16
};

__device__ __forceinline__ uint32_t rgb3(const uint8_t* __restrict__ p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

__device__ __forceinline__ uint32_t blend(uint32_t rgb, uint32_t col, int alpha) {
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t a = (rgb >> (8 * c)) & 0xffu, o = (col >> (8 * c)) & 0xffu;
    out |= (((a * (uint32_t)(256 - alpha) + o * (uint32_t)alpha + 128u) >> 8) & 0xffu) << (8 * c);
  }
  return out;
}

// layers 1 - 3 of pixel (py, px) of scan b: density, predicted instances, ground-truth contour
__device__ __forceinline__ uint32_t shade_cell_layers(const RenderArgs& a, int b, int py, int px) {
  const int s = a.scale;
  const int cy = py / s, cx = px / s;
  const int64_t plane = (int64_t)b * a.gy * a.gx;
  const int64_t cell = plane + (int64_t)cy * a.gx + cx;
  uint32_t rgb = 0;
  if (a.density_lut) {
    const int32_t c = a.counts ? a.counts[cell] : 0;
    int level = c > 0 ? 32 - __clz(c) : 0;                         // bit_length
    level = level > 15 ? 15 : level;
    rgb = rgb3(a.density_lut + 3 * level);
  }
  if (a.instance_map) {
    const int32_t q = a.instance_map[cell];
    if (q >= 0 && q < a.num_queries) {
      const int32_t id = a.id_table ? a.id_table[(int64_t)b * a.num_queries + q] : q;
      const uint32_t col = id >= 0 ? rgb3(a.palette + 3 * (id % a.palette_size)) : a.untracked_rgb;
      rgb = blend(rgb, col, a.alpha);
    }
  }
  if (a.gt_map) {
    const int32_t v = a.gt_map[cell];
    if (v != a.gt_background) {
      // a neighbour pixel in the same cell has the same value; one outside the image counts as background, which v is not
      bool edge = px == 0 || py == 0 || px == a.W - 1 || py == a.H - 1;
      if (!edge) {
        const int lx = (px - 1) / s, rx = (px + 1) / s, uy = (py - 1) / s, dy = (py + 1) / s;
        if (lx != cx) edge = a.gt_map[cell - 1] != v;
        if (!edge && rx != cx) edge = a.gt_map[cell + 1] != v;
        if (!edge && uy != cy) edge = a.gt_map[cell - a.gx] != v;
        if (!edge && dy != cy) edge = a.gt_map[cell + a.gx] != v;
      }
      if (edge) rgb = a.gt_rgb;
    }
  }
  return rgb;
}

// Is P = (px2, py2), in half-pixel units, within line / 2 of one of the four sides of the box with corners c[0..7]
// (x0, y0, .. x3, y3)?  Exact: int64 products, the last compare unsigned (4 cross^2 < 2^64 under the corner bound).
template <typename Corners>
__device__ __forceinline__ bool box_hits(const Corners& c, int px2, int py2, int64_t line2) {
  bool hit = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int n = (k + 1) & 3;
    const int64_t ax = c[2 * k], ay = c[2 * k + 1], bx = c[2 * n], by = c[2 * n + 1];
    const int64_t ux = bx - ax, uy = by - ay, vx = px2 - ax, vy = py2 - ay;
    const int64_t d = ux * vx + uy * vy, L = ux * ux + uy * uy;
    bool h;
    if (d <= 0) {
      h = 4 * (vx * vx + vy * vy) <= line2;
    } else if (d >= L) {
      const int64_t wx = px2 - bx, wy = py2 - by;
      h = 4 * (wx * wx + wy * wy) <= line2;
    } else {
      const int64_t cr = ux * vy - uy * vx;
      h = 4ull * (uint64_t)(cr * cr) <= (uint64_t)(line2 * L);
    }
    hit = hit || h;
  }
  return hit;
}

__device__ __forceinline__ bool corners_out_of_bound(const int32_t* c) {
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) bad = bad || c[k] > kCornerBound || c[k] < -kCornerBound;
  return bad;
}

__global__ void __launch_bounds__(kThreads) k_render_bev(RenderArgs a) {
  __shared__ int32_t s_corner[kBoxChunk][8];
  __shared__ int32_t s_bound[kBoxChunk][4];                        // x_lo, x_hi, y_lo, y_hi of the box grown by `line`
  __shared__ uint32_t s_rgb[kBoxChunk];
  __shared__ unsigned long long s_live;

  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int H = a.H, W = a.W;
  const int oy = blockIdx.y * kTileRows + tid / kTileQuads;        // the output row the lane's quad starts in
  const int j = blockIdx.x * kTileQuads + (tid % kTileQuads);      // the row's j-th quad
  const int64_t row_base = ((int64_t)b * H + oy) * W;              // flat pixel index of the row's first pixel
  const int shift = (int)((4 - (row_base & 3)) & 3);               // pixels of the row that the previous row's last quad owns
  const int ox0 = shift + 4 * j;
  const bool active = oy < H && ox0 < W;
  const int64_t flat0 = row_base + ox0;                            // a multiple of 4

  int p_b[4], p_y[4], p_x[4];
  bool valid[4], local[4];
  uint32_t rgb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int x = ox0 + i, y = oy, bb = b;
    bool wrapped = false;
    if (active) {
      while (x >= W) {                                             // at most three turns (W >= 1)
        x -= W;
        wrapped = true;
        if (++y == H) { y = 0; ++bb; }
      }
    }
    valid[i] = active && bb < a.batch;
    local[i] = valid[i] && !wrapped;
    p_b[i] = bb;
    p_x[i] = x;
    p_y[i] = a.flip ? H - 1 - y : y;                               // the output row y shows pixel row H - 1 - y
    rgb[i] = valid[i] ? shade_cell_layers(a, bb, p_y[i], x) : 0u;
  }

  const int64_t line2 = (int64_t)a.line * a.line;
  int32_t n_skipped = 0;
  if (a.box_corners) {
    int64_t begin = a.box_offsets[b], end = a.box_offsets[b + 1];
    begin = begin < 0 ? 0 : begin;                                 // offsets that point outside the table read nothing
    end = end > a.num_boxes ? a.num_boxes : end;
    // the pixels the tile's in-row quads can hold, as centres in half-pixel units
    const int tx_lo = blockIdx.x * kTileQuads * 4, ty_lo = blockIdx.y * kTileRows;
    int tx_hi = tx_lo + kTileQuads * 4 + 2, ty_hi = ty_lo + kTileRows - 1;     // + 2: `shift` moves a quad by up to 3 pixels
    tx_hi = tx_hi > W - 1 ? W - 1 : tx_hi;
    ty_hi = ty_hi > H - 1 ? H - 1 : ty_hi;
    const int py_lo = a.flip ? H - 1 - ty_hi : ty_lo, py_hi = a.flip ? H - 1 - ty_lo : ty_hi;
    const int cx_lo = 2 * tx_lo + 1, cx_hi = 2 * tx_hi + 1, cy_lo = 2 * py_lo + 1, cy_hi = 2 * py_hi + 1;
    for (int64_t chunk = begin; chunk < end; chunk += kBoxChunk) {
      __syncthreads();                                             // the previous chunk has been walked by every lane
      if (tid < kBoxChunk) {                                       // wave 0, whole
        const int64_t r = chunk + tid;
        bool live = false, bad = false;
        if (r < end) {
          int32_t c[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) c[k] = a.box_corners[r * 8 + k];
          bad = corners_out_of_bound(c);
          int x_lo = c[0], x_hi = c[0], y_lo = c[1], y_hi = c[1];
#pragma unroll
          for (int k = 1; k < 4; ++k) {
            x_lo = c[2 * k] < x_lo ? c[2 * k] : x_lo;
            x_hi = c[2 * k] > x_hi ? c[2 * k] : x_hi;
            y_lo = c[2 * k + 1] < y_lo ? c[2 * k + 1] : y_lo;
            y_hi = c[2 * k + 1] > y_hi ? c[2 * k + 1] : y_hi;
          }
          if (!bad) {                                              // (the bound also keeps these sums inside int32)
            x_lo -= a.line; x_hi += a.line; y_lo -= a.line; y_hi += a.line;
            live = x_hi >= cx_lo && x_lo <= cx_hi && y_hi >= cy_lo && y_lo <= cy_hi;
          }
#pragma unroll
          for (int k = 0; k < 8; ++k) s_corner[tid][k] = c[k];
          s_bound[tid][0] = x_lo; s_bound[tid][1] = x_hi; s_bound[tid][2] = y_lo; s_bound[tid][3] = y_hi;
          s_rgb[tid] = rgb3(a.box_rgb + r * 3);
        }
        const unsigned long long live_mask = __ballot(live), bad_mask = __ballot(bad);
        if (tid == 0) s_live = live_mask;
        n_skipped += __popcll(bad_mask);
      }
      __syncthreads();
      unsigned long long m = s_live;
      while (m) {                                                  // uniform: ascending rows, so later rows win
        const int k = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int x_lo = s_bound[k][0], x_hi = s_bound[k][1], y_lo = s_bound[k][2], y_hi = s_bound[k][3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int px2 = 2 * p_x[i] + 1, py2 = 2 * p_y[i] + 1;
          if (local[i] && px2 >= x_lo && px2 <= x_hi && py2 >= y_lo && py2 <= y_hi && box_hits(s_corner[k], px2, py2, line2))
            rgb[i] = s_rgb[k];
        }
      }
    }
    // pixels of a quad that ran past its row: their scan's table from memory, in row order
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (valid[i] && !local[i]) {
        int64_t r0 = a.box_offsets[p_b[i]], r1 = a.box_offsets[p_b[i] + 1];
        r0 = r0 < 0 ? 0 : r0;
        r1 = r1 > a.num_boxes ? a.num_boxes : r1;
        const int px2 = 2 * p_x[i] + 1, py2 = 2 * p_y[i] + 1;
        for (int64_t r = r0; r < r1; ++r) {
          int32_t c[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) c[k] = a.box_corners[r * 8 + k];
          if (!corners_out_of_bound(c) && box_hits(c, px2, py2, line2)) rgb[i] = rgb3(a.box_rgb + r * 3);
        }
      }
    }
  }
  if (a.skipped && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) a.skipped[b] = n_skipped;

  if (!active) return;                                             // (after the last barrier)
  uint8_t* out = a.image + flat0 * 3;
  if (flat0 + 4 <= a.total_pixels) {
    uint32_t* out4 = reinterpret_cast<uint32_t*>(out);             // flat0 * 3 is a multiple of 12, the base is 4-byte aligned
    out4[0] = rgb[0] | (rgb[1] << 24);
    out4[1] = (rgb[1] >> 8) | (rgb[2] << 16);
    out4[2] = (rgb[2] >> 16) | (rgb[3] << 8);
  } else {                                                         // the image's last quad, when B * H * W % 4 != 0
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (valid[i]) {
        out[3 * i] = (uint8_t)rgb[i];
        out[3 * i + 1] = (uint8_t)(rgb[i] >> 8);
        out[3 * i + 2] = (uint8_t)(rgb[i] >> 16);
      }
    }
  }
}

}  // namespace

extern "C" int32_t mbv_render_box_chunk(void) { return kBoxChunk; }

extern "C" int mbv_cell_counts(const float* points, int32_t point_dim, int64_t total_points, const int32_t* scan_offsets,
                               int32_t batch, float x_min, float y_min, float z_min, float x_max, float y_max, float z_max,
                               float vx, float vy, float vz, int32_t gx, int32_t gy, int32_t gz, int32_t prefilter,
                               int32_t* counts, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (batch < 0 || total_points < 0 || (point_dim != 3 && point_dim != 4) || gx <= 0 || gy <= 0 || gz <= 0)
    return MBV_ERR_BAD_ARG;
  if (batch > 65535 || total_points >= 0x7FFFFFFFll || gx > 65536 || gy > 65536) return MBV_ERR_UNSUPPORTED;
  if (batch == 0) return MBV_OK;
  if (!counts || (total_points > 0 && (!points || !scan_offsets))) return MBV_ERR_BAD_ARG;
  const int64_t cells = (int64_t)batch * gy * gx;
  int64_t zero_blocks = (cells + kThreads - 1) / kThreads;
  zero_blocks = zero_blocks > 4096 ? 4096 : zero_blocks;
  hipLaunchKernelGGL(k_counts_zero, dim3((unsigned)zero_blocks), dim3(kThreads), 0, stream, cells, counts);
  MBV_CHECK_LAUNCH();
  if (total_points > 0) {
    const LiftGeom g{x_min, y_min, z_min, x_max, y_max, z_max, vx, vy, vz, gx, gy, gz};
    // the y dimension of the grid walks the scans; x covers the longest scan (blocks past a scan's end exit at once)
    hipLaunchKernelGGL(k_count_points, dim3((unsigned)((total_points + kThreads - 1) / kThreads), batch), dim3(kThreads), 0,
                       stream, points, (int)point_dim, total_points, scan_offsets, g, (int)prefilter, counts);
    MBV_CHECK_LAUNCH();
  }
  return MBV_OK;
}

extern "C" int mbv_render_bev(int32_t batch, int32_t gx, int32_t gy, int32_t scale, int32_t flip_rows, const int32_t* counts,
                              const uint8_t* density_lut, const int32_t* instance_map, int32_t num_queries,
                              const int32_t* id_table, const uint8_t* palette, int32_t palette_size, int32_t alpha,
                              uint32_t untracked_rgb, const int32_t* gt_map, int32_t gt_background,
                              uint32_t gt_rgb, const int32_t* box_corners, const uint8_t* box_rgb,
                              const int32_t* box_offsets, int64_t num_boxes, int32_t line, uint8_t* image, int32_t* skipped,
                              void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (batch < 0 || gx <= 0 || gy <= 0 || scale < 1 || scale > kMaxScale || num_boxes < 0) return MBV_ERR_BAD_ARG;
  if ((int64_t)gx * scale > kMaxSide || (int64_t)gy * scale > kMaxSide || batch > 65535) return MBV_ERR_UNSUPPORTED;
  if (batch == 0) return MBV_OK;
  if (!image || (reinterpret_cast<uintptr_t>(image) & 3)) return MBV_ERR_BAD_ARG;
  if (counts && !density_lut) return MBV_ERR_BAD_ARG;
  if (instance_map && (!palette || palette_size < 1 || num_queries < 0 || alpha < 0 || alpha > 256)) return MBV_ERR_BAD_ARG;
  if (box_corners && (!box_rgb || !box_offsets || line < 1 || line > kMaxLine)) return MBV_ERR_BAD_ARG;
  if (num_boxes >= 0x7FFFFFFFll) return MBV_ERR_UNSUPPORTED;
  RenderArgs a;
  a.counts = counts;
  a.density_lut = density_lut;
  a.instance_map = instance_map;
  a.id_table = id_table;
  a.palette = palette;
  a.gt_map = gt_map;
  a.box_corners = num_boxes > 0 ? box_corners : nullptr;
  a.box_rgb = box_rgb;
  a.box_offsets = box_offsets;
  a.image = image;
  a.skipped = skipped;
  a.num_boxes = num_boxes;
  a.batch = batch;
  a.gx = gx;
  a.gy = gy;
  a.scale = scale;
  a.H = gy * scale;
  a.W = gx * scale;
  a.total_pixels = (int64_t)batch * a.H * a.W;
  a.num_queries = num_queries;
  a.palette_size = palette_size;
  a.alpha = alpha;
  a.gt_background = gt_background;
  a.line = line;
  a.flip = flip_rows ? 1 : 0;
  a.untracked_rgb = untracked_rgb & 0xffffffu;
  a.gt_rgb = gt_rgb & 0xffffffu;
  const int quads_per_row = (a.W + 3) / 4;
  const dim3 grid((unsigned)((quads_per_row + kTileQuads - 1) / kTileQuads), (unsigned)((a.H + kTileRows - 1) / kTileRows),
                  (unsigned)batch);
  hipLaunchKernelGGL(k_render_bev, grid, dim3(kThreads), 0, stream, a);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
