// K22 — SemanticKITTI scene -> instance-id map on the device (the input of K14).
//
// Replaces SemanticKittiRasterizer.get_mask_around
//   mask_bev/datasets/semantic_kitti/semantic_kitti_rasterizer.py:41-94
// (numpy over the whole aggregated scene + one cv2.morphologyEx pair per instance on a full-size image, 0.5 s and
// more per scan on the host, hence the reference's `.npy` mask cache).
//
// K22a, binning.  The label stream is what is read at full width (int4 per lane); a point's coordinates are loaded only
// when its label is non-zero (a few per cent of a scene), and the f64 transform, the strict range test and the floor
// division run behind that test.
//   k_centre_count   remove_unseen: labels of the centre scan counted per id (integer atomics on a 120 k-point scan)
//   k_stream<.., 0>  otherwise: presence flag of every id with a kept point (plain stores of 1, no atomics)
//   k_scan_table     65 536-entry table: flag / count -> slot, prefix scan in ascending id order (slot order = id order)
//   k_clear_occ      zeroes the bit images of the slots in use
//   k_stream<.., 1>  kept point -> atomicOr of its cell bit into its slot's image; the cell bounding box is widened by
//                    atomicMin / Max only when the cell lies outside the box read first (rare after the first points)
// K34, binning for a whole batch on a scene bank that stays on the device (mbv_rasterize_bank): the same stages on
// sample-major tables, launches independent of the batch size and of the number of scans.
//   k_bank_centre_count / k_bank_stream<0>   as above per sample; one workgroup per host-made chunk of one scan's points
//   k_scan_table, k_clear_occ                sample = blockIdx.y
//   k_bank_stream<1>                         occupancy bits only, the bit read before the atomic
//   k_occ_bbox                               cell bounding boxes read off the finished images
// K22b, morphology + paint.
//   k_morph_paint    one workgroup per slot.  The window (bounding box grown by 2 * (k / 2) cells, clipped to the grid)
//                    is loaded into LDS as bits, rows = ix, 32 cells of iy per word.  close = dilate, erode and
//                    open = erode, dilate run as eight separable passes ping-ponging between two LDS images: along iy by
//                    shifted ORs / ANDs with the carries of the neighbouring words, along ix by word-wise OR / AND over
//                    k rows.  The set bits are painted with atomicMax on the id: THE HIGHEST ID WINS an overlap.
//                    A window above 8192 words (32 KB) is processed in row bands with a halo of 4 * (k / 2) rows (all
//                    four operations run on a band without a round trip through memory, so the halo is twice that of
//                    one closing): correct, not tuned.
// Border rule (cv2 BORDER_CONSTANT + morphologyDefaultBorderValue): a cell outside the GRID is the identity of the
// operation (set for an erosion, clear for a dilation), i.e. it is skipped; a cell inside the grid but outside the
// window is clear — which it truly is at every stage: every intermediate image lies inside the box grown by k / 2.
#include <limits.h>

#include "common.hpp"

namespace {

constexpr int kIds = 65536;          // SemanticKITTI instance ids are 16 bits
constexpr int kImgWords = 8192;      // words of one LDS bit image; two of them = 64 KB
constexpr int kMorphThreads = 512;

struct Geom {
  double x0, x1, y0, y1, z0, z1, vs;
  int nx, ny, wpr;                   // wpr = words per row of a bit image
};

template <typename T, bool F4>
__device__ __forceinline__ void load_xyz(const T* __restrict__ pts, int stride, int64_t i, double& x, double& y, double& z) {
  if constexpr (F4) {                // f32, stride 4: what a .bin holds, one 16-byte load
    const float4 v = reinterpret_cast<const float4*>(pts)[i];
    x = v.x; y = v.y; z = v.z;
  } else {
    const T* p = pts + i * stride;
    x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
  }
}

// the cell of the point (px, py, pz) of a scan with the transform m, false when the point is not kept (:53-68)
__device__ __forceinline__ bool cell_of(const double* __restrict__ m, double px, double py, double pz, const Geom& g,
                                        int& ix, int& iy) {
  const double x = m[0] * px + m[1] * py + m[2] * pz + m[3];
  const double y = m[4] * px + m[5] * py + m[6] * pz + m[7];
  const double z = m[8] * px + m[9] * py + m[10] * pz + m[11];
  if (!(g.x0 < x && x < g.x1 && g.y0 < y && y < g.y1 && g.z0 < z && z < g.z1)) return false;   // NaN fails every test
  const double fx = floor((x - g.x0) / g.vs), fy = floor((y - g.y0) / g.vs);
  if (!(fx < (double)g.nx && fy < (double)g.ny)) return false;
  ix = (int)fx;
  iy = (int)fy;
  return true;
}

// the cell of point i, false when the point is not kept
template <typename T, bool F4>
__device__ __forceinline__ bool point_cell(const T* __restrict__ pts, int stride, int64_t i,
                                           const int32_t* __restrict__ offs, int n_scans,
                                           const double* __restrict__ tf, const Geom& g, int& ix, int& iy) {
  int lo = 0, hi = n_scans - 1;      // the scan that owns point i: the last s with offs[s] <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)offs[mid] <= i) lo = mid; else hi = mid - 1;
  }
  double px, py, pz;
  load_xyz<T, F4>(pts, stride, i, px, py, pz);
  return cell_of(tf + (int64_t)lo * 16, px, py, pz, g, ix, iy);
}

// MODE 0: table[id] = 1 for every id with a kept point.  MODE 1: table = id -> slot; occupancy bits + bounding boxes.
template <typename T, bool F4, int MODE>
__global__ void __launch_bounds__(256) k_stream(const T* __restrict__ pts, int stride, const int32_t* __restrict__ inst,
                                                int64_t n, const int32_t* __restrict__ offs, int n_scans,
                                                const double* __restrict__ tf, Geom g, int32_t* __restrict__ table,
                                                uint32_t* __restrict__ occ, int32_t* __restrict__ bbox,
                                                int32_t* __restrict__ status) {
  const int64_t quads = (n + 3) / 4;
  const int64_t words_per_slot = (int64_t)g.nx * g.wpr;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    const int64_t base = q * 4;
    int32_t id[4] = {0, 0, 0, 0};
    if (base + 4 <= n) {
      const int4 v = reinterpret_cast<const int4*>(inst)[q];
      id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
    } else {
      for (int j = 0; j < 4; ++j) if (base + j < n) id[j] = inst[base + j];
    }
    if ((id[0] | id[1] | id[2] | id[3]) == 0) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (id[j] == 0) continue;
      if ((uint32_t)id[j] >= (uint32_t)kIds) { atomicOr(status, 2); continue; }
      int ix, iy;
      if (!point_cell<T, F4>(pts, stride, base + j, offs, n_scans, tf, g, ix, iy)) continue;
      if (MODE == 0) {
        table[id[j]] = 1;
      } else {
        const int slot = table[id[j]];
        if (slot < 0) continue;
        atomicOr(occ + slot * words_per_slot + (int64_t)ix * g.wpr + (iy >> 5), 1u << (iy & 31));
        int32_t* bb = bbox + slot * 4;
        if (ix < bb[0]) atomicMin(bb + 0, ix);
        if (iy < bb[1]) atomicMin(bb + 1, iy);
        if (ix > bb[2]) atomicMax(bb + 2, ix);
        if (iy > bb[3]) atomicMax(bb + 3, iy);
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_centre_count(const int32_t* __restrict__ inst, int64_t n,
                                                      int32_t* __restrict__ table, int32_t* __restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int32_t id = inst[i];
    if (id == 0) continue;
    if ((uint32_t)id >= (uint32_t)kIds) { atomicOr(status, 2); continue; }
    atomicAdd(table + id, 1);
  }
}

// K34: the scene bank read in place.  One workgroup per chunk = (segment, first point inside it, sample): every point of
// a workgroup has one transform, read through uniform loads.  Points are taken four at a time at bank indices that are
// multiples of 4, so the labels come as one int4 and the coordinates as three float4 whatever the segment's first point
// is; the points of a quad outside [begin, end) are masked.  Both tables come from the host, so every index is checked.
struct BankTables {
  const float* pts;                  // (n_bank, 3)
  const int32_t* inst;               // (n_bank)
  int64_t n_bank;
  const int64_t* seg_start;
  const int32_t* seg_count;
  int n_seg;
  const double* tf;                  // (n_seg, 4, 4)
  const int4* chunks;                // (n_chunks): segment, first point inside the segment, sample, unused
  int chunk_points;
  const int64_t* centre_start;
  const int32_t* centre_count;
  int batch, max_instances;
};

// MODE as in k_stream, on sample-major tables; MODE 0 skips the samples whose centre scan names the instances.  MODE 1 sets
// occupancy bits only: with every point of a bank labelled, widening four box words per instance by atomics from millions
// of points is what the pass would wait for, so k_occ_bbox reads the boxes off the finished images instead.
template <int MODE>
__global__ void __launch_bounds__(256) k_bank_stream(BankTables t, Geom g, int32_t* __restrict__ tables,
                                                     uint32_t* __restrict__ occ, int32_t* __restrict__ status) {
  const int4 c = t.chunks[blockIdx.x];
  const int seg = c.x, sample = c.z;
  if ((uint32_t)seg >= (uint32_t)t.n_seg || (uint32_t)sample >= (uint32_t)t.batch || c.y < 0) return;
  if (MODE == 0 && t.centre_count[sample] >= 0) return;
  const int64_t s0 = t.seg_start[seg];
  const int32_t cnt = t.seg_count[seg];
  if (s0 < 0 || s0 > t.n_bank || cnt <= c.y) return;
  const int64_t begin = s0 + c.y;
  const int64_t len = cnt - c.y < t.chunk_points ? cnt - c.y : t.chunk_points;
  const int64_t end = begin + len < t.n_bank ? begin + len : t.n_bank;
  double m[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) m[j] = t.tf[(int64_t)seg * 16 + j];
  const int64_t words_per_slot = (int64_t)g.nx * g.wpr;
  int32_t* table = tables + (int64_t)sample * kIds;
  uint32_t* socc = occ + (int64_t)sample * t.max_instances * words_per_slot;
  for (int64_t q = (begin >> 2) + threadIdx.x; q * 4 < end; q += 256) {
    const int64_t base = q * 4;
    int32_t id[4] = {0, 0, 0, 0};
    float xyz[12];
    if (base + 4 <= t.n_bank) {
      const int4 v = reinterpret_cast<const int4*>(t.inst)[q];
      id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
      const float4* p = reinterpret_cast<const float4*>(t.pts) + q * 3;
      const float4 a = p[0], b = p[1], d = p[2];
      xyz[0] = a.x; xyz[1] = a.y; xyz[2] = a.z; xyz[3] = a.w; xyz[4] = b.x; xyz[5] = b.y; xyz[6] = b.z; xyz[7] = b.w;
      xyz[8] = d.x; xyz[9] = d.y; xyz[10] = d.z; xyz[11] = d.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = base + j < t.n_bank;
        id[j] = in ? t.inst[base + j] : 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) xyz[j * 3 + e] = in ? t.pts[(base + j) * 3 + e] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (base + j < begin || base + j >= end || id[j] == 0) continue;
      if ((uint32_t)id[j] >= (uint32_t)kIds) { atomicOr(status + sample, 2); continue; }
      // A bank holds labelled points only, hundreds on every cell of an instance: what is already known is read first (a
      // flag or bit only ever gets set during a pass, so a stale 0 costs one redundant store or atomic and nothing else).
      const int known = __atomic_load_n(table + id[j], __ATOMIC_RELAXED);    // MODE 0: the flag, MODE 1: the slot
      if (MODE == 0 ? known != 0 : known < 0) continue;
      int ix, iy;
      if (!cell_of(m, (double)xyz[j * 3], (double)xyz[j * 3 + 1], (double)xyz[j * 3 + 2], g, ix, iy)) continue;
      if (MODE == 0) {
        table[id[j]] = 1;
      } else {
        const uint32_t* word = socc + known * words_per_slot + (int64_t)ix * g.wpr + (iy >> 5);
        if (__atomic_load_n(word, __ATOMIC_RELAXED) & (1u << (iy & 31))) continue;
        atomicOr(socc + known * words_per_slot + (int64_t)ix * g.wpr + (iy >> 5), 1u << (iy & 31));
      }
    }
  }
}

// the inclusive cell bounds of the set bits of slot blockIdx.x of sample blockIdx.y (gridDim.x slots a sample): exactly what
// k_stream's atomicMin / Max leave, (INT_MAX, INT_MAX, -1, -1) for an empty image
__global__ void __launch_bounds__(256) k_occ_bbox(const uint32_t* __restrict__ occ, const int32_t* __restrict__ n_slots,
                                                  int nx, int wpr, int32_t* __restrict__ bbox) {
  __shared__ int bb[4];
  const int slot = blockIdx.x, sample = blockIdx.y;
  if (slot >= n_slots[sample]) return;
  const int64_t first = (int64_t)sample * gridDim.x + slot;
  const uint32_t* img = occ + first * nx * wpr;
  if (threadIdx.x == 0) { bb[0] = INT_MAX; bb[1] = INT_MAX; bb[2] = -1; bb[3] = -1; }
  __syncthreads();
  int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
  for (int i = threadIdx.x; i < nx * wpr; i += 256) {
    const uint32_t v = img[i];
    if (!v) continue;
    const int r = i / wpr, w = i - r * wpr;
    x0 = min(x0, r); x1 = max(x1, r);
    y0 = min(y0, w * 32 + __ffs((int)v) - 1); y1 = max(y1, w * 32 + 31 - __clz((int)v));
  }
  if (x1 >= 0) { atomicMin(&bb[0], x0); atomicMin(&bb[1], y0); atomicMax(&bb[2], x1); atomicMax(&bb[3], y1); }
  __syncthreads();
  if (threadIdx.x < 4) bbox[first * 4 + threadIdx.x] = bb[threadIdx.x];
}

// remove_unseen: the labels of sample blockIdx.y's centre scan counted per id, in the sample's table
__global__ void __launch_bounds__(256) k_bank_centre_count(BankTables t, int32_t* __restrict__ tables,
                                                           int32_t* __restrict__ status) {
  const int sample = blockIdx.y;
  const int64_t n = t.centre_count[sample], s0 = t.centre_start[sample];
  if (n <= 0 || s0 < 0 || s0 > t.n_bank) return;
  const int64_t end = s0 + n < t.n_bank ? s0 + n : t.n_bank;
  int32_t* table = tables + (int64_t)sample * kIds;
  for (int64_t i = s0 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
    const int32_t id = t.inst[i];
    if (id == 0) continue;
    if ((uint32_t)id >= (uint32_t)kIds) { atomicOr(status + sample, 2); continue; }
    atomicAdd(table + id, 1);
  }
}

// table[id] (a flag or a count) >= threshold -> slot (ascending id order), everything else -> -1.  Sample blockIdx.y of
// sample-major tables; `centre_count` (null: `threshold` for every sample) < 0 for a sample makes its threshold 1.
__global__ void __launch_bounds__(1024) k_scan_table(int32_t* __restrict__ table, int threshold,
                                                     const int32_t* __restrict__ centre_count, int max_instances,
                                                     int32_t* __restrict__ slot_ids, int32_t* __restrict__ bbox,
                                                     int32_t* __restrict__ n_slots, int32_t* __restrict__ status) {
  __shared__ int wave_total[16];
  constexpr int kPer = kIds / 1024;
  const int sample = blockIdx.y;
  if (centre_count && centre_count[sample] < 0) threshold = 1;
  table += (int64_t)sample * kIds;
  slot_ids += (int64_t)sample * max_instances;
  bbox += (int64_t)sample * max_instances * 4;
  n_slots += sample;
  status += sample;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // the thread's kPer = 64 entries are 16 int4 (the table is 256-byte aligned): all in flight at once, kept as one bit each
  static_assert(kPer == 64, "one presence bit per entry in a 64-bit word");
  int4* mine4 = reinterpret_cast<int4*>(table + t * kPer);
  uint64_t present = 0;
#pragma unroll
  for (int q = 0; q < kPer / 4; ++q) {
    const int4 v = mine4[q];
    present |= (uint64_t)(v.x >= threshold) << (q * 4) | (uint64_t)(v.y >= threshold) << (q * 4 + 1) |
               (uint64_t)(v.z >= threshold) << (q * 4 + 2) | (uint64_t)(v.w >= threshold) << (q * 4 + 3);
  }
  if (t == 0) present &= ~(uint64_t)1;               // id 0 is no instance
  const int mine = __popcll(present);
  int incl = mine;                                   // inclusive scan inside the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < 16; ++w) {
    if (w < wave) before += wave_total[w];
    total += wave_total[w];
  }
  int slot = before + incl - mine;
#pragma unroll
  for (int q = 0; q < kPer / 4; ++q) {
    int s4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = q * 4 + e, id = t * kPer + j;
      int s = -1;
      if ((present >> j) & 1) {
        if (slot < max_instances) {
          s = slot;
          slot_ids[s] = id;
          bbox[s * 4 + 0] = INT_MAX; bbox[s * 4 + 1] = INT_MAX; bbox[s * 4 + 2] = -1; bbox[s * 4 + 3] = -1;
        }
        ++slot;
      }
      s4[e] = s;
    }
    mine4[q] = make_int4(s4[0], s4[1], s4[2], s4[3]);
  }
  if (t == 0) {
    n_slots[0] = total < max_instances ? total : max_instances;
    if (total > max_instances) atomicOr(status, 1);
  }
}

// sample blockIdx.y: its images start `sample_words` after the previous sample's
__global__ void __launch_bounds__(256) k_clear_occ(uint32_t* __restrict__ occ, const int32_t* __restrict__ n_slots,
                                                   int64_t words_per_slot, int64_t sample_words) {
  const int64_t total = (int64_t)n_slots[blockIdx.y] * words_per_slot;
  occ += blockIdx.y * sample_words;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) occ[i] = 0u;
}

// One separable pass over a band image of `rows` x `wd` words.  Image row 0 is grid row `ir0`, image word 0 is grid word
// `w0`; `tail` = the in-grid bits of the grid's last word (wpr - 1).
template <bool ERODE, bool ALONG_BITS>
__device__ __forceinline__ void morph_pass(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int rows, int wd,
                                           int h, int ir0, int nx, int w0, int wpr, uint32_t tail) {
  const int n = rows * wd;
  for (int i = threadIdx.x; i < n; i += kMorphThreads) {
    const int r = i / wd, w = i - r * wd;
    uint32_t cur = src[i], acc;
    if (ALONG_BITS) {
      const int gw = w0 + w;
      const uint32_t outside = ERODE ? 0xffffffffu : 0u;          // beyond the grid: the identity of the operation
      uint32_t prev = w > 0 ? src[i - 1] : (gw == 0 ? outside : 0u);
      uint32_t next = w + 1 < wd ? src[i + 1] : (gw == wpr - 1 ? outside : 0u);
      if (ERODE) {
        if (gw == wpr - 1) cur |= ~tail;
        if (gw + 1 == wpr - 1) next |= ~tail;
      }
      acc = cur;
      for (int d = 1; d <= h; ++d) {
        const uint32_t a = (cur << d) | (prev >> (32 - d));      // cell c takes cell c - d
        const uint32_t b = (cur >> d) | (next << (32 - d));      // cell c takes cell c + d
        acc = ERODE ? (acc & a & b) : (acc | a | b);
      }
      if (gw == wpr - 1) acc &= tail;
    } else {
      acc = cur;
      for (int dr = -h; dr <= h; ++dr) {
        const int rr = r + dr, gr = ir0 + rr;
        if (dr == 0 || gr < 0 || gr >= nx) continue;             // beyond the grid: skipped
        const uint32_t v = (rr >= 0 && rr < rows) ? src[rr * wd + w] : 0u;
        acc = ERODE ? (acc & v) : (acc | v);
      }
    }
    dst[i] = acc;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kMorphThreads) k_morph_paint(const uint32_t* __restrict__ occ,
                                                               const int32_t* __restrict__ bbox,
                                                               const int32_t* __restrict__ slot_ids,
                                                               const int32_t* __restrict__ n_slots, int nx, int ny, int k,
                                                               int32_t* __restrict__ map) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_img[];      // two images of kImgWords
  const int slot = blockIdx.x;
  {                                  // sample blockIdx.y of sample-major tables of gridDim.x slots each
    const int64_t first = (int64_t)blockIdx.y * gridDim.x;
    n_slots += blockIdx.y;
    bbox += first * 4;
    slot_ids += first;
    occ += first * nx * ((ny + 31) >> 5);
    map += (int64_t)blockIdx.y * nx * ny;
  }
  if (slot >= n_slots[0]) return;
  const int xmin = bbox[slot * 4 + 0], ymin = bbox[slot * 4 + 1], xmax = bbox[slot * 4 + 2], ymax = bbox[slot * 4 + 3];
  if (xmax < 0 || ymax < 0 || xmin > xmax || ymin > ymax || xmin < 0 || ymin < 0 || xmax >= nx || ymax >= ny) return;
  const int32_t id = slot_ids[slot];
  const int h = k >> 1, wpr = (ny + 31) >> 5;
  const uint32_t tail = (ny & 31) ? ((1u << (ny & 31)) - 1u) : 0xffffffffu;
  const int r0 = max(xmin - 2 * h, 0), r1 = min(xmax + 2 * h, nx - 1);
  const int w0 = max(ymin - 2 * h, 0) >> 5, w1 = min(ymax + 2 * h, ny - 1) >> 5;
  const int wd = w1 - w0 + 1, cap = kImgWords / wd;
  const int band = (r1 - r0 + 1 <= cap) ? (r1 - r0 + 1) : (cap - 8 * h);   // output rows per band (host: cap - 8h >= 1)
  const uint32_t* img = occ + (int64_t)slot * nx * wpr;
  uint32_t* A = lds_img;
  uint32_t* B = lds_img + kImgWords;
  for (int o0 = r0; o0 <= r1; o0 += band) {
    const int o1 = min(o0 + band - 1, r1);
    const int ir0 = max(o0 - 4 * h, r0), ir1 = min(o1 + 4 * h, r1), rows = ir1 - ir0 + 1;
    for (int i = threadIdx.x; i < rows * wd; i += kMorphThreads) {
      const int r = i / wd, w = i - r * wd;
      A[i] = img[(int64_t)(ir0 + r) * wpr + w0 + w];
    }
    __syncthreads();
    morph_pass<false, true>(A, B, rows, wd, h, ir0, nx, w0, wpr, tail);    // close: dilate ...
    morph_pass<false, false>(B, A, rows, wd, h, ir0, nx, w0, wpr, tail);
    morph_pass<true, true>(A, B, rows, wd, h, ir0, nx, w0, wpr, tail);     // ... erode
    morph_pass<true, false>(B, A, rows, wd, h, ir0, nx, w0, wpr, tail);
    morph_pass<true, true>(A, B, rows, wd, h, ir0, nx, w0, wpr, tail);     // open: erode ...
    morph_pass<true, false>(B, A, rows, wd, h, ir0, nx, w0, wpr, tail);
    morph_pass<false, true>(A, B, rows, wd, h, ir0, nx, w0, wpr, tail);    // ... dilate
    morph_pass<false, false>(B, A, rows, wd, h, ir0, nx, w0, wpr, tail);
    const int out_rows = o1 - o0 + 1;
    for (int i = threadIdx.x; i < out_rows * wd; i += kMorphThreads) {
      const int r = i / wd, w = i - r * wd;
      uint32_t bits = A[(o0 - ir0 + r) * wd + w];
      if (w0 + w == wpr - 1) bits &= tail;
      int32_t* row = map + (int64_t)(o0 + r) * ny + (w0 + w) * 32;          // bits at iy >= ny are clear
      while (bits) {
        const int b = __ffs((int)bits) - 1;
        bits &= bits - 1;
        atomicMax(row + b, id);
      }
    }
    __syncthreads();
  }
}

struct Workspace {
  int32_t* table;
  int32_t* n_slots;
  int32_t* slot_ids;
  int32_t* bbox;
  uint32_t* occ;
  size_t bytes;
};

// `batch` samples: every table sample-major
Workspace carve(void* base, int nx, int ny, int max_instances, int batch = 1) {
  MbvCarver c(base);
  Workspace w;
  w.table = c.take<int32_t>((size_t)batch * kIds);
  w.n_slots = c.take<int32_t>((size_t)batch);
  w.slot_ids = c.take<int32_t>((size_t)batch * max_instances);
  w.bbox = c.take<int32_t>((size_t)batch * max_instances * 4);
  w.occ = c.take<uint32_t>((size_t)batch * max_instances * nx * ((ny + 31) / 32));
  w.bytes = c.off;
  return w;
}

bool geometry_ok(int nx, int ny) { return nx > 0 && ny > 0 && (int64_t)nx * ny <= (int64_t)1 << 26; }
bool kernel_ok(int k) { return k >= 1 && k <= 31 && (k & 1); }
// a row band of the widest window must hold its halo and at least one output row
bool band_ok(int ny, int k) { return kImgWords / ((ny + 31) / 32) - 8 * (k / 2) >= 1; }

int launch_paint(const uint32_t* occ, const int32_t* bbox, const int32_t* slot_ids, const int32_t* n_slots,
                 int n_slots_max, int nx, int ny, int k, int32_t* map, hipStream_t stream, int batch = 1) {
  MBV_CHECK_HIP(mbv_fill_async(map, 0, sizeof(int32_t) * (size_t)nx * ny * batch, stream));
  hipLaunchKernelGGL(k_morph_paint, dim3(n_slots_max, batch), dim3(kMorphThreads), 2 * kImgWords * sizeof(uint32_t), stream,
                     occ, bbox, slot_ids, n_slots, nx, ny, k, map);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

template <typename T, bool F4, int MODE>
int launch_stream(const void* pts, int stride, const int32_t* inst, int64_t n, const int32_t* offs, int n_scans,
                  const double* tf, const Geom& g, const Workspace& w, int32_t* status, hipStream_t stream) {
  const int64_t quads = (n + 3) / 4;
  const unsigned blocks = (unsigned)((quads + 255) / 256 < 2048 ? (quads + 255) / 256 : 2048);
  hipLaunchKernelGGL((k_stream<T, F4, MODE>), dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const T*>(pts), stride,
                     inst, n, offs, n_scans, tf, g, w.table, w.occ, w.bbox, status);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

template <int MODE>
int dispatch_stream(const void* pts, int f64, int stride, const int32_t* inst, int64_t n, const int32_t* offs,
                    int n_scans, const double* tf, const Geom& g, const Workspace& w, int32_t* status,
                    hipStream_t stream) {
  if (f64) return launch_stream<double, false, MODE>(pts, stride, inst, n, offs, n_scans, tf, g, w, status, stream);
  if (stride == 4 && (reinterpret_cast<uintptr_t>(pts) & 15) == 0)
    return launch_stream<float, true, MODE>(pts, stride, inst, n, offs, n_scans, tf, g, w, status, stream);
  return launch_stream<float, false, MODE>(pts, stride, inst, n, offs, n_scans, tf, g, w, status, stream);
}

}  // namespace

extern "C" size_t mbv_rasterize_workspace_bytes(int32_t nx, int32_t ny, int32_t max_instances) {
  if (!geometry_ok(nx, ny) || max_instances < 1 || max_instances >= kIds) return 0;
  return carve(nullptr, nx, ny, max_instances).bytes;
}

extern "C" int mbv_rasterize(const void* points, int32_t points_f64, int32_t stride, const int32_t* inst, int64_t n_points,
                             const int32_t* scan_offsets, int32_t n_scans, const double* transforms,
                             const int32_t* centre_inst, int64_t n_centre, double x_lo, double x_hi, double y_lo,
                             double y_hi, double z_lo, double z_hi, double voxel_size, int32_t nx, int32_t ny,
                             int32_t morph_kernel, int32_t min_points, int32_t max_instances, int32_t phases,
                             int32_t* instance_map, int32_t* status, void* workspace, size_t workspace_bytes,
                             void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!geometry_ok(nx, ny) || !kernel_ok(morph_kernel) || max_instances < 1 || max_instances >= kIds ||
      n_points < 0 || n_points > INT_MAX || (stride != 3 && stride != 4) || !(voxel_size > 0.0) ||
      (phases & ~3) || phases == 0)
    return MBV_ERR_BAD_ARG;
  if (!band_ok(ny, morph_kernel)) return MBV_ERR_UNSUPPORTED;
  if (!workspace || !status || ((phases & 2) && !instance_map)) return MBV_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) || (reinterpret_cast<uintptr_t>(inst) & 15)) return MBV_ERR_BAD_ARG;
  const Workspace w = carve(workspace, nx, ny, max_instances);
  if (workspace_bytes < w.bytes) return MBV_ERR_WORKSPACE;
  if (phases & 1) {
    if (n_points > 0 && (!points || !inst || !scan_offsets || !transforms || n_scans < 1)) return MBV_ERR_BAD_ARG;
    if (n_centre > 0 && !centre_inst) return MBV_ERR_BAD_ARG;
    Geom g;
    g.x0 = x_lo; g.x1 = x_hi; g.y0 = y_lo; g.y1 = y_hi; g.z0 = z_lo; g.z1 = z_hi; g.vs = voxel_size;
    g.nx = nx; g.ny = ny; g.wpr = (ny + 31) / 32;
    MBV_CHECK_HIP(mbv_fill_async(status, 0, sizeof(int32_t), stream));
    MBV_CHECK_HIP(mbv_fill_async(w.table, 0, sizeof(int32_t) * kIds, stream));
    int threshold = 1;
    if (n_centre >= 0) {                                          // remove_unseen: the centre scan names the instances
      threshold = min_points > 1 ? min_points : 1;
      if (n_centre > 0) {
        const unsigned blocks = (unsigned)((n_centre + 255) / 256 < 2048 ? (n_centre + 255) / 256 : 2048);
        hipLaunchKernelGGL(k_centre_count, dim3(blocks), dim3(256), 0, stream, centre_inst, n_centre, w.table, status);
        MBV_CHECK_LAUNCH();
      }
    } else if (n_points > 0) {
      const int rc = dispatch_stream<0>(points, points_f64, stride, inst, n_points, scan_offsets, n_scans, transforms, g,
                                        w, status, stream);
      if (rc != MBV_OK) return rc;
    }
    hipLaunchKernelGGL(k_scan_table, dim3(1), dim3(1024), 0, stream, w.table, threshold, (const int32_t*)nullptr,
                       max_instances, w.slot_ids, w.bbox, w.n_slots, status);
    MBV_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_clear_occ, dim3(1024), dim3(256), 0, stream, w.occ, w.n_slots, (int64_t)nx * g.wpr, (int64_t)0);
    MBV_CHECK_LAUNCH();
    if (n_points > 0) {
      const int rc = dispatch_stream<1>(points, points_f64, stride, inst, n_points, scan_offsets, n_scans, transforms, g,
                                        w, status, stream);
      if (rc != MBV_OK) return rc;
    }
  }
  if (phases & 2)
    return launch_paint(w.occ, w.bbox, w.slot_ids, w.n_slots, max_instances, nx, ny, morph_kernel, instance_map, stream);
  return MBV_OK;
}

extern "C" int mbv_rasterize_paint(const uint32_t* occupancy, const int32_t* bbox, const int32_t* slot_ids,
                                   const int32_t* n_slots, int32_t n_slots_max, int32_t nx, int32_t ny,
                                   int32_t morph_kernel, int32_t* instance_map, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!geometry_ok(nx, ny) || !kernel_ok(morph_kernel) || n_slots_max < 1 || n_slots_max >= kIds) return MBV_ERR_BAD_ARG;
  if (!band_ok(ny, morph_kernel)) return MBV_ERR_UNSUPPORTED;
  if (!occupancy || !bbox || !slot_ids || !n_slots || !instance_map) return MBV_ERR_BAD_ARG;
  return launch_paint(occupancy, bbox, slot_ids, n_slots, n_slots_max, nx, ny, morph_kernel, instance_map, stream);
}

extern "C" size_t mbv_rasterize_bank_workspace_bytes(int32_t batch, int32_t nx, int32_t ny, int32_t max_instances) {
  if (batch < 1 || batch > 65535 || !geometry_ok(nx, ny) || max_instances < 1 || max_instances >= kIds) return 0;
  return carve(nullptr, nx, ny, max_instances, batch).bytes;
}

extern "C" int mbv_rasterize_bank(const float* points, const int32_t* inst, int64_t n_bank, const int64_t* seg_start,
                                  const int32_t* seg_count, int32_t n_seg, const double* transforms,
                                  const int32_t* chunks, int32_t n_chunks, int32_t chunk_points,
                                  const int64_t* centre_start, const int32_t* centre_count, int32_t batch, double x_lo,
                                  double x_hi, double y_lo, double y_hi, double z_lo, double z_hi, double voxel_size,
                                  int32_t nx, int32_t ny, int32_t morph_kernel, int32_t min_points,
                                  int32_t max_instances, int32_t phases, int32_t* instance_maps, int32_t* status,
                                  void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (batch == 0) return MBV_OK;
  if (batch < 0 || batch > 65535 || !geometry_ok(nx, ny) || !kernel_ok(morph_kernel) || max_instances < 1 ||
      max_instances >= kIds || n_bank < 0 || n_seg < 0 || n_chunks < 0 || chunk_points < 4 || (chunk_points & 3) ||
      !(voxel_size > 0.0) || (phases & ~3) || phases == 0)
    return MBV_ERR_BAD_ARG;
  if (!band_ok(ny, morph_kernel)) return MBV_ERR_UNSUPPORTED;
  if (!workspace || !status || !centre_start || !centre_count || ((phases & 2) && !instance_maps))
    return MBV_ERR_BAD_ARG;
  if (n_chunks > 0 && (!points || !inst || !seg_start || !seg_count || !transforms || !chunks || n_seg < 1 || n_bank < 1))
    return MBV_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) || (reinterpret_cast<uintptr_t>(inst) & 15) ||
      (reinterpret_cast<uintptr_t>(points) & 15) || (reinterpret_cast<uintptr_t>(chunks) & 15))
    return MBV_ERR_BAD_ARG;
  const Workspace w = carve(workspace, nx, ny, max_instances, batch);
  if (workspace_bytes < w.bytes) return MBV_ERR_WORKSPACE;
  if (phases & 1) {
    Geom g;
    g.x0 = x_lo; g.x1 = x_hi; g.y0 = y_lo; g.y1 = y_hi; g.z0 = z_lo; g.z1 = z_hi; g.vs = voxel_size;
    g.nx = nx; g.ny = ny; g.wpr = (ny + 31) / 32;
    BankTables t;
    t.pts = points; t.inst = inst; t.n_bank = n_bank; t.seg_start = seg_start; t.seg_count = seg_count; t.n_seg = n_seg;
    t.tf = transforms; t.chunks = reinterpret_cast<const int4*>(chunks); t.chunk_points = chunk_points;
    t.centre_start = centre_start; t.centre_count = centre_count; t.batch = batch; t.max_instances = max_instances;
    MBV_CHECK_HIP(mbv_fill_async(status, 0, sizeof(int32_t) * (size_t)batch, stream));
    MBV_CHECK_HIP(mbv_fill_async(w.table, 0, sizeof(int32_t) * (size_t)batch * kIds, stream));
    if (inst && n_bank > 0) {                                    // remove_unseen samples; the others leave at once
      hipLaunchKernelGGL(k_bank_centre_count, dim3(16, batch), dim3(256), 0, stream, t, w.table, status);
      MBV_CHECK_LAUNCH();
    }
    if (n_chunks > 0) {
      hipLaunchKernelGGL(k_bank_stream<0>, dim3(n_chunks), dim3(256), 0, stream, t, g, w.table, w.occ, status);
      MBV_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_scan_table, dim3(1, batch), dim3(1024), 0, stream, w.table, min_points > 1 ? min_points : 1,
                       centre_count, max_instances, w.slot_ids, w.bbox, w.n_slots, status);
    MBV_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_clear_occ, dim3(256, batch), dim3(256), 0, stream, w.occ, w.n_slots, (int64_t)nx * g.wpr,
                       (int64_t)max_instances * nx * g.wpr);
    MBV_CHECK_LAUNCH();
    if (n_chunks > 0) {
      hipLaunchKernelGGL(k_bank_stream<1>, dim3(n_chunks), dim3(256), 0, stream, t, g, w.table, w.occ, status);
      MBV_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_occ_bbox, dim3(max_instances, batch), dim3(256), 0, stream, w.occ, w.n_slots, nx, g.wpr, w.bbox);
      MBV_CHECK_LAUNCH();
    }
  }
  if (phases & 2)
    return launch_paint(w.occ, w.bbox, w.slot_ids, w.n_slots, max_instances, nx, ny, morph_kernel, instance_maps, stream,
                        batch);
  return MBV_OK;
}
