// K30a — the largest 8-connected component of a bit-packed mask.
//
// The first half of what mask_to_pred (mask_bev/evaluation/kitti_eval.py:27-45) does with cv2.findContours: keep one blob of
// the mask.  The reference picks the contour by cv2.contourArea (the polygon area through the border pixels' centres), which
// cannot be restated without OpenCV; here the component with the most CELLS is kept, ties going to the component that holds
// the lowest raster index.
//
// One workgroup per listed row.  Sweep 1 finds the bounding box of the set cells.  The box is repacked ROW-ALIGNED (each box
// row starts a word, a power-of-two number of words per row) into the plane `rem`; a second plane `cur` holds the fill.  Both
// live in LDS when the box plane fits 16 KiB, in the caller's workspace otherwise (a typical car mask is a few hundred bytes).
// Pass 1: seed with the lowest set bit of rem, dilate cur by the 8-neighbourhood (word shifts with carries between
// neighbouring words, the rows above and below) under rem until a sweep adds nothing, count it, clear it from rem; seeds come
// in raster order, so "strictly larger" keeps the first of equals.  Pass 2: repack again and flood from the best seed; the
// result is scattered back into the map's unaligned layout.  A map of one component needs no pass 2: it is copied.
//
// Every loop is bounded by construction: a sweep that adds no cell ends a fill, a fill clears at least its seed from rem, the
// seed search only moves forward.  A fill sweeps only the rows its cells have reached (plus one each way), so a stray cell in
// a large box costs two short sweeps.  The fill updates cur in place: a thread may read a neighbour's word before or after
// that neighbour's update of this sweep; both are subsets of the component, and a sweep in which nobody wrote read the final
// state, so the fixed point — and with it every output — does not depend on the order.
#include <limits.h>

#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsWords = 4096;                                        // per plane: 16 KiB
enum { S_XMIN, S_XMAX, S_YMIN, S_YMAX, S_LO, S_HI, S_CHANGED, S_SEED, S_COUNT, S_SLOTS };

__device__ __forceinline__ uint32_t low_mask(int len) { return len >= 32 ? 0xffffffffu : ((1u << len) - 1u); }

// the word `wi` of a map of `npix` pixels with the bits at and beyond npix cleared
__device__ __forceinline__ uint32_t load_word(const uint32_t* __restrict__ map, int wi, int npix) {
  const int left = npix - wi * 32;
  if (left <= 0) return 0u;
  const uint32_t w = map[wi];
  return left >= 32 ? w : (w & ((1u << left) - 1u));
}

// `len` (1 .. 32) bits of the map's bit stream from pixel p on; the caller keeps p + len inside the map
__device__ __forceinline__ uint32_t stream_bits(const uint32_t* __restrict__ map, int p, int len) {
  const int wi = p >> 5, sh = p & 31;
  uint64_t v = map[wi];
  if (sh + len > 32) v |= (uint64_t)map[wi + 1] << 32;
  return (uint32_t)(v >> sh) & low_mask(len);
}

// bits c .. c + len - 1 (len 1 .. 32) of row y of a plane of 2^rwl words per row; columns outside the plane read as 0
__device__ __forceinline__ uint32_t plane_bits(const uint32_t* plane, int rwl, int y, int c, int len) {
  int skip = 0;
  if (c < 0) { skip = -c; c = 0; len -= skip; }
  const int rwp = 1 << rwl, j = c >> 5, sh = c & 31;
  if (len <= 0 || j >= rwp) return 0u;
  const uint32_t* row = plane + ((size_t)y << rwl);
  uint64_t v = row[j];
  if (j + 1 < rwp) v |= (uint64_t)row[j + 1] << 32;
  return ((uint32_t)(v >> sh) & low_mask(len)) << skip;
}

__host__ __device__ inline int ceil_log2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// rem <- the bounding box of the map, row-aligned; cur <- 0
__device__ void repack(const uint32_t* __restrict__ map, int W, int bx0, int by0, int bw, int bh, int rwl, uint32_t* rem,
                       uint32_t* cur, int t) {
  const int rwp = 1 << rwl, nplane = bh << rwl;
  for (int i = t; i < nplane; i += kThreads) {
    const int y = i >> rwl, j = i & (rwp - 1), len = min(32, bw - j * 32);
    rem[i] = len > 0 ? stream_bits(map, (by0 + y) * W + bx0 + j * 32, len) : 0u;
    cur[i] = 0u;
  }
  __syncthreads();
}

// the first non-zero word of rem at or after pos, -1 when there is none; the same value in every thread
__device__ int find_seed(const uint32_t* rem, int nplane, int pos, int* s, int t) {
  for (; pos < nplane; pos += kThreads) {                              // bounded by the plane
    if (t == 0) s[S_SEED] = INT_MAX;
    __syncthreads();
    const int i = pos + t;
    if (i < nplane && rem[i] != 0u) atomicMin(&s[S_SEED], i);
    __syncthreads();
    const int seed = s[S_SEED];
    __syncthreads();
    if (seed != INT_MAX) return seed;
  }
  return -1;
}

// cur (all 0 on entry) <- the component of rem that holds bit `bit` of word `seed`; s[S_LO] .. s[S_HI] are left as a row
// range that holds it.  Bounded: every sweep but the last adds a cell of rem to cur.
__device__ void flood(const uint32_t* rem, uint32_t* cur, int rwl, int bh, int seed, uint32_t bit, int* s, int t) {
  const int rwp = 1 << rwl, sy = seed >> rwl;
  if (t == 0) {
    cur[seed] = bit;
    s[S_LO] = max(sy - 1, 0);
    s[S_HI] = min(sy + 1, bh - 1);
    s[S_CHANGED] = 0;
    s[S_COUNT] = 0;
  }
  __syncthreads();
  for (;;) {
    const int lo = s[S_LO], hi = s[S_HI];
    __syncthreads();                                                   // everyone holds this sweep's rows
    const int nw = (hi - lo + 1) << rwl;
    int ylo = INT_MAX, yhi = -1;
    for (int i = t; i < nw; i += kThreads) {
      const int idx = (lo << rwl) + i, y = idx >> rwl, j = idx & (rwp - 1);
      const uint32_t r = rem[idx], old = cur[idx];
      if ((r & ~old) == 0u) continue;                                  // nothing left to add in this word
      const bool left = j > 0, right = j + 1 < rwp;
      uint32_t c = old, l = left ? cur[idx - 1] : 0u, g = right ? cur[idx + 1] : 0u;
      if (y > 0) {
        c |= cur[idx - rwp];
        if (left) l |= cur[idx - rwp - 1];
        if (right) g |= cur[idx - rwp + 1];
      }
      if (y + 1 < bh) {
        c |= cur[idx + rwp];
        if (left) l |= cur[idx + rwp - 1];
        if (right) g |= cur[idx + rwp + 1];
      }
      uint32_t now = old | ((c | (c << 1) | (c >> 1) | (l >> 31) | (g << 31)) & r);
      for (int k = 0; k < 31; ++k) {                                   // along the row inside the word
        const uint32_t more = now | (((now << 1) | (now >> 1)) & r);
        if (more == now) break;
        now = more;
      }
      if (now != old) {
        cur[idx] = now;
        ylo = min(ylo, y - 1);
        yhi = max(yhi, y + 1);
      }
    }
    if (yhi >= 0) {
      atomicMin(&s[S_LO], max(ylo, 0));
      atomicMax(&s[S_HI], min(yhi, bh - 1));
      s[S_CHANGED] = 1;
    }
    __syncthreads();
    const int changed = s[S_CHANGED];
    __syncthreads();
    if (!changed) break;
    if (t == 0) s[S_CHANGED] = 0;                                      // ordered before the next sweep's writes by its barrier
  }
}

__global__ void __launch_bounds__(kThreads) k_largest_component(const uint32_t* __restrict__ packed, int64_t num_maps,
                                                                int64_t words, int H, int W,
                                                                const int32_t* __restrict__ rows,
                                                                uint32_t* __restrict__ out, int32_t* __restrict__ n_out,
                                                                int32_t* __restrict__ comps_out, uint32_t* ws,
                                                                int64_t cap_words) {
  __shared__ uint32_t s_planes[2 * kLdsWords];
  __shared__ int s[S_SLOTS];
  const int r = blockIdx.x, t = threadIdx.x;
  const int64_t row = rows[r];
  const bool valid = row >= 0 && row < num_maps;                       // a row outside the table counts as an empty map
  const uint32_t* __restrict__ map = packed + (valid ? row : 0) * words;
  uint32_t* __restrict__ o = out + (int64_t)r * words;
  const int npix = valid ? H * W : 0;
  const int nwords = (npix + 31) / 32;

  // ---- sweep 1: the bounding box of the set cells
  if (t == 0) { s[S_XMIN] = INT_MAX; s[S_XMAX] = -1; s[S_YMIN] = INT_MAX; s[S_YMAX] = -1; }
  __syncthreads();
  int xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
  for (int wi = t; wi < nwords; wi += kThreads) {
    const uint32_t w = load_word(map, wi, npix);
    if (w == 0u) continue;
    const int p0 = wi * 32, end = min(p0 + 32, npix);
    int y = p0 / W, x = p0 - y * W;
    for (int p = p0; p < end;) {                                       // the word's pieces, one per image row it touches
      const int seg = min(W - x, end - p);
      const uint32_t bits = (w >> (p - p0)) & low_mask(seg);
      if (bits) {
        xmin = min(xmin, x + __ffs((int)bits) - 1);
        xmax = max(xmax, x + 31 - __clz((int)bits));
        ymin = min(ymin, y);
        ymax = max(ymax, y);
      }
      p += seg; x = 0; ++y;
    }
  }
  if (ymax >= 0) {
    atomicMin(&s[S_XMIN], xmin); atomicMax(&s[S_XMAX], xmax); atomicMin(&s[S_YMIN], ymin); atomicMax(&s[S_YMAX], ymax);
  }
  __syncthreads();
  const int bx0 = s[S_XMIN], by0 = s[S_YMIN], bw = s[S_XMAX] - bx0 + 1, bh = s[S_YMAX] - by0 + 1;
  if (s[S_YMAX] < 0) {                                                 // uniform: an empty map
    for (int64_t wi = t; wi < words; wi += kThreads) o[wi] = 0u;
    if (t == 0) { n_out[r] = 0; comps_out[r] = 0; }
    return;
  }
  const int rwl = ceil_log2((bw + 31) >> 5), nplane = bh << rwl;
  uint32_t* rem = nplane <= kLdsWords ? s_planes : ws + (int64_t)r * 2 * cap_words;       // nplane <= cap_words
  uint32_t* cur = nplane <= kLdsWords ? s_planes + kLdsWords : rem + cap_words;

  // ---- pass 1: the size of every component, in raster order of their first cells
  repack(map, W, bx0, by0, bw, bh, rwl, rem, cur, t);
  int best = 0, best_seed = 0, comps = 0, pos = 0;
  uint32_t best_bit = 0u;
  for (;;) {                                                           // bounded: every turn clears at least the seed from rem
    const int seed = find_seed(rem, nplane, pos, s, t);
    if (seed < 0) break;
    pos = seed;
    const uint32_t word = rem[seed], bit = word & (0u - word);
    flood(rem, cur, rwl, bh, seed, bit, s, t);
    const int lo = s[S_LO] << rwl, hi = (s[S_HI] + 1) << rwl;
    int cnt = 0;
    for (int i = lo + t; i < hi; i += kThreads) {
      const uint32_t c = cur[i];
      if (c) { cnt += __popc(c); rem[i] &= ~c; cur[i] = 0u; }
    }
    if (cnt) atomicAdd(&s[S_COUNT], cnt);
    __syncthreads();
    const int total = s[S_COUNT];
    __syncthreads();
    ++comps;
    if (total > best) { best = total; best_seed = seed; best_bit = bit; }
  }

  if (comps == 1) {                                                    // uniform: the map is its own largest component
    for (int64_t wi = t; wi < words; wi += kThreads) o[wi] = load_word(map, (int)wi, npix);
    if (t == 0) { n_out[r] = best; comps_out[r] = 1; }
    return;
  }

  // ---- pass 2: the best component again, scattered back into the map's layout
  repack(map, W, bx0, by0, bw, bh, rwl, rem, cur, t);
  flood(rem, cur, rwl, bh, best_seed, best_bit, s, t);
  for (int64_t wi = t; wi < words; wi += kThreads) {
    uint32_t w = 0u;
    if (wi < nwords) {
      const int p0 = (int)wi * 32, end = min(p0 + 32, npix);
      int y = p0 / W, x = p0 - y * W;
      for (int p = p0; p < end;) {
        const int seg = min(W - x, end - p);
        if (y >= by0 && y < by0 + bh) w |= plane_bits(cur, rwl, y - by0, x - bx0, seg) << (p - p0);
        p += seg; x = 0; ++y;
      }
    }
    o[wi] = w;
  }
  if (t == 0) { n_out[r] = best; comps_out[r] = comps; }
}

// words of one plane that can hold the whole map row-aligned; planes of that size live in the workspace
inline int64_t plane_capacity(int H, int W) { return (int64_t)H << ceil_log2((W + 31) >> 5); }

inline bool grid_ok(int H, int W) { return H >= 1 && W >= 1 && H <= 1024 && W <= 1024; }

}  // namespace

extern "C" int64_t mbv_largest_component_workspace_bytes(int32_t H, int32_t W, int32_t num_rows) {
  if (!grid_ok(H, W) || num_rows <= 0) return 0;
  const int64_t cap = plane_capacity(H, W);
  return cap <= kLdsWords ? 0 : (int64_t)num_rows * 2 * cap * (int64_t)sizeof(uint32_t);
}

extern "C" int mbv_largest_component(const uint32_t* packed, int64_t num_maps, int32_t H, int32_t W, const int32_t* rows,
                                     int32_t num_rows, uint32_t* out_packed, int32_t* n, int32_t* components,
                                     void* workspace, int64_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (num_rows < 0 || num_maps < 0 || !grid_ok(H, W)) return MBV_ERR_BAD_ARG;
  if (num_rows == 0) return MBV_OK;
  if (!packed || !rows || !out_packed || !n || !components || num_maps == 0) return MBV_ERR_BAD_ARG;
  const int64_t need = mbv_largest_component_workspace_bytes(H, W, num_rows);
  if (need > 0 && (!workspace || workspace_bytes < need)) return MBV_ERR_WORKSPACE;
  hipLaunchKernelGGL(k_largest_component, dim3((unsigned)num_rows), dim3(kThreads), 0, stream, packed, num_maps,
                     mbv_packed_mask_words(H, W), (int)H, (int)W, rows, out_packed, n, components,
                     reinterpret_cast<uint32_t*>(workspace), plane_capacity(H, W));
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
