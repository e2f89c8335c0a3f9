// K30b — the minimum-area rectangle of the set cells of a bit-packed mask.
//
// The second half of what mask_to_pred (mask_bev/evaluation/kitti_eval.py:27-45) does with cv2.minAreaRect; the rectangle is
// over ALL set cells of the map it is given (K30a, csrc/mask_components.hip, keeps the largest blob in front of it).
// OpenCV's own floating-point rectangle arithmetic is not restated: the choice of the rectangle here is exact.
//
// One workgroup per listed row.  Sweep: the popcount and, per image row, the leftmost and the rightmost set cell (LDS integer
// min / max) — the only candidates for the hull, at most 2 H points, already sorted by (y, x).  Hull: Andrew's monotone chain
// over that order, the lower chain by one thread and the upper chain by a thread of another wave, popping on cross <= 0, so
// the hull is strictly convex; each stack is bounded by the points pushed.  Edges: every hull edge against every hull vertex,
// the edges spread over the workgroup: min / max of p . e and of p x e in int32, the area as the ratio
// (du dv) / |e|^2 with du dv < 2^42 and |e|^2 < 2^21; two areas are compared exactly by cross-multiplication (in 128 bits,
// though the products stay below 2^63), ties by the canonical direction (ex > 0, -ex < ey <= ex): smallest |ey| / ex, then
// ey >= 0.  Each thread keeps the best of its edges, thread 0 the best of those, and forms the box in f64 with one rounding
// per operation (no contraction: build.py), one rounding to f32 at the store.
#include <limits.h>

#include "common.hpp"

namespace {

constexpr int kThreads = 256, kMaxH = 1024;

__device__ __forceinline__ uint32_t low_mask(int len) { return len >= 32 ? 0xffffffffu : ((1u << len) - 1u); }

// the word `wi` of a map of `npix` pixels with the bits at and beyond npix cleared
__device__ __forceinline__ uint32_t load_word(const uint32_t* __restrict__ map, int wi, int npix) {
  const int left = npix - wi * 32;
  if (left <= 0) return 0u;
  const uint32_t w = map[wi];
  return left >= 32 ? w : (w & ((1u << left) - 1u));
}

__device__ __forceinline__ uint32_t pt(int x, int y) { return (uint32_t)x | ((uint32_t)y << 16); }
__device__ __forceinline__ int pt_x(uint32_t p) { return (int)(p & 0xffffu); }
__device__ __forceinline__ int pt_y(uint32_t p) { return (int)(p >> 16); }

// one step of the monotone chain over points sorted by (y, x): the cross product with the roles of x and y exchanged
__device__ __forceinline__ int chain_push(uint32_t* st, int k, uint32_t p) {
  while (k >= 2) {                                                     // bounded by the stack
    const uint32_t o = st[k - 2], a = st[k - 1];
    const int cross = (pt_y(a) - pt_y(o)) * (pt_x(p) - pt_x(o)) - (pt_x(a) - pt_x(o)) * (pt_y(p) - pt_y(o));
    if (cross > 0) break;
    --k;
  }
  st[k] = p;
  return k + 1;
}

struct Edge {                                                          // an edge's rectangle: area = num / den, canonical direction
  unsigned long long num;
  uint32_t den;                                                        // 0: no edge
  int cx, cy;
};

// e turned by multiples of 90 degrees to ex > 0, -ex < ey <= ex
__device__ __forceinline__ void canonical(int ex, int ey, int& cx, int& cy) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (ex > 0 && ey > -ex && ey <= ex) break;
    const int tmp = ex;
    ex = -ey;
    ey = tmp;
  }
  cx = ex;
  cy = ey;
}

__device__ __forceinline__ bool better(const Edge& a, const Edge& b) {
  if (b.den == 0u) return a.den != 0u;
  if (a.den == 0u) return false;
  const unsigned __int128 l = (unsigned __int128)a.num * b.den, r = (unsigned __int128)b.num * a.den;
  if (l != r) return l < r;
  const long long sa = (long long)abs(a.cy) * b.cx, sb = (long long)abs(b.cy) * a.cx;
  if (sa != sb) return sa < sb;
  return a.cy >= 0 && b.cy < 0;
}

__global__ void __launch_bounds__(kThreads) k_min_area_boxes(const uint32_t* __restrict__ packed, int64_t num_maps,
                                                             int64_t words, int H, int W,
                                                             const int32_t* __restrict__ rows, int32_t* __restrict__ n_out,
                                                             int32_t* __restrict__ hull_out, float* __restrict__ boxes) {
  __shared__ int s_xl[kMaxH], s_xr[kMaxH];
  __shared__ uint32_t s_lower[2 * kMaxH], s_upper[2 * kMaxH];
  __shared__ Edge s_edge[kThreads];
  __shared__ int s_n, s_nl, s_nu, s_ymin, s_ymax;
  const int r = blockIdx.x, t = threadIdx.x;
  const int64_t row = rows[r];
  const bool valid = row >= 0 && row < num_maps;                       // a row outside the table counts as an empty map
  const uint32_t* __restrict__ map = packed + (valid ? row : 0) * words;
  const int npix = valid ? H * W : 0;
  const int nwords = (npix + 31) / 32;
  float* __restrict__ o = boxes + (int64_t)r * 5;

  for (int y = t; y < H; y += kThreads) { s_xl[y] = INT_MAX; s_xr[y] = -1; }
  if (t == 0) { s_n = 0; s_ymin = INT_MAX; s_ymax = -1; }
  __syncthreads();
  int cnt = 0, ymin = INT_MAX, ymax = -1;
  for (int wi = t; wi < nwords; wi += kThreads) {
    const uint32_t w = load_word(map, wi, npix);
    if (w == 0u) continue;
    cnt += __popc(w);
    const int p0 = wi * 32, end = min(p0 + 32, npix);
    int y = p0 / W, x = p0 - y * W;
    for (int p = p0; p < end;) {                                       // the word's pieces, one per image row it touches
      const int seg = min(W - x, end - p);
      const uint32_t bits = (w >> (p - p0)) & low_mask(seg);
      if (bits) {
        atomicMin(&s_xl[y], x + __ffs((int)bits) - 1);
        atomicMax(&s_xr[y], x + 31 - __clz((int)bits));
        ymin = min(ymin, y);
        ymax = max(ymax, y);
      }
      p += seg; x = 0; ++y;
    }
  }
  if (cnt) { atomicAdd(&s_n, cnt); atomicMin(&s_ymin, ymin); atomicMax(&s_ymax, ymax); }
  __syncthreads();
  const int n = s_n;
  if (n == 0) {                                                        // uniform: a box of zeros, reported through n
    if (t < 5) o[t] = 0.f;
    if (t == 0) { n_out[r] = 0; hull_out[r] = 0; }
    return;
  }

  // ---- the hull: two chains over the candidates in (y, x) order, between the first and the last row that hold a cell
  const int y0 = s_ymin, y1 = s_ymax;
  if (t == 0) {
    int k = 0;
    for (int y = y0; y <= y1; ++y) {
      if (s_xr[y] < 0) continue;
      k = chain_push(s_lower, k, pt(s_xl[y], y));
      if (s_xr[y] > s_xl[y]) k = chain_push(s_lower, k, pt(s_xr[y], y));
    }
    s_nl = k;
  } else if (t == MBV_WAVE) {
    int k = 0;
    for (int y = y1; y >= y0; --y) {
      if (s_xr[y] < 0) continue;
      k = chain_push(s_upper, k, pt(s_xr[y], y));
      if (s_xr[y] > s_xl[y]) k = chain_push(s_upper, k, pt(s_xl[y], y));
    }
    s_nu = k;
  }
  __syncthreads();
  const int nl = s_nl, nu = s_nu;
  const int h = nl == 1 ? 1 : (nl - 1) + (nu - 1);                     // each chain ends where the other begins
  if (h == 1) {                                                        // uniform: a single cell
    if (t == 0) {
      n_out[r] = n; hull_out[r] = 1;
      o[0] = (float)pt_x(s_lower[0]); o[1] = (float)pt_y(s_lower[0]); o[2] = 1.f; o[3] = 1.f; o[4] = 0.f;
    }
    return;
  }
  auto vertex = [&](int k) { return k < nl - 1 ? s_lower[k] : s_upper[k - (nl - 1)]; };

  // ---- every edge against every vertex
  Edge mine = {0ull, 0u, 0, 0};
  for (int i = t; i < h; i += kThreads) {
    const uint32_t a = vertex(i), b = vertex(i + 1 == h ? 0 : i + 1);
    const int ex = pt_x(b) - pt_x(a), ey = pt_y(b) - pt_y(a);
    int umin = INT_MAX, umax = INT_MIN, vmin = INT_MAX, vmax = INT_MIN;
    for (int k = 0; k < h; ++k) {
      const uint32_t p = vertex(k);
      const int u = pt_x(p) * ex + pt_y(p) * ey, v = ex * pt_y(p) - ey * pt_x(p);
      umin = min(umin, u); umax = max(umax, u); vmin = min(vmin, v); vmax = max(vmax, v);
    }
    Edge e;
    e.num = (unsigned long long)(umax - umin) * (unsigned long long)(vmax - vmin);
    e.den = (uint32_t)(ex * ex + ey * ey);
    canonical(ex, ey, e.cx, e.cy);
    if (better(e, mine)) mine = e;
  }
  s_edge[t] = mine;
  __syncthreads();
  if (t != 0) return;
  Edge best = s_edge[0];
  const int cand = min(h, kThreads);
  for (int k = 1; k < cand; ++k) {
    const Edge e = s_edge[k];
    if (better(e, best)) best = e;
  }

  // ---- the box of the chosen direction
  int umin = INT_MAX, umax = INT_MIN, vmin = INT_MAX, vmax = INT_MIN;
  for (int k = 0; k < h; ++k) {
    const uint32_t p = vertex(k);
    const int u = pt_x(p) * best.cx + pt_y(p) * best.cy, v = best.cx * pt_y(p) - best.cy * pt_x(p);
    umin = min(umin, u); umax = max(umax, u); vmin = min(vmin, v); vmax = max(vmax, v);
  }
  const double ex = (double)best.cx, ey = (double)best.cy;
  const double theta = atan2(ey, ex), c = cos(theta), sn = sin(theta), len = sqrt(ex * ex + ey * ey);
  const double cell = fabs(c) + fabs(sn);
  const double uc = 0.5 * (double)(umax + umin) / len, vc = 0.5 * (double)(vmax + vmin) / len;
  n_out[r] = n;
  hull_out[r] = h;
  o[0] = (float)(uc * c - vc * sn);
  o[1] = (float)(uc * sn + vc * c);
  o[2] = (float)((double)(umax - umin) / len + cell);
  o[3] = (float)((double)(vmax - vmin) / len + cell);
  o[4] = (float)theta;
}

}  // namespace

extern "C" int mbv_min_area_boxes(const uint32_t* packed, int64_t num_maps, int32_t H, int32_t W, const int32_t* rows,
                                  int32_t num_rows, int32_t* n, int32_t* hull, float* boxes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (num_rows < 0 || num_maps < 0 || H < 1 || W < 1 || H > kMaxH || W > 1024) return MBV_ERR_BAD_ARG;
  if (num_rows == 0) return MBV_OK;
  if (!packed || !rows || !n || !hull || !boxes || num_maps == 0) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_min_area_boxes, dim3((unsigned)num_rows), dim3(kThreads), 0, stream, packed, num_maps,
                     mbv_packed_mask_words(H, W), (int)H, (int)W, rows, n, hull, boxes);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
