// K21 — instance extraction at inference: query selection and BEV mask extraction of one decoder output.
//
// Replaces the per-query host loops of the reference's consumers
//   c = cls.argmax(); if c > 0: sigmoid(F.interpolate(mask, (ny, nx), 'bilinear', align_corners=False)) > 0.5
// (mask_bev/evaluation/kitti_eval.py:27-44, mask_bev/mask_bev_module.py:286-294), which materialise B·Q·ny·nx f32
// upsampled logits (420 MB at 512², B = 4; 5 GB at 1024², Q = 300).
//
// (a) k_select_queries: one wave per row of class logits (K+1 <= 256, f32 / bf16 / fp16): max-subtracted softmax in f32,
//     label = first argmax, score = softmax[label] (= 1 / Σ exp(x - max)), keep = label > 0 && score >= threshold.
// (b) k_extract_masks: one workgroup per (tile of TILE consecutive BEV pixels, scan).  A tile stages, query by query, only
//     the logit rows its pixels touch (K15 stages a whole map and stops at 128²; here 256² logits cost 2-3 rows of 1 KB per
//     tile), interpolates every pixel with K15's upsample_bilinear2d arithmetic (mask_iou.hip), thresholds v > 0, ballots
//     64 pixels into the two words of mbv_pack_binary_masks' layout, and keeps per pixel the best kept query by
//     score · sigmoid(v) in registers (ascending q with a strict compare: ties go to the smaller q).  Per-tile float sums
//     of sigmoid(v) and integer counts go to the workspace; k_finish_masks adds them per query in tile order
//     (deterministic: no float atomics, no inter-workgroup counter, no memset — every output element is written by a kernel).
#include "common.hpp"

namespace {

constexpr int kSelThreads = 256;                 // 4 rows per workgroup, one wave each
constexpr int kThreads = 256;                    // extraction: 4 waves
constexpr int kMaxPpt = 8;                       // pixels per thread (a tile is kThreads * ppt consecutive pixels)
constexpr int kTileFloatsMax = 16384;            // 64 KB of dynamic LDS for the staged logit rows
constexpr int kPre = 4;                          // staged floats per thread prefetched into registers for the next query

template <typename T>
__device__ __forceinline__ float to_f32(T v) { return (float)v; }

template <typename T>
__global__ void __launch_bounds__(kSelThreads) k_select_queries(const T* __restrict__ cls, int64_t rows, int classes,
                                                                 float threshold, int32_t* __restrict__ label,
                                                                 float* __restrict__ score, uint8_t* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kSelThreads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;                        // whole waves only: no barrier below
  const T* x = cls + row * classes;
  float v[4];
  float m = -INFINITY;
  int mi = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    v[k] = c < classes ? to_f32(x[c]) : -INFINITY;
    if (c < classes && (v[k] > m || mi == 0x7fffffff)) { m = v[k]; mi = c; }   // ascending c: the first maximum stays
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float om = __shfl_xor(m, off);
    const int oi = __shfl_xor(mi, off);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane + 64 * k < classes) s += expf(v[k] - m);
  s = wave_sum(s);
  if (lane == 0) {
    const float sc = 1.f / s;
    label[row] = mi;
    score[row] = sc;
    keep[row] = (mi > 0 && sc >= threshold) ? 1 : 0;
  }
}

// source row of BEV row y (PyTorch's upsample_bilinear2d, align_corners=False): the same expression K15 evaluates
__host__ __device__ inline int src_row(int y, float sh) {
  const float f = sh * ((float)y + 0.5f) - 0.5f;
  return (int)(f > 0.f ? f : 0.f);
}

// the logit rows [first, last] the pixels [p_lo, p_lo + tile) ∩ [0, H·W) of a map touch
__host__ __device__ inline void tile_rows(int64_t p_lo, int tile, int64_t hw, int W, int h, float sh, int* first,
                                          int* last) {
  const int64_t p_hi = (p_lo + tile < hw ? p_lo + tile : hw) - 1;
  *first = src_row((int)(p_lo / W), sh);
  const int r = src_row((int)(p_hi / W), sh) + 1;
  *last = r < h - 1 ? r : h - 1;
}

struct Plan {
  int ppt, tiles, tile_floats;
};

// pixels per thread: the largest of 8, 4, 2, 1 whose staged rows fit kTileFloatsMax (ppt = 0: unsupported)
Plan make_plan(int h, int w, int H, int W) {
  const int64_t hw = (int64_t)H * W, cover = mbv_packed_mask_words(H, W) * 32;
  const float sh = (float)h / (float)H;
  for (int ppt = kMaxPpt; ppt >= 1; ppt >>= 1) {
    const int tile = kThreads * ppt;
    const int tiles = (int)((cover + tile - 1) / tile);
    int rows = 0;
    for (int t = 0; t < tiles; ++t) {
      int a, b;
      tile_rows((int64_t)t * tile, tile, hw, W, h, sh, &a, &b);
      rows = b - a + 1 > rows ? b - a + 1 : rows;
    }
    if ((int64_t)rows * w <= kTileFloatsMax) return Plan{ppt, tiles, rows * w};
  }
  return Plan{0, 0, 0};
}

__global__ void __launch_bounds__(kThreads) k_extract_masks(const float* __restrict__ logits, const float* __restrict__ score,
                                                            const uint8_t* __restrict__ keep, int Q, int h, int w, int H,
                                                            int W, int ppt, int tiles, int64_t words,
                                                            uint32_t* __restrict__ masks, float* __restrict__ ws_sum,
                                                            int32_t* __restrict__ ws_cnt, int32_t* __restrict__ imap) {
  extern __shared__ __attribute__((aligned(16))) float tile_lds[];
  __shared__ uint32_t bits[kMaxPpt * kThreads / 32];
  __shared__ float red_s[kThreads / 64];
  __shared__ int red_c[kThreads / 64];
  const int t = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = kThreads * ppt;
  const int64_t hw = (int64_t)H * W;
  const int64_t p_lo = (int64_t)t * tile;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  int ry0, ry1;
  tile_rows(p_lo, tile, hw, W, h, sh, &ry0, &ry1);
  const int staged = (ry1 - ry0 + 1) * w;
  const bool sums = ws_sum != nullptr;
  const bool every = masks != nullptr || sums;    // else only kept queries matter (the instance map)

  // per-pixel interpolation geometry, once for all queries: LDS offset of the top-left neighbour, steps, weights
  int off[kMaxPpt], xp[kMaxPpt], ypw[kMaxPpt];
  float lx[kMaxPpt], ly[kMaxPpt], best[kMaxPpt];
  int bq[kMaxPpt];
#pragma unroll
  for (int i = 0; i < kMaxPpt; ++i) {
    const int64_t p = p_lo + (int64_t)i * kThreads + tid;
    off[i] = -1; xp[i] = 0; ypw[i] = 0; lx[i] = 0.f; ly[i] = 0.f; best[i] = -1.f; bq[i] = -1;
    if (i < ppt && p < hw) {
      const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
      const float fy = fmaxf(sh * ((float)y + 0.5f) - 0.5f, 0.f), fx = fmaxf(sw * ((float)x + 0.5f) - 0.5f, 0.f);
      const int y0 = (int)fy, x0 = (int)fx;
      off[i] = (y0 - ry0) * w + x0;
      xp[i] = x0 < w - 1 ? 1 : 0;
      ypw[i] = y0 < h - 1 ? w : 0;
      ly[i] = fy - (float)y0;
      lx[i] = fx - (float)x0;
    }
  }
  const int64_t word0 = p_lo / 32;
  const int nwords = (int)((words - word0) < tile / 32 ? (words - word0) : tile / 32);

  // software pipeline over the queries: the next needed query's rows (the first kPre * kThreads staged floats), score and
  // keep flag are loaded into registers while this query's pixels are computed
  const int64_t map_elems = (int64_t)h * w;
  const float* maps = logits + (int64_t)b * Q * map_elems + (int64_t)ry0 * w;
  auto next_query = [&](int q) {
    if (!every)
      while (q < Q && keep[(int64_t)b * Q + q] == 0) ++q;
    return q;
  };
  float pre[kPre];
  float sc_next = 0.f;
  bool kq_next = false;
  auto issue = [&](int q) {
    if (q >= Q) return;
    const float* src = maps + (int64_t)q * map_elems;
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      const int j = tid + k * kThreads;
      pre[k] = j < staged ? src[j] : 0.f;
    }
    sc_next = score[(int64_t)b * Q + q];
    kq_next = keep[(int64_t)b * Q + q] != 0;
  };
  int q = next_query(0);
  issue(q);
  while (q < Q) {
    const int64_t bq_row = (int64_t)b * Q + q;
    const bool kq = kq_next;
    const float sc = sc_next;
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      const int j = tid + k * kThreads;
      if (j < staged) tile_lds[j] = pre[k];
    }
    const float* src = maps + (int64_t)q * map_elems;
    for (int j = tid + kPre * kThreads; j < staged; j += kThreads) tile_lds[j] = src[j];   // rows beyond the registers
    __syncthreads();
    const int qn = next_query(q + 1);
    issue(qn);
    float ssum = 0.f;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < kMaxPpt; ++i) {
      if (i < ppt) {                              // block-uniform
        bool bit = false;
        float v = 0.f;
        if (off[i] >= 0) {
          const float* r0 = tile_lds + off[i];
          const float* r1 = r0 + ypw[i];
          const float hy = 1.f - ly[i], hx = 1.f - lx[i];
          v = hy * (hx * r0[0] + lx[i] * r0[xp[i]]) + ly[i] * (hx * r1[0] + lx[i] * r1[xp[i]]);
          bit = v > 0.f;
        }
        const unsigned long long bal = __ballot(bit);
        if (lane == 0) {
          bits[(i * (kThreads / 64) + wave) * 2] = (uint32_t)bal;
          bits[(i * (kThreads / 64) + wave) * 2 + 1] = (uint32_t)(bal >> 32);
        }
        cnt += __popcll(bal);                     // wave-uniform
        if (bit && (sums || kq)) {
          const float sg = 1.f / (1.f + expf(-v));
          ssum += sg;
          const float pr = sc * sg;
          if (kq && pr > best[i]) { best[i] = pr; bq[i] = q; }
        }
      }
    }
    if (sums) {
      ssum = wave_sum(ssum);                      // fixed shuffle order: deterministic
      if (lane == 0) { red_s[wave] = ssum; red_c[wave] = cnt; }
    }
    __syncthreads();
    if (masks != nullptr)
      for (int j = tid; j < nwords; j += kThreads) masks[bq_row * words + word0 + j] = bits[j];
    if (sums && tid == 0) {
      float s = 0.f;
      int c = 0;
      for (int k = 0; k < kThreads / 64; ++k) { s += red_s[k]; c += red_c[k]; }
      ws_sum[bq_row * tiles + t] = s;
      ws_cnt[bq_row * tiles + t] = c;
    }
    // every thread has passed the barrier above: the LDS tile may be restaged; `bits` / `red_*` are next written after the
    // next query's barrier, by which time the reads above are done
    q = qn;
  }
  if (imap != nullptr) {
#pragma unroll
    for (int i = 0; i < kMaxPpt; ++i) {
      const int64_t p = p_lo + (int64_t)i * kThreads + tid;
      if (i < ppt && p < hw) imap[(int64_t)b * hw + p] = bq[i];
    }
  }
}

__global__ void __launch_bounds__(256) k_finish_masks(const float* __restrict__ ws_sum, const int32_t* __restrict__ ws_cnt,
                                                      int64_t maps, int tiles, int32_t* __restrict__ areas,
                                                      float* __restrict__ mask_scores) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= maps) return;
  double s = 0.0;                                 // up to 512 tile partials: f64 keeps the mean at f32 accuracy
  int c = 0;
  for (int t = 0; t < tiles; ++t) {               // fixed order
    s += (double)ws_sum[r * tiles + t];
    c += ws_cnt[r * tiles + t];
  }
  if (areas) areas[r] = c;
  if (mask_scores) mask_scores[r] = c > 0 ? (float)(s / (double)c) : 0.f;
}

}  // namespace

extern "C" int mbv_select_queries(const void* cls, int32_t cls_dtype, int64_t rows, int32_t classes, float score_threshold,
                                  int32_t* label, float* score, uint8_t* keep, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (rows < 0 || classes <= 0 || classes > 256) return MBV_ERR_BAD_ARG;
  if (rows == 0) return MBV_OK;
  if (!cls || !label || !score || !keep) return MBV_ERR_BAD_ARG;
  const int64_t blocks = (rows + kSelThreads / 64 - 1) / (kSelThreads / 64);
  if (blocks > 0x7fffffff) return MBV_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks), block(kSelThreads);
  if (cls_dtype == MBV_DT_F32)
    hipLaunchKernelGGL(k_select_queries<float>, grid, block, 0, stream, (const float*)cls, rows, classes, score_threshold,
                       label, score, keep);
  else if (cls_dtype == MBV_DT_BF16)
    hipLaunchKernelGGL(k_select_queries<__bf16>, grid, block, 0, stream, (const __bf16*)cls, rows, classes,
                       score_threshold, label, score, keep);
  else if (cls_dtype == MBV_DT_F16)
    hipLaunchKernelGGL(k_select_queries<_Float16>, grid, block, 0, stream, (const _Float16*)cls, rows, classes,
                       score_threshold, label, score, keep);
  else
    return MBV_ERR_BAD_ARG;
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" size_t mbv_extract_masks_workspace_bytes(int32_t batch, int32_t num_queries, int32_t h, int32_t w, int32_t H,
                                                    int32_t W) {
  if (batch <= 0 || num_queries <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
  const Plan pl = make_plan(h, w, H, W);
  if (pl.ppt == 0) return 0;
  const size_t n = (size_t)batch * num_queries * pl.tiles;
  return mbv_align_up(n * sizeof(float), 256) + mbv_align_up(n * sizeof(int32_t), 256);
}

extern "C" int mbv_extract_masks(const float* logits, const float* score, const uint8_t* keep, int32_t batch,
                                 int32_t num_queries, int32_t h, int32_t w, int32_t H, int32_t W, uint32_t* masks_packed,
                                 int32_t* areas, float* mask_scores, int32_t* instance_map, void* workspace,
                                 size_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (batch < 0 || num_queries < 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return MBV_ERR_BAD_ARG;
  if ((int64_t)H * W > 1024 * 1024 || batch > 65535) return MBV_ERR_UNSUPPORTED;
  if ((int64_t)batch * num_queries == 0) {       // no query: the map of every scan is "none"
    if (batch > 0 && instance_map) MBV_CHECK_HIP(mbv_fill_async(instance_map, 0xff, (size_t)batch * H * W * 4, stream));
    return MBV_OK;
  }
  if (!logits || !score || !keep) return MBV_ERR_BAD_ARG;
  const bool sums = areas != nullptr || mask_scores != nullptr;
  const Plan pl = make_plan(h, w, H, W);
  if (pl.ppt == 0) return MBV_ERR_UNSUPPORTED;
  float* ws_sum = nullptr;
  int32_t* ws_cnt = nullptr;
  if (sums) {
    const size_t n = (size_t)batch * num_queries * pl.tiles;
    if (!workspace || workspace_bytes < mbv_extract_masks_workspace_bytes(batch, num_queries, h, w, H, W))
      return MBV_ERR_WORKSPACE;
    MbvCarver carve(workspace);
    ws_sum = carve.take<float>(n);
    ws_cnt = carve.take<int32_t>(n);
  }
  if (!masks_packed && !sums && !instance_map) return MBV_OK;
  hipLaunchKernelGGL(k_extract_masks, dim3((unsigned)pl.tiles, (unsigned)batch), dim3(kThreads),
                     (size_t)pl.tile_floats * sizeof(float), stream, logits, score, keep, num_queries, h, w, H, W, pl.ppt,
                     pl.tiles, mbv_packed_mask_words(H, W), masks_packed, ws_sum, ws_cnt, instance_map);
  MBV_CHECK_LAUNCH();
  if (sums) {
    const int64_t maps = (int64_t)batch * num_queries;
    hipLaunchKernelGGL(k_finish_masks, dim3((unsigned)((maps + 255) / 256)), dim3(256), 0, stream, ws_sum, ws_cnt, maps,
                       pl.tiles, areas, mask_scores);
    MBV_CHECK_LAUNCH();
  }
  return MBV_OK;
}
