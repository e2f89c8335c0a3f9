// K32 — panoptic quality of point or BEV instances: the per-frame tp / fp / fn, IoU sums and confusion of the SemanticKITTI
// panoptic protocol (semantic-kitti-api, eval_np.py, PanopticEval.addBatchPanoptic; restated, not repaired) for all frames of a
// batch, from two id arrays: the query that owns an element (K31's point_query, K21's instance_map) and the ground truth's
// `.label` word (semantic id in the low, instance id in the high 16 bits).
//
// Five launches, whatever the number of frames:
//   1. init      zeroes the presence bitmaps, the pair table and the outputs that take atomics; gt_key gets -1.
//   2. mark      one thread per element (blocks of 256, grid.y = frame): a non-ignored element of a thing class sets bit
//                key = class << 16 | instance of its frame's bitmap (C * 65536 bits) with an integer OR.
//   3. index     one workgroup per frame: popcounts of the bitmap's words, an exclusive scan over them (the word-prefix
//                table), n_gt, and the ascending keys of the first max_gt segments.  The dense, ascending index of a key is
//                prefix[word] + popc(word & lower bits).
//   4. count     one thread per element again: pred_area and the C x C confusion in LDS tables (integer LDS atomics, one
//                flush per block with integer global atomics); gt_area and the (frames, max_gt, P) pair table take plain
//                global integer atomics.
//   5. match     one workgroup per frame: a wave per ground-truth row of the pair table; iou = (double)inter / (double)union
//                > 0.5 holds for at most one entry of a row and of a column, so the marks on both sides are plain stores;
//                then one thread per class walks the segments in ascending order: tp, iou_sum, fn, fp.
// Integer atomics only, and the f64 sum in a fixed order: two runs are bit-equal.  Every index comes from the sizes: a query,
// a semantic id, a table value or a frame offset that disagrees with them changes results, never addresses.
#include "common.hpp"

namespace {

constexpr int kThreads = 256, kWide = 1024, kMaxQueries = 1024, kMaxGt = 1024, kMaxClasses = 16;
constexpr int kWordsPerClass = 65536 / 32;

struct PanopticWorkspace {
  uint32_t* bitmap;      // (frames, C * 2048): bit key of frame f
  int32_t* prefix;       // (frames, C * 2048): set bits in the words before
  int32_t* pair;         // (frames, max_gt, P): elements in both segments, classes equal
  size_t bytes;
};

PanopticWorkspace carve_panoptic(void* ws, int64_t frames, int P, int max_gt, int C) {
  MbvCarver c(ws);
  PanopticWorkspace w;
  w.bitmap = c.take<uint32_t>(frames * C * kWordsPerClass);
  w.prefix = c.take<int32_t>(frames * C * kWordsPerClass);
  w.pair = c.take<int32_t>(frames * max_gt * P);
  w.bytes = c.off;
  return w;
}

// the class of a ground-truth word: -1 ignored, 0 everything else, 1 .. C-1 a thing
__device__ __forceinline__ int gt_class_of(uint32_t word, const int32_t* __restrict__ class_lut, int lut_len, int C) {
  const int sem = (int)(word & 0xffffu);
  if (sem >= lut_len) return -1;
  const int c = class_lut[sem];
  return (c < 0 || c >= C) ? -1 : c;
}

__device__ __forceinline__ void frame_range(const int32_t* __restrict__ frame_offsets, int f, int64_t total, int64_t& begin,
                                            int64_t& end) {
  begin = frame_offsets[f];
  end = frame_offsets[f + 1];
  begin = begin < 0 ? 0 : begin;                                   // offsets that point outside the arrays read nothing
  end = end > total ? total : end;
}

__global__ void __launch_bounds__(kThreads) k_panoptic_init(int64_t bitmap_words, int64_t pair_elems, int64_t gt_elems,
                                                            int64_t pred_elems, int64_t conf_elems,
                                                            uint32_t* __restrict__ bitmap, int32_t* __restrict__ pair,
                                                            int32_t* __restrict__ gt_key, int32_t* __restrict__ gt_area,
                                                            int32_t* __restrict__ pred_area, int64_t* __restrict__ confusion) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  for (int64_t i = t; i < bitmap_words; i += stride) bitmap[i] = 0u;
  for (int64_t i = t; i < pair_elems; i += stride) pair[i] = 0;
  for (int64_t i = t; i < gt_elems; i += stride) {
    gt_key[i] = -1;
    gt_area[i] = 0;
  }
  for (int64_t i = t; i < pred_elems; i += stride) pred_area[i] = 0;
  for (int64_t i = t; i < conf_elems; i += stride) confusion[i] = 0;
}

__global__ void __launch_bounds__(kThreads) k_panoptic_mark(const uint32_t* __restrict__ gt_word, int64_t total,
                                                            const int32_t* __restrict__ frame_offsets,
                                                            const int32_t* __restrict__ class_lut, int lut_len, int C,
                                                            uint32_t* __restrict__ bitmap) {
  const int f = blockIdx.y;
  int64_t begin, end;
  frame_range(frame_offsets, f, total, begin, end);
  const int64_t i = begin + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= end) return;
  const uint32_t word = gt_word[i];
  const int c = gt_class_of(word, class_lut, lut_len, C);
  if (c < 1) return;
  const uint32_t key = ((uint32_t)c << 16) | (word >> 16);         // < C * 65536
  uint32_t* w = bitmap + (int64_t)f * C * kWordsPerClass + (key >> 5);
  const uint32_t bit = 1u << (key & 31u);
  if (!(*w & bit)) atomicOr(w, bit);                               // a stale read costs one more OR, nothing else
}

__global__ void __launch_bounds__(kWide) k_panoptic_index(int C, int max_gt, const uint32_t* __restrict__ bitmap,
                                                          int32_t* __restrict__ prefix, int32_t* __restrict__ n_gt,
                                                          int32_t* __restrict__ gt_key) {
  __shared__ int32_t s_sum[kWide];
  const int f = blockIdx.x, t = threadIdx.x;
  const int words = C * kWordsPerClass;                            // a multiple of kWide
  const int per = words / kWide;
  const uint32_t* bm = bitmap + (int64_t)f * words;
  int32_t* px = prefix + (int64_t)f * words;
  int32_t mine = 0;
  for (int k = 0; k < per; ++k) mine += __popc(bm[t * per + k]);
  s_sum[t] = mine;
  __syncthreads();
  for (int o = 1; o < kWide; o <<= 1) {                            // inclusive scan over the threads' sums
    const int32_t v = t >= o ? s_sum[t - o] : 0;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  int32_t run = s_sum[t] - mine;
  if (t == kWide - 1) n_gt[f] = s_sum[t];
  for (int k = 0; k < per; ++k) {
    const int w = t * per + k;
    uint32_t bits = bm[w];
    px[w] = run;
    while (bits) {
      const int b = __ffs(bits) - 1;
      bits &= bits - 1;
      if (run < max_gt) gt_key[(int64_t)f * max_gt + run] = (w << 5) | b;
      ++run;
    }
  }
}

__global__ void __launch_bounds__(kThreads) k_panoptic_count(const int32_t* __restrict__ pred_query,
                                                             const uint32_t* __restrict__ gt_word, int64_t total,
                                                             const int32_t* __restrict__ frame_offsets,
                                                             const int32_t* __restrict__ query_class, int P,
                                                             const int32_t* __restrict__ class_lut, int lut_len, int C,
                                                             int max_gt, const uint32_t* __restrict__ bitmap,
                                                             const int32_t* __restrict__ prefix, int32_t* __restrict__ pair,
                                                             int32_t* __restrict__ gt_area, int32_t* __restrict__ pred_area,
                                                             int64_t* __restrict__ confusion) {
  __shared__ int32_t s_pred[kMaxQueries];
  __shared__ int32_t s_conf[kMaxClasses * kMaxClasses];
  const int f = blockIdx.y;
  int64_t begin, end;
  frame_range(frame_offsets, f, total, begin, end);
  const int64_t first = begin + (int64_t)blockIdx.x * kThreads;
  if (first >= end) return;                                        // the whole block: no barrier has been reached
  for (int q = threadIdx.x; q < P; q += kThreads) s_pred[q] = 0;
  for (int k = threadIdx.x; k < C * C; k += kThreads) s_conf[k] = 0;
  __syncthreads();
  const int64_t i = first + threadIdx.x;
  if (i < end) {
    const uint32_t word = gt_word[i];
    const int c = gt_class_of(word, class_lut, lut_len, C);
    if (c >= 0) {                                                  // an ignored element takes part in nothing
      int q = pred_query[i];
      int pc = 0;
      if (q >= 0 && q < P) pc = query_class[(int64_t)f * P + q];
      if (pc < 1 || pc >= C) {                                     // no query, or a query of no thing class: class 0, no instance
        pc = 0;
        q = -1;
      }
      atomicAdd(&s_conf[c * C + pc], 1);
      if (q >= 0) atomicAdd(&s_pred[q], 1);
      if (c >= 1) {
        const uint32_t key = ((uint32_t)c << 16) | (word >> 16);
        const int64_t w = (int64_t)f * C * kWordsPerClass + (key >> 5);
        const int g = prefix[w] + __popc(bitmap[w] & ((1u << (key & 31u)) - 1u));
        if (g >= 0 && g < max_gt) {
          const int64_t row = (int64_t)f * max_gt + g;
          atomicAdd(&gt_area[row], 1);
          if (q >= 0 && pc == c) atomicAdd(&pair[row * P + q], 1);
        }
      }
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < P; q += kThreads) {
    const int32_t n = s_pred[q];
    if (n > 0) atomicAdd(&pred_area[(int64_t)f * P + q], n);
  }
  for (int k = threadIdx.x; k < C * C; k += kThreads) {
    const int32_t n = s_conf[k];
    if (n > 0) atomicAdd(reinterpret_cast<unsigned long long*>(&confusion[(int64_t)f * C * C + k]), (unsigned long long)n);
  }
}

__global__ void __launch_bounds__(kWide) k_panoptic_match(const int32_t* __restrict__ query_class, int P, int C, int max_gt,
                                                          int min_points, const int32_t* __restrict__ pair,
                                                          const int32_t* __restrict__ n_gt, const int32_t* __restrict__ gt_key,
                                                          const int32_t* __restrict__ gt_area,
                                                          const int32_t* __restrict__ pred_area,
                                                          int32_t* __restrict__ frame_stats, double* __restrict__ frame_iou) {
  __shared__ double s_iou[kMaxGt];                                 // the IoU of a matched ground-truth segment, else 0
  __shared__ int32_t s_gt[kMaxGt];                                 // class << 1 | counted as fn (unmatched, area >= min_points)
  __shared__ int32_t s_pred[kMaxQueries];                          // matched
  const int f = blockIdx.x, t = threadIdx.x;
  const int n_all = n_gt[f];
  if (n_all > max_gt || n_all < 0) {                               // more segments than the tables hold: no numbers for the frame
    if (t < C) {
      for (int k = 0; k < 3; ++k) frame_stats[((int64_t)f * C + t) * 3 + k] = 0;
      frame_iou[(int64_t)f * C + t] = 0.0;
    }
    return;
  }
  const int n = n_all;
  for (int q = t; q < P; q += kWide) s_pred[q] = 0;
  __syncthreads();
  const int lane = t & (MBV_WAVE - 1), wave = t / MBV_WAVE;
  for (int g = wave; g < n; g += kWide / MBV_WAVE) {
    const int64_t row = (int64_t)f * max_gt + g;
    const int32_t ga = gt_area[row];
    double hit = 0.0;
    for (int q = lane; q < P; q += MBV_WAVE) {
      const int32_t inter = pair[row * P + q];
      if (inter > 0) {
        const int64_t uni = (int64_t)ga + pred_area[(int64_t)f * P + q] - inter;
        const double iou = (double)inter / (double)uni;
        if (iou > 0.5) {                                           // at most one entry of a row, and of a column
          hit = iou;
          s_pred[q] = 1;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hit += __shfl_xor(hit, o, 64);   // one lane holds the IoU, the others 0: exact
    if (lane == 0) {
      int cls = gt_key[row] >> 16;
      cls = (cls < 1 || cls >= C) ? 0 : cls;
      s_iou[g] = hit;
      s_gt[g] = (cls << 1) | ((hit == 0.0 && ga >= min_points) ? 1 : 0);
    }
  }
  __syncthreads();
  if (t < C) {
    int32_t tp = 0, fp = 0, fn = 0;
    double sum = 0.0;
    if (t >= 1) {
      for (int g = 0; g < n; ++g) {                                // ascending segment order: the sum's order is fixed
        if ((s_gt[g] >> 1) != t) continue;
        const double v = s_iou[g];
        if (v > 0.0) {
          ++tp;
          sum += v;
        } else {
          fn += s_gt[g] & 1;
        }
      }
      for (int q = 0; q < P; ++q) {
        const int32_t a = pred_area[(int64_t)f * P + q];
        if (a >= 1 && a >= min_points && !s_pred[q] && query_class[(int64_t)f * P + q] == t) ++fp;
      }
    }
    frame_stats[((int64_t)f * C + t) * 3 + 0] = tp;
    frame_stats[((int64_t)f * C + t) * 3 + 1] = fp;
    frame_stats[((int64_t)f * C + t) * 3 + 2] = fn;
    frame_iou[(int64_t)f * C + t] = sum;
  }
}

bool panoptic_sizes_supported(int64_t frames, int P, int max_gt, int C) {
  return frames >= 0 && frames <= 65535 && P >= 0 && P <= kMaxQueries && max_gt >= 1 && max_gt <= kMaxGt && C >= 1 &&
         C <= kMaxClasses;
}

}  // namespace

extern "C" size_t mbv_panoptic_frames_workspace_bytes(int32_t frames, int32_t P, int32_t max_gt, int32_t C) {
  if (!panoptic_sizes_supported(frames, P, max_gt, C)) return 0;
  return carve_panoptic(nullptr, frames, P, max_gt, C).bytes;
}

extern "C" int mbv_panoptic_frames(const int32_t* pred_query, const uint32_t* gt_word, int64_t total,
                                   const int32_t* frame_offsets, int32_t frames, const int32_t* query_class, int32_t P,
                                   const int32_t* class_lut, int32_t lut_len, int32_t C, int32_t max_gt, int32_t min_points,
                                   int32_t* frame_stats, double* frame_iou, int64_t* confusion, int32_t* n_gt,
                                   int32_t* gt_key, int32_t* gt_area, int32_t* pred_area, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (frames == 0) return MBV_OK;
  if (frames < 0 || total < 0 || P < 0 || lut_len < 0 || C < 1 || max_gt < 1 || min_points < 0) return MBV_ERR_BAD_ARG;
  if (!panoptic_sizes_supported(frames, P, max_gt, C) || total >= 0x7FFFFFFFll) return MBV_ERR_UNSUPPORTED;
  if (!frame_offsets || !frame_stats || !frame_iou || !confusion || !n_gt || !gt_key || !gt_area || (P > 0 && !pred_area) ||
      (P > 0 && !query_class) || (lut_len > 0 && !class_lut) || (total > 0 && (!pred_query || !gt_word)))
    return MBV_ERR_BAD_ARG;
  PanopticWorkspace w = carve_panoptic(workspace, frames, P, max_gt, C);
  if (!workspace || workspace_bytes < w.bytes) return MBV_ERR_WORKSPACE;

  const int64_t bitmap_words = (int64_t)frames * C * kWordsPerClass, pair_elems = (int64_t)frames * max_gt * P;
  const int64_t gt_elems = (int64_t)frames * max_gt, pred_elems = (int64_t)frames * P, conf_elems = (int64_t)frames * C * C;
  int64_t most = bitmap_words > pair_elems ? bitmap_words : pair_elems;
  int64_t init_blocks = (most + kThreads - 1) / kThreads;
  init_blocks = init_blocks > 4096 ? 4096 : init_blocks;
  hipLaunchKernelGGL(k_panoptic_init, dim3((unsigned)init_blocks), dim3(kThreads), 0, stream, bitmap_words, pair_elems,
                     gt_elems, pred_elems, conf_elems, w.bitmap, w.pair, gt_key, gt_area, pred_area, confusion);
  MBV_CHECK_LAUNCH();
  // the y dimension of the grid walks the frames; x covers the longest frame (blocks past a frame's end exit at once)
  const unsigned bx = (unsigned)((total + kThreads - 1) / kThreads);
  if (total > 0) {
    hipLaunchKernelGGL(k_panoptic_mark, dim3(bx, frames), dim3(kThreads), 0, stream, gt_word, total, frame_offsets, class_lut,
                       (int)lut_len, (int)C, w.bitmap);
    MBV_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_panoptic_index, dim3(frames), dim3(kWide), 0, stream, (int)C, (int)max_gt, w.bitmap, w.prefix, n_gt,
                     gt_key);
  MBV_CHECK_LAUNCH();
  if (total > 0) {
    hipLaunchKernelGGL(k_panoptic_count, dim3(bx, frames), dim3(kThreads), 0, stream, pred_query, gt_word, total,
                       frame_offsets, query_class, (int)P, class_lut, (int)lut_len, (int)C, (int)max_gt, w.bitmap, w.prefix,
                       w.pair, gt_area, pred_area, confusion);
    MBV_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_panoptic_match, dim3(frames), dim3(kWide), 0, stream, query_class, (int)P, (int)C, (int)max_gt,
                     (int)min_points, w.pair, n_gt, gt_key, gt_area, pred_area, frame_stats, frame_iou);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
