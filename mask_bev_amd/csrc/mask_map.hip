// K29 — COCO mask AP on the device: the per-image part of the `map_metric` slot (mask_bev/mask_bev_module.py:85-94,
// fed at mask_bev/models/head/mask_bev_panoptic_head.py:87-96), which the reference hands as dense masks to torchmetrics'
// MeanAveragePrecision(iou_type='segm') and, through it, to pycocotools at `compute`.
//
// K29a  mbv_pairwise_mask_overlap: a binary GEMM per image on bit-packed masks, inter[q][g] = Σ_k popc(pred[q][k] & gt[g][k]),
//       with the row areas from a pre-pass.  A workgroup owns a 64 x 32 (pred x gt) tile of one image and up to 1024 words of
//       the contraction; it streams 128-word chunks of both operands through LDS.  A thread owns one pred row and eight gt
//       rows: the lanes of a wave read 64 different pred rows (row stride 129 words: 32 consecutive lanes on 32 banks) and
//       the same gt words (one address: a broadcast, read 16 bytes at a time), 32 popcounts per 12 LDS reads, accumulators
//       in registers.  The contraction splits are joined with integer atomics: exact, so their order does not matter.
//       Most ground-truth slots are zero padding (the dataset pads to num_queries): a tile whose gt rows are all empty
//       leaves the zeros of the fill.  Integer work only, no MFMA.
// K29b  mbv_coco_match: COCOeval.evaluateImg (pycocotools cocoeval.py) for every image, class, area range and IoU threshold
//       in one launch, from K29a's integer tables.  One workgroup per image; the score order is computed once per image in
//       LDS; one thread per (class, area range, threshold) then runs the greedy matching serially — clarity beats speed, as in
//       K27.  Its "taken" flags are bit a * T + t of one 64-bit LDS word per ground truth, the matched / ignored flags the
//       same bit of one word per detection; the words are stored coalesced at the end.
//
// The protocol of K29b, per (image, class c, area range [lo, hi], threshold t):
//   detections of label c in descending score, ties in index order, the first max_det of them; rank = position in that order;
//   a ground truth of label c is ignored iff its area is outside [lo, hi] (f64 comparison);
//   iou = (double)inter / (double)(pred_area + gt_area - inter), 0 when the union is 0;
//   a detection looks through the not yet taken, not ignored ground truths of its class in index order, then — only if it
//   found nothing — through the ignored ones; every comparison is `iou >= best` with best starting at min(t, 1 - 1e-10), so
//   the last of equal IoUs wins;
//   matched: the ground truth is taken, and the detection is ignored iff the ground truth is;
//   unmatched: the detection is ignored iff its own area is outside [lo, hi].
#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kTileQ = 64;              // pred rows of a tile: one per lane
constexpr int kTileG = 32;              // gt rows of a tile: kGPerThread for each of the four waves
constexpr int kGPerThread = 8;
constexpr int kChunk = 128;             // words of the contraction staged per pass
constexpr int kPredStride = kChunk + 1; // odd: lane l reads bank (l + k) % 32
constexpr int kSplitWords = 1024;       // words of the contraction per workgroup
constexpr int kMaxRows = 1024;          // Q, G
constexpr int kRankNone = 1 << 30;

static_assert(kTileG == kGPerThread * (kThreads / 64), "a wave owns kGPerThread gt rows");
static_assert(kChunk % 4 == 0, "16-byte reads of the gt rows");

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one workgroup per row of the two tables: the first pred_rows blocks take the pred rows, the others the gt rows
__global__ void __launch_bounds__(kThreads) k_mask_row_areas(const uint32_t* __restrict__ pred, int64_t pred_rows,
                                                             const uint32_t* __restrict__ gt, int64_t gt_rows, int64_t words,
                                                             int32_t* __restrict__ pred_area, int32_t* __restrict__ gt_area) {
  __shared__ int s_part[kThreads / 64];
  const int64_t b = blockIdx.x;
  const bool is_pred = b < pred_rows;
  const int64_t row = is_pred ? b : b - pred_rows;
  if (!is_pred && row >= gt_rows) return;
  const uint32_t* __restrict__ src = (is_pred ? pred : gt) + row * words;
  int n = 0;
  for (int64_t k = threadIdx.x; k < words; k += kThreads) n += __popc(src[k]);
  n = wave_sum_i(n);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) total += s_part[i];
    (is_pred ? pred_area : gt_area)[row] = total;
  }
}

// grid: x = image * ksplit + split of the contraction, y = pred tile, z = gt tile; `inter` arrives zeroed
__global__ void __launch_bounds__(kThreads) k_pairwise_overlap(const uint32_t* __restrict__ pred,
                                                               const uint32_t* __restrict__ gt, int Q, int G, int64_t words,
                                                               int ksplit, const int32_t* __restrict__ gt_area,
                                                               int32_t* __restrict__ inter) {
  __shared__ uint32_t s_pred[kTileQ * kPredStride];
  __shared__ __attribute__((aligned(16))) uint32_t s_gt[kTileG * kChunk];
  const int64_t n = blockIdx.x / ksplit;
  const int split = blockIdx.x % ksplit;
  const int q0 = blockIdx.y * kTileQ, g0 = blockIdx.z * kTileG;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  int any = 0;
  if (tid < kTileG && g0 + tid < G) any = gt_area[n * G + g0 + tid] > 0;
  if (!__syncthreads_or(any)) return;                       // only empty ground truths: the zeros stay

  const int64_t kbeg = (int64_t)split * kSplitWords;
  const int64_t kend = kbeg + kSplitWords < words ? kbeg + kSplitWords : words;
  const uint32_t* __restrict__ pred_n = pred + n * Q * words;
  const uint32_t* __restrict__ gt_n = gt + n * G * words;
  int acc[kGPerThread];
#pragma unroll
  for (int j = 0; j < kGPerThread; ++j) acc[j] = 0;

  for (int64_t k0 = kbeg; k0 < kend; k0 += kChunk) {
    for (int i = tid; i < kTileQ * kChunk; i += kThreads) {
      const int r = i / kChunk, k = i % kChunk;
      const bool in = q0 + r < Q && k0 + k < kend;
      s_pred[r * kPredStride + k] = in ? pred_n[(int64_t)(q0 + r) * words + k0 + k] : 0u;
    }
    for (int i = tid; i < kTileG * kChunk; i += kThreads) {
      const int r = i / kChunk, k = i % kChunk;
      const bool in = g0 + r < G && k0 + k < kend;
      s_gt[i] = in ? gt_n[(int64_t)(g0 + r) * words + k0 + k] : 0u;
    }
    __syncthreads();
    const uint32_t* __restrict__ p_row = s_pred + lane * kPredStride;
    const uint32_t* __restrict__ g_rows = s_gt + wave * kGPerThread * kChunk;
#pragma unroll 2
    for (int k = 0; k < kChunk; k += 4) {
      const uint32_t p0 = p_row[k], p1 = p_row[k + 1], p2 = p_row[k + 2], p3 = p_row[k + 3];
#pragma unroll
      for (int j = 0; j < kGPerThread; ++j) {
        const uint4 g = *reinterpret_cast<const uint4*>(g_rows + j * kChunk + k);
        acc[j] += __popc(p0 & g.x) + __popc(p1 & g.y) + __popc(p2 & g.z) + __popc(p3 & g.w);
      }
    }
    __syncthreads();
  }

  const int q = q0 + lane;
  if (q >= Q) return;
#pragma unroll
  for (int j = 0; j < kGPerThread; ++j) {
    const int g = g0 + wave * kGPerThread + j;
    if (g < G && acc[j] != 0) atomicAdd(inter + (n * Q + q) * G + g, acc[j]);
  }
}

// one workgroup per image
__global__ void __launch_bounds__(kThreads) k_coco_match(const int32_t* __restrict__ inter, const int32_t* __restrict__ pred_area,
                                                         const int32_t* __restrict__ gt_area, const float* __restrict__ scores,
                                                         const int32_t* __restrict__ pred_labels,
                                                         const int32_t* __restrict__ gt_labels, int Q, int G, int L,
                                                         const double* __restrict__ iou_thrs, int T,
                                                         const double* __restrict__ area_ranges, int A, int max_det,
                                                         int32_t* __restrict__ rank, unsigned long long* __restrict__ matched,
                                                         unsigned long long* __restrict__ ignored, int32_t* __restrict__ npig) {
  __shared__ float s_score[kMaxRows];
  __shared__ int s_label[kMaxRows];            // -1: outside 0 .. L-1
  __shared__ int s_parea[kMaxRows];
  __shared__ int s_order[kMaxRows];            // detections by (label, -score, index); -1: no detection
  __shared__ int s_glabel[kMaxRows];
  __shared__ int s_garea[kMaxRows];
  __shared__ unsigned long long s_taken[kMaxRows];
  __shared__ unsigned long long s_matched[kMaxRows];
  __shared__ unsigned long long s_ignored[kMaxRows];
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x;
  for (int d = tid; d < Q; d += kThreads) {
    const int lab = pred_labels[n * Q + d];
    s_label[d] = (lab >= 0 && lab < L) ? lab : -1;
    s_score[d] = scores[n * Q + d];
    s_parea[d] = pred_area[n * Q + d];
    s_order[d] = -1;
    s_matched[d] = 0ull;
    s_ignored[d] = 0ull;
  }
  for (int g = tid; g < G; g += kThreads) {
    const int lab = gt_labels[n * G + g];
    s_glabel[g] = (lab >= 0 && lab < L) ? lab : -1;
    s_garea[g] = gt_area[n * G + g];
    s_taken[g] = 0ull;
  }
  __syncthreads();

  // the score order: position among all detections with a label, and rank inside the own class
  for (int d = tid; d < Q; d += kThreads) {
    const int lab = s_label[d];
    int r = kRankNone;
    if (lab >= 0) {
      const float sc = s_score[d];
      int before = 0, same = 0;
      for (int e = 0; e < Q; ++e) {
        const int le = s_label[e];
        if (le < 0) continue;
        if (le < lab) {
          ++before;
        } else if (le == lab) {
          const float se = s_score[e];
          same += (se > sc || (se == sc && e < d)) ? 1 : 0;
        }
      }
      s_order[before + same] = d;
      if (same < max_det) r = same;
    }
    rank[n * Q + d] = r;
  }
  __syncthreads();

  const int AT = A * T;
  for (int item = tid; item < L * AT; item += kThreads) {
    const int c = item / AT, at = item % AT, a = at / T, t = at % T;
    const unsigned long long bit = 1ull << at;
    const double lo = area_ranges[2 * a], hi = area_ranges[2 * a + 1];
    const double thr = iou_thrs[t];
    int start = 0, count = 0;
    for (int e = 0; e < Q; ++e) {
      start += (s_label[e] >= 0 && s_label[e] < c) ? 1 : 0;
      count += s_label[e] == c ? 1 : 0;
    }
    if (t == 0) {
      int counted = 0;
      for (int g = 0; g < G; ++g) {
        const double ga = (double)s_garea[g];
        counted += (s_glabel[g] == c && lo <= ga && ga <= hi) ? 1 : 0;
      }
      npig[(n * L + c) * A + a] = counted;
    }
    if (count > max_det) count = max_det;
    for (int r = 0; r < count; ++r) {
      const int d = s_order[start + r];
      if (d < 0) continue;                                  // scores that do not order (NaN) leave holes
      const int pa = s_parea[d];
      const int32_t* __restrict__ row = inter + (n * Q + d) * G;
      double best = thr < 1.0 - 1e-10 ? thr : 1.0 - 1e-10;
      int m = -1;
      bool m_ignored = false;
      for (int pass = 0; pass < 2 && m < 0; ++pass) {      // the ignored ground truths only if nothing was found
        for (int g = 0; g < G; ++g) {
          if (s_glabel[g] != c) continue;
          const int ga = s_garea[g];
          const bool g_ignored = !(lo <= (double)ga && (double)ga <= hi);
          if (g_ignored != (pass == 1) || (s_taken[g] & bit)) continue;
          const int in = row[g];
          const int64_t uni = (int64_t)pa + ga - in;
          const double iou = uni > 0 ? (double)in / (double)uni : 0.0;
          if (iou < best) continue;
          best = iou;
          m = g;
          m_ignored = g_ignored;
        }
      }
      if (m >= 0) {
        atomicOr(&s_taken[m], bit);
        atomicOr(&s_matched[d], bit);
        if (m_ignored) atomicOr(&s_ignored[d], bit);
      } else if (!(lo <= (double)pa && (double)pa <= hi)) {
        atomicOr(&s_ignored[d], bit);
      }
    }
  }
  __syncthreads();
  for (int d = tid; d < Q; d += kThreads) {
    matched[n * Q + d] = s_matched[d];
    ignored[n * Q + d] = s_ignored[d];
  }
}

}  // namespace

extern "C" int mbv_pairwise_mask_overlap(const uint32_t* pred_words, const uint32_t* gt_words, int32_t N, int32_t Q, int32_t G,
                                         int64_t words, int32_t* inter, int32_t* pred_area, int32_t* gt_area, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (N < 0 || Q < 0 || G < 0 || words < 0) return MBV_ERR_BAD_ARG;
  if (Q > kMaxRows || G > kMaxRows || words > ((int64_t)1 << 26)) return MBV_ERR_UNSUPPORTED;
  const int64_t pred_rows = (int64_t)N * Q, gt_rows = (int64_t)N * G;
  const bool empty = pred_rows == 0 || gt_rows == 0;      // no pair: MBV_OK whatever the pointers are
  const int ksplit = (int)((words + kSplitWords - 1) / kSplitWords);
  if (pred_rows + gt_rows > 0x7fffffff || (int64_t)N * (ksplit > 0 ? ksplit : 1) > 0x7fffffff) return MBV_ERR_UNSUPPORTED;
  // the area pre-pass; without pairs it fills the table that has rows, if it was given
  const bool do_pred = pred_rows > 0 && pred_area && (words == 0 || pred_words);
  const bool do_gt = gt_rows > 0 && gt_area && (words == 0 || gt_words);
  if (!empty && (!inter || !do_pred || !do_gt)) return MBV_ERR_BAD_ARG;
  const int64_t blocks_pred = do_pred ? pred_rows : 0, blocks_gt = do_gt ? gt_rows : 0;
  if (blocks_pred + blocks_gt > 0) {
    hipLaunchKernelGGL(k_mask_row_areas, dim3((unsigned)(blocks_pred + blocks_gt)), dim3(kThreads), 0, stream, pred_words,
                       blocks_pred, gt_words, blocks_gt, words, pred_area, gt_area);
    MBV_CHECK_LAUNCH();
  }
  if (empty) return MBV_OK;
  MBV_CHECK_HIP(mbv_fill_async(inter, 0, sizeof(int32_t) * (size_t)pred_rows * (size_t)G, stream));
  if (words == 0) return MBV_OK;
  const dim3 grid((unsigned)((int64_t)N * ksplit), (unsigned)((Q + kTileQ - 1) / kTileQ), (unsigned)((G + kTileG - 1) / kTileG));
  hipLaunchKernelGGL(k_pairwise_overlap, grid, dim3(kThreads), 0, stream, pred_words, gt_words, (int)Q, (int)G, words, ksplit,
                     gt_area, inter);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_coco_match(const int32_t* inter, const int32_t* pred_area, const int32_t* gt_area, const float* scores,
                              const int32_t* pred_labels, const int32_t* gt_labels, int32_t N, int32_t Q, int32_t G,
                              int32_t num_labels, const double* iou_thrs, int32_t T, const double* area_ranges, int32_t A,
                              int32_t max_det, int32_t* rank, int64_t* matched, int64_t* ignored, int32_t* npig, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (N < 0 || Q < 0 || G < 0 || num_labels < 1 || T < 1 || A < 1 || max_det < 1) return MBV_ERR_BAD_ARG;
  if (Q > kMaxRows || G > kMaxRows || (int64_t)T * A > 64 || num_labels > (1 << 16)) return MBV_ERR_UNSUPPORTED;
  if (N == 0) return MBV_OK;
  if (!iou_thrs || !area_ranges || !npig) return MBV_ERR_BAD_ARG;
  if (Q > 0 && (!pred_area || !scores || !pred_labels || !rank || !matched || !ignored)) return MBV_ERR_BAD_ARG;
  if (G > 0 && (!gt_area || !gt_labels)) return MBV_ERR_BAD_ARG;
  if (Q > 0 && G > 0 && !inter) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_coco_match, dim3((unsigned)N), dim3(kThreads), 0, stream, inter, pred_area, gt_area, scores, pred_labels,
                     gt_labels, (int)Q, (int)G, (int)num_labels, iou_thrs, (int)T, area_ranges, (int)A, (int)max_det, rank,
                     reinterpret_cast<unsigned long long*>(matched), reinterpret_cast<unsigned long long*>(ignored), npig);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
