// K27 — the inner loop of the KITTI object protocol for the BEV metric, for every frame and every score threshold at once.
//
// Stands where compute_statistics_jit / fused_compute_statistics (mask_bev/evaluation/kitti_eval.py:266-443, metric == 1) run
// on the host, frame by frame and threshold by threshold.  One thread per (frame, threshold) runs the protocol's greedy
// assignment serially — a few dozen ground truths times up to a few hundred detections: clarity beats speed — with its
// "assigned" flags in a global workspace, and adds its tp / fp / fn to the (T, 3) int64 sums with integer atomics: the sums
// are exact, so their order does not matter.
//
// The protocol, per frame.  Codes: ground truth 0 = counted, 1 = of the class but ignored at this difficulty (or a
// neighbouring class), -1 = another class; detection 0 = counted, 1 = ignored, -1 = another class.
//   Every ground truth that is not -1 looks, in table order, for a detection that is not -1, not yet assigned and (when
//   false positives are counted) not below the score threshold, with overlap > min_overlap:
//     without false positives: the one with the highest score (the first of equal scores);
//     with false positives: among the counted detections the one with the largest overlap (the first of equal overlaps); an
//     ignored detection is taken only while nothing else has been found, and any counted candidate replaces it.
//   Nothing found and the ground truth counted: a false negative.  Found, and the ground truth or the detection ignored:
//   the detection is assigned, nothing is counted.  Found otherwise: a true positive, the detection is assigned.
//   False positives: the detections that are counted, not below the threshold and not assigned.
// DontCare regions and the orientation score belong to the image-box metric and are not part of this kernel.
#include "common.hpp"

namespace {

constexpr int kThreads = 64;

__global__ void __launch_bounds__(kThreads) k_kitti_stats(const float* __restrict__ overlaps,
                                                          const int64_t* __restrict__ pair_offsets,
                                                          const int32_t* __restrict__ dt_offsets,
                                                          const int32_t* __restrict__ gt_offsets, int frames,
                                                          int64_t n_dt, int64_t n_gt, int64_t n_pairs,
                                                          const int32_t* __restrict__ ignored_gt,
                                                          const int32_t* __restrict__ ignored_dt,
                                                          const float* __restrict__ dt_scores, double min_overlap,
                                                          const float* __restrict__ thresholds, int num_thresholds,
                                                          int compute_fp, unsigned long long* __restrict__ stats,
                                                          float* __restrict__ tp_scores, int32_t* __restrict__ tp_flags,
                                                          uint8_t* __restrict__ assigned_ws) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (int64_t)frames * num_thresholds) return;
  const int f = (int)(idx / num_thresholds), t = (int)(idx % num_thresholds);
  const int64_t d0 = dt_offsets[f], d1 = dt_offsets[f + 1], g0 = gt_offsets[f], g1 = gt_offsets[f + 1];
  const int64_t p0 = pair_offsets[f];
  const int64_t nd = d1 - d0, ng = g1 - g0;
  // offsets that disagree with the tables: the frame is left out, nothing outside the tables is touched
  if (d0 < 0 || g0 < 0 || nd < 0 || ng < 0 || d1 > n_dt || g1 > n_gt || p0 < 0 || p0 + nd * ng > n_pairs) return;
  const float thresh = thresholds[t];
  const float* __restrict__ ov = overlaps + p0;                        // (nd, ng): detection j, ground truth i at j * ng + i
  uint8_t* __restrict__ assigned = assigned_ws + (int64_t)t * n_dt + d0;
  for (int64_t j = 0; j < nd; ++j) assigned[j] = 0;

  unsigned long long tp = 0, fp = 0, fn = 0;
  for (int64_t i = 0; i < ng; ++i) {
    const int gcode = ignored_gt[g0 + i];
    const bool record = tp_flags != nullptr && t == 0;
    if (record) { tp_flags[g0 + i] = 0; tp_scores[g0 + i] = 0.f; }
    if (gcode == -1) continue;
    int64_t det = -1;
    float best_score = 0.f;
    double best_overlap = 0.0;
    bool took_ignored = false;
    for (int64_t j = 0; j < nd; ++j) {
      const int dcode = ignored_dt[d0 + j];
      if (dcode == -1 || assigned[j]) continue;
      const float score = dt_scores[d0 + j];
      if (compute_fp && score < thresh) continue;
      const double o = (double)ov[j * ng + i];
      if (!(o > min_overlap)) continue;
      if (!compute_fp) {
        if (det < 0 || score > best_score) { det = j; best_score = score; }
      } else if (dcode == 0 && (o > best_overlap || took_ignored)) {
        det = j; best_overlap = o; took_ignored = false;
      } else if (dcode == 1 && det < 0) {
        det = j; took_ignored = true;
      }
    }
    if (det < 0) {
      fn += gcode == 0 ? 1 : 0;
    } else {
      assigned[det] = 1;
      if (gcode == 0 && ignored_dt[d0 + det] == 0) {
        tp += 1;
        if (record) { tp_flags[g0 + i] = 1; tp_scores[g0 + i] = dt_scores[d0 + det]; }
      }
    }
  }
  if (compute_fp) {
    for (int64_t j = 0; j < nd; ++j)
      fp += (ignored_dt[d0 + j] == 0 && !assigned[j] && !(dt_scores[d0 + j] < thresh)) ? 1 : 0;
  }
  if (tp) atomicAdd(stats + t * 3 + 0, tp);
  if (fp) atomicAdd(stats + t * 3 + 1, fp);
  if (fn) atomicAdd(stats + t * 3 + 2, fn);
}

}  // namespace

extern "C" size_t mbv_kitti_statistics_workspace_bytes(int64_t n_dt, int32_t num_thresholds) {
  if (n_dt < 0 || num_thresholds < 1) return 0;
  return mbv_align_up((size_t)(n_dt > 0 ? n_dt : 1) * (size_t)num_thresholds, 256);
}

extern "C" int mbv_kitti_statistics(const float* overlaps, const int64_t* pair_offsets, const int32_t* dt_offsets,
                                    const int32_t* gt_offsets, int32_t frames, int64_t n_dt, int64_t n_gt, int64_t n_pairs,
                                    const int32_t* ignored_gt, const int32_t* ignored_dt, const float* dt_scores,
                                    double min_overlap, const float* thresholds, int32_t num_thresholds, int32_t compute_fp,
                                    int64_t* stats, float* tp_scores, int32_t* tp_flags, void* workspace,
                                    size_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (frames < 1 || n_dt < 0 || n_gt < 0 || n_pairs < 0 || num_thresholds < 1 || num_thresholds > 65535) return MBV_ERR_BAD_ARG;
  if (!pair_offsets || !dt_offsets || !gt_offsets || !thresholds || !stats || !workspace) return MBV_ERR_BAD_ARG;
  if ((n_dt > 0 && (!ignored_dt || !dt_scores)) || (n_gt > 0 && !ignored_gt) || (n_pairs > 0 && !overlaps)) return MBV_ERR_BAD_ARG;
  if ((tp_scores == nullptr) != (tp_flags == nullptr)) return MBV_ERR_BAD_ARG;
  if (workspace_bytes < mbv_kitti_statistics_workspace_bytes(n_dt, num_thresholds)) return MBV_ERR_WORKSPACE;
  MBV_CHECK_HIP(mbv_fill_async(stats, 0, sizeof(int64_t) * 3 * (size_t)num_thresholds, stream));
  const int64_t threads = (int64_t)frames * num_thresholds;
  hipLaunchKernelGGL(k_kitti_stats, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, overlaps,
                     pair_offsets, dt_offsets, gt_offsets, (int)frames, n_dt, n_gt, n_pairs, ignored_gt, ignored_dt, dt_scores,
                     min_overlap, thresholds, (int)num_thresholds, (int)compute_fp,
                     reinterpret_cast<unsigned long long*>(stats), tp_scores, tp_flags, reinterpret_cast<uint8_t*>(workspace));
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
