// K33 — instance tracking over a sequence and tube association (the S_assoc term of LSTQ).  The rules are in
// include/maskbev_hip.h (K33a, K37, K38b, K33b); this file restates nothing, it implements them.
//
// The tracker is ONE step with two optional parts, behind one host driver (track_frames) that the three entries fill a
// TrackCall for: mbv_track_frames (K33a, neither part), mbv_track_frames_motion (K37, the motion part) and
// mbv_track_frames_occluded (K38b, both).  Per frame, all on the caller's stream, no host synchronisation:
//   1. clear     zeroes area_q, area_t and the (Q, P) intersection table of the workspace.  [motion] also fills the advected
//                map, zeroes the centroid sums and writes the cell shift of every live track; [occlusion] zeroes hidden.
//   2. advect    [motion only, the fifth launch] one thread per cell, unsigned atomicMin: the smallest track index wins a cell.
//   3. count     one thread per cell (blocks of 256): the f64 warp of the cell centre into the previous frame's grid, one
//                rounding per operation (-ffp-contract=off), the warped track index to the workspace; area_q and area_t in
//                LDS tables (integer LDS atomics, one flush per block), the intersection table with global integer atomics.
//                [motion] reads the advected map instead of the state map; the index sums of a query's cells per block in
//                LDS, flushed with 64-bit global atomics.  [occlusion] also sums hidden[t], the cells of a warped footprint
//                whose visibility byte is 0, in a fifth LDS table.
//   4. match     ONE workgroup of 1024: the candidate pairs are compacted into a list; then rounds in which every untaken
//                row and column takes its best candidate under the exact order (IoU by i64 cross-multiplication, then q,
//                then t) and a pair that is the best of both is taken.  Such a pair is the first of the remaining order
//                among all pairs that share its query or its track, so the greedy walk takes it too; taking it removes
//                what the walk would skip.  By induction the rounds end with the walk's result, and each round takes at
//                least the first remaining pair.  Then the update of the live list with three block scans.  [motion] after
//                the IoU rounds: centroids, predictions, the gate candidates and the same mutual-best rounds under the order
//                (d2, q, t); the update also of pos / vel.  [occlusion] reads hidden and live_held and lets an unmatched
//                track whose footprint was mostly out of sight keep its age; live_held goes through the compaction.
//   5. paint     one thread per cell: the new state map and the optional map of global ids.
// clear, count and match are one template each: <false> is K33a's kernel and touches nothing of the motion part; K37 runs
// <true> / <true, false>; K38b runs <true, true> whatever `visibility` is, and with visibility == NULL or max_hold == 0 holds
// no track: the step is then K37's bit for bit.
// K33b: accumulate (grid-stride blocks with LDS tables for the two size tables where they fit), scores (one workgroup per
// row; the terms of 256 tracks at a time in LDS, summed by one thread in ascending order) and the class sums.
// Integer atomics only; every f64 sum in a fixed order: two runs are bit-equal.  Every index comes from the sizes: a query, a
// stored track index, a counter or a label word that disagrees with them changes results, never addresses.
#include "common.hpp"

namespace {

constexpr int kThreads = 256, kWide = 1024, kMaxTracks = 1024, kMaxClasses = 16, kLdsTable = 4096;
constexpr int64_t kMaxCells = 1024 * 1024;

struct TrackWorkspace {
  int32_t* warped;   // (H, W): the old track index under every current cell, -1 for none
  int32_t* area_q;   // (Q)
  int32_t* area_t;   // (P)
  int32_t* inter;    // (Q, P)
  int32_t* cand;     // (Q * P): q * P + t of the candidate pairs, in no order
  int32_t* q_new;    // (Q): the new local index of a present query, else -1
  int32_t* t_new;    // (P): the new local index of an appended old track, else -1
  // K37 only
  uint32_t* moved;   // (H, W): the advected state map; all-ones (-1 as i32) for none
  int64_t* sum_ix;   // (Q): the sum of ix over the cells of a query
  int64_t* sum_iy;   // (Q)
  int32_t* shift;    // (P, 2): sx, sy of every live track in cells
  double* cq;        // (Q, 2): the centroid of a present query
  double* pred;      // (P, 2): the predicted centroid of a live track in the current frame
  double* velr;      // (P, 2): its velocity in the current frame's axes
  // K38b only
  int32_t* hidden;   // (P): the cells of a warped footprint with visibility 0
  size_t bytes;
};

TrackWorkspace carve_track(void* ws, int64_t cells, int Q, int P, bool motion = false, bool occlusion = false) {
  MbvCarver c(ws);
  TrackWorkspace w{};
  w.warped = c.take<int32_t>(cells);
  w.area_q = c.take<int32_t>(Q);
  w.area_t = c.take<int32_t>(P);
  w.inter = c.take<int32_t>((int64_t)Q * P);
  w.cand = c.take<int32_t>((int64_t)Q * P);
  w.q_new = c.take<int32_t>(Q);
  w.t_new = c.take<int32_t>(P);
  if (motion) {
    w.moved = c.take<uint32_t>(cells);
    w.sum_ix = c.take<int64_t>(Q);
    w.sum_iy = c.take<int64_t>(Q);
    w.shift = c.take<int32_t>(2 * (int64_t)P);
    w.cq = c.take<double>(2 * (int64_t)Q);
    w.pred = c.take<double>(2 * (int64_t)P);
    w.velr = c.take<double>(2 * (int64_t)P);
  }
  if (occlusion) w.hidden = c.take<int32_t>(P);
  w.bytes = c.off;
  return w;
}

__device__ __forceinline__ int live_count(const int32_t* __restrict__ counters, int P) {
  const int n = counters[0];
  return n < 0 ? 0 : (n > P ? P : n);
}

__device__ __forceinline__ void add64(int64_t* p, int64_t n) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)n);
}

// <false>: area_q, area_t and the intersection table, and nothing else is read or written.  <true>: also the advected map,
// the centroid sums and step 0's cell shift of every track; the hidden table where there is one.
template <bool kMotion>
__global__ void __launch_bounds__(kThreads) k_track_clear(int64_t cells, int Q, int P, double voxel, int max_shift,
                                                          const int32_t* __restrict__ counters, const double* __restrict__ vel,
                                                          int32_t* __restrict__ area_q, int32_t* __restrict__ area_t,
                                                          int32_t* __restrict__ inter, uint32_t* __restrict__ moved,
                                                          int64_t* __restrict__ sum_ix, int64_t* __restrict__ sum_iy,
                                                          int32_t* __restrict__ shift, int32_t* __restrict__ hidden) {
  const int64_t stride = (int64_t)gridDim.x * kThreads, n = (int64_t)Q * P;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int n_live = 0;
  if constexpr (kMotion) n_live = live_count(counters, P);
  for (int64_t i = t; i < n; i += stride) inter[i] = 0;
  if constexpr (kMotion)
    for (int64_t i = t; i < cells; i += stride) moved[i] = 0xffffffffu;
  for (int64_t i = t; i < Q; i += stride) {
    area_q[i] = 0;
    if constexpr (kMotion) {
      sum_ix[i] = 0;
      sum_iy[i] = 0;
    }
  }
  for (int64_t i = t; i < P; i += stride) {
    area_t[i] = 0;
    if constexpr (kMotion) {
      if (hidden) hidden[i] = 0;
      double sx = 0.0, sy = 0.0;
      if (i < n_live) {
        sx = rint(vel[2 * i] / voxel);
        sy = rint(vel[2 * i + 1] / voxel);
        if (!(fabs(sx) <= (double)max_shift && fabs(sy) <= (double)max_shift)) sx = sy = 0.0;   // NaN and inf land here
      }
      shift[2 * i] = (int32_t)sx;                                  // |sx| <= max_shift < 2^31
      shift[2 * i + 1] = (int32_t)sy;
    }
  }
}

__global__ void __launch_bounds__(kThreads) k_track_advect(const int32_t* __restrict__ state_map, int H, int W, int P,
                                                           const int32_t* __restrict__ counters,
                                                           const int32_t* __restrict__ shift, uint32_t* __restrict__ moved) {
  const int64_t cells = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= cells) return;
  const int t = state_map[i];
  if (t < 0 || t >= live_count(counters, P)) return;
  const int iy = (int)(i / W), ix = (int)(i - (int64_t)iy * W);
  const int64_t tx = (int64_t)ix + shift[2 * t], ty = (int64_t)iy + shift[2 * t + 1];
  if (tx >= 0 && tx < W && ty >= 0 && ty < H) atomicMin(&moved[ty * W + tx], (uint32_t)t);
}

template <bool kMotion, bool kOcclusion = false>
__global__ void __launch_bounds__(kThreads) k_track_count(const int32_t* __restrict__ instance_map,
                                                          const int32_t* __restrict__ state_map,
                                                          const double* __restrict__ prev_from_cur, int H, int W, double x_lo,
                                                          double y_lo, double voxel, int Q, int P,
                                                          const int32_t* __restrict__ counters, int32_t* __restrict__ warped,
                                                          int32_t* __restrict__ area_q, int32_t* __restrict__ area_t,
                                                          int32_t* __restrict__ inter, int64_t* __restrict__ sum_ix,
                                                          int64_t* __restrict__ sum_iy,
                                                          const uint8_t* __restrict__ visibility,
                                                          int32_t* __restrict__ hidden) {
  __shared__ int32_t s_q[kMaxTracks];
  __shared__ int32_t s_t[kMaxTracks];
  // K37: a block of 256 cells adds at most 256 * 2^20 < 2^31 to a slot, so i32 holds a block's index sums
  __shared__ int32_t s_x[kMotion ? kMaxTracks : 1];
  __shared__ int32_t s_y[kMotion ? kMaxTracks : 1];
  __shared__ int32_t s_h[kOcclusion ? kMaxTracks : 1];             // K38b: hidden, per block
  const int n_live = live_count(counters, P);
  if constexpr (kOcclusion)
    for (int k = threadIdx.x; k < P; k += kThreads) s_h[k] = 0;
  if constexpr (kMotion)
    for (int k = threadIdx.x; k < Q; k += kThreads) s_x[k] = s_y[k] = 0;
  for (int k = threadIdx.x; k < Q; k += kThreads) s_q[k] = 0;
  for (int k = threadIdx.x; k < P; k += kThreads) s_t[k] = 0;
  __syncthreads();
  const int64_t cells = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < cells) {
    const int iy = (int)(i / W), ix = (int)(i - (int64_t)iy * W);
    const double x = x_lo + ((double)ix + 0.5) * voxel;
    const double y = y_lo + ((double)iy + 0.5) * voxel;
    const double xp = (prev_from_cur[0] * x + prev_from_cur[1] * y) + prev_from_cur[2];
    const double yp = (prev_from_cur[3] * x + prev_from_cur[4] * y) + prev_from_cur[5];
    const double fx = floor((xp - x_lo) / voxel), fy = floor((yp - y_lo) / voxel);
    int t = -1;
    if (fx >= 0.0 && fx < (double)W && fy >= 0.0 && fy < (double)H) {       // NaN and inf fail a comparison
      t = state_map[(int64_t)(int)fy * W + (int)fx];
      if (t < 0 || t >= n_live) t = -1;
    }
    warped[i] = t;
    int q = instance_map[i];
    if (q < 0 || q >= Q) q = -1;
    if (q >= 0) atomicAdd(&s_q[q], 1);
    if constexpr (kMotion) {
      if (q >= 0) {
        atomicAdd(&s_x[q], ix);
        atomicAdd(&s_y[q], iy);
      }
    }
    if (t >= 0) atomicAdd(&s_t[t], 1);
    if constexpr (kOcclusion) {
      if (t >= 0 && visibility && visibility[i] == 0) atomicAdd(&s_h[t], 1);
    }
    if (q >= 0 && t >= 0) atomicAdd(&inter[(int64_t)q * P + t], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < Q; k += kThreads) {
    const int32_t n = s_q[k];
    if (n > 0) atomicAdd(&area_q[k], n);
    if constexpr (kMotion) {
      if (n > 0) {
        add64(&sum_ix[k], s_x[k]);
        add64(&sum_iy[k], s_y[k]);
      }
    }
  }
  for (int k = threadIdx.x; k < P; k += kThreads) {
    const int32_t n = s_t[k];
    if (n > 0) atomicAdd(&area_t[k], n);
    if constexpr (kOcclusion) {
      if (n > 0 && s_h[k] > 0) atomicAdd(&hidden[k], s_h[k]);
    }
  }
}

// inclusive scan of one value per thread of a workgroup of kWide, through s_scan; every thread must call it
__device__ __forceinline__ int32_t block_scan(int32_t mine, int32_t* s_scan) {
  const int t = threadIdx.x;
  __syncthreads();
  s_scan[t] = mine;
  __syncthreads();
  for (int o = 1; o < kWide; o <<= 1) {
    const int32_t v = t >= o ? s_scan[t - o] : 0;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  return s_scan[t];
}

struct MatchTables {
  const int32_t* inter;
  const int32_t* area_q;     // LDS
  const int32_t* area_t;     // LDS
  int P;
};

// whether candidate pair a (= q * P + t) comes before pair b in the matching order
__device__ __forceinline__ bool pair_before(const MatchTables& m, int32_t a, int32_t b) {
  const int qa = a / m.P, ta = a - qa * m.P, qb = b / m.P, tb = b - qb * m.P;
  const int64_t ia = m.inter[a], ib = m.inter[b];
  const int64_t ua = (int64_t)m.area_q[qa] + m.area_t[ta] - ia, ub = (int64_t)m.area_q[qb] + m.area_t[tb] - ib;
  const int64_t lhs = ia * ub, rhs = ib * ua;                      // < 2^41: areas are at most 2^20 cells
  if (lhs != rhs) return lhs > rhs;
  return a < b;                                                    // q * P + t: the smaller q, then the smaller t
}

// K37's second stage: the tables are in global memory, written by this workgroup before a barrier (no __restrict__)
struct GateTables {
  const double* cq;          // (Q, 2)
  const double* pred;        // (P, 2)
  int P;
};

__device__ __forceinline__ double gate_d2(const double* cq, const double* pred, int q, int t) {
  const double dx = cq[2 * q] - pred[2 * t], dy = cq[2 * q + 1] - pred[2 * t + 1];
  return dx * dx + dy * dy;
}

// the order (d2, q, t); a candidate's d2 is never NaN: it passed d2 <= gate * gate
__device__ __forceinline__ bool pair_before(const GateTables& m, int32_t a, int32_t b) {
  const int qa = a / m.P, ta = a - qa * m.P, qb = b / m.P, tb = b - qb * m.P;
  const double da = gate_d2(m.cq, m.pred, qa, ta), db = gate_d2(m.cq, m.pred, qb, tb);
  if (da != db) return da < db;
  return a < b;
}

template <class Tables>
__device__ __forceinline__ void offer_best(const Tables& m, int32_t* slot, int32_t pair) {
  int32_t cur = *slot;
  while (cur < 0 || pair_before(m, pair, cur)) {
    const int32_t seen = atomicCAS(slot, cur, pair);
    if (seen == cur) break;
    cur = seen;
  }
}

// The mutual-best rounds over cand[0 .. n_cand) under the order of `m`: valid for any strict total order.  Every thread of
// the workgroup must call it.
template <class Tables>
__device__ __forceinline__ void match_rounds(const Tables& m, const int32_t* cand, int n_cand, int Q, int P, int32_t* s_best_q,
                                             int32_t* s_best_t, int32_t* s_q_match, int32_t* s_t_taken, int32_t* s_open) {
  const int t = threadIdx.x;
  for (int round = 0; round < kMaxTracks; ++round) {               // every round takes a pair or is the last
    if (t < Q) s_best_q[t] = -1;
    if (t < P) s_best_t[t] = -1;
    if (t == 0) *s_open = 0;
    __syncthreads();
    for (int k = t; k < n_cand; k += kWide) {
      const int32_t pair = cand[k];
      const int q = pair / P, tr = pair - q * P;
      if (s_q_match[q] >= 0 || s_t_taken[tr]) continue;
      *s_open = 1;
      offer_best(m, &s_best_q[q], pair);
      offer_best(m, &s_best_t[tr], pair);
    }
    __syncthreads();
    if (!*s_open) break;                                           // uniform: read after the barrier
    if (t < Q) {
      const int32_t pair = s_best_q[t];
      if (pair >= 0) {
        const int tr = pair - t * P;
        if (s_best_t[tr] == pair) {
          s_q_match[t] = tr;
          s_t_taken[tr] = 1;
        }
      }
    }
    __syncthreads();
  }
}

// K37's per-frame arguments of the match kernel; unused (and empty) in K33a's instantiation
struct MotionArgs {
  const double* cur_from_prev;     // (6): n of this frame
  double gain, gate, x_lo, y_lo, voxel;
  const int64_t* sum_ix;           // (Q)
  const int64_t* sum_iy;
  double* cq;                      // workspace (Q, 2)
  double* pred;                    // workspace (P, 2)
  double* velr;                    // workspace (P, 2)
  double* pos;                     // state (P, 2)
  double* vel;
  int32_t* motion_counters;        // state (2)
  double* query_velocity;          // this frame's (Q, 2)
};

// K38b's per-frame arguments of the match kernel; unused (and empty) in the other instantiations
struct OcclusionArgs {
  const int32_t* hidden;           // workspace (P)
  int32_t* live_held;              // state (P)
  int32_t* occlusion_counters;     // state (2)
  int hold_num, hold_den, max_hold;
  int have_visibility;
};

__device__ __forceinline__ double finite_or_zero(double v) { return fabs(v) <= 1.7976931348623157e308 ? v : 0.0; }

template <bool kMotion, bool kOcclusion = false>
__global__ void __launch_bounds__(kWide) k_track_match(int Q, int P, double min_iou, int max_age, int min_cells,
                                                       const int32_t* __restrict__ g_area_q,
                                                       const int32_t* __restrict__ g_area_t,
                                                       const int32_t* __restrict__ inter, int32_t* __restrict__ cand,
                                                       int32_t* __restrict__ live_id, int32_t* __restrict__ live_seen,
                                                       int32_t* __restrict__ counters, int32_t* __restrict__ query_track,
                                                       int32_t* __restrict__ q_new, int32_t* __restrict__ t_new,
                                                       MotionArgs mo, OcclusionArgs oc) {
  __shared__ int32_t s_area_q[kMaxTracks];
  __shared__ int32_t s_area_t[kMaxTracks];
  __shared__ int32_t s_best_q[kMaxTracks];                         // the round's best pair of a row
  __shared__ int32_t s_best_t[kMaxTracks];                         // ... of a column
  __shared__ int32_t s_q_match[kMaxTracks];                        // the track a query took, -1
  __shared__ int32_t s_t_taken[kMaxTracks];
  __shared__ int32_t s_id[kMaxTracks];
  __shared__ int32_t s_seen[kMaxTracks];
  __shared__ int32_t s_scan[kWide];
  __shared__ int32_t s_held[kOcclusion ? kMaxTracks : 1];          // K38b: live_held of the old list
  __shared__ int32_t s_n_cand, s_open, s_n_held;
  const int t = threadIdx.x;
  const int n_live = live_count(counters, P);
  const int32_t next_id = counters[1], frame = counters[2], dropped = counters[3];
  if (t < Q) {
    s_area_q[t] = g_area_q[t];
    s_q_match[t] = -1;
  }
  if (t < P) {
    s_area_t[t] = g_area_t[t];
    s_t_taken[t] = 0;
    s_id[t] = t < n_live ? live_id[t] : -1;
    s_seen[t] = t < n_live ? live_seen[t] : -1;
    if constexpr (kOcclusion) s_held[t] = t < n_live ? oc.live_held[t] : 0;
  }
  if (t == 0) {
    s_n_cand = 0;
    s_n_held = 0;
  }
  __syncthreads();

  // the candidate list
  const int64_t table = (int64_t)Q * n_live;
  for (int64_t k = t; k < table; k += kWide) {
    const int q = (int)(k / n_live), tr = (int)(k - (int64_t)q * n_live);
    const int32_t pair = q * P + tr;
    const int32_t n = inter[pair];
    if (n > 0 && s_area_q[q] >= min_cells) {
      const int64_t uni = (int64_t)s_area_q[q] + s_area_t[tr] - n;
      if ((double)n / (double)uni >= min_iou) cand[atomicAdd(&s_n_cand, 1)] = pair;
    }
  }
  __syncthreads();
  const int n_cand = s_n_cand;
  MatchTables m{inter, s_area_q, s_area_t, P};
  match_rounds(m, cand, n_cand, Q, P, s_best_q, s_best_t, s_q_match, s_t_taken, &s_open);

  // K37, step 3b: the centroids, the predictions, and the gated second stage over what step 3 left open
  __shared__ int32_t s_gated;
  if constexpr (kMotion) {
    const double* n = mo.cur_from_prev;
    if (t < Q && s_area_q[t] >= min_cells) {
      const double area = (double)s_area_q[t];
      mo.cq[2 * t] = mo.x_lo + ((double)mo.sum_ix[t] / area + 0.5) * mo.voxel;
      mo.cq[2 * t + 1] = mo.y_lo + ((double)mo.sum_iy[t] / area + 0.5) * mo.voxel;
    }
    if (t < n_live) {
      const double vx = mo.vel[2 * t], vy = mo.vel[2 * t + 1];
      const double ax = mo.pos[2 * t] + vx, ay = mo.pos[2 * t + 1] + vy;
      mo.pred[2 * t] = (n[0] * ax + n[1] * ay) + n[2];
      mo.pred[2 * t + 1] = (n[3] * ax + n[4] * ay) + n[5];
      mo.velr[2 * t] = n[0] * vx + n[1] * vy;
      mo.velr[2 * t + 1] = n[3] * vx + n[4] * vy;
    }
    if (t == 0) {
      s_n_cand = 0;
      s_gated = 0;
    }
    __syncthreads();                                               // cq, pred and velr are read by other threads from here
    if (mo.gate > 0.0) {                                           // uniform
      const double g2 = mo.gate * mo.gate;
      for (int64_t k = t; k < table; k += kWide) {
        const int q = (int)(k / n_live), tr = (int)(k - (int64_t)q * n_live);
        if (s_area_q[q] < min_cells || s_q_match[q] >= 0 || s_t_taken[tr]) continue;
        if (gate_d2(mo.cq, mo.pred, q, tr) <= g2) cand[atomicAdd(&s_n_cand, 1)] = q * P + tr;   // NaN fails
      }
      const bool open_before = t < Q && s_q_match[t] < 0;
      __syncthreads();
      GateTables g{mo.cq, mo.pred, P};
      match_rounds(g, cand, s_n_cand, Q, P, s_best_q, s_best_t, s_q_match, s_t_taken, &s_open);
      if (open_before && s_q_match[t] >= 0) atomicAdd(&s_gated, 1);
    }
  }

  // the new live list: the present queries in ascending q, then the unmatched old tracks that are young enough
  const bool present = t < Q && s_area_q[t] >= min_cells;
  const int matched = present ? s_q_match[t] : -1;
  const int32_t pos_q = block_scan(present ? 1 : 0, s_scan);
  const int32_t n_present = s_scan[kWide - 1];
  const int32_t born = block_scan(present && matched < 0 ? 1 : 0, s_scan);
  const int32_t n_born = s_scan[kWide - 1];
  // K38b, step 4: an unmatched track whose warped footprint was mostly out of sight keeps its age (seen' and held' are
  // written back to this thread's own slots of the old list, read again only by this thread)
  if constexpr (kOcclusion) {
    if (t < n_live && !s_t_taken[t] && oc.have_visibility && s_area_t[t] > 0 &&
        (int64_t)oc.hidden[t] * oc.hold_den >= (int64_t)s_area_t[t] * oc.hold_num && s_held[t] < oc.max_hold) {
      s_seen[t] += 1;
      s_held[t] += 1;
      atomicAdd(&s_n_held, 1);
    }
  }
  const bool old = t < n_live && !s_t_taken[t] && (int64_t)frame - s_seen[t] <= (int64_t)max_age;
  const int32_t pos_t = block_scan(old ? 1 : 0, s_scan);
  const int32_t n_old = s_scan[kWide - 1];
  const int32_t id_q = present ? (matched >= 0 ? s_id[matched] : next_id + born - 1) : -1;
  const int room = P - n_present;                                  // >= 0: Q <= P
  const int kept = n_old < room ? n_old : room;
  const int n_new = n_present + kept;
  // the old list lives in s_id / s_seen from here on, so every slot of the new one has exactly one writer
  if (t >= n_new && t < P) {
    live_id[t] = -1;
    live_seen[t] = -1;
    if constexpr (kOcclusion) oc.live_held[t] = 0;
  }
  if (t < Q) {
    query_track[t] = id_q;
    q_new[t] = present ? pos_q - 1 : -1;
    if (present) {
      live_id[pos_q - 1] = id_q;
      live_seen[pos_q - 1] = frame;
      if constexpr (kOcclusion) oc.live_held[pos_q - 1] = 0;
    }
  }
  if (t < P) {
    int32_t idx = -1;
    if (old && pos_t - 1 < room) {
      idx = n_present + pos_t - 1;
      live_id[idx] = s_id[t];
      live_seen[idx] = s_seen[t];
      if constexpr (kOcclusion) oc.live_held[idx] = s_held[t];
    }
    t_new[t] = idx;
    if constexpr (kMotion) {
      if (idx >= 0) {                                              // a coasting track moves on with its prediction
        mo.pos[2 * idx] = mo.pred[2 * t];
        mo.pos[2 * idx + 1] = mo.pred[2 * t + 1];
        mo.vel[2 * idx] = finite_or_zero(mo.velr[2 * t]);
        mo.vel[2 * idx + 1] = finite_or_zero(mo.velr[2 * t + 1]);
      }
    }
  }
  if constexpr (kMotion) {
    // pos and vel of the old list were last read before the barrier of step 3b: every slot of the new one has one writer
    if (t >= n_new && t < P) mo.pos[2 * t] = mo.pos[2 * t + 1] = mo.vel[2 * t] = mo.vel[2 * t + 1] = 0.0;
    if (t < Q) {
      double vx = 0.0, vy = 0.0;
      if (present) {
        const double cx = mo.cq[2 * t], cy = mo.cq[2 * t + 1];
        if (matched >= 0) {
          vx = finite_or_zero(mo.velr[2 * matched] + mo.gain * (cx - mo.pred[2 * matched]));
          vy = finite_or_zero(mo.velr[2 * matched + 1] + mo.gain * (cy - mo.pred[2 * matched + 1]));
        }
        mo.pos[2 * (pos_q - 1)] = cx;
        mo.pos[2 * (pos_q - 1) + 1] = cy;
        mo.vel[2 * (pos_q - 1)] = vx;
        mo.vel[2 * (pos_q - 1) + 1] = vy;
      }
      mo.query_velocity[2 * t] = vx;
      mo.query_velocity[2 * t + 1] = vy;
    }
    if (t == 0) {
      mo.motion_counters[0] += s_gated;
      mo.motion_counters[1] = 0;
    }
  }
  if constexpr (kOcclusion) {
    if (t == 0) {
      oc.occlusion_counters[0] += s_n_held;
      oc.occlusion_counters[1] = 0;
    }
  }
  if (t == 0) {
    counters[0] = n_new;
    counters[1] = next_id + n_born;
    counters[2] = frame + 1;
    counters[3] = dropped + (n_old - kept);
  }
}

__global__ void __launch_bounds__(kThreads) k_track_paint(const int32_t* __restrict__ instance_map, int64_t cells, int Q, int P,
                                                          const int32_t* __restrict__ warped,
                                                          const int32_t* __restrict__ q_new, const int32_t* __restrict__ t_new,
                                                          const int32_t* __restrict__ query_track,
                                                          int32_t* __restrict__ state_map, int32_t* __restrict__ track_map) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= cells) return;
  const int q = instance_map[i];
  int32_t idx = -1, id = -1;
  if (q >= 0 && q < Q && q_new[q] >= 0) {
    idx = q_new[q];
    id = query_track[q];
  } else {
    const int w = warped[i];                                       // -1 or below the old n_live <= P
    if (w >= 0 && w < P) idx = t_new[w];
  }
  state_map[i] = idx;
  if (track_map) track_map[i] = id;
}

bool track_sizes_supported(int64_t H, int64_t W, int Q, int P) {
  return H >= 0 && W >= 0 && H <= kMaxCells && W <= kMaxCells && H * W <= kMaxCells && Q >= 0 && Q <= P && P <= kMaxTracks;
}

// ---- K33b -------------------------------------------------------------------------------------------------------------

// the class of a ground-truth word: -1 ignored, 0 everything else, 1 .. C-1 a thing (K32's rule)
__device__ __forceinline__ int tube_class_of(uint32_t word, const int32_t* __restrict__ class_lut, int lut_len, int C) {
  const int sem = (int)(word & 0xffffu);
  if (sem >= lut_len) return -1;
  const int c = class_lut[sem];
  return (c < 0 || c >= C) ? -1 : c;
}

__global__ void __launch_bounds__(kThreads) k_tube_accumulate(const int32_t* __restrict__ pred_track,
                                                              const uint32_t* __restrict__ gt_word, int64_t total,
                                                              const int32_t* __restrict__ class_lut, int lut_len, int C, int I,
                                                              int T, int64_t* __restrict__ gt_size,
                                                              int64_t* __restrict__ pred_size, int32_t* __restrict__ pair,
                                                              int64_t* __restrict__ overflow) {
  __shared__ int32_t s_gt[kLdsTable];
  __shared__ int32_t s_pred[kLdsTable];
  __shared__ int32_t s_over[2];
  const int rows = (C - 1) * I;
  const bool lds_gt = rows <= kLdsTable, lds_pred = T <= kLdsTable;   // a block adds fewer than 2^31 elements to a slot
  if (lds_gt)
    for (int k = threadIdx.x; k < rows; k += kThreads) s_gt[k] = 0;
  if (lds_pred)
    for (int k = threadIdx.x; k < T; k += kThreads) s_pred[k] = 0;
  if (threadIdx.x < 2) s_over[threadIdx.x] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
    const uint32_t word = gt_word[i];
    const int c = tube_class_of(word, class_lut, lut_len, C);
    if (c < 0) continue;                                           // an ignored element takes part in nothing
    int r = -1;
    if (c >= 1) {
      const int inst = (int)(word >> 16);
      if (inst >= I) {
        atomicAdd(&s_over[0], 1);
      } else if (inst >= 1) {
        r = (c - 1) * I + inst;
        if (lds_gt) atomicAdd(&s_gt[r], 1);
        else add64(&gt_size[r], 1);
      }
    }
    const int p = pred_track[i];
    if (p >= T) {
      atomicAdd(&s_over[1], 1);
    } else if (p >= 0) {
      if (lds_pred) atomicAdd(&s_pred[p], 1);
      else add64(&pred_size[p], 1);
      if (r >= 0) atomicAdd(&pair[(int64_t)r * T + p], 1);
    }
  }
  __syncthreads();
  if (lds_gt)
    for (int k = threadIdx.x; k < rows; k += kThreads)
      if (s_gt[k] > 0) add64(&gt_size[k], s_gt[k]);
  if (lds_pred)
    for (int k = threadIdx.x; k < T; k += kThreads)
      if (s_pred[k] > 0) add64(&pred_size[k], s_pred[k]);
  if (threadIdx.x < 2 && s_over[threadIdx.x] > 0) add64(&overflow[threadIdx.x], s_over[threadIdx.x]);
}

__global__ void __launch_bounds__(kThreads) k_tube_scores(const int64_t* __restrict__ gt_size,
                                                          const int64_t* __restrict__ pred_size,
                                                          const int32_t* __restrict__ pair, int T, double* __restrict__ assoc) {
  __shared__ double s_term[kThreads];
  __shared__ int32_t s_any;
  const int64_t r = blockIdx.x;
  const int64_t g = gt_size[r];
  if (g <= 0) {                                                    // the whole block
    if (threadIdx.x == 0) assoc[r] = 0.0;
    return;
  }
  double sum = 0.0;                                                // thread 0's
  for (int base = 0; base < T; base += kThreads) {
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    const int p = base + threadIdx.x;
    double term = 0.0;
    if (p < T) {
      const int32_t n = pair[r * T + p];
      if (n > 0) {
        const double tpa = (double)n;
        const double iou = tpa / (double)(g + pred_size[p] - (int64_t)n);
        term = tpa * iou;
        s_any = 1;
      }
    }
    s_term[threadIdx.x] = term;
    __syncthreads();
    if (threadIdx.x == 0 && s_any) {
      const int lim = T - base < kThreads ? T - base : kThreads;
      for (int k = 0; k < lim; ++k) {                              // ascending p; a term of a pair is > 0
        const double v = s_term[k];
        if (v > 0.0) sum = sum + v;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) assoc[r] = sum / (double)g;
}

__global__ void __launch_bounds__(MBV_WAVE) k_tube_classes(const int64_t* __restrict__ gt_size, const double* __restrict__ assoc,
                                                           int C, int I, double* __restrict__ class_assoc,
                                                           int32_t* __restrict__ class_tubes) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double sum = 0.0;
  int32_t n = 0;
  if (c >= 1) {
    for (int64_t r = (int64_t)(c - 1) * I; r < (int64_t)c * I; ++r) {
      if (gt_size[r] > 0) {
        ++n;
        sum = sum + assoc[r];
      }
    }
  }
  class_assoc[c] = sum;
  class_tubes[c] = n;
}

bool tube_sizes_supported(int C, int I, int T) {
  return C >= 1 && C <= kMaxClasses && I >= 1 && I <= 65536 && T >= 1 && T <= (1 << 20) &&
         (int64_t)(C - 1) * I * T < 0x7FFFFFFFll;
}

}  // namespace

namespace {

// One call on the host: K33a's arguments in the order of mbv_track_frames, and the two optional parts.
struct TrackCall {
  const int32_t* instance_maps;
  const double* prev_from_cur;
  int32_t F, H, W;
  double x_lo, y_lo, voxel;
  int32_t Q, P;
  double min_iou;
  int32_t max_age, min_cells;
  int32_t *state_map, *live_id, *live_seen, *counters, *query_track, *track_map;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
  struct Motion {
    const double* cur_from_prev;
    double gain, gate;
    int32_t max_shift;
    double *pos, *vel;
    int32_t* motion_counters;
    double* query_velocity;
  };
  struct Occlusion {
    const uint8_t* visibility;     // (F, H, W) or null
    int32_t *live_held, *occlusion_counters;
    int32_t hold_num, hold_den, max_hold;
  };
  const Motion* motion;            // null: K33a's step, four launches
  const Occlusion* occlusion;      // null: nothing of K38b; with it the <true, true> kernels run whatever `visibility` is
};

// The one driver behind the three entries.
int track_frames(const TrackCall& c) {
  const TrackCall::Motion* mo = c.motion;
  const TrackCall::Occlusion* oc = c.occlusion;
  const int32_t F = c.F, H = c.H, W = c.W, Q = c.Q, P = c.P;
  hipStream_t stream = reinterpret_cast<hipStream_t>(c.stream);
  if (F == 0) return MBV_OK;
  if (F < 0 || H < 0 || W < 0 || Q < 0 || P < 0 || c.min_cells < 1 || c.max_age < 0) return MBV_ERR_BAD_ARG;
  if (mo && (mo->max_shift < 0 || !(mo->gain >= 0.0 && mo->gain <= 1.0) ||
             !(mo->gate >= 0.0 && mo->gate <= 1.7976931348623157e308)))                 // NaN, inf
    return MBV_ERR_BAD_ARG;
  if (oc && (oc->hold_num <= 0 || oc->hold_num > oc->hold_den || oc->max_hold < 0)) return MBV_ERR_BAD_ARG;
  if (!track_sizes_supported(H, W, Q, P)) return MBV_ERR_UNSUPPORTED;
  const int64_t cells = (int64_t)H * W;
  if (!c.prev_from_cur || !c.counters || (cells > 0 && (!c.instance_maps || !c.state_map)) ||
      (P > 0 && (!c.live_id || !c.live_seen)) || (Q > 0 && !c.query_track))
    return MBV_ERR_BAD_ARG;
  if (mo && (!mo->cur_from_prev || !mo->motion_counters || (P > 0 && (!mo->pos || !mo->vel)) || (Q > 0 && !mo->query_velocity)))
    return MBV_ERR_BAD_ARG;
  if (oc && (!oc->occlusion_counters || (P > 0 && !oc->live_held))) return MBV_ERR_BAD_ARG;
  TrackWorkspace w = carve_track(c.workspace, cells, Q, P, mo != nullptr, oc != nullptr);
  if (!c.workspace || c.workspace_bytes < w.bytes) return MBV_ERR_WORKSPACE;

  // K33a's clear covers the (Q, P) table; with the motion part it covers the advected map too
  const int64_t most = mo && cells > (int64_t)Q * P ? cells : (int64_t)Q * P;
  int64_t clear_blocks = (most + kThreads - 1) / kThreads;
  clear_blocks = clear_blocks < 1 ? 1 : (clear_blocks > 1024 ? 1024 : clear_blocks);
  const unsigned cell_blocks = (unsigned)((cells + kThreads - 1) / kThreads);
  const auto clear = mo ? k_track_clear<true> : k_track_clear<false>;
  const auto count = !mo ? k_track_count<false> : (oc ? k_track_count<true, true> : k_track_count<true, false>);
  const auto match = !mo ? k_track_match<false> : (oc ? k_track_match<true, true> : k_track_match<true, false>);
  for (int f = 0; f < F; ++f) {
    const int32_t* imap = c.instance_maps + (int64_t)f * cells;
    const double* m = c.prev_from_cur + (int64_t)f * 6;
    int32_t* query_track = c.query_track + (int64_t)f * Q;
    const uint8_t* vis = oc && oc->visibility ? oc->visibility + (int64_t)f * cells : nullptr;
    // the tables of a part that is absent are null in `w`
    hipLaunchKernelGGL(clear, dim3((unsigned)clear_blocks), dim3(kThreads), 0, stream, cells, (int)Q, (int)P, c.voxel,
                       mo ? (int)mo->max_shift : 0, c.counters, mo ? mo->vel : nullptr, w.area_q, w.area_t, w.inter, w.moved,
                       w.sum_ix, w.sum_iy, w.shift, w.hidden);
    MBV_CHECK_LAUNCH();
    if (cells > 0) {
      if (mo) {
        hipLaunchKernelGGL(k_track_advect, dim3(cell_blocks), dim3(kThreads), 0, stream, c.state_map, (int)H, (int)W, (int)P,
                           c.counters, w.shift, w.moved);
        MBV_CHECK_LAUNCH();
      }
      hipLaunchKernelGGL(count, dim3(cell_blocks), dim3(kThreads), 0, stream, imap,
                         mo ? reinterpret_cast<const int32_t*>(w.moved) : c.state_map, m, (int)H, (int)W, c.x_lo, c.y_lo, c.voxel,
                         (int)Q, (int)P, c.counters, w.warped, w.area_q, w.area_t, w.inter, w.sum_ix, w.sum_iy, vis, w.hidden);
      MBV_CHECK_LAUNCH();
    }
    MotionArgs ma{};
    if (mo) ma = MotionArgs{mo->cur_from_prev + (int64_t)f * 6, mo->gain, mo->gate, c.x_lo, c.y_lo, c.voxel, w.sum_ix, w.sum_iy,
                            w.cq, w.pred, w.velr, mo->pos, mo->vel, mo->motion_counters, mo->query_velocity + (int64_t)f * Q * 2};
    OcclusionArgs oa{};
    if (oc) oa = OcclusionArgs{w.hidden, oc->live_held, oc->occlusion_counters, (int)oc->hold_num, (int)oc->hold_den,
                               (int)oc->max_hold, vis != nullptr};
    hipLaunchKernelGGL(match, dim3(1), dim3(kWide), 0, stream, (int)Q, (int)P, c.min_iou, (int)c.max_age, (int)c.min_cells,
                       w.area_q, w.area_t, w.inter, w.cand, c.live_id, c.live_seen, c.counters, query_track, w.q_new, w.t_new, ma,
                       oa);
    MBV_CHECK_LAUNCH();
    if (cells > 0) {
      hipLaunchKernelGGL(k_track_paint, dim3(cell_blocks), dim3(kThreads), 0, stream, imap, cells, (int)Q, (int)P, w.warped,
                         w.q_new, w.t_new, query_track, c.state_map, c.track_map ? c.track_map + (int64_t)f * cells : nullptr);
      MBV_CHECK_LAUNCH();
    }
  }
  return MBV_OK;
}

}  // namespace

extern "C" size_t mbv_track_frames_workspace_bytes(int32_t H, int32_t W, int32_t Q, int32_t P) {
  if (!track_sizes_supported(H, W, Q, P)) return 0;
  return carve_track(nullptr, (int64_t)H * W, Q, P).bytes;
}

extern "C" size_t mbv_track_frames_motion_workspace_bytes(int32_t H, int32_t W, int32_t Q, int32_t P) {
  if (!track_sizes_supported(H, W, Q, P)) return 0;
  return carve_track(nullptr, (int64_t)H * W, Q, P, true).bytes;
}

extern "C" size_t mbv_track_frames_occluded_workspace_bytes(int32_t H, int32_t W, int32_t Q, int32_t P) {
  if (!track_sizes_supported(H, W, Q, P)) return 0;
  return carve_track(nullptr, (int64_t)H * W, Q, P, true, true).bytes;
}

extern "C" int mbv_track_frames(const int32_t* instance_maps, const double* prev_from_cur, int32_t F, int32_t H, int32_t W,
                                double x_lo, double y_lo, double voxel, int32_t Q, int32_t P, double min_iou, int32_t max_age,
                                int32_t min_cells, int32_t* state_map, int32_t* live_id, int32_t* live_seen, int32_t* counters,
                                int32_t* query_track, int32_t* track_map, void* workspace, size_t workspace_bytes,
                                void* stream_) {
  return track_frames(TrackCall{instance_maps, prev_from_cur, F, H, W, x_lo, y_lo, voxel, Q, P, min_iou, max_age, min_cells,
                                state_map, live_id, live_seen, counters, query_track, track_map, workspace, workspace_bytes,
                                stream_, nullptr, nullptr});
}

extern "C" int mbv_track_frames_motion(const int32_t* instance_maps, const double* prev_from_cur, const double* cur_from_prev,
                                       int32_t F, int32_t H, int32_t W, double x_lo, double y_lo, double voxel, int32_t Q,
                                       int32_t P, double min_iou, int32_t max_age, int32_t min_cells, double gain, double gate,
                                       int32_t max_shift, int32_t* state_map, int32_t* live_id, int32_t* live_seen,
                                       int32_t* counters, double* pos, double* vel, int32_t* motion_counters,
                                       int32_t* query_track, int32_t* track_map, double* query_velocity, void* workspace,
                                       size_t workspace_bytes, void* stream_) {
  const TrackCall::Motion mo{cur_from_prev, gain, gate, max_shift, pos, vel, motion_counters, query_velocity};
  return track_frames(TrackCall{instance_maps, prev_from_cur, F, H, W, x_lo, y_lo, voxel, Q, P, min_iou, max_age, min_cells,
                                state_map, live_id, live_seen, counters, query_track, track_map, workspace, workspace_bytes,
                                stream_, &mo, nullptr});
}

extern "C" int mbv_track_frames_occluded(const int32_t* instance_maps, const double* prev_from_cur, const double* cur_from_prev,
                                         const uint8_t* visibility, int32_t F, int32_t H, int32_t W, double x_lo, double y_lo,
                                         double voxel, int32_t Q, int32_t P, double min_iou, int32_t max_age, int32_t min_cells,
                                         double gain, double gate, int32_t max_shift, int32_t hold_num, int32_t hold_den,
                                         int32_t max_hold, int32_t* state_map, int32_t* live_id, int32_t* live_seen,
                                         int32_t* live_held, int32_t* counters, double* pos, double* vel,
                                         int32_t* motion_counters, int32_t* occlusion_counters, int32_t* query_track,
                                         int32_t* track_map, double* query_velocity, void* workspace, size_t workspace_bytes,
                                         void* stream_) {
  const TrackCall::Motion mo{cur_from_prev, gain, gate, max_shift, pos, vel, motion_counters, query_velocity};
  const TrackCall::Occlusion oc{visibility, live_held, occlusion_counters, hold_num, hold_den, max_hold};
  return track_frames(TrackCall{instance_maps, prev_from_cur, F, H, W, x_lo, y_lo, voxel, Q, P, min_iou, max_age, min_cells,
                                state_map, live_id, live_seen, counters, query_track, track_map, workspace, workspace_bytes,
                                stream_, &mo, &oc});
}

extern "C" int mbv_tube_accumulate(const int32_t* pred_track, const uint32_t* gt_word, int64_t total, const int32_t* class_lut,
                                   int32_t lut_len, int32_t C, int32_t id_limit, int32_t max_tracks, int64_t* gt_size,
                                   int64_t* pred_size, int32_t* pair, int64_t* overflow, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (total == 0) return MBV_OK;
  if (total < 0 || lut_len < 0 || C < 1 || id_limit < 1 || max_tracks < 1) return MBV_ERR_BAD_ARG;
  if (!tube_sizes_supported(C, id_limit, max_tracks) || total >= 0x7FFFFFFFll) return MBV_ERR_UNSUPPORTED;
  if (!pred_track || !gt_word || (lut_len > 0 && !class_lut) || !pred_size || !overflow || (C > 1 && (!gt_size || !pair)))
    return MBV_ERR_BAD_ARG;
  int64_t blocks = (total + kThreads - 1) / kThreads;
  blocks = blocks > 1024 ? 1024 : blocks;
  hipLaunchKernelGGL(k_tube_accumulate, dim3((unsigned)blocks), dim3(kThreads), 0, stream, pred_track, gt_word, total,
                     class_lut, (int)lut_len, (int)C, (int)id_limit, (int)max_tracks, gt_size, pred_size, pair, overflow);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_tube_scores(const int64_t* gt_size, const int64_t* pred_size, const int32_t* pair, int32_t C,
                               int32_t id_limit, int32_t max_tracks, double* assoc, double* class_assoc, int32_t* class_tubes,
                               void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (C < 1 || id_limit < 1 || max_tracks < 1) return MBV_ERR_BAD_ARG;
  if (!tube_sizes_supported(C, id_limit, max_tracks)) return MBV_ERR_UNSUPPORTED;
  if (!class_assoc || !class_tubes || !pred_size || (C > 1 && (!gt_size || !pair || !assoc))) return MBV_ERR_BAD_ARG;
  const int rows = (C - 1) * id_limit;
  if (rows > 0) {
    hipLaunchKernelGGL(k_tube_scores, dim3((unsigned)rows), dim3(kThreads), 0, stream, gt_size, pred_size, pair,
                       (int)max_tracks, assoc);
    MBV_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_tube_classes, dim3(1), dim3(MBV_WAVE), 0, stream, gt_size, assoc, (int)C, (int)id_limit, class_assoc,
                     class_tubes);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
