// K42 — reconciling the kept queries of one decoder output with each other: greedy mask NMS and Mask2Former's overlap
// filter (panoptic_postprocess: per-pixel argmax over the kept queries, a segment dropped when it wins less than
// OVERLAP_THRESHOLD of its own mask).  The reference's consumers keep every `argmax > 0` query
// (mask_bev/mask_bev_module.py:286-294, mask_bev/evaluation/kitti_eval.py:27-44).  The rule is stated in
// include/maskbev_hip.h; everything here is integer arithmetic, so every result is exact and order-independent.
//
// K42a  k_self_overlap: inter[i][j] = Σ_k popc(row_i[k] & row_j[k]) over the KEPT rows of a frame only.  K29a called with
//       pred = gt would AND all Q x Q rows; here every workgroup first compacts the frame's keep flags (ballots and a
//       16-entry prefix in LDS), takes a pair of 32-row tiles (ti <= tj) of the compacted list and leaves when the pair lies
//       beyond the kept count, which only the device knows.  The 64 rows stream through LDS 128 words at a time; a thread
//       owns one row of tile i and four of tile j: the 32 lanes of a half-wave read 32 different rows of i 8 bytes at a time
//       (row stride 65 x 8 bytes: the 32 rows start on 32 different bank pairs) and the same 16 bytes of a row of j (a
//       broadcast) — 8 AND + popcount-64 per 6 LDS reads.  The contraction is split 512 words to a workgroup and joined with
//       integer atomics, into both triangles.
// K42b  k_mask_nms: one workgroup per frame.  The order by counting (descending f32 score, ties to the smaller q), then the
//       walk over it; a survivor's later candidates are tested in parallel, one barrier per survivor.
// K42c  k_owned_hist: per-workgroup histogram of the map's cells in LDS, flushed with integer atomics for kept queries.
//       k_filter_map: the decision for every query of the frame in LDS, then the rewrite of the workgroup's cells.
#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxQ = 1024;
constexpr int kMaxWords = 32768;          // H * W <= 2^20 cells
constexpr int kTile = 32;                 // kept rows per tile side
constexpr int kJPerThread = 4;            // rows of tile j per thread: 32 rows of i x 8 groups of 4 rows of j = 256 threads
constexpr int kChunk = 128;               // u32 words of the contraction staged per pass
constexpr int kChunk64 = kChunk / 2;
constexpr int kStrideI = kChunk64 + 1;    // u64 per staged row of tile i: odd, so 32 rows start on 32 different bank pairs
constexpr int kSplitWords = 512;          // u32 words of the contraction per workgroup
constexpr int kSegs = kMaxQ / 64;         // 64-query segments of the keep flags

static_assert(kTile * (kTile / kJPerThread) == kThreads, "one thread per (row of i, group of rows of j)");
static_assert(kSplitWords % kChunk == 0 && kChunk % 4 == 0, "whole chunks, 16-byte loads");
static_assert(kMaxQ == 4 * kThreads, "a thread looks at four keep flags");

// grid: x = pair of tiles * ksplit + split of the contraction, y = frame; `inter` arrives zeroed
__global__ void __launch_bounds__(kThreads) k_self_overlap(const uint32_t* __restrict__ words, const uint8_t* __restrict__ keep,
                                                           int Q, int nwords, int ksplit, int ntiles, int wide,
                                                           int32_t* __restrict__ inter) {
  __shared__ unsigned long long s_i[kTile * kStrideI];
  __shared__ __attribute__((aligned(16))) unsigned long long s_j[kTile * kChunk64];
  __shared__ int s_cnt[kSegs];
  __shared__ int s_qi[kTile], s_qj[kTile];
  const int b = blockIdx.y;
  const int split = blockIdx.x % ksplit;
  int pair = blockIdx.x / ksplit;
  int ti = 0;
  while (ti < ntiles - 1 && pair >= ntiles - ti) { pair -= ntiles - ti; ++ti; }   // row ti of the upper triangle of tiles
  const int tj = ti + pair;                                                      // < ntiles by the grid's size
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the frame's kept queries in ascending q: position of every kept q in the compacted list
  if (tid < kTile) { s_qi[tid] = -1; s_qj[tid] = -1; }
  bool flag[4];
  unsigned long long bal[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int q = c * kThreads + tid;
    flag[c] = q < Q && keep[(int64_t)b * Q + q] != 0;
    bal[c] = __ballot(flag[c]);
    if (lane == 0) s_cnt[c * (kThreads / 64) + wave] = __popcll(bal[c]);
  }
  __syncthreads();
  int kept = 0;
#pragma unroll
  for (int s = 0; s < kSegs; ++s) kept += s_cnt[s];
  if (tj * kTile >= kept) return;                 // block-uniform; ti <= tj: no kept pair in this tile pair
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (!flag[c]) continue;
    const int seg = c * (kThreads / 64) + wave;
    int pos = __popcll(bal[c] & ((1ull << lane) - 1ull));
    for (int s = 0; s < seg; ++s) pos += s_cnt[s];
    const int q = c * kThreads + tid;
    if (pos >= ti * kTile && pos < ti * kTile + kTile) s_qi[pos - ti * kTile] = q;
    if (pos >= tj * kTile && pos < tj * kTile + kTile) s_qj[pos - tj * kTile] = q;
  }
  __syncthreads();

  const int kbeg = split * kSplitWords;
  const int kend = kbeg + kSplitWords < nwords ? kbeg + kSplitWords : nwords;
  const uint32_t* __restrict__ frame = words + (int64_t)b * Q * nwords;
  const int ri = tid & (kTile - 1);               // row of tile i
  const int gj = tid / kTile;                     // rows gj * 4 .. gj * 4 + 3 of tile j
  int acc[kJPerThread];
#pragma unroll
  for (int j = 0; j < kJPerThread; ++j) acc[j] = 0;
  uint32_t* si32 = reinterpret_cast<uint32_t*>(s_i);
  uint32_t* sj32 = reinterpret_cast<uint32_t*>(s_j);

  for (int k0 = kbeg; k0 < kend; k0 += kChunk) {
    if (wide) {                                    // nwords % 4 == 0 and a 16-byte aligned base: every row starts aligned
      for (int i = tid; i < 2 * kTile * (kChunk / 4); i += kThreads) {
        const int r = i / (kChunk / 4), k = (i % (kChunk / 4)) * 4;
        const int q = r < kTile ? s_qi[r] : s_qj[r - kTile];
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (q >= 0 && k0 + k < kend) v = *reinterpret_cast<const uint4*>(frame + (int64_t)q * nwords + k0 + k);
        if (r < kTile) {
          uint32_t* d = si32 + r * (2 * kStrideI) + k;          // 8-byte aligned rows only: four 4-byte stores
          d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {
          *reinterpret_cast<uint4*>(sj32 + (r - kTile) * kChunk + k) = v;
        }
      }
    } else {
      for (int i = tid; i < 2 * kTile * kChunk; i += kThreads) {
        const int r = i / kChunk, k = i % kChunk;
        const int q = r < kTile ? s_qi[r] : s_qj[r - kTile];
        const uint32_t v = (q >= 0 && k0 + k < kend) ? frame[(int64_t)q * nwords + k0 + k] : 0u;
        if (r < kTile) si32[r * (2 * kStrideI) + k] = v;
        else sj32[(r - kTile) * kChunk + k] = v;
      }
    }
    __syncthreads();
    const unsigned long long* __restrict__ pi = s_i + ri * kStrideI;
    const unsigned long long* __restrict__ pj = s_j + gj * kJPerThread * kChunk64;
#pragma unroll 4
    for (int k = 0; k < kChunk64; k += 2) {
      const unsigned long long a0 = pi[k], a1 = pi[k + 1];
#pragma unroll
      for (int j = 0; j < kJPerThread; ++j) {
        const ulonglong2 g = *reinterpret_cast<const ulonglong2*>(pj + j * kChunk64 + k);
        acc[j] += __popcll(a0 & g.x) + __popcll(a1 & g.y);
      }
    }
    __syncthreads();
  }

  const int qi = s_qi[ri];
  if (qi < 0) return;
#pragma unroll
  for (int j = 0; j < kJPerThread; ++j) {
    const int qj = s_qj[gj * kJPerThread + j];
    // a diagonal pair of tiles holds every pair twice: the half with qi <= qj writes.  qi, qj < Q: they come from the flags' indices
    if (qj < 0 || acc[j] == 0 || (ti == tj && qj < qi)) continue;
    atomicAdd(inter + ((int64_t)b * Q + qi) * Q + qj, acc[j]);
    if (qi != qj) atomicAdd(inter + ((int64_t)b * Q + qj) * Q + qi, acc[j]);
  }
}

// one workgroup per frame
__global__ void __launch_bounds__(kThreads) k_mask_nms(const int32_t* __restrict__ inter, const float* __restrict__ scores,
                                                       const int32_t* __restrict__ labels, const uint8_t* __restrict__ keep,
                                                       int Q, int num, int den, int same_label, uint8_t* __restrict__ keep_out,
                                                       int32_t* __restrict__ suppressed_by) {
  __shared__ float s_score[kMaxQ];
  __shared__ int s_label[kMaxQ];
  __shared__ int s_area[kMaxQ];
  __shared__ int s_keep[kMaxQ];
  __shared__ int s_order[kMaxQ];               // kept queries in walking order; -1: a hole (a score that does not order)
  __shared__ int s_sup[kMaxQ];
  __shared__ int s_part[kThreads / 64];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int32_t* __restrict__ table = inter + b * Q * Q;
  int mine = 0;
  for (int q = tid; q < Q; q += kThreads) {
    const int k = keep[b * Q + q] != 0;
    s_keep[q] = k;
    s_score[q] = scores[b * Q + q];
    s_label[q] = labels[b * Q + q];
    s_area[q] = table[(int64_t)q * Q + q];
    s_order[q] = -1;
    s_sup[q] = -1;
    mine += k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = mine;
  __syncthreads();
  int kept = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) kept += s_part[w];

  for (int d = tid; d < Q; d += kThreads) {
    if (!s_keep[d]) continue;
    const float sc = s_score[d];
    int before = 0;
    for (int e = 0; e < Q; ++e) {
      const float se = s_score[e];
      before += (s_keep[e] && (se > sc || (se == sc && e < d))) ? 1 : 0;
    }
    s_order[before] = d;                         // before < kept <= Q
  }
  __syncthreads();

  const int64_t n64 = num, d64 = den;
  for (int r = 0; r + 1 < kept; ++r) {
    const int i = s_order[r];                    // the same LDS word for every thread: the branch is block-uniform
    if (i < 0 || s_sup[i] >= 0) continue;
    const int ai = s_area[i], li = s_label[i];
    const int32_t* __restrict__ row = table + (int64_t)i * Q;
    for (int c = r + 1 + tid; c < kept; c += kThreads) {
      const int j = s_order[c];
      if (j < 0 || s_sup[j] >= 0) continue;
      if (same_label && s_label[j] != li) continue;
      const int64_t in = row[j];
      const int64_t uni = (int64_t)ai + s_area[j] - in;
      if (uni > 0 && in * d64 >= n64 * uni) s_sup[j] = i;
    }
    __syncthreads();
  }
  __syncthreads();
  for (int q = tid; q < Q; q += kThreads) {
    suppressed_by[b * Q + q] = s_sup[q];
    keep_out[b * Q + q] = (s_keep[q] && s_sup[q] < 0) ? 1 : 0;
  }
}

constexpr int kCellsPerBlock = kThreads * 16;    // four 16-byte loads per thread

// grid: x = tile of kCellsPerBlock cells, y = frame; `owned` arrives zeroed
__global__ void __launch_bounds__(kThreads) k_owned_hist(const int32_t* __restrict__ maps, const uint8_t* __restrict__ keep,
                                                         int hw, int Q, int wide, int32_t* __restrict__ owned) {
  __shared__ int s_hist[kMaxQ];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int q = tid; q < Q; q += kThreads) s_hist[q] = 0;
  __syncthreads();
  const int32_t* __restrict__ m = maps + (int64_t)b * hw;
  const int p0 = blockIdx.x * kCellsPerBlock;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int p = p0 + (it * kThreads + tid) * 4;
    int v[4] = {-1, -1, -1, -1};
    if (wide && p + 4 <= hw) {                    // hw % 4 == 0 and a 16-byte aligned base: every frame starts aligned
      const int4 t = *reinterpret_cast<const int4*>(m + p);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p + e < hw) v[e] = m[p + e];
    }
    // runs of one query are the rule in a map: equal neighbours are counted together
    int run = 0, cur = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (v[e] == cur) { ++run; continue; }
      if (run > 0 && cur >= 0 && cur < Q) atomicAdd(&s_hist[cur], run);
      cur = v[e];
      run = 1;
    }
    if (run > 0 && cur >= 0 && cur < Q) atomicAdd(&s_hist[cur], run);
  }
  __syncthreads();
  for (int q = tid; q < Q; q += kThreads) {
    const int n = s_hist[q];
    if (n > 0 && keep[(int64_t)b * Q + q] != 0) atomicAdd(owned + (int64_t)b * Q + q, n);
  }
}

// grid as k_owned_hist; block x == 0 of a frame also writes keep_out
__global__ void __launch_bounds__(kThreads) k_filter_map(int32_t* __restrict__ maps, const int32_t* __restrict__ areas,
                                                         const uint8_t* __restrict__ keep, const int32_t* __restrict__ owned,
                                                         int hw, int Q, int num, int den, int min_cells, int wide,
                                                         uint8_t* __restrict__ keep_out) {
  __shared__ int s_ok[kMaxQ];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n64 = num, d64 = den;
  for (int q = tid; q < Q; q += kThreads) {
    const int64_t own = owned[(int64_t)b * Q + q];
    const int ok = keep[(int64_t)b * Q + q] != 0 && own >= min_cells && own * d64 >= n64 * (int64_t)areas[(int64_t)b * Q + q];
    s_ok[q] = ok;
  }
  __syncthreads();
  if (blockIdx.x == 0)
    for (int q = tid; q < Q; q += kThreads) keep_out[(int64_t)b * Q + q] = (uint8_t)s_ok[q];
  int32_t* __restrict__ m = maps + (int64_t)b * hw;
  const int p0 = blockIdx.x * kCellsPerBlock;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int p = p0 + (it * kThreads + tid) * 4;
    if (wide && p + 4 <= hw) {
      int4 t = *reinterpret_cast<const int4*>(m + p);
      const int4 o = t;
      if (t.x >= 0 && t.x < Q && !s_ok[t.x]) t.x = -1;
      if (t.y >= 0 && t.y < Q && !s_ok[t.y]) t.y = -1;
      if (t.z >= 0 && t.z < Q && !s_ok[t.z]) t.z = -1;
      if (t.w >= 0 && t.w < Q && !s_ok[t.w]) t.w = -1;
      if (t.x != o.x || t.y != o.y || t.z != o.z || t.w != o.w) *reinterpret_cast<int4*>(m + p) = t;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (p + e >= hw) continue;
        const int v = m[p + e];
        if (v >= 0 && v < Q && !s_ok[v]) m[p + e] = -1;
      }
    }
  }
}

bool ratio_ok(int32_t num, int32_t den, int32_t num_min) { return num >= num_min && num <= den && den >= 1 && den <= 65535; }

}  // namespace

extern "C" int mbv_mask_self_overlap(const uint32_t* words, const uint8_t* keep, int32_t B, int32_t Q, int64_t nwords,
                                     int32_t* inter, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (B < 0 || Q < 0 || nwords < 0) return MBV_ERR_BAD_ARG;
  if ((int64_t)B * Q == 0) return MBV_OK;
  if (Q > kMaxQ || B > 65535 || nwords > kMaxWords) return MBV_ERR_UNSUPPORTED;
  if (!keep || !inter || (nwords > 0 && !words)) return MBV_ERR_BAD_ARG;
  MBV_CHECK_HIP(mbv_fill_async(inter, 0, sizeof(int32_t) * (size_t)B * Q * Q, stream));
  if (nwords == 0) return MBV_OK;
  const int ntiles = (Q + kTile - 1) / kTile;
  const int ksplit = (int)((nwords + kSplitWords - 1) / kSplitWords);
  const int wide = (nwords % 4 == 0 && (reinterpret_cast<uintptr_t>(words) & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)(ntiles * (ntiles + 1) / 2 * ksplit), (unsigned)B);
  hipLaunchKernelGGL(k_self_overlap, grid, dim3(kThreads), 0, stream, words, keep, (int)Q, (int)nwords, ksplit, ntiles, wide,
                     inter);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_mask_nms(const int32_t* inter, const float* scores, const int32_t* labels, const uint8_t* keep, int32_t B,
                            int32_t Q, int32_t num, int32_t den, int32_t same_label, uint8_t* keep_out, int32_t* suppressed_by,
                            void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (B < 0 || Q < 0) return MBV_ERR_BAD_ARG;
  if ((int64_t)B * Q == 0) return MBV_OK;
  if (Q > kMaxQ || B > 65535) return MBV_ERR_UNSUPPORTED;
  if (!inter || !scores || !labels || !keep || !keep_out || !suppressed_by || !ratio_ok(num, den, 1)) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_mask_nms, dim3((unsigned)B), dim3(kThreads), 0, stream, inter, scores, labels, keep, (int)Q, (int)num,
                     (int)den, same_label ? 1 : 0, keep_out, suppressed_by);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_overlap_filter(int32_t* instance_map, const int32_t* areas, const uint8_t* keep, int32_t B, int32_t H,
                                  int32_t W, int32_t Q, int32_t num, int32_t den, int32_t min_cells, int32_t* owned,
                                  uint8_t* keep_out, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (B < 0 || Q < 0 || H < 0 || W < 0) return MBV_ERR_BAD_ARG;
  if ((int64_t)B * Q == 0) return MBV_OK;
  if (H < 1 || W < 1 || min_cells < 0 || !ratio_ok(num, den, 0)) return MBV_ERR_BAD_ARG;
  if (Q > kMaxQ || B > 65535 || (int64_t)H * W > 1024 * 1024) return MBV_ERR_UNSUPPORTED;
  if (!instance_map || !areas || !keep || !owned || !keep_out) return MBV_ERR_BAD_ARG;
  const int hw = H * W;
  const int wide = (hw % 4 == 0 && (reinterpret_cast<uintptr_t>(instance_map) & 15) == 0) ? 1 : 0;
  MBV_CHECK_HIP(mbv_fill_async(owned, 0, sizeof(int32_t) * (size_t)B * Q, stream));
  const dim3 grid((unsigned)((hw + kCellsPerBlock - 1) / kCellsPerBlock), (unsigned)B);
  hipLaunchKernelGGL(k_owned_hist, grid, dim3(kThreads), 0, stream, instance_map, keep, hw, (int)Q, wide, owned);
  MBV_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_filter_map, grid, dim3(kThreads), 0, stream, instance_map, areas, keep, owned, hw, (int)Q, (int)num,
                     (int)den, (int)min_cells, wide, keep_out);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
