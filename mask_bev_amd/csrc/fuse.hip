// K39 — tracked BEV footprints fused over time in a rolling world grid, and a query map back to bit-packed masks.  The rules
// are in include/maskbev_hip.h (K39a, K39b); this file restates nothing, it implements them.
//
// K39a, per frame, all on the caller's stream, no host synchronisation, no workspace:
//   1. update   one thread per STORE cell: the new window corner from the pose (one thread of every block computes the same
//               integers into LDS), the clear of a cell whose world cell changed, then the gather of the frame's
//               detection under the cell's world centre and the step of (owner, count).  Reads the old window, writes none of it.
//   2. read     one thread per SENSOR cell: the frame's Q ids and moving flags in LDS, the gather from the store, the
//               owner -> query lookup as a scan of the LDS table (every lane of a wave reads the same slot; skipped
//               when fused_queries is NULL).  Thread 0 of
//               block 0 writes the window; no other thread of this launch reads it.
// An invalid pose is seen alike by every thread of both launches: the first returns, the second writes -1.
// No atomics.  Every index comes from the sizes and from range-checked values.
// K39b: two fills, then one thread per pixel, coalesced.  A wave ballots every distinct query of its 64 pixels and its first
// lane stores the two words of that query's row: a word of a row has ONE writer, so these are plain stores of whole words.  The
// areas go through an LDS table per block (integer atomicAdd).  (One thread per 32-pixel word, each walking 128 B of its own,
// took 37 us for 8 frames of 1024 x 1024 with atomicOr and 39 us with a plain read-modify-write: the strided reads, not the
// atomics, were the cost.)
#include "common.hpp"

namespace {

constexpr int kThreads = 256, kMaxQueries = 1024, kMaxStore = 8192;
constexpr int64_t kMaxCells = 1024 * 1024;
constexpr double kMaxFinite = 1.7976931348623157e308, kMaxWorldCell = 1099511627776.0;   // 2^40

struct FuseGrid {
  int H, W, S, Q;
  double x_lo, y_lo, voxel;
};

__device__ __forceinline__ int64_t mod_floor(int64_t a, int64_t s) {
  const int64_t r = a % s;
  return r < 0 ? r + s : r;
}

// What every thread of a frame's two launches needs of step 1, computed by ONE thread of each block into LDS: 64-bit
// divisions are emulated and cost more than the rest of a thread's work together.
struct FrameInfo {
  int valid;                // 0: an invalid frame
  int clear_all;            // frames == 0
  int64_t wx0, wy0;         // the new corner
  int64_t ox0, oy0;         // the stored one
  int rnx, rny, rox, roy;   // the corners mod S
};

__device__ __forceinline__ void frame_info(const FuseGrid& g, const double* __restrict__ m, const double* __restrict__ n,
                                           const int64_t* window, FrameInfo* f) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) ok = ok && fabs(m[k]) <= kMaxFinite && fabs(n[k]) <= kMaxFinite;
  const double cx = g.x_lo + ((double)g.W * 0.5) * g.voxel, cy = g.y_lo + ((double)g.H * 0.5) * g.voxel;
  const double X = (m[0] * cx + m[1] * cy) + m[2], Y = (m[3] * cx + m[4] * cy) + m[5];
  const double qx = X / g.voxel, qy = Y / g.voxel;
  ok = ok && fabs(qx) < kMaxWorldCell && fabs(qy) < kMaxWorldCell;             // NaN fails
  f->valid = ok ? 1 : 0;
  if (!ok) return;
  f->wx0 = (int64_t)floor(qx) - g.S / 2;
  f->wy0 = (int64_t)floor(qy) - g.S / 2;
  f->rnx = (int)mod_floor(f->wx0, g.S);
  f->rny = (int)mod_floor(f->wy0, g.S);
  if (!window) return;                                                        // the read-out does not look at the old window
  f->ox0 = window[0];
  f->oy0 = window[1];
  f->clear_all = window[2] == 0;
  f->rox = (int)mod_floor(f->ox0, g.S);
  f->roy = (int)mod_floor(f->oy0, g.S);
}

// the world cell that store column (or row) `s` represents under the corner `w0` with w0 mod S = r: w0 + ((s - w0) mod S);
// unsigned so that a garbage corner wraps
__device__ __forceinline__ int64_t world_of(int s, int64_t w0, int r, int S) {
  const int off = s - r;
  return (int64_t)((uint64_t)w0 + (uint64_t)(off < 0 ? off + S : off));
}

__device__ __forceinline__ bool is_moving(const double* __restrict__ velocity, int q, double static_speed) {
  if (!velocity) return false;
  const double vx = velocity[2 * q], vy = velocity[2 * q + 1];
  return vx * vx + vy * vy > static_speed * static_speed;                     // NaN fails
}

__global__ void __launch_bounds__(kThreads) k_fuse_update(FuseGrid g, const int32_t* __restrict__ instance_map,
                                                          const int32_t* __restrict__ query_track,
                                                          const double* __restrict__ world_from_cur,
                                                          const double* __restrict__ cur_from_world,
                                                          const uint8_t* __restrict__ visibility,
                                                          const double* __restrict__ velocity, int cap, int hit, int miss,
                                                          double static_speed, const int64_t* __restrict__ window,
                                                          int32_t* __restrict__ owner, int32_t* __restrict__ count) {
  __shared__ FrameInfo s_f;
  if (threadIdx.x == 0) frame_info(g, world_from_cur, cur_from_world, window, &s_f);
  __syncthreads();
  if (!s_f.valid) return;                                                      // uniform
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;            // S * S <= 2^26
  if (i >= (uint32_t)g.S * (uint32_t)g.S) return;
  const int sy = (int)(i / (uint32_t)g.S), sx = (int)(i - (uint32_t)sy * (uint32_t)g.S);
  const int64_t gx = world_of(sx, s_f.wx0, s_f.rnx, g.S), gy = world_of(sy, s_f.wy0, s_f.rny, g.S);
  int32_t own = owner[i];
  int64_t cnt = count[i];
  const int32_t own_in = own, cnt_in = (int32_t)cnt;
  if (s_f.clear_all || gx != world_of(sx, s_f.ox0, s_f.rox, g.S) || gy != world_of(sy, s_f.oy0, s_f.roy, g.S)) {
    own = -1;
    cnt = 0;
  }
  const double* n = cur_from_world;
  const double x = ((double)gx + 0.5) * g.voxel, y = ((double)gy + 0.5) * g.voxel;
  const double xs = (n[0] * x + n[1] * y) + n[2], ys = (n[3] * x + n[4] * y) + n[5];
  const double fx = floor((xs - g.x_lo) / g.voxel), fy = floor((ys - g.y_lo) / g.voxel);
  if (fx >= 0.0 && fx < (double)g.W && fy >= 0.0 && fy < (double)g.H) {        // NaN and inf fail a comparison
    const int cell = (int)fy * g.W + (int)fx;                                  // H * W <= 2^20
    const int q = instance_map[cell];
    const bool is_query = q >= 0 && q < g.Q;
    if (!(is_query && is_moving(velocity, q, static_speed))) {
      const int32_t id = is_query ? query_track[q] : -1;
      if (id >= 0) {
        if (own == id) {
          cnt += hit;
          cnt = cnt > cap ? cap : cnt;
        } else {
          cnt -= hit;
          if (cnt <= 0) {
            own = id;
            cnt = hit;
          }
        }
      } else if (!visibility || visibility[cell] != 0) {
        cnt -= miss;
        if (cnt <= 0) {
          own = -1;
          cnt = 0;
        }
      }
    }
  }
  if (own != own_in) owner[i] = own;
  if ((int32_t)cnt != cnt_in) count[i] = (int32_t)cnt;
}

__global__ void __launch_bounds__(kThreads) k_fuse_read(FuseGrid g, const int32_t* __restrict__ instance_map,
                                                        const int32_t* __restrict__ query_track,
                                                        const double* __restrict__ world_from_cur,
                                                        const double* __restrict__ cur_from_world,
                                                        const double* __restrict__ velocity, int min_count,
                                                        double static_speed, const int32_t* __restrict__ owner,
                                                        const int32_t* __restrict__ count, int64_t* window,
                                                        int32_t* __restrict__ fused_ids, int32_t* __restrict__ fused_queries) {
  __shared__ int32_t s_id[kMaxQueries];
  __shared__ uint8_t s_moving[kMaxQueries];
  __shared__ __attribute__((aligned(16))) int32_t s_key[kMaxQueries];          // the id of a static query, else -1: four per LDS read
  __shared__ FrameInfo s_f;
  // no thread reads the window here but the one that writes it below
  if (threadIdx.x == 0) frame_info(g, world_from_cur, cur_from_world, nullptr, &s_f);
  __syncthreads();
  const bool valid = s_f.valid != 0;                                           // uniform
  if (valid) {
    for (int k = threadIdx.x; k < g.Q; k += kThreads) {
      const int32_t id = query_track[k];
      const bool moving = is_moving(velocity, k, static_speed);
      s_id[k] = id;
      s_moving[k] = moving ? 1 : 0;
      s_key[k] = moving ? -1 : id;
    }
    if (threadIdx.x < 3 && g.Q + (int)threadIdx.x < ((g.Q + 3) & ~3)) s_key[g.Q + threadIdx.x] = -1;   // the tail of the last four
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;            // H * W <= 2^20
  if (i < (uint32_t)g.H * (uint32_t)g.W) {
    int32_t id = -1, query = -1;
    if (valid) {
      const int q = instance_map[i];
      if (q >= 0 && q < g.Q && s_moving[q] && s_id[q] >= 0) {
        id = s_id[q];
        query = q;
      } else {
        const double* m = world_from_cur;
        const int iy = (int)(i / (uint32_t)g.W), ix = (int)(i - (uint32_t)iy * (uint32_t)g.W);
        const double x = g.x_lo + ((double)ix + 0.5) * g.voxel, y = g.y_lo + ((double)iy + 0.5) * g.voxel;
        const double X = (m[0] * x + m[1] * y) + m[2], Y = (m[3] * x + m[4] * y) + m[5];
        const double wgx = floor(X / g.voxel), wgy = floor(Y / g.voxel);
        const double lo_x = (double)s_f.wx0, lo_y = (double)s_f.wy0;          // exact: below 2^41
        if (wgx >= lo_x && wgx < lo_x + (double)g.S && wgy >= lo_y && wgy < lo_y + (double)g.S) {
          // gx mod S = (wx0 mod S + (gx - wx0)) mod S, the offset an exact small integer in [0, S)
          int sx = s_f.rnx + (int)(wgx - lo_x), sy = s_f.rny + (int)(wgy - lo_y);
          sx = sx >= g.S ? sx - g.S : sx;
          sy = sy >= g.S ? sy - g.S : sy;
          const int at = sy * g.S + sx;                                        // S * S <= 2^26
          const int32_t own = owner[at];
          if (own >= 0 && count[at] >= min_count) {
            id = own;
            if (fused_queries) {                                               // the ids alone need no lookup
              for (int k = 0; k < g.Q; k += 4) {                               // own >= 0 never equals a -1
                const int4 key = *reinterpret_cast<const int4*>(&s_key[k]);
                const int hit = key.x == own ? 0 : (key.y == own ? 1 : (key.z == own ? 2 : (key.w == own ? 3 : -1)));
                if (hit >= 0) {
                  query = k + hit;
                  break;
                }
              }
            }
          }
        }
      }
    }
    fused_ids[i] = id;
    if (fused_queries) fused_queries[i] = query;
  }
  if (valid && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t frames = window[2];
    window[0] = s_f.wx0;
    window[1] = s_f.wy0;
    window[2] = (int64_t)((uint64_t)frames + 1u);
    window[3] = 0;
  }
}

// ---- K39b -------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) k_masks_from_map(const int32_t* __restrict__ maps, int64_t hw, int Q, int64_t words,
                                                             uint32_t* __restrict__ packed, int32_t* __restrict__ areas) {
  __shared__ int32_t s_area[kMaxQueries];
  for (int k = threadIdx.x; k < Q; k += kThreads) s_area[k] = 0;
  __syncthreads();
  const int64_t f = blockIdx.y;
  const int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x;           // the grid covers words * 32 pixels
  int q = pix < hw ? maps[f * hw + pix] : -1;
  if (q < 0 || q >= Q) q = -1;
  const int lane = threadIdx.x & (MBV_WAVE - 1);
  uint32_t* pair = packed + f * Q * words + (pix - lane) / 32;                 // the wave's two words of row 0
  unsigned long long todo = __ballot(q >= 0);                                  // uniform over the wave
  while (todo) {
    const int q0 = __shfl(q, __ffsll(todo) - 1, MBV_WAVE);                     // in [0, Q)
    const unsigned long long m = __ballot(q == q0);
    if (lane == 0) {
      uint32_t* row = pair + (int64_t)q0 * words;
      const uint32_t lo = (uint32_t)(m & 0xffffffffull), hi = (uint32_t)(m >> 32);
      if (lo) row[0] = lo;
      if (hi) row[1] = hi;
      atomicAdd(&s_area[q0], __popcll(m));
    }
    todo &= ~m;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < Q; k += kThreads)
    if (s_area[k] > 0) atomicAdd(&areas[f * Q + k], s_area[k]);
}

bool store_supported(int64_t H, int64_t W, int64_t S) {
  return S % 2 == 0 && S >= 4 && S <= kMaxStore && (S - 4) * (S - 4) >= H * H + W * W;
}

}  // namespace

extern "C" int mbv_fuse_frames(const int32_t* instance_maps, const int32_t* query_track, const double* world_from_cur,
                               const double* cur_from_world, const uint8_t* visibility, const double* query_velocity, int32_t F,
                               int32_t H, int32_t W, int32_t S, double x_lo, double y_lo, double voxel, int32_t Q, int32_t cap,
                               int32_t hit, int32_t miss, int32_t min_count, double static_speed, int32_t* owner, int32_t* count,
                               int64_t* window, int32_t* fused_ids, int32_t* fused_queries, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (F < 0 || H < 0 || W < 0 || S < 0 || Q < 0 || cap < 1 || hit < 1 || miss < 0 || min_count < 1 || !(static_speed >= 0.0) ||
      !(voxel > 0.0 && voxel <= kMaxFinite))
    return MBV_ERR_BAD_ARG;
  const int64_t cells = (int64_t)H * W;
  if (F == 0 || cells == 0) return MBV_OK;
  if (Q > kMaxQueries || H > kMaxCells || W > kMaxCells || cells > kMaxCells || !store_supported(H, W, S)) return MBV_ERR_UNSUPPORTED;
  if (!instance_maps || (Q > 0 && !query_track) || !world_from_cur || !cur_from_world || !owner || !count || !window || !fused_ids)
    return MBV_ERR_BAD_ARG;
  const FuseGrid g{(int)H, (int)W, (int)S, (int)Q, x_lo, y_lo, voxel};
  const unsigned store_blocks = (unsigned)(((int64_t)S * S + kThreads - 1) / kThreads);
  const unsigned cell_blocks = (unsigned)((cells + kThreads - 1) / kThreads);
  for (int f = 0; f < F; ++f) {
    const int32_t* imap = instance_maps + (int64_t)f * cells;
    const int32_t* ids = query_track ? query_track + (int64_t)f * Q : nullptr;
    const double* m = world_from_cur + (int64_t)f * 6;
    const double* n = cur_from_world + (int64_t)f * 6;
    const double* vel = query_velocity ? query_velocity + (int64_t)f * Q * 2 : nullptr;
    hipLaunchKernelGGL(k_fuse_update, dim3(store_blocks), dim3(kThreads), 0, stream, g, imap, ids, m, n,
                       visibility ? visibility + (int64_t)f * cells : nullptr, vel, (int)cap, (int)hit, (int)miss, static_speed,
                       window, owner, count);
    MBV_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fuse_read, dim3(cell_blocks), dim3(kThreads), 0, stream, g, imap, ids, m, n, vel, (int)min_count,
                       static_speed, owner, count, window, fused_ids + (int64_t)f * cells,
                       fused_queries ? fused_queries + (int64_t)f * cells : nullptr);
    MBV_CHECK_LAUNCH();
  }
  return MBV_OK;
}

extern "C" int mbv_masks_from_map(const int32_t* maps, int32_t F, int32_t H, int32_t W, int32_t Q, uint32_t* masks_packed,
                                  int32_t* areas, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (F < 0 || Q < 0 || H < 1 || W < 1) return MBV_ERR_BAD_ARG;
  if (F == 0 || Q == 0) return MBV_OK;
  const int64_t hw = (int64_t)H * W;
  if (Q > kMaxQueries || F > 65535 || H > kMaxCells || W > kMaxCells || hw > kMaxCells) return MBV_ERR_UNSUPPORTED;
  if (!maps || !masks_packed || !areas) return MBV_ERR_BAD_ARG;
  const int64_t words = mbv_packed_mask_words(H, W);
  MBV_CHECK_HIP(mbv_fill_async(masks_packed, 0, (size_t)F * Q * words * sizeof(uint32_t), stream));
  MBV_CHECK_HIP(mbv_fill_async(areas, 0, (size_t)F * Q * sizeof(int32_t), stream));
  hipLaunchKernelGGL(k_masks_from_map, dim3((unsigned)((words * 32 + kThreads - 1) / kThreads), (unsigned)F), dim3(kThreads), 0, stream,
                     maps, hw, (int)Q, words, masks_packed, areas);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
