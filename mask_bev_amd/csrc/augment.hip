// K23 — training augmentations of scans and instance maps on the device.
//
// Replaces mask_bev/augmentations/semantic_kitti_mask_augmentations.py:44-161 (Flip, ShufflePoints, RandomRotate,
// DecimatePoints, JitterPoints, RandomDropPoints: numpy on the host, one sample at a time, cv2.warpAffine for the mask) and
// the point half of kitti_mask_augmentations.py:196-217 (GlobalNoise: one scale and one translation per sample).
//
// K23a, the per-point program.  The y dimension of the grid walks the scans, so a workgroup's op record (656 bytes, built on
// the host) is the same for all its lanes: it is read through uniform loads, and the op switch does not diverge.  A point's
// value stays in f32 registers between ops (the reference stores into an f32 array after each transform); `linear` and
// `jitter` compute in f64 with one rounding per operation (compiled with -ffp-contract=off).  Every random draw is a pure
// function of (sample seed, op slot, ORIGINAL index of the point in its scan, component): see maskbev_hip.h.
//   k_program<MODE 0>   no point is removed or moved: the result goes straight to the output
//   k_program<MODE 1/2> the result goes to a staging buffer, with a kept flag per point and (MODE 2) its sort key
// K23b, order and selection.
//   MODE 1 (drops only)  exclusive scan of the kept flags = the output row of every kept point: count, scan, scatter.
//   MODE 2 (a shuffle or a decimate somewhere in the batch)  key = scan << 26 | (order hash >> 6), or scan << 26 | index for
//                        a scan that keeps its order, or the invalid key B << 26 for a dropped point; K1's stable LSD sort;
//                        a scan's survivors are then adjacent, and the first keep_b of them are gathered.
//   No atomics anywhere: the output order is a pure function of the inputs.
// K23c, instance-map warp: one thread per output cell, nearest source cell under the transposed 2 x 2 matrix.
// All three are streaming kernels, latency-bound at 4 x 120 k points / 500 x 500 cells; no MFMA, LDS only in the block scans.
#include <limits.h>

#include "common.hpp"
#include "rng.hpp"
#include "sort.hpp"

namespace {

constexpr int kMaxOps = 8;
constexpr int kOrderSlot = 8;          // the op slot of the order hash (past the op list)
constexpr int kMaxBatch = 4096;
constexpr int kLowBits = 26;           // mode 2: key = scan << 26 | 26 bits of order hash or index (the same for every batch size)
constexpr int kMaxSortBatch = 63;      // ... so that the invalid key, batch << 26, fits 32 bits

enum : int32_t { OP_NONE = 0, OP_LINEAR = 1, OP_JITTER = 2, OP_DROP = 3, OP_SHUFFLE = 4, OP_DECIMATE = 5, OP_GLOBAL_NOISE = 6 };

struct AugOp {                         // 80 bytes
  int32_t code;
  uint32_t arg;                        // drop: T; decimate: k
  double p[9];                         // linear: a00 a01 a10 a11; jitter: magnitude, std x y z i, max_delta x y z i;
                                       // global noise: scale, tx, ty, tz
};
struct AugRecord {                     // 656 bytes
  uint32_t seed_lo, seed_hi;
  int32_t n_ops;
  int32_t flags;                       // bit 0: the scan's output order is the order hash's (a shuffle or decimate was drawn)
  AugOp ops[kMaxOps];
};
static_assert(sizeof(AugOp) == 80 && sizeof(AugRecord) == 656, "record layout is part of the C ABI");

__device__ __forceinline__ uint32_t aug_stream(uint32_t seed_lo, uint32_t seed_hi, uint32_t slot) {
  return pcg_hash(seed_lo ^ pcg_hash(seed_hi + slot * 0x9E3779B9u));
}
__device__ __forceinline__ uint32_t aug_draw(uint32_t stream, uint32_t idx, uint32_t comp, uint32_t j) {
  return pcg_hash(stream + (idx * 8u + comp * 2u + j));
}
__device__ __forceinline__ float aug_normal(uint32_t stream, uint32_t idx, uint32_t comp) {
  const uint32_t h1 = aug_draw(stream, idx, comp, 0u), h2 = aug_draw(stream, idx, comp, 1u);
  const float u1 = (float)((h1 >> 8) + 1u) * 5.9604644775390625e-08f;        // (0, 1]
  const float u2 = (float)(h2 >> 8) * 5.9604644775390625e-08f;               // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

template <int MODE>
__global__ void __launch_bounds__(256) k_program(const float* __restrict__ points, int dim, int64_t n,
                                                 const int32_t* __restrict__ offs, const AugRecord* __restrict__ records,
                                                 int low_bits, int scan_bits, uint32_t invalid_key,
                                                 float* __restrict__ dst, uint32_t* __restrict__ flags,
                                                 uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int b = blockIdx.y;
  const int64_t begin = offs[b] > 0 ? offs[b] : 0, end = offs[b + 1] < n ? offs[b + 1] : n;   // never past the buffers
  const AugRecord* __restrict__ rec = records + b;
  const uint32_t seed_lo = rec->seed_lo, seed_hi = rec->seed_hi;
  const int n_ops = rec->n_ops < kMaxOps ? rec->n_ops : kMaxOps;
  const bool permute = (rec->flags & 1) != 0;
  for (int64_t i = begin + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
    const uint32_t idx = (uint32_t)(i - begin);
    const float* p = points + i * dim;
    float v[4];
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    v[3] = dim == 4 ? p[3] : 0.f;
    bool keep = true;
    for (int s = 0; s < n_ops; ++s) {
      const AugOp& op = rec->ops[s];
      const int32_t code = op.code;
      if (code == OP_LINEAR) {
        const double x = (double)v[0], y = (double)v[1];
        v[0] = (float)(op.p[0] * x + op.p[1] * y);
        v[1] = (float)(op.p[2] * x + op.p[3] * y);
      } else if (code == OP_JITTER) {
        const uint32_t st = aug_stream(seed_lo, seed_hi, (uint32_t)s);
        const double mag = op.p[0];
        for (int c = 0; c < dim; ++c) {
          double d = op.p[1 + c] * (double)aug_normal(st, idx, (uint32_t)c);
          const double lim = op.p[5 + c];
          d = d < -lim ? -lim : (d > lim ? lim : d);
          v[c] = (float)((double)v[c] + mag * d);
        }
        if (dim == 4) v[3] = v[3] < 0.f ? 0.f : (v[3] > 1.f ? 1.f : v[3]);       // a NaN stays a NaN, as in np.clip
      } else if (code == OP_DROP) {
        const uint32_t h = aug_draw(aug_stream(seed_lo, seed_hi, (uint32_t)s), idx, 0u, 0u);
        keep = keep && (h >> 8) >= op.arg;
      } else if (code == OP_GLOBAL_NOISE) {
        for (int c = 0; c < 3; ++c) v[c] = (float)((double)v[c] * op.p[0] + op.p[1 + c]);
      }
    }
    float* o = dst + i * dim;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    if (dim == 4) o[3] = v[3];
    if (MODE >= 1) flags[i] = keep ? 1u : 0u;
    if (MODE == 2) {
      uint32_t key = invalid_key;
      if (keep) {
        const uint32_t low = permute ? (aug_draw(aug_stream(seed_lo, seed_hi, (uint32_t)kOrderSlot), idx, 0u, 0u) >> scan_bits)
                                     : idx;
        key = ((uint32_t)b << low_bits) | low;
      }
      keys[i] = key;
      vals[i] = (uint32_t)i;
    }
  }
}

// One thread: the survivors and the kept count of every scan, the new offsets.
template <int MODE>
__global__ void k_finish(const int32_t* __restrict__ offs, const AugRecord* __restrict__ records, int batch,
                         const uint32_t* __restrict__ fscan, int32_t* __restrict__ src_start, int32_t* __restrict__ out_offs,
                         int32_t* __restrict__ out_counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t acc_src = 0, acc_out = 0;
  for (int b = 0; b < batch; ++b) {
    int64_t m = MODE == 0 ? (int64_t)offs[b + 1] - offs[b] : (int64_t)fscan[offs[b + 1]] - (int64_t)fscan[offs[b]];
    int64_t keep = m;
    if (MODE == 2) {
      const AugRecord* rec = records + b;
      const int n_ops = rec->n_ops < kMaxOps ? rec->n_ops : kMaxOps;
      for (int s = 0; s < n_ops; ++s)
        if (rec->ops[s].code == OP_DECIMATE && rec->ops[s].arg > 1u) keep = (keep + rec->ops[s].arg - 1) / rec->ops[s].arg;
      src_start[b] = (int32_t)acc_src;
    }
    out_offs[b] = (int32_t)acc_out;
    out_counts[b] = (int32_t)keep;
    acc_src += m;
    acc_out += keep;
  }
  out_offs[batch] = (int32_t)acc_out;
}

__device__ __forceinline__ void copy_point(const float* __restrict__ src, float* __restrict__ dst, int dim) {
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
  if (dim == 4) dst[3] = src[3];
}

__global__ void __launch_bounds__(256) k_compact(const float* __restrict__ staged, int dim, int64_t n,
                                                 const uint32_t* __restrict__ flags, const uint32_t* __restrict__ fscan,
                                                 float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    if (flags[i]) copy_point(staged + i * dim, out + (int64_t)fscan[i] * dim, dim);      // fscan[i] < number kept <= n
}

__global__ void __launch_bounds__(256) k_gather_sorted(const float* __restrict__ staged, int dim, int64_t n,
                                                       const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                       int low_bits, int batch, uint32_t invalid_key,
                                                       const int32_t* __restrict__ src_start,
                                                       const int32_t* __restrict__ out_offs,
                                                       const int32_t* __restrict__ out_counts, float* __restrict__ out) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const uint32_t key = keys[p];
    if (key >= invalid_key) continue;
    const int b = (int)(key >> low_bits);                  // < batch: key < batch << low_bits
    const int64_t r = p - src_start[b];
    const uint32_t src = vals[p];
    if (r < 0 || r >= out_counts[b] || src >= (uint64_t)n) continue;
    copy_point(staged + (int64_t)src * dim, out + ((int64_t)out_offs[b] + r) * dim, dim);
  }
}

__global__ void __launch_bounds__(256) k_warp_maps(const int32_t* __restrict__ maps, const double* __restrict__ mats,
                                                   int nx, int ny, double cx, double cy, int32_t* __restrict__ out) {
  const int b = blockIdx.y;
  const double* a = mats + (int64_t)b * 4;
  const double a00 = a[0], a01 = a[1], a10 = a[2], a11 = a[3];
  const int64_t cells = (int64_t)nx * ny;
  const int32_t* __restrict__ in = maps + (int64_t)b * cells;
  int32_t* __restrict__ o = out + (int64_t)b * cells;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < cells; c += (int64_t)gridDim.x * 256) {
    const int ix = (int)(c / ny), iy = (int)(c - (int64_t)ix * ny);
    const double du = ((double)ix + 0.5) - cx, dv = ((double)iy + 0.5) - cy;
    const double su = floor((a00 * du + a10 * dv) + cx), sv = floor((a01 * du + a11 * dv) + cy);
    int32_t val = 0;
    if (su >= 0.0 && su < (double)nx && sv >= 0.0 && sv < (double)ny) val = in[(int64_t)su * ny + (int64_t)sv];   // NaN fails
    o[c] = val;
  }
}

int bit_length(uint32_t v) {
  int n = 0;
  while (v) { ++n; v >>= 1; }
  return n;
}

struct AugWorkspace {
  float* staged;
  uint32_t *flags, *fscan, *partials, *keys_a, *keys_b, *vals_a, *vals_b, *hist;
  int32_t* src_start;
  size_t bytes;
};

AugWorkspace carve_augment(void* ws, int64_t n, int batch, int mode) {
  MbvCarver c(ws);
  AugWorkspace w = {};
  if (mode >= 1) {
    w.staged = c.take<float>((size_t)n * 4);
    w.flags = c.take<uint32_t>((size_t)n + 1);
    w.fscan = c.take<uint32_t>((size_t)n + 1);
    const int64_t hist_words = 256 * (radix_sort_blocks(n) > 0 ? radix_sort_blocks(n) : 1);
    const int64_t scan_len = n + 1 > hist_words ? n + 1 : hist_words;
    w.partials = c.take<uint32_t>((size_t)((scan_len + kScanTile - 1) / kScanTile + 1));
    if (mode == 2) {
      w.keys_a = c.take<uint32_t>((size_t)n);
      w.keys_b = c.take<uint32_t>((size_t)n);
      w.vals_a = c.take<uint32_t>((size_t)n);
      w.vals_b = c.take<uint32_t>((size_t)n);
      w.hist = c.take<uint32_t>((size_t)hist_words);
      w.src_start = c.take<int32_t>((size_t)batch + 1);
    }
  }
  w.bytes = c.off;
  return w;
}

unsigned stream_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b < 2048 ? b : 2048));
}

}  // namespace

extern "C" size_t mbv_augment_workspace_bytes(int64_t n_points, int32_t batch, int32_t mode) {
  if (n_points < 0 || n_points > INT_MAX || batch < 1 || batch > kMaxBatch || mode < 0 || mode > 2) return 0;
  const size_t b = carve_augment(nullptr, n_points, batch, mode).bytes;
  return b ? b : 256;
}

extern "C" int mbv_augment_points(const float* points, int32_t dim, int64_t n_points, const int32_t* scan_offsets,
                                  int32_t batch, const void* records, int32_t mode, float* out, int32_t* out_offsets,
                                  int32_t* out_counts, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if ((dim != 3 && dim != 4) || n_points < 0 || n_points > INT_MAX || batch < 1 || batch > kMaxBatch || mode < 0 ||
      mode > 2)
    return MBV_ERR_BAD_ARG;
  if (!scan_offsets || !records || !out_offsets || !out_counts || (n_points > 0 && (!points || !out)))
    return MBV_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(records) & 7) return MBV_ERR_BAD_ARG;
  const int64_t n = n_points;
  const int low_bits = kLowBits, scan_bits = 32 - kLowBits;
  // an index key and the draw counter idx * 8 + ... must fit
  if (mode == 2 && (n >= ((int64_t)1 << kLowBits) || batch > kMaxSortBatch)) return MBV_ERR_UNSUPPORTED;
  if (n >= ((int64_t)1 << 28)) return MBV_ERR_UNSUPPORTED;
  const AugWorkspace w = carve_augment(workspace, n, batch, mode);
  if (mode >= 1 && (!workspace || workspace_bytes < w.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)))
    return MBV_ERR_WORKSPACE;
  const AugRecord* rec = reinterpret_cast<const AugRecord*>(records);
  const uint32_t invalid_key = (uint32_t)batch << low_bits;
  const dim3 grid(stream_blocks(n) < 1024 ? stream_blocks(n) : 1024, batch);

  if (mode == 0) {
    if (n > 0) {
      hipLaunchKernelGGL(k_program<0>, grid, dim3(256), 0, stream, points, dim, n, scan_offsets,
                       rec, low_bits, scan_bits,
                         invalid_key, out, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
      MBV_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_finish<0>, dim3(1), dim3(64), 0, stream, scan_offsets, rec, batch, (const uint32_t*)nullptr,
                       (int32_t*)nullptr, out_offsets, out_counts);
    MBV_CHECK_LAUNCH();
    return MBV_OK;
  }
  if (n == 0) {
    MBV_CHECK_HIP(mbv_fill_async(out_offsets, 0, sizeof(int32_t) * ((size_t)batch + 1), stream));
    MBV_CHECK_HIP(mbv_fill_async(out_counts, 0, sizeof(int32_t) * (size_t)batch, stream));
    return MBV_OK;
  }
  MBV_CHECK_HIP(mbv_fill_async(w.flags + n, 0, sizeof(uint32_t), stream));          // the scan's one-past-the-end input
  if (mode == 1) {
    hipLaunchKernelGGL(k_program<1>, grid, dim3(256), 0, stream, points, dim, n, scan_offsets,
                       rec, low_bits, scan_bits,
                       invalid_key, w.staged, w.flags, (uint32_t*)nullptr, (uint32_t*)nullptr);
  } else {
    hipLaunchKernelGGL(k_program<2>, grid, dim3(256), 0, stream, points, dim, n, scan_offsets,
                       rec, low_bits, scan_bits,
                       invalid_key, w.staged, w.flags, w.keys_a, w.vals_a);
  }
  MBV_CHECK_LAUNCH();
  int rc = launch_exclusive_scan(w.flags, w.fscan, n + 1, w.partials, stream);
  if (rc) return rc;
  if (mode == 1) {
    hipLaunchKernelGGL(k_finish<1>, dim3(1), dim3(64), 0, stream, scan_offsets, rec, batch, w.fscan, (int32_t*)nullptr,
                       out_offsets, out_counts);
    MBV_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_compact, dim3(stream_blocks(n)), dim3(256), 0, stream, w.staged, dim, n, w.flags, w.fscan, out);
    MBV_CHECK_LAUNCH();
    return MBV_OK;
  }
  hipLaunchKernelGGL(k_finish<2>, dim3(1), dim3(64), 0, stream, scan_offsets, rec, batch, w.fscan, w.src_start, out_offsets,
                     out_counts);
  MBV_CHECK_LAUNCH();
  uint32_t *ks, *vs;
  rc = launch_radix_sort(w.keys_a, w.vals_a, w.keys_b, w.vals_b, n, bit_length(invalid_key), w.hist, w.partials, stream, &ks, &vs);
  if (rc) return rc;
  hipLaunchKernelGGL(k_gather_sorted, dim3(stream_blocks(n)), dim3(256), 0, stream, w.staged, dim, n, ks, vs, low_bits,
                     batch, invalid_key, w.src_start, out_offsets, out_counts, out);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_warp_instance_maps(const int32_t* maps, const double* mats, int32_t batch, int32_t nx, int32_t ny,
                                      double cx, double cy, int32_t* out, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (batch < 0 || batch > 65535 || nx < 1 || ny < 1 || (int64_t)nx * ny > ((int64_t)1 << 26)) return MBV_ERR_BAD_ARG;
  if (batch == 0) return MBV_OK;
  if (!maps || !mats || !out || maps == out) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_warp_maps, dim3(stream_blocks((int64_t)nx * ny), batch), dim3(256), 0, stream, maps, mats, nx, ny, cx,
                     cy, out);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
