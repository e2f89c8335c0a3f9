// K25 — oriented box of a bit-packed BEV mask: the moment-axis box of ALL set cells.
//
// Stands where mask_to_pred (mask_bev/evaluation/kitti_eval.py:27-45) takes cv2.minAreaRect of the largest contour on the
// host.  One workgroup per listed row.  Sweep 1: popcount + bit iteration over the row's words gives n and the raw integer
// moments Σx, Σy, Σx², Σy², Σxy (int64, exact), reduced across the workgroup by shuffles and one LDS step.  Thread 0 forms the
// central moments n Σxy - Σx Σy, ... in int64 (exact up to a full 1024 x 1024 mask), converts them to f64 and takes
// theta = atan2(2 m11, m20 - m02) / 2.  Sweep 2: the projections of the set cells' centres on the axis at theta and on its
// normal, min and max per thread, reduced the same way (min / max: no order dependence, no float atomics).  The extents add
// |cos| + |sin|, the support of the unit cell, so an axis-aligned a x b block of cells gives exactly (a, b).  All of it in
// f64 with one rounding per operation (no contraction: build.py), one rounding to f32 at the store.
#include "common.hpp"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / MBV_WAVE;

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// the word `wi` of a map of `npix` pixels with the bits at and beyond npix cleared
__device__ __forceinline__ uint32_t load_word(const uint32_t* __restrict__ map, int64_t wi, int64_t npix) {
  const int64_t left = npix - wi * 32;
  if (left <= 0) return 0u;
  const uint32_t w = map[wi];
  return left >= 32 ? w : (w & ((1u << (int)left) - 1u));
}

__global__ void __launch_bounds__(kThreads) k_fit_boxes(const uint32_t* __restrict__ packed, int64_t num_maps, int64_t words,
                                                        int H, int W, const int32_t* __restrict__ rows,
                                                        int32_t* __restrict__ n_out, int64_t* __restrict__ moments,
                                                        float* __restrict__ boxes) {
  __shared__ long long s_sum[6][kWaves];
  __shared__ double s_ext[4][kWaves];
  __shared__ double s_axis[2];
  __shared__ int s_empty;
  const int r = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t row = rows[r];
  const bool valid = row >= 0 && row < num_maps;                       // a row outside the table counts as an empty mask
  const uint32_t* __restrict__ map = packed + (valid ? row : 0) * words;
  const int64_t npix = valid ? (int64_t)H * W : 0;
  const int64_t nwords = (npix + 31) / 32;

  long long acc[6] = {0, 0, 0, 0, 0, 0};                               // n, Σx, Σy, Σx², Σy², Σxy
  for (int64_t wi = t; wi < nwords; wi += kThreads) {
    uint32_t bits = load_word(map, wi, npix);
    while (bits) {
      const int b = __ffs((int)bits) - 1;
      bits &= bits - 1;
      const int p = (int)(wi * 32) + b;
      const long long y = p / W, x = p - (int)y * W;
      acc[0] += 1; acc[1] += x; acc[2] += y; acc[3] += x * x; acc[4] += y * y; acc[5] += x * y;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const long long v = wave_sum_ll(acc[k]);
    if (lane == 0) s_sum[k][wave] = v;
  }
  __syncthreads();
  long long m[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    m[k] = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) m[k] += s_sum[k][w];              // the same order in every thread: the same value
  }
  if (t == 0) {
    n_out[r] = (int32_t)m[0];
#pragma unroll
    for (int k = 0; k < 5; ++k) moments[(int64_t)r * 5 + k] = m[k + 1];
    double c = 1.0, s = 0.0;
    if (m[0] > 0) {
      const long long m20 = m[0] * m[3] - m[1] * m[1], m02 = m[0] * m[4] - m[2] * m[2], m11 = m[0] * m[5] - m[1] * m[2];
      const long long d = m20 - m02;
      const double theta = (m11 == 0 && d == 0) ? 0.0 : 0.5 * atan2(2.0 * (double)m11, (double)d);
      c = cos(theta);
      s = sin(theta);
      boxes[(int64_t)r * 5 + 4] = (float)theta;
    }
    s_axis[0] = c;
    s_axis[1] = s;
    s_empty = m[0] == 0;
  }
  __syncthreads();
  if (s_empty) {                                                       // uniform: a box of zeros, reported through n
    if (t < 5) boxes[(int64_t)r * 5 + t] = 0.f;
    return;
  }
  const double c = s_axis[0], s = s_axis[1];
  double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300;
  for (int64_t wi = t; wi < nwords; wi += kThreads) {
    uint32_t bits = load_word(map, wi, npix);
    while (bits) {
      const int b = __ffs((int)bits) - 1;
      bits &= bits - 1;
      const int p = (int)(wi * 32) + b;
      const int yi = p / W, xi = p - yi * W;
      const double x = (double)xi, y = (double)yi;
      const double u = x * c + y * s, v = y * c - x * s;
      umin = fmin(umin, u); umax = fmax(umax, u); vmin = fmin(vmin, v); vmax = fmax(vmax, v);
    }
  }
  umin = wave_min_d(umin); umax = wave_max_d(umax); vmin = wave_min_d(vmin); vmax = wave_max_d(vmax);
  if (lane == 0) { s_ext[0][wave] = umin; s_ext[1][wave] = umax; s_ext[2][wave] = vmin; s_ext[3][wave] = vmax; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      umin = fmin(umin, s_ext[0][w]); umax = fmax(umax, s_ext[1][w]);
      vmin = fmin(vmin, s_ext[2][w]); vmax = fmax(vmax, s_ext[3][w]);
    }
    const double cell = fabs(c) + fabs(s), n = (double)m[0];
    float* __restrict__ o = boxes + (int64_t)r * 5;
    o[0] = (float)((double)m[1] / n);
    o[1] = (float)((double)m[2] / n);
    o[2] = (float)((umax - umin) + cell);
    o[3] = (float)((vmax - vmin) + cell);                              // o[4] = theta: stored above
  }
}

}  // namespace

extern "C" int mbv_fit_boxes(const uint32_t* packed, int64_t num_maps, int32_t H, int32_t W, const int32_t* rows,
                             int32_t num_rows, int32_t* n, int64_t* moments, float* boxes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (num_rows < 0 || num_maps < 0 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1024 * 1024) return MBV_ERR_BAD_ARG;
  if (num_rows == 0) return MBV_OK;
  if (!packed || !rows || !n || !moments || !boxes || num_maps == 0) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_fit_boxes, dim3((unsigned)num_rows), dim3(kThreads), 0, stream, packed, num_maps,
                     mbv_packed_mask_words(H, W), (int)H, (int)W, rows, n, moments, boxes);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
