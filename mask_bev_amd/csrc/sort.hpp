// Exclusive scan (u32) and stable LSD radix sort of (key, value) pairs, 8-bit digits: K1's sort (voxelize.hip), shared with
// K23b (augment.hip).  Kernels sit in an anonymous namespace: every translation unit that includes this gets its own copy.
#pragma once
#include "common.hpp"

namespace {

constexpr int kSortThreads = 256;
constexpr int kSortItems = 16;
constexpr int kSortTile = kSortThreads * kSortItems;  // keys per block and pass
constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanThreads * kScanItems;

// ---------------------------------------------------------------------------------------------
// exclusive scan (u32), three small kernels: tile sums → scan of sums → tile scan + offset
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* total, uint32_t* lds /*>=4*/) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint32_t wave_off = 0, tot = 0;
  const int nw = blockDim.x >> 6;
  for (int w = 0; w < nw; ++w) {
    const uint32_t s = lds[w];
    if (w < wave) wave_off += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return wave_off + inc - v;
}

__global__ void __launch_bounds__(kScanThreads) k_scan_reduce(const uint32_t* __restrict__ in, int64_t n,
                                                              uint32_t* __restrict__ partials) {
  __shared__ uint32_t lds[4];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j)
    if (base + j < n) s += in[base + j];
  uint32_t tot;
  block_exclusive_scan(s, &tot, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(1024) k_scan_partials(uint32_t* __restrict__ partials, int64_t nb) {
  __shared__ uint32_t lds[16];
  __shared__ uint32_t carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < nb; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? partials[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan(v, &tot, lds);
    const uint32_t carry = carry_s;
    if (i < nb) partials[i] = carry + ex;
    __syncthreads();
    if (threadIdx.x == 0) carry_s = carry + tot;
    __syncthreads();
  }
}

// `in` may alias `out` (in-place scan of the radix histogram): no __restrict__ on them.
__global__ void __launch_bounds__(kScanThreads) k_scan_apply(const uint32_t* in, int64_t n_in, int64_t n,
                                                             const uint32_t* __restrict__ partials, uint32_t* out) {
  __shared__ uint32_t lds[4];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t v[kScanItems];
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    v[j] = (base + j < n_in) ? in[base + j] : 0u;
    s += v[j];
  }
  uint32_t tot;
  uint32_t ex = block_exclusive_scan(s, &tot, lds) + partials[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    if (base + j < n) out[base + j] = ex;
    ex += v[j];
  }
}

// out[i] = sum of in[0 .. i) for i < n.  `in` holds n_in <= n elements (elements from n_in on count as zero and are never
// read): the row-start scan has one more output than inputs (row_start[V] = K) and must not read past the caller's array.
// `partials` holds ceil(n / kScanTile) words.
int launch_exclusive_scan(const uint32_t* in, uint32_t* out, int64_t n, uint32_t* partials, hipStream_t s,
                          int64_t n_in = -1) {
  if (n <= 0) return 0;
  if (n_in < 0 || n_in > n) n_in = n;
  const int64_t nb = (n + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)nb), dim3(kScanThreads), 0, s, in, n_in, partials);
  MBV_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(1024), 0, s, partials, nb);
  MBV_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(kScanThreads), 0, s, in, n_in, n, partials, out);
  MBV_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// stable LSD radix sort, 8-bit digits
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSortThreads) k_radix_hist(const uint32_t* __restrict__ keys, int64_t n, int shift,
                                                             uint32_t* __restrict__ hist, int nblocks) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSortTile;
#pragma unroll 4
  for (int j = 0; j < kSortItems; ++j) {
    const int64_t i = base + j * kSortThreads + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];  // digit-major
}

__global__ void __launch_bounds__(kSortThreads) k_radix_scatter(const uint32_t* __restrict__ keys_in,
                                                                const uint32_t* __restrict__ vals_in,
                                                                uint32_t* __restrict__ keys_out,
                                                                uint32_t* __restrict__ vals_out, int64_t n, int shift,
                                                                const uint32_t* __restrict__ hist_scanned,
                                                                int nblocks) {
  __shared__ uint32_t base[256];     // next free global slot of each digit for this block
  __shared__ uint32_t wcnt[4][256];  // per-wave digit counts of the current 256-key slice
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  base[tid] = hist_scanned[(int64_t)tid * nblocks + blockIdx.x];
  const int64_t tile = (int64_t)blockIdx.x * kSortTile;
  for (int j = 0; j < kSortItems; ++j) {
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const int64_t i = tile + j * kSortThreads + tid;
    const bool valid = i < n;
    const uint32_t key = valid ? keys_in[i] : 0u;
    const uint32_t val = valid ? vals_in[i] : 0u;
    const uint32_t d = (key >> shift) & 255u;
    // lanes of this wave holding the same digit: 8 ballots instead of a serial match loop
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const uint32_t rank = __popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcnt[wave][d] = __popcll(same);
    __syncthreads();
    if (valid) {
      uint32_t pos = base[d] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
      keys_out[pos] = key;
      vals_out[pos] = val;
    }
    __syncthreads();
    base[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
    __syncthreads();
  }
}

inline int64_t radix_sort_blocks(int64_t n) { return (n + kSortTile - 1) / kSortTile; }

// Sorts n > 0 (key, value) pairs by the low `bits` bits of the key, ascending and stable.  (keys_a, vals_a) hold the input;
// the sorted pairs end up in (*keys_out, *vals_out), one of the two buffer pairs.  `hist`: 256 * radix_sort_blocks(n) words,
// `partials`: ceil(256 * radix_sort_blocks(n) / kScanTile) words.
int launch_radix_sort(uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, int64_t n, int bits,
                      uint32_t* hist, uint32_t* partials, hipStream_t stream, uint32_t** keys_out, uint32_t** vals_out) {
  const int passes = (bits + 7) / 8;
  const int nblocks = (int)radix_sort_blocks(n);
  uint32_t *ka = keys_a, *kb = keys_b, *va = vals_a, *vb = vals_b;
  for (int p = 0; p < passes; ++p) {
    hipLaunchKernelGGL(k_radix_hist, dim3(nblocks), dim3(kSortThreads), 0, stream, ka, n, p * 8, hist, nblocks);
    MBV_CHECK_LAUNCH();
    int rc = launch_exclusive_scan(hist, hist, (int64_t)256 * nblocks, partials, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_radix_scatter, dim3(nblocks), dim3(kSortThreads), 0, stream, ka, va, kb, vb, n, p * 8, hist,
                       nblocks);
    MBV_CHECK_LAUNCH();
    uint32_t* t = ka; ka = kb; kb = t;
    t = va; va = vb; vb = t;
  }
  *keys_out = ka;
  *vals_out = va;
  return 0;
}

}  // namespace
