// stand-alone: variants of the K43 blend stream at the bench arena size (not part of the product)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("hip error %d line %d\n", (int)e, __LINE__); return 1; } } while (0)

__device__ __forceinline__ f4 blend4(f4 a, f4 p, float w) {
#pragma clang fp contract(off)
  f4 r;
  for (int k = 0; k < 4; ++k) { const float d = p[k] - a[k]; r[k] = a[k] + w * d; }
  return r;
}

template <int U, bool NTL, bool NTS>
__global__ void __launch_bounds__(256) k_blend(const float* __restrict__ param, float* __restrict__ avg, long n4, const float* wp) {
  const float w = *wp;
  if (w == 0.f) return;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + (U - 1) * stride < n4; i += U * stride) {
    f4 p[U], a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long j = i + u * stride;
      p[u] = NTL ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(param) + j) : reinterpret_cast<const f4*>(param)[j];
      a[u] = NTL ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(avg) + j) : reinterpret_cast<const f4*>(avg)[j];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long j = i + u * stride;
      const f4 r = blend4(a[u], p[u], w);
      if (NTS) __builtin_nontemporal_store(r, reinterpret_cast<f4*>(avg) + j); else reinterpret_cast<f4*>(avg)[j] = r;
    }
  }
  for (; i < n4; i += stride) {
    const f4 p = reinterpret_cast<const f4*>(param)[i];
    const f4 a = reinterpret_cast<const f4*>(avg)[i];
    reinterpret_cast<f4*>(avg)[i] = blend4(a, p, w);
  }
}

// blocked partition: block b walks its own contiguous chunk of f4 items
template <bool NT>
__global__ void __launch_bounds__(256) k_blend_chunk(const float* __restrict__ param, float* __restrict__ avg, long n4, const float* wp) {
  const float w = *wp;
  if (w == 0.f) return;
  const long chunk = ((n4 + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
  const long lo = (long)blockIdx.x * chunk;
  const long hi = lo + chunk < n4 ? lo + chunk : n4;
  for (long i = lo + threadIdx.x; i < hi; i += 256) {
    const f4 p = NT ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(param) + i) : reinterpret_cast<const f4*>(param)[i];
    const f4 a = NT ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(avg) + i) : reinterpret_cast<const f4*>(avg)[i];
    const f4 r = blend4(a, p, w);
    if (NT) __builtin_nontemporal_store(r, reinterpret_cast<f4*>(avg) + i); else reinterpret_cast<f4*>(avg)[i] = r;
  }
}

int main() {
  const long n = 200812352, n4 = n / 4;
  float *p, *a, *w;
  CK(hipMalloc(&p, n * 4)); CK(hipMalloc(&a, n * 4)); CK(hipMalloc(&w, 4));
  CK(hipMemset(p, 0, n * 4)); CK(hipMemset(a, 0, n * 4));
  const float hw = 1e-4f;
  CK(hipMemcpy(w, &hw, 4, hipMemcpyHostToDevice));
  struct V { const char* name; void (*k)(const float*, float*, long, const float*); unsigned blocks; };
  const unsigned cap = 4096, full = (unsigned)((n4 + 255) / 256);
  std::vector<V> vs = {
    {"U1 nt/nt cap4096 (product)", k_blend<1, true, true>, cap},
    {"U2 nt/nt cap4096", k_blend<2, true, true>, cap},
    {"U4 nt/nt cap4096", k_blend<4, true, true>, cap},
    {"U1 plain/nt cap4096", k_blend<1, false, true>, cap},
    {"U1 plain/plain cap4096", k_blend<1, false, false>, cap},
    {"U2 plain/plain cap4096", k_blend<2, false, false>, cap},
    {"U1 nt/nt cap2048", k_blend<1, true, true>, 2048},
    {"U1 nt/nt cap8192", k_blend<1, true, true>, 8192},
    {"U2 nt/nt cap2048", k_blend<2, true, true>, 2048},
    {"U1 nt/nt full grid", k_blend<1, true, true>, full},
    {"chunk nt cap4096", k_blend_chunk<true>, cap},
    {"chunk nt cap2048", k_blend_chunk<true>, 2048},
    {"chunk nt cap16384", k_blend_chunk<true>, 16384},
    {"chunk plain cap4096", k_blend_chunk<false>, cap},
    {"U1 nt/nt cap65536", k_blend<1, true, true>, 65536},
  };
  const int rounds = 23, warm = 3;
  std::vector<std::vector<float>> t(vs.size());
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int r = 0; r < rounds; ++r)
    for (size_t v = 0; v < vs.size(); ++v) {
      const size_t idx = (v + r) % vs.size();          // rotate the order
      CK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(vs[idx].k, dim3(vs[idx].blocks), dim3(256), 0, 0, p, a, n4, w);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      CK(hipGetLastError());
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= warm) t[idx].push_back(ms);
    }
  for (size_t v = 0; v < vs.size(); ++v) {
    std::sort(t[v].begin(), t[v].end());
    const float med = t[v][t[v].size() / 2];
    printf("%-30s median %.4f ms  min %.4f  max %.4f  %.2f TB/s\n", vs[v].name, med, t[v].front(), t[v].back(), n * 12.0 / (med * 1e-3) / 1e12);
  }
  return 0;
}
