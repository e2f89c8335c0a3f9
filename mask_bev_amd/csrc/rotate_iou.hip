// K26 — rotated-box overlap of every (box, query box) pair of every frame, one launch for a whole validation set.
//
// Stands where rotate_iou_gpu_eval (mask_bev/evaluation/rotate_iou.py, numba-CUDA) is called once per part of the set.  One
// thread per pair; the frame is found by a binary search in the pair offsets.  The intersection is the first rectangle
// clipped against the four half-planes of the second (Sutherland-Hodgman) and the shoelace area of what is left — not the
// reference's "collect vertices, sort by angle", which is discontinuous for identical and edge-sharing boxes.
//
// The corners are those of rasterize.box_vertices: centre ± (dx / 2) d ± (dy / 2) d_bar with d = (cos a, sin a) and
// d_bar = (-sin a, cos a), i.e. the angle turns counter-clockwise.  The first box's corners are taken relative to the second
// box's centre and expressed in its axes (d2, d_bar2), where the four half-planes are |x| <= dx2 / 2 and |y| <= dy2 / 2: a
// clipped coordinate is then set to the bound itself, and the differences of centres are formed before anything is rotated.
//
// The polygon (at most 8 vertices) lives in two fixed arrays that are only ever indexed by unrolled loop counters; a vertex
// is appended by a select over the slots, so nothing is addressed dynamically and the kernel needs no scratch.
//
// K26b — the same pairs for boxes with a height, (x, y, z, dx, dy, dz, angle) with z the bottom face: the BEV intersection of
// the same device function times the length of the common z-interval, over the volumes (the reference's d3_box_overlap_kernel
// with z_center = 1, in a z-up frame).  mbv_rotate_iou keeps its signature and its arithmetic.
#include "common.hpp"

namespace {

constexpr int kThreads = 256, kMaxVerts = 8;

struct Poly {
  float x[kMaxVerts], y[kMaxVerts];
  int n;
};

__device__ __forceinline__ void push(Poly& p, float vx, float vy) {
#pragma unroll
  for (int k = 0; k < kMaxVerts; ++k) {
    const bool here = p.n == k;
    p.x[k] = here ? vx : p.x[k];
    p.y[k] = here ? vy : p.y[k];
  }
  p.n += p.n < kMaxVerts ? 1 : 0;
}

// One Sutherland-Hodgman pass against the half-plane sign * coord <= bound (kAxis 0: x, 1: y).  A point on the boundary is
// inside.  The crossing point takes the bound itself as its clipped coordinate.
template <int kAxis>
__device__ __forceinline__ Poly clip(const Poly& in, float sign, float bound) {
  Poly out;
  out.n = 0;
#pragma unroll
  for (int k = 0; k < kMaxVerts; ++k) { out.x[k] = 0.f; out.y[k] = 0.f; }
  // the vertex in front of vertex 0: the last one
  float px = 0.f, py = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxVerts; ++k) {
    const bool last = k == in.n - 1;
    px = last ? in.x[k] : px;
    py = last ? in.y[k] : py;
  }
#pragma unroll
  for (int k = 0; k < kMaxVerts; ++k) {
    if (k < in.n) {
      const float cx = in.x[k], cy = in.y[k];
      const float sp = bound - sign * (kAxis == 0 ? px : py), sc = bound - sign * (kAxis == 0 ? cx : cy);   // >= 0: inside
      const bool pin = sp >= 0.f, cin = sc >= 0.f;
      if (pin != cin) {
        const float t = sp / (sp - sc);
        const float ix = kAxis == 0 ? sign * bound : px + t * (cx - px);
        const float iy = kAxis == 1 ? sign * bound : py + t * (cy - py);
        push(out, ix, iy);
      }
      if (cin) push(out, cx, cy);
      px = cx;
      py = cy;
    }
  }
  return out;
}

__device__ __forceinline__ float intersection_area(const float* __restrict__ a, const float* __restrict__ b) {
  float sa, ca, sb, cb;
  sincosf(a[4], &sa, &ca);
  sincosf(b[4], &sb, &cb);
  const float ox = a[0] - b[0], oy = a[1] - b[1];
  const float hl = 0.5f * a[2], hw = 0.5f * a[3];
  // box_vertices' order: +d +d_bar, -d +d_bar, -d -d_bar, +d -d_bar
  const float sl[4] = {1.f, -1.f, -1.f, 1.f}, sw[4] = {1.f, 1.f, -1.f, -1.f};
  Poly p;
  p.n = 4;
#pragma unroll
  for (int k = 0; k < kMaxVerts; ++k) { p.x[k] = 0.f; p.y[k] = 0.f; }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float wx = ox + (sl[k] * hl) * ca - (sw[k] * hw) * sa;       // relative to the second box's centre, world axes
    const float wy = oy + (sl[k] * hl) * sa + (sw[k] * hw) * ca;
    p.x[k] = wx * cb + wy * sb;                                        // along d2
    p.y[k] = wy * cb - wx * sb;                                        // along d_bar2
  }
  const float bx = 0.5f * fabsf(b[2]), by = 0.5f * fabsf(b[3]);
  p = clip<0>(p, 1.f, bx);
  p = clip<0>(p, -1.f, bx);
  p = clip<1>(p, 1.f, by);
  p = clip<1>(p, -1.f, by);
  if (p.n < 3) return 0.f;
  // shoelace about vertex 0: the terms stay of the size of the intersection
  float twice = 0.f;
#pragma unroll
  for (int k = 1; k + 1 < kMaxVerts; ++k) {
    if (k + 1 < p.n) {
      twice += (p.x[k] - p.x[0]) * (p.y[k + 1] - p.y[0]) - (p.x[k + 1] - p.x[0]) * (p.y[k] - p.y[0]);
    }
  }
  return 0.5f * fabsf(twice);
}

// The pair a thread works on: frame f is the last one with pair_offsets[f] <= idx (frames without pairs share their offset
// with the next one); false when the frame has no query box or the tables and offsets disagree (such a pair reads nothing).
__device__ __forceinline__ bool locate_pair(int64_t idx, const int32_t* __restrict__ box_offsets,
                                            const int32_t* __restrict__ qbox_offsets,
                                            const int64_t* __restrict__ pair_offsets, int frames, int64_t n_boxes,
                                            int64_t n_qboxes, int64_t& i, int64_t& j) {
  int lo = 0, hi = frames - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pair_offsets[mid] <= idx) lo = mid; else hi = mid - 1;
  }
  const int f = lo;
  const int64_t local = idx - pair_offsets[f];
  const int64_t k_f = (int64_t)qbox_offsets[f + 1] - qbox_offsets[f];
  if (k_f <= 0 || local < 0) return false;
  i = box_offsets[f] + local / k_f;
  j = qbox_offsets[f] + local % k_f;
  return i >= 0 && i < n_boxes && j >= 0 && j < n_qboxes;
}

__global__ void __launch_bounds__(kThreads) k_rotate_iou(const float* __restrict__ boxes, const float* __restrict__ qboxes,
                                                         const int32_t* __restrict__ box_offsets,
                                                         const int32_t* __restrict__ qbox_offsets,
                                                         const int64_t* __restrict__ pair_offsets, int frames,
                                                         int64_t n_boxes, int64_t n_qboxes, int64_t total, int criterion,
                                                         float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  float r = 0.f;
  int64_t i, j;
  if (locate_pair(idx, box_offsets, qbox_offsets, pair_offsets, frames, n_boxes, n_qboxes, i, j)) {
    float a[5], b[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) { a[c] = boxes[i * 5 + c]; b[c] = qboxes[j * 5 + c]; }
    const float inter = intersection_area(a, b);
    if (inter > 0.f) {
      const float area_a = fabsf(a[2] * a[3]), area_b = fabsf(b[2] * b[3]);
      const float den = criterion == -1 ? area_a + area_b - inter : criterion == 0 ? area_a : criterion == 1 ? area_b : 1.f;
      r = inter / den;
    }
  }
  out[idx] = r;
}

// K26b — the same pairs for boxes with a height: (x, y, z, dx, dy, dz, angle), z the BOTTOM face.  The overlap is K26's BEV
// intersection times the length of the common z-interval; exactly 0 where either is empty.
__global__ void __launch_bounds__(kThreads) k_rotate_iou_3d(const float* __restrict__ boxes, const float* __restrict__ qboxes,
                                                            const int32_t* __restrict__ box_offsets,
                                                            const int32_t* __restrict__ qbox_offsets,
                                                            const int64_t* __restrict__ pair_offsets, int frames,
                                                            int64_t n_boxes, int64_t n_qboxes, int64_t total, int criterion,
                                                            float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  float r = 0.f;
  int64_t i, j;
  if (locate_pair(idx, box_offsets, qbox_offsets, pair_offsets, frames, n_boxes, n_qboxes, i, j)) {
    float p[7], q[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) { p[c] = boxes[i * 7 + c]; q[c] = qboxes[j * 7 + c]; }
    const float a[5] = {p[0], p[1], p[3], p[4], p[6]}, b[5] = {q[0], q[1], q[3], q[4], q[6]};
    const float inter_bev = intersection_area(a, b);
    const float dz = fminf(p[2] + p[5], q[2] + q[5]) - fmaxf(p[2], q[2]);
    if (inter_bev > 0.f && dz > 0.f) {
      const float inter = inter_bev * dz;
      const float vol_a = fabsf(p[3] * p[4] * p[5]), vol_b = fabsf(q[3] * q[4] * q[5]);
      const float den = criterion == -1 ? vol_a + vol_b - inter : criterion == 0 ? vol_a : criterion == 1 ? vol_b : 1.f;
      r = inter / den;
    }
  }
  out[idx] = r;
}

}  // namespace

extern "C" int mbv_rotate_iou(const float* boxes, int64_t n_boxes, const float* qboxes, int64_t n_qboxes,
                              const int32_t* box_offsets, const int32_t* qbox_offsets, const int64_t* pair_offsets,
                              int32_t frames, int64_t total_pairs, int32_t criterion, float* overlaps, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (frames < 1 || n_boxes < 0 || n_qboxes < 0 || total_pairs < 0 || criterion < -1 || criterion > 2) return MBV_ERR_BAD_ARG;
  if (!box_offsets || !qbox_offsets || !pair_offsets) return MBV_ERR_BAD_ARG;
  if (total_pairs == 0) return MBV_OK;
  if (!boxes || !qboxes || !overlaps) return MBV_ERR_BAD_ARG;
  const int64_t blocks = (total_pairs + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return MBV_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_rotate_iou, dim3((unsigned)blocks), dim3(kThreads), 0, stream, boxes, qboxes, box_offsets, qbox_offsets,
                     pair_offsets, (int)frames, n_boxes, n_qboxes, total_pairs, (int)criterion, overlaps);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}

extern "C" int mbv_rotate_iou_3d(const float* boxes, int64_t n_boxes, const float* qboxes, int64_t n_qboxes,
                                 const int32_t* box_offsets, const int32_t* qbox_offsets, const int64_t* pair_offsets,
                                 int32_t frames, int64_t total_pairs, int32_t criterion, float* overlaps, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (frames < 1 || n_boxes < 0 || n_qboxes < 0 || total_pairs < 0 || criterion < -1 || criterion > 2) return MBV_ERR_BAD_ARG;
  if (!box_offsets || !qbox_offsets || !pair_offsets) return MBV_ERR_BAD_ARG;
  if (total_pairs == 0) return MBV_OK;
  if (!boxes || !qboxes || !overlaps) return MBV_ERR_BAD_ARG;
  const int64_t blocks = (total_pairs + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return MBV_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_rotate_iou_3d, dim3((unsigned)blocks), dim3(kThreads), 0, stream, boxes, qboxes, box_offsets,
                     qbox_offsets, pair_offsets, (int)frames, n_boxes, n_qboxes, total_pairs, (int)criterion, overlaps);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
