// K28 — KITTI object augmentations on the device: per-object perturbation and ground-truth pasting of points.
//
// Replaces the per-point halves of BoxNoise and ObjectSample (mask_bev/augmentations/kitti_mask_augmentations.py:227-323):
// mmdet3d's points_in_rbbox + points_transform_ (numba, every point against every box) and the numpy mask / concatenate
// that removes the scene points inside pasted boxes and appends the pasted points.  The per-frame decisions (which bank
// entries are pasted, each box's selected noise) are made on the host (object_augment.py) and arrive as one box table.
//
//   k_obj_scene    grid y walks the scans, so a workgroup's rows of the box table are the same for all its lanes: the box
//                  loop has a uniform trip count and uniform addresses (scalar loads), no divergent exit.  Every point is
//                  tested against every box of its scan; the moved value goes to a staging buffer with a kept flag.
//   scan           exclusive scan of the kept flags (sort.hpp), as K23b's mode 1.
//   k_obj_finish   one thread: the kept count and first output row of every scan, the first output row of every pasted
//                  segment (clipped to the bank and to the output's capacity).
//   k_obj_compact  kept scene points to their rows, input order kept.
//   k_obj_paste    grid y walks the pasted segments: bank rows → the rows behind the scan's kept points, moved by the
//                  first containing box with the move bit.
// No atomics: the output is a pure function of the inputs.  All arithmetic on coordinates is f64 with one rounding per
// operation (-ffp-contract=off); the kernels call no transcendental function.
#include <limits.h>

#include "common.hpp"
#include "sort.hpp"

namespace {

constexpr int kRow = 14;               // f64 per box-table row
constexpr int kMaxBoxes = 128;         // per scan
constexpr int kMaxBatch = 4096;
constexpr int kMaxSegments = 65535;
constexpr int kPasteBlocksX = 4;

// row: 0 cx, 1 cy, 2 cz, 3 l/2, 4 w/2, 5 h, 6 cos t, 7 sin t, 8 cos r, 9 sin r, 10 tx, 11 ty, 12 tz, 13 flags
__device__ __forceinline__ bool inside_box(const double* __restrict__ r, double x, double y, double z) {
  const double dx = x - r[0], dy = y - r[1];
  const double lx = r[6] * dx + r[7] * dy;
  const double ly = r[6] * dy - r[7] * dx;
  const double dz = z - r[2];
  return fabs(lx) < r[3] && fabs(ly) < r[4] && dz > 0.0 && dz < r[5];
}

// The fate of one point among `nb` rows: *drop = inside a row with bit 0; returns the first row with bit 1 that holds it, or -1.
__device__ __forceinline__ int visit_boxes(const double* __restrict__ rows, int nb, double x, double y, double z, bool* drop) {
  int mover = -1;
  bool d = false;
  for (int j = 0; j < nb; ++j) {                       // uniform: no early exit
    const double* __restrict__ r = rows + (int64_t)j * kRow;
    const int fl = (int)r[13];
    const bool in = inside_box(r, x, y, z);
    d = d || (in && (fl & 1));
    if (in && (fl & 2) && mover < 0) mover = j;
  }
  *drop = d;
  return mover;
}

__device__ __forceinline__ void move_point(const double* __restrict__ r, float* v) {
  const double dx = (double)v[0] - r[0], dy = (double)v[1] - r[1];
  v[0] = (float)(((r[8] * dx - r[9] * dy) + r[0]) + r[10]);
  v[1] = (float)(((r[9] * dx + r[8] * dy) + r[1]) + r[11]);
  v[2] = (float)((double)v[2] + r[12]);
}

struct ScanBoxes {
  const double* rows;
  int nb;
};

__device__ __forceinline__ ScanBoxes scan_boxes(const double* __restrict__ table, const int32_t* __restrict__ box_offs, int b,
                                                int64_t n_boxes, int max_boxes) {
  int64_t b0 = box_offs[b], b1 = box_offs[b + 1];
  b0 = b0 < 0 ? 0 : (b0 > n_boxes ? n_boxes : b0);
  b1 = b1 < b0 ? b0 : (b1 > n_boxes ? n_boxes : b1);               // never past the table
  int64_t nb = b1 - b0;
  if (nb > max_boxes) nb = max_boxes;
  ScanBoxes s = {table + b0 * kRow, (int)nb};
  return s;
}

__global__ void __launch_bounds__(256) k_obj_scene(const float* __restrict__ points, int dim, int64_t n,
                                                   const int32_t* __restrict__ offs, const double* __restrict__ table,
                                                   const int32_t* __restrict__ box_offs, int64_t n_boxes, int max_boxes,
                                                   float* __restrict__ staged, uint32_t* __restrict__ flags) {
  const int b = blockIdx.y;
  const int64_t begin = offs[b] > 0 ? offs[b] : 0, end = offs[b + 1] < n ? offs[b + 1] : n;   // never past the buffers
  const ScanBoxes sb = scan_boxes(table, box_offs, b, n_boxes, max_boxes);
  for (int64_t i = begin + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
    const float* p = points + i * dim;
    float v[4];
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    v[3] = dim == 4 ? p[3] : 0.f;
    bool drop;
    const int mover = visit_boxes(sb.rows, sb.nb, (double)v[0], (double)v[1], (double)v[2], &drop);
    if (mover >= 0) move_point(sb.rows + (int64_t)mover * kRow, v);
    float* o = staged + i * dim;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    if (dim == 4) o[3] = v[3];
    flags[i] = drop ? 0u : 1u;
  }
}

// One thread.  seg_info[s] = {scan, first output row, rows, first bank row}; a segment no scan owns keeps rows = 0.
__global__ void k_obj_finish(const int32_t* __restrict__ offs, int batch, int64_t n, const uint32_t* __restrict__ fscan,
                             const int32_t* __restrict__ segments, const int32_t* __restrict__ paste_offs, int n_segments,
                             int64_t n_bank, int64_t n_paste, int32_t* __restrict__ seg_info,
                             int32_t* __restrict__ out_offs, int32_t* __restrict__ out_counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int s = 0; s < n_segments; ++s) seg_info[4 * s + 2] = 0;
  int64_t acc = 0, pasted = 0, scene = 0;
  for (int b = 0; b < batch; ++b) {
    int64_t i0 = offs[b] > 0 ? offs[b] : 0, i1 = offs[b + 1] < n ? offs[b + 1] : n;
    if (i0 > n) i0 = n;
    if (i1 < i0) i1 = i0;
    int64_t kept = (int64_t)fscan[i1] - (int64_t)fscan[i0];
    if (kept > n - scene) kept = n - scene;                          // overlapping offsets: never past the output
    if (kept < 0) kept = 0;
    scene += kept;
    out_offs[b] = (int32_t)acc;
    int64_t rows = kept;
    int64_t s0 = paste_offs[b], s1 = paste_offs[b + 1];
    s0 = s0 < 0 ? 0 : (s0 > n_segments ? n_segments : s0);
    s1 = s1 < s0 ? s0 : (s1 > n_segments ? n_segments : s1);
    for (int64_t s = s0; s < s1; ++s) {
      int64_t first = segments[2 * s], cnt = segments[2 * s + 1];
      if (first < 0 || first > n_bank) { first = 0; cnt = 0; }
      if (cnt < 0) cnt = 0;
      if (cnt > n_bank - first) cnt = n_bank - first;                // never past the bank
      if (cnt > n_paste - pasted) cnt = n_paste - pasted;            // never past the output
      seg_info[4 * s + 0] = b;
      seg_info[4 * s + 1] = (int32_t)(acc + rows);
      seg_info[4 * s + 2] = (int32_t)cnt;
      seg_info[4 * s + 3] = (int32_t)first;
      rows += cnt;
      pasted += cnt;
    }
    out_counts[b] = (int32_t)rows;
    acc += rows;
  }
  out_offs[batch] = (int32_t)acc;
}

__global__ void __launch_bounds__(256) k_obj_compact(const float* __restrict__ staged, int dim, int64_t n,
                                                     const int32_t* __restrict__ offs, const uint32_t* __restrict__ flags,
                                                     const uint32_t* __restrict__ fscan, const int32_t* __restrict__ out_offs,
                                                     int64_t capacity, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int64_t begin = offs[b] > 0 ? offs[b] : 0, end = offs[b + 1] < n ? offs[b + 1] : n;
  if (begin >= end) return;
  const int64_t base = (int64_t)out_offs[b] - (int64_t)fscan[begin];
  for (int64_t i = begin + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
    if (!flags[i]) continue;
    const int64_t row = base + (int64_t)fscan[i];
    if (row < 0 || row >= capacity) continue;
    const float* src = staged + i * dim;
    float* dst = out + row * dim;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    if (dim == 4) dst[3] = src[3];
  }
}

__global__ void __launch_bounds__(256) k_obj_paste(const float* __restrict__ bank, const int32_t* __restrict__ seg_info,
                                                   const double* __restrict__ table, const int32_t* __restrict__ box_offs,
                                                   int64_t n_boxes, int max_boxes, int dim, int64_t capacity,
                                                   float* __restrict__ out) {
  const int s = blockIdx.y;
  const int b = seg_info[4 * s + 0];
  const int64_t dst0 = seg_info[4 * s + 1], cnt = seg_info[4 * s + 2], first = seg_info[4 * s + 3];
  if (cnt <= 0) return;
  const ScanBoxes sb = scan_boxes(table, box_offs, b, n_boxes, max_boxes);
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cnt; k += (int64_t)gridDim.x * 256) {
    const int64_t row = dst0 + k;
    if (row < 0 || row >= capacity) continue;
    const float* p = bank + (first + k) * 4;
    float v[4];
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    bool drop;                                                       // a pasted point is never dropped
    const int mover = visit_boxes(sb.rows, sb.nb, (double)v[0], (double)v[1], (double)v[2], &drop);
    if (mover >= 0) move_point(sb.rows + (int64_t)mover * kRow, v);
    float* o = out + row * dim;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    if (dim == 4) o[3] = v[3];
  }
}

__global__ void __launch_bounds__(256) k_points_in_boxes(const float* __restrict__ points, int dim, int64_t n,
                                                         const double* __restrict__ table, int n_boxes,
                                                         int32_t* __restrict__ index) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float* p = points + i * dim;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    int first = -1;
    for (int j = 0; j < n_boxes; ++j)                                // uniform: no early exit
      if (inside_box(table + (int64_t)j * kRow, x, y, z) && first < 0) first = j;
    index[i] = first;
  }
}

struct ObjWorkspace {
  float* staged;
  uint32_t *flags, *fscan, *partials;
  int32_t* seg_info;
  size_t bytes;
};

ObjWorkspace carve_object(void* ws, int64_t n, int n_segments) {
  MbvCarver c(ws);
  ObjWorkspace w = {};
  w.staged = c.take<float>((size_t)n * 4);
  w.flags = c.take<uint32_t>((size_t)n + 1);
  w.fscan = c.take<uint32_t>((size_t)n + 1);
  w.partials = c.take<uint32_t>((size_t)((n + 1 + kScanTile - 1) / kScanTile + 1));
  w.seg_info = c.take<int32_t>((size_t)n_segments * 4 + 4);
  w.bytes = c.off;
  return w;
}

unsigned stream_blocks(int64_t n, int64_t cap) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b < cap ? b : cap));
}

bool sizes_ok(int64_t n_points, int32_t batch, int32_t n_segments, int64_t n_paste) {
  return n_points >= 0 && n_points <= INT_MAX && batch >= 1 && batch <= kMaxBatch && n_segments >= 0 &&
         n_segments <= kMaxSegments && n_paste >= 0 && n_paste <= INT_MAX;
}

}  // namespace

extern "C" size_t mbv_object_augment_workspace_bytes(int64_t n_points, int32_t batch, int32_t n_segments) {
  if (!sizes_ok(n_points, batch, n_segments, 0)) return 0;
  return carve_object(nullptr, n_points, n_segments).bytes;
}

extern "C" int mbv_object_augment(const float* points, int32_t dim, int64_t n_points, const int32_t* scan_offsets,
                                  int32_t batch, const double* box_table, const int32_t* box_offsets, int64_t n_boxes,
                                  int32_t max_boxes, const float* bank_points, int64_t n_bank_points,
                                  const int32_t* paste_segments, const int32_t* paste_offsets, int32_t n_segments,
                                  int64_t n_paste_points, float* out, int32_t* out_offsets, int32_t* out_counts,
                                  void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if ((dim != 3 && dim != 4) || !sizes_ok(n_points, batch, n_segments, n_paste_points) || n_boxes < 0 || n_boxes > INT_MAX ||
      max_boxes < 0 || n_bank_points < 0 || n_bank_points > INT_MAX)
    return MBV_ERR_BAD_ARG;
  if (!scan_offsets || !box_offsets || !paste_offsets || !out_offsets || !out_counts) return MBV_ERR_BAD_ARG;
  if ((n_points > 0 && !points) || (n_boxes > 0 && !box_table) || (n_segments > 0 && (!paste_segments || !bank_points)))
    return MBV_ERR_BAD_ARG;
  const int64_t capacity = n_points + n_paste_points;
  if (capacity > 0 && !out) return MBV_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(box_table) & 7) return MBV_ERR_BAD_ARG;
  if (max_boxes > kMaxBoxes || capacity >= ((int64_t)1 << 28)) return MBV_ERR_UNSUPPORTED;
  const int64_t n = n_points;
  const ObjWorkspace w = carve_object(workspace, n, n_segments);
  if (!workspace || workspace_bytes < w.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255)) return MBV_ERR_WORKSPACE;

  MBV_CHECK_HIP(mbv_fill_async(w.flags + n, 0, sizeof(uint32_t), stream));          // the scan's one-past-the-end input
  if (n > 0) {
    hipLaunchKernelGGL(k_obj_scene, dim3(stream_blocks(n, 1024), batch), dim3(256), 0, stream, points, dim, n, scan_offsets,
                       box_table, box_offsets, n_boxes, max_boxes, w.staged, w.flags);
    MBV_CHECK_LAUNCH();
  }
  int rc = launch_exclusive_scan(w.flags, w.fscan, n + 1, w.partials, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_obj_finish, dim3(1), dim3(64), 0, stream, scan_offsets, batch, n, w.fscan, paste_segments,
                     paste_offsets, n_segments, n_bank_points, n_paste_points, w.seg_info, out_offsets, out_counts);
  MBV_CHECK_LAUNCH();
  if (n > 0) {
    hipLaunchKernelGGL(k_obj_compact, dim3(stream_blocks(n, 1024), batch), dim3(256), 0, stream, w.staged, dim, n,
                       scan_offsets, w.flags, w.fscan, out_offsets, capacity, out);
    MBV_CHECK_LAUNCH();
  }
  if (n_segments > 0 && n_paste_points > 0) {
    hipLaunchKernelGGL(k_obj_paste, dim3(kPasteBlocksX, n_segments), dim3(256), 0, stream, bank_points, w.seg_info, box_table,
                       box_offsets, n_boxes, max_boxes, dim, capacity, out);
    MBV_CHECK_LAUNCH();
  }
  return MBV_OK;
}

extern "C" int mbv_points_in_boxes(const float* points, int32_t dim, int64_t n_points, const double* box_table,
                                   int32_t n_boxes, int32_t* index, void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if ((dim != 3 && dim != 4) || n_points < 0 || n_points > INT_MAX || n_boxes < 0) return MBV_ERR_BAD_ARG;
  if (n_points == 0) return MBV_OK;
  if (!points || !index || (n_boxes > 0 && !box_table) || (reinterpret_cast<uintptr_t>(box_table) & 7)) return MBV_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_points_in_boxes, dim3(stream_blocks(n_points, 2048)), dim3(256), 0, stream, points, dim, n_points,
                     box_table, n_boxes, index);
  MBV_CHECK_LAUNCH();
  return MBV_OK;
}
