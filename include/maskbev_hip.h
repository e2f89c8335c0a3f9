/*
 * libmaskbev_hip.so — C ABI of the MI355X (gfx950) hot-path kernels of mask_bev_amd.
 *
 * Conventions (SURVEY.md §8b "Native (C-ABI) layer"):
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *   - the caller owns every buffer, including `workspace`; the library never allocates, frees or
 *     retains pointers, keeps no mutable global state and is re-entrant;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no hidden device sync;
 *   - return value: 0 = success, < 0 = an `mbv_status` code: bad argument, > 0 = hipError_t of a failed launch;
 *   - no exceptions, no abort, no stdout.
 *
 * Each entry point cites the reference interface it replaces (file:line under the reference tree).
 */
#ifndef MASKBEV_HIP_H_
#define MASKBEV_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MBV_OK = 0,
  MBV_ERR_BAD_ARG = -1,
  MBV_ERR_WORKSPACE = -2,
  MBV_ERR_UNSUPPORTED = -3
} mbv_status;

/* Library/ABI version; bumped whenever a signature below changes. */
int mbv_abi_version(void);

/* Storage type of an activation tensor.  Every `is_bf16` / `*_bf16` / `*_dtype` flag below takes one of these (the
 * flags were 0 / 1 before fp16 existed, hence their names): 2 selects IEEE half, computed by the same kernels
 * instantiated for `_Float16` (v_mfma_f32_32x32x16_f16; conversions round to nearest even, overflow -> inf).
 * Accumulation, softmax, LayerNorm statistics and every gradient of a parameter stay f32 for all three. */
#define MBV_DT_F32 0
#define MBV_DT_BF16 1
#define MBV_DT_F16 2

/* ------------------------------------------------------------------------------------------------
 * K1 — range filter + hard voxelisation of a batch of scans.
 * Replaces: MaskBevEncoder._filter_in_range (mask_bev/models/encoders/mask_bev_encoders.py:113-117)
 *           + MaskBevEncoder.voxelize (:95-111) → mmcv.ops.Voxelization (:69,100; mmcv 2.0.0
 *           hard_voxelize_forward, deterministic).
 * Semantics (bit-exact with the CPU reference): per point c = floor((p - min) / vs) in f32 with IEEE
 * division; pillar ids in order of FIRST APPEARANCE in the scan's point list; a pillar keeps its first
 * `max_points` points in input order; pillars beyond `max_voxels` per scan are dropped.
 *
 * points        (total_points, point_dim) f32, scans concatenated
 * scan_offsets  (batch + 1) i32, scan b owns points [scan_offsets[b], scan_offsets[b+1])
 * range/vs/grid x,y,z bounds (already rounded to f32), voxel sizes, grid sizes
 * prefilter     1 → apply the strict `min < p < max` test of :113-117 first
 * pillar_capacity  rows available in the outputs (>= min(total_points, batch*max_voxels))
 * coors         (pillar_capacity, 4) i32  (b, z, y, x)
 * num_points    (pillar_capacity) i32
 * pillar_points (pillar_capacity, max_points) i32: index into `points` of each kept point, -1 padded
 * row_start     (pillar_capacity + 1) i32: exclusive prefix sum of num_points (compact row of slot 0)
 * cell_to_pillar (batch, gz*gy*gx) i32: pillar id of every BEV cell, -1 if empty
 * counts        (batch + 2) i32: pillars per scan, then total pillars V, then total kept points K
 */
size_t mbv_voxelize_workspace_bytes(int64_t total_points, int32_t batch, int64_t cells_per_scan);

int mbv_voxelize(const float* points, int32_t point_dim, int64_t total_points,
                 const int32_t* scan_offsets, int32_t batch,
                 float x_min, float y_min, float z_min, float x_max, float y_max, float z_max,
                 float vx, float vy, float vz, int32_t gx, int32_t gy, int32_t gz,
                 int32_t prefilter, int32_t max_points, int32_t max_voxels, int64_t pillar_capacity,
                 int32_t* coors, int32_t* num_points, int32_t* pillar_points, int32_t* row_start,
                 int32_t* cell_to_pillar, int32_t* counts,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Dense (V, max_points, point_dim) zero-padded voxel tensor, i.e. the first return value of
 * mmcv.ops.Voxelization as exposed by MaskBevEncoder.voxelize (mask_bev_encoders.py:95-111). */
int mbv_gather_voxels(const float* points, int32_t point_dim, const int32_t* pillar_points,
                      int64_t num_pillars, int32_t max_points, float* voxels, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K2a — pillar decoration over REAL points only (no zero padding).
 * Replaces the input stage of mmdet3d PillarFeatureNet.forward(legacy=True, with_distance=True)
 * reached from MaskBevEncoder.encode (mask_bev_encoders.py:70-72,119-120).
 * rows  (K, point_dim + 7) f32 : [fc_x, fc_y, fc_z, extra.., cl_x, cl_y, cl_z, fc_x, fc_y, fc_z, |fc|]
 *        (fc = offset from the pillar centre — the legacy aliasing — cl = offset from the pillar mean)
 * row_pillar (K) i64 : pillar of each compact row
 */
int mbv_pfn_decorate(const float* points, int32_t point_dim, const int32_t* pillar_points,
                     const int32_t* num_points, const int32_t* row_start, const int32_t* coors,
                     int64_t num_pillars, int32_t max_points,
                     float vx, float vy, float vz, float x_off, float y_off, float z_off,
                     float* rows, int64_t* row_pillar, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K2b — the per-pillar (non-GEMM) parts of the PFNLayer stack, on real points + one representative padded row
 * per pillar with multiplicity max_points - n (identical to mmdet3d's dense zero-padded evaluation).
 * Replaces: mmdet3d PFNLayer.forward (Linear → BatchNorm1d(eps 1e-3, momentum 0.01) → ReLU → max over the point
 * slots → concat) reached from MaskBevEncoder.encode (mask_bev/models/encoders/mask_bev_encoders.py:70-72,
 * 119-120).  The Linear parts stay library GEMMs (y = a_prev W_a^T, t = max_prev W_b^T, y_pad = a_pad_prev W_a^T).
 * All tensors f32; `units` <= 128 channels; rows of pillar v are [row_start[v], row_start[v] + num_points[v]).
 * With 32 / 64 / 128 units and 16-byte aligned tensors the walks (apply_max, bwd_route, bwd_bn) give a lane four adjacent
 * channels: a wave instruction covers 64 / (units / 4) whole rows, and the wave's next pillar is requested while this one is
 * computed (pfn.hip k_pfn_*_v4); other unit counts take the lane = channel kernels.  Same results either way.
 * PRECONDITION of every mbv_pfn_* entry and of mbv_pfn_decorate: 1 <= num_points[v] <= max_points for every pillar v <
 * num_pillars (K1 never emits an empty pillar: a pillar exists because a point fell into its cell).  The walks request a
 * pillar's first rows unconditionally on a clamped index and the decoration reads slot num_points - 1; num_points lives on
 * the device, so the library cannot check it per call — an empty pillar is the caller's error (reads one row past the
 * compact rows for an empty LAST pillar).
 *   mbv_pfn_stats       y[r] += t[v], y_pad[v] += t[v] (when t != NULL); sums[0:U] = sum y, sums[U:2U] = sum y^2
 *                       over all V * max_points rows (padded rows weighted by their multiplicity), f64
 *   mbv_pfn_bn_finalize batch (training != 0) or running statistics → scale, shift, mean, rstd; updates the
 *                       running buffers in training mode (momentum, unbiased variance)
 *   mbv_pfn_apply_max   a = relu(y*scale+shift) (K, U), a_pad (V, U), m[v] = max over the pillar's rows and, if
 *                       n < max_points, its padded row; a / a_pad may be NULL for the last layer
 *   mbv_pfn_bwd_route   dz = relu'(.) * (dA + dM routed to the first maximal row [padded row last]); dz_pad holds
 *                       the SUM over the padded copies; sums = (sum dz, sum dz*xhat) f64 → d beta, d gamma
 *   mbv_pfn_bwd_bn      BatchNorm backward in place (dz → dy, dz_pad → summed dy_pad), dt[v] = sum_r dy[r] + dy_pad[v]
 */
/* K2c — the PFNLayer's `nn.Linear(in, out, bias=False)` (same reference lines) as a streaming exact-f32 GEMM for M >> C, N:
 * weight_is_nk != 0: y (m, n) = x (m, c) . w^T, w (n, c) with row stride ldw (forward; ldw > c reads a column block of a wider
 * weight: the [a | max] halves of a layer);  == 0: y (m, n) = x (m, c) . w, w (c, n) with row stride ldw (data gradient).
 * x, y contiguous f32; c <= 128, n in {32, 64, 96, 128} (mbv_skinny_gemm_f32_supported); c % 4 == 0 needs a 16-byte aligned x.
 * v_mfma_f32_32x32x2_f32 with the weight held in registers and 32-row tiles of x through wave-private LDS. */
int mbv_skinny_gemm_f32_supported(int64_t m, int32_t contraction, int32_t out_cols);
int mbv_skinny_gemm_f32(const float* x, const float* w, float* y, int64_t m, int32_t c, int32_t n, int32_t ldw,
                        int32_t weight_is_nk, void* stream);
/* y (m, n) = x (m, c) . w^T + add[index[row]] (add (*, n) f32, index (m) i64): the forward form with a gathered row addend. */
int mbv_skinny_gemm_f32_addrows(const float* x, const float* w, float* y, int64_t m, int32_t c, int32_t n, int32_t ldw,
                                const float* add, const int64_t* index, void* stream);

/* The forward of ALL PFN layers behind one call (the launches above + K2c, issued from inside): the eager section in front of
 * the captured step pays the host's time per launch.  rows (num_rows, in_features) f32 = the decorated compact rows;
 * weights[l] (units[l], in_features) for l = 0 and (units[l], 2 * units[l-1]) behind it ([a | max], mmdet3d PFNLayer);
 * gammas / betas / running_means / running_vars: the layer's BatchNorm1d (running statistics updated in place when training).
 * Every tensor of the pass lives in `workspace` (f32) at the offsets (in floats) mbv_pfn_forward_layout writes — 11 per
 * layer: y, y_pad, t, sums (2 units doubles), scale, shift, mean, rstd, a, a_pad, m; -1 = none — and returns the total for;
 * the last layer's m (num_pillars, units) is the result.  units[l] in {32, 64, 96, 128}, in_features <= 128, <= 8 layers.
 * row_pillar (num_rows) i64, nullable: the pillar of every row (mbv_pfn_decorate writes it).  Given, a layer's pillar term
 * W_b . max is added to y inside the Linear's launch (mbv_skinny_gemm_f32_addrows) and the BatchNorm statistics are a
 * streaming column-sum pass over y; without it the per-pillar walk of mbv_pfn_stats does both. */
int64_t mbv_pfn_forward_layout(int64_t num_rows, int64_t num_pillars, const int32_t* units, int32_t num_layers,
                               int64_t* offsets);
int mbv_pfn_forward(const float* rows, int32_t in_features, const int32_t* row_start, const int32_t* num_points,
                    const int64_t* row_pillar, int64_t num_rows, int64_t num_pillars, int32_t max_points,
                    const float* const* weights,
                    const float* const* gammas, const float* const* betas, float* const* running_means,
                    float* const* running_vars, const int32_t* units, int32_t num_layers, float eps, float momentum,
                    int32_t training, float* workspace, int64_t workspace_floats, void* stream);

int mbv_pfn_stats(float* y, const float* t, float* y_pad, const int32_t* row_start, const int32_t* num_points,
                  int64_t num_pillars, int32_t units, int32_t max_points, double* sums, void* stream);

int mbv_pfn_bn_finalize(const double* sums, double count, const float* gamma, const float* beta, float eps,
                        float momentum, int32_t training, float* running_mean, float* running_var, int32_t units,
                        float* scale, float* shift, float* mean, float* rstd, void* stream);

int mbv_pfn_apply_max(const float* y, const float* y_pad, const float* scale, const float* shift,
                      const int32_t* row_start, const int32_t* num_points, int64_t num_pillars, int32_t units,
                      int32_t max_points, float* a, float* a_pad, float* m, void* stream);

int mbv_pfn_bwd_route(const float* y, const float* y_pad, const float* scale, const float* shift,
                      const float* mean, const float* rstd, float* dz, int32_t has_da, const float* sum_da_pad,
                      const float* dm, const int32_t* row_start, const int32_t* num_points, int64_t num_pillars,
                      int32_t units, int32_t max_points, float* dz_pad, double* sums, void* stream);

int mbv_pfn_bwd_bn(const float* y, const float* y_pad, float* dz, float* dz_pad, const float* mean,
                   const float* rstd, const float* gamma, const double* sums, double count, int32_t training,
                   const int32_t* row_start, const int32_t* num_points, int64_t num_pillars, int32_t units,
                   int32_t max_points, float* dt, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K3 — PointPillarsScatter fused with the (C, H, W) LayerNorm; the dense canvas is never built.
 * Replaces: MaskBevEncoder.middle_encode (mask_bev_encoders.py:122-123 → mmdet3d PointPillarsScatter)
 *           + nn.LayerNorm([C, ny, nx], eps) (:75, :92).
 * feats (V, C) f32; pillar_batch_start (batch+1) i32 prefix of pillars per scan (scan b owns pillars
 * [start[b], start[b+1])); cell_to_pillar (batch, cells) i32; weight/bias (C, cells) f32;
 * out (batch, C, cells) f32; stats (batch, 2) f32 = (mean, rstd), saved for backward.
 * workspace: mbv_scatter_layernorm_workspace_bytes(batch).
 * ev_start / ev_stop: optional hipEvent_t (NULL = none) recorded on `stream` immediately before and
 * after the dominant streaming kernel of the call (the apply kernel / the dense backward kernel), so
 * that a caller can time exactly that kernel (bench.py's roofline figure).
 */
size_t mbv_scatter_layernorm_workspace_bytes(int32_t batch);

/* `patch` selects the layout of `out` (forward) and `grad_out` (backward):
 *   0  (batch, C, ny, nx) f32 — the reference's NCHW pseudo-image;
 *   4  (batch, ny/4, nx/4, 16*C) patch tokens in bf16 or half (`patch_dtype` = MBV_DT_BF16 / MBV_DT_F16), element (y%4)*4C + c*4 + x%4 of row (b, y/4, x/4): the input
 *      rows of the backbone's 4 x 4 non-overlapping patch projection (mmdet PatchEmbed built at
 *      mask_bev/models/backbones/swin.py:579-586), which then is one GEMM with no layout or cast pass.
 *      Needs mbv_scatter_layernorm_patch_supported(C, ny, nx, 4) (C % 32 == 0, ny % 4 == 0, nx % 4 == 0). */
int mbv_scatter_layernorm_patch_supported(int32_t channels, int32_t ny, int32_t nx, int32_t patch);

int mbv_scatter_layernorm_fwd(const float* feats, const int32_t* pillar_batch_start,
                              const int32_t* cell_to_pillar, const float* weight, const float* bias,
                              int32_t batch, int32_t channels, int32_t ny, int32_t nx, float eps,
                              int32_t patch, int32_t patch_dtype, void* out, float* stats, void* workspace,
                              size_t workspace_bytes, void* stream, void* ev_start, void* ev_stop);
/* ... with amax_out: an optional absmax record (64 zeroed words, mbv_f32_absmax_group's format) of the f32 (B, C, ny, nx) map
 * (patch == 0), max-combined by one atomic per workgroup: the K20 patch projection behind it (fp32 compute) then needs no pass
 * over the 0.5 GB map. */
int mbv_scatter_layernorm_fwd2(const float* feats, const int32_t* pillar_batch_start, const int32_t* cell_to_pillar,
                               const float* weight, const float* bias, int32_t batch, int32_t channels, int32_t ny, int32_t nx,
                               float eps, int32_t patch, int32_t patch_dtype, void* out, float* stats, void* workspace,
                               size_t workspace_bytes, uint32_t* amax_out, void* stream, void* ev_start, void* ev_stop);

/* Backward: grad_out (layout per `patch`) → grad_feats (V, C), grad_weight / grad_bias (C, cells).
 * `accumulate` != 0 adds into grad_weight / grad_bias instead of overwriting them. */
int mbv_scatter_layernorm_bwd(const void* grad_out, int32_t patch, int32_t patch_dtype, const float* feats,
                              const int32_t* pillar_batch_start, const int32_t* cell_to_pillar,
                              const float* weight, const float* stats,
                              int32_t batch, int32_t channels, int32_t ny, int32_t nx, int64_t num_pillars,
                              float* grad_feats, float* grad_weight, float* grad_bias, int32_t accumulate,
                              void* workspace, size_t workspace_bytes, void* stream,
                              void* ev_start, void* ev_stop);

/* The same backward with the AdamW update of the two (C, ny, nx) affine parameters fused into it (one GPU, one backward
 * per optimizer step): their gradients are complete in registers inside this kernel (the batch sum is per thread), so they
 * never go to memory — no grad_weight / grad_bias traffic, no read of them by mbv_adamw_step, no zero fill.  `weight` and
 * `bias` (C, cells) f32 are read-modify-written together with their moments exp_avg_* / exp_avg_sq_* and, when given, their
 * 16-bit shadows (`shadow_dtype` = MBV_DT_BF16 / MBV_DT_F16); the arithmetic is mbv_adamw_step's (torch/optim/adamw.py's
 * single-tensor order; `step` >= 1 = the optimizer's step count INCLUDING this update; grad_scale 1, no loss scaling).
 * Replaces: mmdet3d / torch nn.LayerNorm([C, ny, nx]) backward (mask_bev_encoders.py:75,92) + the optimizer step of those
 * two parameters (mask_bev_module.py:131-166). */
int mbv_scatter_layernorm_bwd_adamw(const void* grad_out, int32_t patch, int32_t patch_dtype, const float* feats,
                                    const int32_t* pillar_batch_start, const int32_t* cell_to_pillar, float* weight,
                                    float* bias, const float* stats, int32_t batch, int32_t channels, int32_t ny, int32_t nx,
                                    int64_t num_pillars, float* grad_feats, float* exp_avg_w, float* exp_avg_sq_w,
                                    float* exp_avg_b, float* exp_avg_sq_b, void* shadow_w, void* shadow_b,
                                    int32_t shadow_dtype, float lr, float beta1, float beta2, float eps, float weight_decay,
                                    int64_t step, int32_t decoupled, void* workspace, size_t workspace_bytes, void* stream,
                                    void* ev_start, void* ev_stop);

/* ------------------------------------------------------------------------------------------------
 * K5 — multi-scale deformable attention of the pixel decoder, forward / backward.
 * Replaces: mmcv MultiScaleDeformableAttention's `ms_deform_attn_forward/backward` CUDA op (or its
 * grid_sample fallback), configured at mask_bev/models/head/mask_bev_panoptic_head.py:127-136 and run inside
 * `self.pixel_decoder(x)` (mask_bev/models/networks/mask2former_head/mask2former_head.py:500).
 * value (B, Nv, H, D) f32; spatial_shapes (L, 2) i64 (h, w); level_start (L) i64; sampling_loc
 * (B, Nq, H, L, P, 2) f32 in [0, 1] (x, y); attn_weight (B, Nq, H, L, P) f32; out (B, Nq, H*D) f32.
 * Bilinear sampling at loc*size - 0.5 with zero padding (grid_sample align_corners=False).
 * head_dim must be a power of two <= 64.  spatial_shapes_host (nullable): the same (L, 2) shapes in HOST memory.
 * Backward, three forms: (a) head_dim == 32, host shapes given, every level map <= 4096 pixels — no global atomics:
 * d(value) is accumulated per (batch, head, 4-channel group) in a whole-map f64 LDS image and stored once (bitwise
 * reproducible up to the order of the LDS adds), d(location) / d(weight) are a separate gather; mbv_ms_deform_attn_bwd_split
 * says whether that form applies, and `part` (1 = the value part, 2 = the location / weight part, 3 = both) lets a
 * caller enqueue the two independent parts on two streams.  (b) host shapes given and num_query == num_value
 * (self-attention over the multi-scale map): bands of every level's map in LDS (f64), flushed bands and out-of-band
 * corners as global f32 atomics.  (c) otherwise: global f32 atomics.  (b) and (c) zero-fill grad_value themselves and
 * take only part == 3.  In form (a) with part == 1, bits 2.. of `part` may carry a mask of the levels whose d(value) this
 * call produces (0 = all): the per-level launches are independent (A/B experiments put them on different streams).
 */
int mbv_ms_deform_attn_fwd(const float* value, const int64_t* spatial_shapes, const int64_t* level_start,
                           const float* sampling_loc, const float* attn_weight,
                           int32_t batch, int32_t num_value, int32_t num_heads, int32_t head_dim,
                           int32_t num_levels, int32_t num_query, int32_t num_points,
                           float* out, void* stream);

/* The same forward, and the d(location) / d(weight) part of the split backward on its own, with the value map stored in
 * value_dtype (MBV_DT_F32 / _BF16 / _F16; head_dim % 4 == 0 resp. == 32): a 16-bit map halves the bytes of every bilinear tap
 * — what the two kernels are bound by — and is what the reference's value projection produces under 16-bit autocast. */
int mbv_ms_deform_attn_fwd_v(const void* value, int32_t value_dtype, const int64_t* spatial_shapes, const int64_t* level_start,
                             const float* sampling_loc, const float* attn_weight, int32_t batch, int32_t num_value,
                             int32_t num_heads, int32_t head_dim, int32_t num_levels, int32_t num_query, int32_t num_points,
                             float* out, void* stream);
int mbv_ms_deform_attn_bwd_locattn(const float* grad_out, const void* value, int32_t value_dtype, const int64_t* spatial_shapes,
                                   const int64_t* level_start, const float* sampling_loc, const float* attn_weight,
                                   int32_t batch, int32_t num_value, int32_t num_heads, int32_t head_dim, int32_t num_levels,
                                   int32_t num_query, int32_t num_points, float* grad_loc, float* grad_attn, void* stream);

int mbv_ms_deform_attn_bwd_split(int32_t head_dim, int32_t num_levels, const int64_t* spatial_shapes_host);

/* d(value) of form (a) with packed fixed-point LDS accumulators (16-bit compute modes): two adjacent channels of a
 * contribution are rounded to signed 32-bit fixed point and added as ONE `ds_add_u64` — half the LDS-atomic instructions
 * of the f64 form, all levels in one launch, order-independent (integer) sums.  The scale is taken per block from
 * L1 = sum over queries of (|attention weights| of the level) x (largest |grad_out| of the block's channels), an upper
 * bound of every pixel's sum for any sampling pattern, so the 32-bit halves cannot wrap; addends are rounded to
 * 2^-30 of that bound's power of two.  head_dim == 32, num_points == 4, every level map <= 16 384 pixels (one 128 KB plane of
 * packed pairs per block in dynamic LDS; the location / weight part the caller runs next is mbv_ms_deform_attn_bwd_locattn,
 * gathers without a map-size limit), host shapes required.  grad_value is written in `out_dtype` (MBV_DT_F32 / BF16 / F16) with `out_ld` elements between
 * consecutive (batch, value) rows — e.g. straight into the first H*D columns of the 16-bit matrix
 * [d value | d offsets | d logits] whose product with [Wv; Wo; Wa] is d(x).  Every element of that block is written
 * (no zero fill needed).  `_supported` returns 1 when the shape qualifies.  A first launch
 * re-lays grad_out (by 4-channel group), the locations and the weights (by level) into the caller's workspace
 * (`_workspace_bytes`), so that every block of the accumulation kernel reads contiguous streams (full cache lines).
 * Replaces the same mmcv backward as mbv_ms_deform_attn_bwd (value part). */
int mbv_ms_deform_attn_bwd_value_packed_supported(int32_t head_dim, int32_t num_levels, int32_t num_points,
                                                  int32_t num_query, const int64_t* spatial_shapes_host);
size_t mbv_ms_deform_attn_bwd_value_packed_workspace_bytes(int32_t batch, int32_t num_heads, int32_t num_levels,
                                                           int32_t num_query);
int mbv_ms_deform_attn_bwd_value_packed(const float* grad_out, const float* sampling_loc, const float* attn_weight,
                                        int32_t batch, int32_t num_value, int32_t num_heads, int32_t head_dim,
                                        int32_t num_levels, int32_t num_query, int32_t num_points,
                                        const int64_t* spatial_shapes_host, void* grad_value, int32_t out_dtype,
                                        int64_t out_ld, void* workspace, size_t workspace_bytes, void* stream);

int mbv_ms_deform_attn_bwd(const float* grad_out, const float* value, const int64_t* spatial_shapes,
                           const int64_t* level_start, const float* sampling_loc, const float* attn_weight,
                           int32_t batch, int32_t num_value, int32_t num_heads, int32_t head_dim,
                           int32_t num_levels, int32_t num_query, int32_t num_points,
                           const int64_t* spatial_shapes_host, float* grad_value, float* grad_loc, float* grad_attn,
                           int32_t part, void* stream);

/* K16 — the element-wise chain in front of K5, fused (mmcv MultiScaleDeformableAttention.forward:
 * `attention_weights.softmax(-1)`, `offset_normalizer = stack([W_l, H_l])`, `sampling_locations =
 * reference_points + sampling_offsets / offset_normalizer`; same call site as K5).
 * offsets (B, Nq, H, L, P, 2) and logits (B, Nq, H, L*P): both f32 (is_bf16 = 0) or both bf16 (is_bf16 = 1, the
 * autocast projections; the quotient is then rounded to bf16 before the f32 add, as torch's type promotion does);
 * ref_points (Nq, 2) f32 (x, y) in [0, 1]; spatial_shapes_host (L, 2) int64 (h, w) in HOST memory.
 * Outputs loc (B, Nq, H, L, P, 2) f32 and attn (B, Nq, H, L*P) f32 = softmax over the L*P samples of a head.
 * Backward: grad_loc / grad_attn (f32, from K5) and attn → grad_offsets / grad_logits in the input dtype.
 * Supported: L <= 8, L*P <= 16 (mbv_msda_prepare_supported); the caller composes torch ops otherwise. */
int mbv_msda_prepare_supported(int32_t num_levels, int32_t num_points);

/* The 16-bit GEMM inputs of the query side in one pass: x_lo = lo(x) (value projection input) and q_lo = lo(x + pos)
 * (offset / attention-weight projection input) for x (rows, C) f32 and pos (pos_rows, C) f32 repeating every pos_rows
 * rows — `query = query + query_pos` of mmcv MultiScaleDeformableAttention.forward under autocast (same call site).
 * dtype: MBV_DT_BF16 / MBV_DT_F16; C % 4 == 0. */
int mbv_msda_query_inputs(const float* x, const float* pos, int64_t rows, int64_t pos_rows, int32_t C, int32_t dtype,
                          void* x_lo, void* q_lo, void* stream);

int mbv_msda_prepare_fwd(const void* offsets, const void* logits, int32_t is_bf16, const float* ref_points,
                         const int64_t* spatial_shapes_host, int32_t batch, int32_t num_query, int32_t num_heads,
                         int32_t num_levels, int32_t num_points, float* loc, float* attn, void* stream);

/* Same with (batch, query) row strides (elements) for the two inputs — they can then be column blocks of ONE projection
 * GEMM's output, [offsets | logits] — and optional f32 biases (H*L*P*2) / (H*L*P) added to the loaded values in f32, for a
 * GEMM that left them out.  With L*P % 4 == 0 both pointers and strides must keep 4-element alignment. */
int mbv_msda_prepare_fwd_ld(const void* offsets, int64_t ld_offsets, const void* logits, int64_t ld_logits,
                            const float* bias_offsets, const float* bias_logits, int32_t is_bf16, const float* ref_points,
                            const int64_t* spatial_shapes_host, int32_t batch, int32_t num_query, int32_t num_heads,
                            int32_t num_levels, int32_t num_points, float* loc, float* attn, void* stream);

int mbv_msda_prepare_bwd(const float* grad_loc, const float* grad_attn, const float* attn,
                         const int64_t* spatial_shapes_host, int32_t batch, int32_t num_query, int32_t num_heads,
                         int32_t num_levels, int32_t num_points, int32_t out_bf16, void* grad_offsets,
                         void* grad_logits, void* stream);

/* Same with (batch, query) row strides for the two outputs (elements): they can then be columns of one wider gradient
 * matrix — next to the gradient of the value projection — that a single data-gradient GEMM consumes. */
int mbv_msda_prepare_bwd_ld(const float* grad_loc, const float* grad_attn, const float* attn,
                            const int64_t* spatial_shapes_host, int32_t batch, int32_t num_query, int32_t num_heads,
                            int32_t num_levels, int32_t num_points, int32_t out_bf16, void* grad_offsets,
                            int64_t ld_offsets, void* grad_logits, int64_t ld_logits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K4 — fused shifted-window multi-head attention (between the qkv and the output projection).
 * Replaces: ShiftWindowMSA.forward (mask_bev/models/networks/swin/swin.py:179-253: pad, roll, window
 * partition, mask, reverse, un-roll, crop) + WindowMSA.forward (:80-118: head split, q k^T * scale +
 * relative-position bias [+ shift mask], softmax, . v) + window_partition/reverse (:255-284).
 * qkv (B, H, W, 3C) channels-last, f32 (is_bf16 = 0: exact-f32 MFMA) or bf16 (is_bf16 = 1); tokens the
 * reference pads in take qkv_bias (3C) f32; bias_table ((2ws-1)^2, heads) f32; out (B, H, W, C) same dtype
 * as qkv; lse: mbv_window_attn_lse_elems(...) f32, saved for backward.  head_dim = C / heads must be
 * 16, 32 or 64 and ws <= 11.
 * Backward zero-fills grad_table ((2ws-1)^2, heads) and grad_qkv_bias (3C: gradient reaching the bias
 * through padded tokens; with full_bias_grad != 0 also the column sums of grad_qkv over the real tokens, i.e.
 * the whole bias gradient of the qkv Linear, which then skips its own pass over grad_qkv) itself, then accumulates them
 * with f32 atomics — unless accumulate != 0: then they are gradients to be added INTO (parameter-arena views), no fill.
 * grad_qkv (B, H, W, 3C) is written in full.
 */
int64_t mbv_window_attn_lse_elems(int32_t batch, int32_t H, int32_t W, int32_t heads, int32_t ws);

int mbv_window_attn_fwd(const void* qkv, const float* qkv_bias, const float* bias_table, int32_t is_bf16,
                        int32_t batch, int32_t H, int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t shift,
                        void* out, float* lse, void* stream);

int mbv_window_attn_bwd(const void* qkv, const float* qkv_bias, const float* bias_table, const void* out,
                        const void* grad_out, const float* lse, int32_t is_bf16,
                        int32_t batch, int32_t H, int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t shift,
                        void* grad_qkv, float* grad_table, float* grad_qkv_bias, int32_t full_bias_grad,
                        int32_t accumulate, void* stream);

/* K4 on f32 tensors in the SPLIT mode (fp32 compute; same tensors, results and reference lines as mbv_window_attn_fwd / _bwd with
 * is_bf16 = 0): every f32 operand element is split into an IEEE-half pair while its tile is staged (x 2^e = hi + lo: 22
 * significant bits) and every product is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_f16 with f32 accumulation — K20's arithmetic
 * (mbv_gemm32s_*) inside the attention — instead of v_mfma_f32_32x32x2_f32 at the f32 vector rate out of word-wise LDS images.
 * amax_qkv / amax_grad_out: absmax records of the tensors (64 words each, mbv_f32_absmax_group or a producing kernel's epilogue;
 * NULL = unscaled); amax_grad_qkv (optional): the record of what the backward stores, max-combined by one atomic per workgroup.
 * Requires head dims 16 / 32 / 64, C % 4 == 0, 16-byte aligned tensors (mbv_window_attn_split_supported; else
 * MBV_ERR_UNSUPPORTED and the caller keeps the exact-f32 form).  Accuracy: <= 2e-6 of the result's maximum (tests). */
int mbv_window_attn_split_supported(int32_t C, int32_t heads, int32_t ws);
int mbv_window_attn_split_fwd(const float* qkv, const float* qkv_bias, const float* bias_table, int32_t batch, int32_t H,
                              int32_t W, int32_t C, int32_t heads, int32_t ws, int32_t shift, const uint32_t* amax_qkv,
                              float* out, float* lse, void* stream);
int mbv_window_attn_split_bwd(const float* qkv, const float* qkv_bias, const float* bias_table, const float* out,
                              const float* grad_out, const float* lse, int32_t batch, int32_t H, int32_t W, int32_t C,
                              int32_t heads, int32_t ws, int32_t shift, const uint32_t* amax_qkv,
                              const uint32_t* amax_grad_out, float* grad_qkv, float* grad_table, float* grad_qkv_bias,
                              int32_t full_bias_grad, int32_t accumulate, uint32_t* amax_grad_qkv, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K8 — indexed bilinear point sampling of mask maps (loss and Hungarian targets).
 * Replaces: mmcv point_sample (= F.grid_sample, align_corners=False, zeros) at
 * mask_bev/models/networks/mask2former_head/mask2former_head.py:194-200,402-410 and the tensor gathers
 * feeding it (:227 `gt_masks[pos_assigned_gt_inds]`, :393 `mask_preds[mask_weights > 0]`).
 * out[g][p] = bilinear(src[src_index[g]] (H, W), coords[coord_index[g]][p] (x, y in [0, 1])).
 * src (num_src_maps, H, W) f32; src_index, coord_index (num_rows) i32; coords (*, num_points, 2) f32;
 * out / grad_out (num_rows, num_points) f32.
 * Backward zero-fills grad_src (num_src_maps, H, W) itself (skipped when every map is sampled: num_rows == num_src_maps).  For H*W <= 16384 each row's gradient tile is
 * accumulated in LDS and stored once, which requires src_index to hold no duplicates; larger maps use
 * global f32 atomics.
 */
int mbv_point_sample_fwd(const float* src, const int32_t* src_index, const float* coords,
                         const int32_t* coord_index, int32_t num_rows, int32_t num_points, int32_t H, int32_t W,
                         float* out, void* stream);

int mbv_point_sample_bwd(const float* grad_out, const int32_t* src_index, const float* coords,
                         const int32_t* coord_index, int32_t num_rows, int32_t num_points, int32_t H, int32_t W,
                         int64_t num_src_maps, float* grad_src, void* stream);

/* The same backward for a STACK of maps, (outer, inner, rows) of them, each sampled exactly once (num_rows == outer * inner *
 * rows, H*W <= 16384): the gradient of map (o, n, r) is stored at row (n, o, r) of grad_src — the two leading axes exchanged
 * — in f32, bf16 or fp16 (out_dtype).  The stacked mask logits of the D decoder outputs, (D, B, Q, H, W), hand their
 * gradient to the batched backward of the prediction heads sample-major and in the GEMM's operand type: no permute + cast
 * pass over the 262 MB gradient (mask2former_head.py:406-424 → :459). */
int mbv_point_sample_bwd_stack(const float* grad_out, const int32_t* src_index, const float* coords,
                               const int32_t* coord_index, int32_t num_rows, int32_t num_points, int32_t H, int32_t W,
                               int32_t outer, int32_t inner, int32_t rows, void* grad_src, int32_t out_dtype, void* stream);

/* Binary ({0, 1}-valued) maps packed 32 pixels per word, and K8's forward on the packed form: a whole
 * 512 x 512 ground-truth mask is 32 KB and is staged in LDS by the workgroup that samples it.
 * The batch contract of the reference makes GT masks float32 {0, 1}
 * (mask_bev/datasets/semantic_kitti/semantic_kitti_transforms.py:77-81,95-106); bit = (value != 0).
 * packed: (num_maps, mbv_packed_mask_words(H, W)) u32.  H*W <= 1024*1024. */
int64_t mbv_packed_mask_words(int32_t H, int32_t W);

int mbv_pack_binary_masks(const float* src, int64_t num_maps, int32_t H, int32_t W, uint32_t* packed, void* stream);

int mbv_point_sample_packed_fwd(const uint32_t* packed, const int32_t* src_index, const float* coords,
                                const int32_t* coord_index, int32_t num_rows, int32_t num_points,
                                int32_t H, int32_t W, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K10 — importance sampling of the mask loss: the k points with the smallest |logit| of each row.
 * Replaces: torch.topk(-|logits|, k) + coordinate gather of mmdet's get_uncertain_point_coords_with_randomness,
 * called at mask_bev/models/networks/mask2former_head/mask2former_head.py:401-404.
 * logits (rows, n) f32; coords (rows, n, 2) f32; out_coords (rows, k, 2) f32: the coordinates of the selected
 * points in ascending index order (same SET as top-k; ties at the threshold resolved towards lower indices).
 */
int mbv_select_uncertain_points(const float* logits, const float* coords, int64_t rows, int32_t n, int32_t k,
                                float* out_coords, void* stream);

/* Fused K8 + K10: sample the n candidate points of each row from its source map and keep the k most uncertain,
 * without materialising the (rows, n) sampled logits (the whole of get_uncertain_point_coords_with_randomness,
 * mask2former_head.py:401-404).  src (N, H, W) f32 with H*W <= 16384; src_index (rows) i32 → source map of a row;
 * n <= 40960 candidates per row, k <= 16384 of them kept, given EITHER as coords (rows, n, 2) f32 in [0, 1] (seed NULL) OR generated in the
 * kernel from the device-resident 64-bit *seed (coords NULL): point p of row r is mbv_uniform_points' value, so
 * the 1.2 GB candidate tensor of a training step is never written or read.  rand_coords (rows, n_rand, 2) f32
 * (nullable when n_rand == 0): the uniform tail, copied behind the selected points; out_coords
 * (rows, k + n_rand, 2).  Same selection, order and tie rule as mbv_point_sample_fwd followed by
 * mbv_select_uncertain_points.  MBV_ERR_UNSUPPORTED outside those limits (callers use the two-kernel form). */
int mbv_sample_select_uncertain(const float* src, const int32_t* src_index, const float* coords, const int64_t* seed,
                                int64_t rows, int32_t n, int32_t k, int32_t H, int32_t W, const float* rand_coords,
                                int32_t n_rand, float* out_coords, void* stream);

/* The generator behind the seed form above, written out: out_coords (rows, n, 2) f32 uniform in [0, 1), a pure
 * function of (*seed, row, point) — replaces torch.rand of mmdet's get_uncertain_point_coords_with_randomness. */
int mbv_uniform_points(const int64_t* seed, int64_t rows, int32_t n, float* out_coords, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K11 — parameter-arena kernels of the optimisation step.
 * Replaces: torch.optim.AdamW / Adam built by MaskBevModule.configure_optimizers
 * (mask_bev/mask_bev_module.py:131-166; update order of torch/optim/adamw.py `_single_tensor_adamw`) and the
 * bias-gradient reductions of every nn.Linear on the path.
 * mbv_adamw_step: ONE pass over a flat f32 arena of n parameters: param, grad, exp_avg, exp_avg_sq (all 16-byte
 *   aligned, n elements).  step >= 1 is the 1-based update count (bias corrections are computed on the host in
 *   f64).  decoupled=1 → AdamW (param *= 1 - lr*wd), 0 → Adam (grad += wd*param).  grad is multiplied by
 *   grad_scale first (1/world_size after a SUM all-reduce).  shadow_bf16 (nullable, 8-byte aligned) receives the
 *   updated parameters rounded to nearest-even bf16 or half (shadow_dtype = MBV_DT_BF16 / MBV_DT_F16) — the copy the
 *   16-bit GEMMs read.  zero_grad=1 clears grad in the same pass.
 *   fp16 loss scaling, without a host round trip: loss_scale (device f32 scalar, nullable) is the factor the loss was
 *   multiplied by — grad is divided by it on the fly; skip_flag (device i32, nullable) non-zero = the gradient held
 *   inf / nan: parameters, moments and shadow are left as they are and only zero_grad is honoured.  applied_steps
 *   (device i32, nullable): the count of updates applied so far — the bias corrections then use t = *applied_steps + 1
 *   instead of `step` (torch.amp.GradScaler skips optimizer.step() on an overflow: Adam's count must not advance).
 * mbv_grad_nonfinite: *flag |= 1 if any of grad[0..n) is inf or nan (torch.amp.GradScaler's found_inf).
 * mbv_loss_scale_update: GradScaler.update() on the device — flag set: scale = max(scale * backoff, 1), streak = 0;
 *   else streak += 1 and scale *= growth every growth_interval clean steps (and ++*applied_steps, nullable); clears
 *   the flag.
 * mbv_refresh_shadow: shadow[i] = bf16 / half (param[i]) (after load_state_dict / broadcast).
 * mbv_colsum_accum: out[c] += sum_r g[r, c] for row-major g (rows, n), bf16 (is_bf16=1) or f32; f32 atomics.
 */
int mbv_adamw_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int32_t shadow_dtype,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                   float grad_scale, int32_t decoupled, int32_t zero_grad, const float* loss_scale,
                   const int32_t* skip_flag, const int32_t* applied_steps, void* stream);

/* mbv_adamw_step over `count` element ranges [start[i], start[i] + len[i]) of arenas of n elements, one launch per 64 ranges
 * (start / len: HOST arrays, multiples of 4, inside the arena): the short ranges a step leaves between weights whose update
 * another kernel performed (K3's backward, mbv_gemm16_tn_group_adam).  Arithmetic and loss-scaling protocol of mbv_adamw_step. */
int mbv_adamw_step_ranges(float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                          int32_t shadow_dtype, int64_t n, const int64_t* start, const int64_t* len, int32_t count, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                          int32_t decoupled, int32_t zero_grad, const float* loss_scale, const int32_t* skip_flag,
                          const int32_t* applied_steps, void* stream);

int mbv_grad_nonfinite(const float* grad, int64_t n, int32_t* flag, void* stream);

int mbv_loss_scale_update(float* loss_scale, int32_t* clean_steps, int32_t* flag, float growth, float backoff,
                          int32_t growth_interval, int32_t* applied_steps, void* stream);

int mbv_refresh_shadow(const float* param, void* shadow_bf16, int32_t shadow_dtype, int64_t n, void* stream);

int mbv_colsum_accum(const void* g, int32_t is_bf16, int64_t rows, int32_t n, float* out, void* stream);
/* count independent column sums out[i] (n[i]) += sum_r g[i][r, 0:n[i]] with row stride ld[i] (elements) and storage
 * dtype[i] (MBV_DT_*), one launch per 64.  All array arguments are HOST arrays of length count.  Bias gradients and
 * LayerNorm-parameter partials are nobody's input: a caller may collect them during the backward and issue them
 * together at its end. */
int mbv_colsum_accum_group(const void* const* g, const int32_t* dtype, const int64_t* rows, const int32_t* n,
                           const int64_t* ld, float* const* out, int32_t count, void* stream);

/* Exact-f32 weight gradient of a few-row Linear (the decoder's B*Q tokens): acc (O, I) += g (T, O)^T x (T, I) with
 * v_mfma_f32_32x32x2_f32 from global memory, f32 atomics into the (arena) gradient; bias_acc (O) nullable += column
 * sums of g.  mbv_wgrad_small_f32_group: n such products in one launch per 48 — every array argument is a HOST array
 * of length n (device pointers / sizes per product; bias_acc may be NULL or hold NULL entries).  These gradients are
 * nobody's input, so a caller may collect them during the backward and issue them together at its end. */
int mbv_wgrad_small_f32_group(const float* const* g, const float* const* x, float* const* acc, float* const* bias_acc,
                              const int32_t* T, const int32_t* O, const int32_t* I, int32_t n, void* stream);

/* Activation backward fused with the bias gradient of the Linear in front of it (the fc1 layers of mmcv FFN,
 * mask_bev/models/networks/swin/swin.py:347-355, mask_bev_panoptic_head.py:137-142): grad_pre = grad_act * act'(pre_act)
 * with act = ReLU (kind 0) or erf-GELU (kind 1), all (rows, n) f32 or bf16, n % 4 == 0;
 * bias_acc (n) f32 (nullable) += column sums of grad_pre. */
int mbv_act_bwd_colsum(const void* grad_act, const void* pre_act, int32_t is_bf16, int32_t kind, int64_t rows, int32_t n,
                       void* grad_pre, float* bias_acc, void* stream);

/* Weight (and bias) gradient of a Linear applied to few tokens (the decoder's B*Q query rows), exact f32:
 * acc (O, I) += g^T x with g (T, O), x (T, I) row-major f32; bias_acc (O) += column sums of g when not NULL;
 * f32 MFMA, f32 atomics into acc / bias_acc. */
int mbv_wgrad_small_f32(const float* g, const float* x, int32_t T, int32_t O, int32_t I, float* acc, float* bias_acc,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * K13 — row sums of the point-sampled mask losses and their gradient.
 * Replaces: the elementwise chains of mmdet DiceLoss(naive_dice=True, eps=1) and CrossEntropyLoss(use_sigmoid=True)
 * on the sampled points (mask_bev/models/networks/mask2former_head/mask2former_head.py:406-424).
 * logits, targets (rows, points) f32.  out_sums (rows, 4) f32 = [sum sigmoid(x)*t, sum sigmoid(x), sum t,
 * sum bce_with_logits(x, t)].  bwd: grad_sums (rows, 4) → grad_logits (rows, points); the gradient of sum t
 * (column 2) is ignored (targets carry no gradient).
 */
int mbv_mask_loss_rows_fwd(const float* logits, const float* targets, int64_t rows, int32_t points, float* out_sums,
                           void* stream);

int mbv_mask_loss_rows_bwd(const float* logits, const float* targets, const float* grad_sums, int64_t rows,
                           int32_t points, float* grad_logits, void* stream);

/* The dice / BCE algebra on K13's row sums, per decoder output — mmdet DiceLoss(naive_dice, eps 1) and
 * CrossEntropyLoss(use_sigmoid) reduced with their avg_factor as at mask2former_head.py:406-424, for `outputs` decoder outputs of
 * rows / outputs rows each:  den = S1 + S2 + 1, dice = (2 S0 + 1) / den;
 *   loss_dice[d] = c_dice * sum_rows(1 - dice),  loss_mask[d] = c_mask * sum_rows(S3)
 * (c_dice = loss weight / avg_factor, c_mask likewise).  coef (rows, 3) f32 receives the gradient of the two losses with respect
 * to each row's sums for unit upstream gradients: (-2 c_dice / den, c_dice dice / den, c_mask).  sums 16-byte aligned. */
int mbv_dice_bce_reduce(const float* sums, int64_t rows, int32_t outputs, float c_dice, float c_mask, float* loss_dice,
                        float* loss_mask, float* coef, void* stream);

/* mbv_mask_loss_rows_bwd with the per-row gradient of the sums assembled in the kernel from mbv_dice_bce_reduce's `coef` and
 * the upstream gradients of the row's decoder output: grad_dice / grad_mask (outputs,) f32 with element strides
 * stride_dice / stride_mask (0 = one broadcast value; NULL = zero gradient). */
int mbv_mask_loss_rows_bwd_coef(const float* logits, const float* targets, const float* coef, const float* grad_dice,
                                int32_t stride_dice, const float* grad_mask, int32_t stride_mask, int64_t rows,
                                int32_t outputs, int32_t points, float* grad_logits, void* stream);

/* Matching-cost terms (mmdet CrossEntropyLossCost(use_sigmoid) + DiceCost on the sampled points,
 * mask2former_head.py:199-205): logits (groups, queries, points) f32 → terms (groups, 3, queries, points) f32 =
 * [softplus(-x), softplus(x), sigmoid(x)] — one batched GEMM against the sampled ground truth then gives all three
 * cost matrices — and row_sums (groups*queries, 2) = [sum softplus(x), sum sigmoid(x)].  ones_row != 0: a group has
 * 3 * queries + 1 rows, the last one all ones, so that the same GEMM also returns the targets' row sums. */
int mbv_match_cost_terms(const float* logits, int64_t groups, int32_t queries, int32_t points, int32_t ones_row,
                         float* terms, float* row_sums, void* stream);

/* The matching cost matrices from those products (HungarianAssigner's ClassificationCost 2.0 + CrossEntropyLossCost 5.0 +
 * DiceCost 5.0 as configured at mask_bev/models/head/mask_bev_panoptic_head.py and evaluated at mask2former_head.py:199-210):
 * cls (groups, queries, classes_plus_one) f32 logits, labels (batch, targets) i64, prod (groups, 3 * queries + 1, targets)
 * f32 = terms . sampled targets (ones row last), row_sums as above; group = (decoder output, image), image fastest.
 * cost (groups, queries, targets) f32. */
int mbv_match_cost(const float* cls, const int64_t* labels, const float* prod, const float* row_sums, int64_t groups,
                   int32_t queries, int32_t targets, int32_t classes_plus_one, int32_t batch, int32_t points, float* cost,
                   void* stream);

/* The same costs without the term planes and without a library GEMM (K13c, csrc/match_products.hip): the products
 * x . t and sigmoid(x) . t and the row sums come from ONE kernel that evaluates the terms per 32-point chunk, splits them
 * into IEEE-half pairs (22 significant bits) and contracts them on v_mfma_f32_32x32x16_f16 with f32 accumulation.
 * logits (groups, queries, points) f32 = the sampled mask logits, targets (groups, targets_n, points) f32 = the sampled
 * ground truth (any values in [0, 1]); both 16-byte aligned.  A group's points are cut into `splits` slices (one workgroup
 * each: choose groups * splits ~ 2 workgroups per CU; 1 <= splits <= ceil(points / 32)); slice s of group n writes
 *   prod[n][s] (2 * queries + 1, targets_n + 1) f32 = [x ; sigmoid(x) ; ones] . [t ; ones]^T   and
 *   neg_sums[n][s] (queries) f32 = sum softplus(x),
 * which mbv_match_cost_split adds in slice order (no atomics: bit-reproducible) into cost (groups, queries, targets) f32 =
 * -2 softmax(cls)[label] + 5 (sum softplus(x) - x . t) / points + 5 (1 - (2 sigmoid(x) . t + 1) / (sum sigmoid(x) + sum t + 1)).
 * Supported (mbv_match_products_supported != 0): 2 * queries + 1 <= 224, targets_n + 1 <= 128, points % 8 == 0; otherwise
 * MBV_ERR_UNSUPPORTED and the caller keeps mbv_match_cost_terms + a GEMM + mbv_match_cost. */
int mbv_match_products_supported(int32_t queries, int32_t targets_n, int32_t points);
int mbv_match_products(const float* logits, const float* targets, int64_t groups, int32_t queries, int32_t targets_n,
                       int32_t points, int32_t splits, float* prod, float* neg_sums, void* stream);
int mbv_match_cost_split(const float* cls, const int64_t* labels, const float* prod, const float* neg_sums, int64_t groups,
                         int32_t queries, int32_t targets, int32_t classes_plus_one, int32_t batch, int32_t points,
                         int32_t splits, float* cost, void* stream);

/* Classification loss of all decoder outputs (mmdet CrossEntropyLoss(class_weight), avg_factor = sum of the targets' class
 * weights: mask2former_head.py:393-404): cls (outputs, batch * queries, classes_plus_one) f32, assigned (outputs, batch,
 * queries) i32 = ground-truth column or -1 (→ label classes_plus_one - 1, "no object"), labels (batch, targets) i64.
 * loss (outputs) f32, weight_sum (outputs) f32 (kept for the backward); grad_cls has the shape of cls. */
int mbv_cls_loss_fwd(const float* cls, const int32_t* assigned, const int64_t* labels, const float* class_weight,
                     int32_t outputs, int32_t batch, int32_t queries, int32_t targets, int32_t classes_plus_one,
                     float loss_weight, float eps, float* loss, float* weight_sum, void* stream);
int mbv_cls_loss_bwd(const float* cls, const int32_t* assigned, const int64_t* labels, const float* class_weight,
                     const float* weight_sum, const float* grad_loss, int32_t outputs, int32_t batch, int32_t queries,
                     int32_t targets, int32_t classes_plus_one, float loss_weight, float eps, float* grad_cls, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K12 — fused residual-add + LayerNorm over the last (channel) axis of token-major activations.
 * Replaces: the `x + f(x)` → nn.LayerNorm(C) pairs of SwinBlock.forward (mask_bev/models/networks/swin/swin.py:
 * 357-377), of the pixel-decoder and masked-attention decoder layers (mmdet, configured at
 * mask_bev/models/head/mask_bev_panoptic_head.py:119-176) and the decoder's post_norm
 * (mask2former_head.py:448), forward and backward.
 * a, b: (rows, C) f32 or bf16 (`*_bf16` flags; b nullable = plain LayerNorm); gamma, beta (C) f32; C % 4 == 0,
 * C <= 2048 (mbv_add_layernorm_supported; the patch-merging form below takes 4 c <= 3072).  fwd writes sum_out = a + b (f32, the tensor the backward needs; may be
 * NULL only for a lone f32 `a`, which then serves as the saved input), y in f32 or bf16, mean / rstd (rows) f32.
 * bwd: dy (rows, C) f32/bf16, ds nullable (gradient reaching the sum from the residual path), s = the saved sum;
 * writes dx (rows, C) f32 (the gradient of a and of b), optionally the same in 16 bits (dx_lo, of dx_lo_dtype), and
 * dgamma / dbeta (C) f32 — overwritten, or accumulated into when accumulate != 0 (parameter-arena gradients).
 * dbranch_bias (C) f32, nullable: += the column sums of dx — the bias gradient of the Linear that produced the
 * residual branch b (its output gradient IS dx), saving that layer a pass over dx.
 * partial_ws: mbv_add_layernorm_bwd_blocks(rows, C) * 3 * C floats.
 */
int mbv_add_layernorm_supported(int32_t C);
int64_t mbv_add_layernorm_bwd_blocks(int64_t rows, int32_t C);
int mbv_add_layernorm_fwd(const void* a, int32_t a_bf16, const void* b, int32_t b_bf16, const float* gamma,
                          const float* beta, int64_t rows, int32_t C, float eps, float* sum_out, void* y, int32_t y_bf16,
                          float* mean, float* rstd, void* stream);
/* Same forward with a second copy of y in another storage type (y2 nullable): a post-LN layer's output has two consumers
 * — the next residual add takes it in f32, the branch GEMM that follows in 16 bits — and the cast launch between them goes.
 * The two copies hold the same f32 value rounded to their types; their gradients return through dy / dy2 of the backward.
 * b_rows > 0 (a divisor of rows): b has only b_rows rows and repeats — a per-sample map added to every sample of the batch
 * (the gradient of such a b is the batch sum of dx: the caller's to take).  0 or rows: b has `rows` rows. */
int mbv_add_layernorm_fwd2(const void* a, int32_t a_bf16, const void* b, int32_t b_bf16, int64_t b_rows, const float* gamma,
                           const float* beta, int64_t rows, int32_t C, float eps, float* sum_out, void* y, int32_t y_bf16,
                           void* y2, int32_t y2_dtype, float* mean, float* rstd, void* stream);

/* acc (C, R) f32 += the batch sum of g (batch, R, C) f32, transposed: the gradient of a per-sample token map that was added to
 * every sample, accumulated into the (1, C, H, W) parameter it is a transposed view of — the backbone's absolute position
 * embedding (mask_bev/models/networks/swin/swin.py:579-586, added at :750-760); one pass instead of a batch reduction and a
 * transposed accumulate. */
int mbv_transposed_batch_sum_accum(const float* g, int32_t batch, int64_t R, int32_t C, float* acc, void* stream);
int mbv_add_layernorm_bwd(const void* dy, int32_t dy_bf16, const void* ds, int32_t ds_bf16, const float* s,
                          const float* mean, const float* rstd, const float* gamma, int64_t rows, int32_t C, float* dx,
                          void* dx_lo, int32_t dx_lo_dtype, float* dgamma, float* dbeta, int32_t accumulate,
                          float* dbranch_bias, float* partial_ws, int32_t defer_reduce, void* stream);
/* mbv_add_layernorm_bwd with a second gradient of y (dy2, nullable, dy2_dtype = MBV_DT_*) that is added to dy on load:
 * the output of a post-LN layer feeds both the next residual add and the next branch (mask_bev_panoptic_head.py:119-176),
 * and its two gradients arrive separately instead of through an element-wise add launch. */
int mbv_add_layernorm_bwd2(const void* dy, int32_t dy_bf16, const void* dy2, int32_t dy2_dtype, const void* ds,
                           int32_t ds_bf16, const float* s, const float* mean, const float* rstd, const float* gamma,
                           int64_t rows, int32_t C, float* dx, void* dx_lo, int32_t dx_lo_dtype, float* dgamma,
                           float* dbeta, int32_t accumulate, float* dbranch_bias, float* partial_ws, int32_t defer_reduce,
                           void* stream);
/* mbv_add_layernorm_bwd2 with amax_dx: an optional absmax record (64 zeroed words, mbv_f32_absmax_group's format) that receives the
 * bits of max|dx| — one max-combine per block — so that the K20 products of the Linear backward that takes dx as its output
 * gradient need no pass over it (fp32 compute). */
int mbv_add_layernorm_bwd3(const void* dy, int32_t dy_bf16, const void* dy2, int32_t dy2_dtype, const void* ds,
                           int32_t ds_bf16, const float* s, const float* mean, const float* rstd, const float* gamma,
                           int64_t rows, int32_t C, float* dx, void* dx_lo, int32_t dx_lo_dtype, float* dgamma, float* dbeta,
                           int32_t accumulate, float* dbranch_bias, float* partial_ws, int32_t defer_reduce, uint32_t* amax_dx,
                           void* stream);
/* 1 = the backward of (rows, C) adds the parameter gradients from inside its one kernel; 0 = it writes per-block
 * partial rows (nblk = mbv_add_layernorm_bwd_blocks, layout [nblk][np][C], np = 3 with dbranch_bias else 2) and reduces
 * them with a second launch — unless defer_reduce != 0 (accumulating callers only), in which case the caller adds
 * the partials' column sums itself, typically for many layers at once with mbv_colsum_accum_group. */
int mbv_add_layernorm_bwd_direct(int64_t rows, int32_t C);

/* Patch merging without the unfolded copy: y (batch, h/2, w/2, 4c) = LayerNorm_{4c}(unfold_{2x2, stride 2}(x)) for a
 * channels-last f32 token map x (batch, h, w, c), h and w even, channel order c*4 + kh*2 + kw — the nn.Unfold order of
 * mmdet's PatchMerging as built at mask_bev/models/networks/swin/swin.py:611-616 (its `sampler` + `norm`; the `reduction`
 * Linear follows as a GEMM on y).  Element 4v + k of row (b, oh, ow) is channel v of pixel (2oh + k/2, 2ow + k%2): K12's
 * kernels gather / scatter with that addressing, so the (batch, h/2, w/2, 4c) copy, whose elements land 4 bytes at a
 * time, is never written and the backward's dx arrives in x's layout (every pixel belongs to exactly one row).
 * y: MBV_DT_F32 / BF16 / F16 (y_dtype); mean / rstd (batch*h/2*w/2) f32 are saved for the backward; dgamma / dbeta (4c),
 * accumulate, partial_ws (mbv_add_layernorm_bwd_blocks(rows, 4c) * 2 * 4c floats) and defer_reduce as in
 * mbv_add_layernorm_bwd. */
int mbv_merge_layernorm_supported(int32_t h, int32_t w, int32_t c);
int mbv_merge_layernorm_fwd(const float* x, int64_t batch, int32_t h, int32_t w, int32_t c, const float* gamma,
                            const float* beta, float eps, void* y, int32_t y_dtype, float* mean, float* rstd,
                            void* stream);
int mbv_merge_layernorm_bwd(const void* dy, int32_t dy_dtype, const float* x, const float* mean, const float* rstd,
                            const float* gamma, int64_t batch, int32_t h, int32_t w, int32_t c, float* dx, float* dgamma,
                            float* dbeta, int32_t accumulate, float* partial_ws, int32_t defer_reduce, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K14 — batch producer: instance-id map → instance ids → per-instance binary masks.
 * Replaces: FilterSmallMasks + MaskToLabelInstanceMasks of the reference's data pipeline
 * (mask_bev/datasets/semantic_kitti/semantic_kitti_transforms.py:11-26, 66-81) and the host→device copy of the
 * dense (B, Q, ny, nx) f32 masks they produce.
 * instance_map (B, nx, ny) i32, 0 = background (the layout of the reference's mask cache; the transform's `.T` is
 * applied here).  mbv_instance_ids: ids (B, Q) i32 = the ids with >= min_pixels pixels in ascending order, -1
 * padded (the reference enumerates a Python set: same set, unspecified order — the Hungarian matcher makes the
 * loss independent of it); counts (B) i32; *status (device i32) bit 0 = a scan had more than Q instances (the
 * reference raises IndexError; here the Q smallest ids are kept), bit 1 = more than 4096 distinct ids.
 * mbv_expand_instance_masks: masks_f32 (B, Q, ny, nx) f32 {0,1} and / or masks_packed (B*Q, words) u32 in the
 * bit-packed layout of mbv_pack_binary_masks (either may be NULL): masks[b, q, y, x] = (map[b, x, y] == ids[b, q]).
 */
int mbv_instance_ids(const int32_t* instance_map, int32_t batch, int32_t nx, int32_t ny, int32_t num_queries,
                     int32_t min_pixels, int32_t* ids, int32_t* counts, int32_t* status, void* stream);

int mbv_expand_instance_masks(const int32_t* instance_map, const int32_t* ids, int32_t batch, int32_t nx, int32_t ny,
                              int32_t num_queries, float* masks_f32, uint32_t* masks_packed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K15 — mask IoU of matched (prediction, ground truth) pairs at ground-truth resolution.
 * Replaces: the upsample → sigmoid > 0.5 → batched_mask_iou chain of MaskBevPanopticHead.update_mAP_metrics
 * (mask_bev/models/head/mask_bev_panoptic_head.py:74-85; mask_bev/evaluation/average_precision.py:78-81).
 * logits (N, h, w) f32 with h*w <= 16384; pred_row / gt_row (pairs) i32: rows of `logits` and of the bit-packed
 * ground truth (mbv_pack_binary_masks layout, maps of H x W pixels); gt_row < 0 marks an unmatched prediction.
 * inter / uni (pairs) i32 pixel counts; IoU = inter / (uni + 1e-12) like the reference.
 */
int mbv_matched_mask_iou(const float* logits, const int32_t* pred_row, const uint32_t* gt_packed,
                         const int32_t* gt_row, int32_t num_pairs, int32_t h, int32_t w, int32_t H, int32_t W,
                         int32_t* inter, int32_t* uni, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K9 — batched linear-sum assignment on the device (one wavefront per cost matrix).
 * Replaces: mmdet HungarianAssigner → scipy.optimize.linear_sum_assignment on the host, reached from
 * Mask2FormerHead._get_targets_single (mask_bev/models/networks/mask2former_head/mask2former_head.py:207-210).
 * cost (batch, num_rows, num_cols) f32 (finite); row_to_col (batch, num_rows) i32 = assigned column of each
 * row, -1 for rows left unassigned when num_rows > num_cols.  Up to 128 x 128 the cost matrix lives in LDS (the
 * 100-query configurations); up to 320 x 320 (200 / 300 queries) it is read from global memory one coalesced row
 * per search step, which needs num_rows <= num_cols: for num_rows > num_cols > 128 call mbv_hungarian_wide_t with
 * the materialised transpose cost_t (batch, num_cols, num_rows) — same row_to_col (batch, num_rows) output.
 */
int mbv_hungarian(const float* cost, int32_t batch, int32_t num_rows, int32_t num_cols,
                  int32_t* row_to_col, void* stream);

/* The same for matrices (rows = predictions) x (cols = ground-truth slots, rows <= cols <= 320; above 128 columns the
 * wide kernel with the real columns' block staged in LDS) whose trailing columns
 * are identical padding — the dataset pads the instance list to num_queries with all-zero masks of label 0
 * (semantic_kitti_transforms.py:66-81), so for a given prediction those columns hold one and the same cost.
 * real_cols (batch) i32 ON THE DEVICE: the number of leading real columns of each problem.  Solves the equivalent
 * rectangular problem of the real columns (the padded columns' cost enters as the start value of the predictions'
 * duals) — the same optimum, the same real pairs whenever it is unique, at about (real / rows)^2 of the search steps;
 * the predictions left over take the padded columns in ascending order.  Problems without padding (real_cols ==
 * cols) and non-square problems (a real column may then stay unmatched) are solved like mbv_hungarian. */
int mbv_hungarian_padded(const float* cost, int32_t batch, int32_t num_rows, int32_t num_cols, const int32_t* real_cols,
                         int32_t* row_to_col, void* stream);
int mbv_hungarian_wide_t(const float* cost_t, int32_t batch, int32_t num_rows, int32_t num_cols,
                         int32_t* row_to_col, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K7 — per-query mask logits on MFMA, and the boolean cross-attention mask of the next decoder layer.
 * Replaces: torch.einsum('bqc,bchw->bqhw', mask_embed, mask_feature)
 * (mask_bev/models/networks/mask2former_head/mask2former_head.py:459) and :460-470 + :538-539
 * (F.interpolate bilinear → sigmoid() < 0.5 → repeat over heads; a row that would block every key is unblocked).
 * mask_embed (B, Q, C), mask_feature (B, C, pixels), logits (B, Q, pixels): all f32 (is_bf16 = 0, exact-f32 MFMA,
 * C even) or all bf16 (is_bf16 = 1, C % 16 == 0); with bf16 inputs, logits_f32 != 0 stores the f32 accumulators
 * as f32 logits (the loss consumes f32; saves the cast pass).
 * mbv_attn_mask_from_logits: logits (rows, H, W) → blocked (rows, h*w) u8 (1 = may not attend), kept once per
 * query (the reference materialises it 8x, once per head).
 */
int mbv_mask_logits_fwd(const void* mask_embed, const void* mask_feature, int32_t is_bf16, int32_t batch,
                        int32_t num_queries, int32_t channels, int64_t pixels, void* logits, int32_t logits_f32,
                        void* stream);

int mbv_attn_mask_from_logits(const void* logits, int32_t is_bf16, int64_t rows, int32_t H, int32_t W,
                              int32_t h, int32_t w, uint8_t* blocked, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K6 — multi-head (masked) attention of the transformer decoder, forward / backward on MFMA.
 * Replaces: the nn.MultiheadAttention cores (via mmcv MultiheadAttention) of the decoder loop at
 * mask_bev/models/networks/mask2former_head/mask2former_head.py:542-553 (masked cross-attention over the
 * L = h*w memory tokens of one level, then query self-attention); heads/ffn configured at
 * mask_bev/models/head/mask_bev_panoptic_head.py:150-176.
 * q (B, Q, heads*D), k, v (B, L, heads*D): projected inputs, all f32 (is_bf16 = 0) or all bf16; the softmax
 * scale 1/sqrt(D) is applied inside.  blocked (B, Q, L) u8, 1 = may not attend, or NULL (self-attention);
 * every row must keep at least one attendable key (mbv_attn_mask_from_logits guarantees it).
 * out (B, Q, heads*D) same dtype; lse (B, heads, Q) f32 saved for backward.  head_dim in {16, 32, 64}.
 * Backward writes f32 gradients grad_q (B, Q, E), grad_k / grad_v (B, L, E) in full.
 */
size_t mbv_attn_workspace_bytes(int32_t batch, int32_t num_queries, int32_t num_keys, int32_t heads, int32_t head_dim);

int mbv_attn_fwd(const void* q, const void* k, const void* v, const uint8_t* blocked, int32_t is_bf16,
                 int32_t batch, int32_t num_queries, int32_t num_keys, int32_t heads, int32_t head_dim,
                 void* out, float* lse, void* workspace, size_t workspace_bytes, void* stream);

int mbv_attn_bwd(const void* q, const void* k, const void* v, const uint8_t* blocked, const void* out,
                 const void* grad_out, const float* lse, int32_t is_bf16,
                 int32_t batch, int32_t num_queries, int32_t num_keys, int32_t heads, int32_t head_dim,
                 float* grad_q, float* grad_k, float* grad_v, void* stream);

/* Same kernels with strided key / value operands: k and v point at columns of a wider row-major matrix whose rows are
 * `ld_kv` elements apart (the key / value projections of SEVERAL decoder layers that attend to the same memory are
 * then produced side by side by one GEMM — the three layers of a level in mask2former_head.py:535-560 — and the
 * gradient of that matrix is assembled in place: grad_k / grad_v rows are `ld_grad_kv` apart, optionally stored as
 * bf16, ready to be the operand of the batched data / weight-gradient GEMMs).  Strided or bf16 key / value gradients
 * need num_queries <= 128. */
int mbv_attn_fwd_ld(const void* q, const void* k, const void* v, int32_t ld_kv, const uint8_t* blocked,
                    int32_t is_bf16, int32_t batch, int32_t num_queries, int32_t num_keys, int32_t heads,
                    int32_t head_dim, void* out, float* lse, void* workspace, size_t workspace_bytes, void* stream);

int mbv_attn_bwd_ld(const void* q, const void* k, const void* v, int32_t ld_kv, const uint8_t* blocked,
                    const void* out, const void* grad_out, const float* lse, int32_t is_bf16, int32_t batch,
                    int32_t num_queries, int32_t num_keys, int32_t heads, int32_t head_dim, float* grad_q,
                    void* grad_k, void* grad_v, int32_t ld_grad_kv, int32_t grad_kv_bf16, void* stream);

/* K6 on f32 tensors in the SPLIT mode (fp32 compute; the arguments, results and reference lines of mbv_attn_fwd_ld / _bwd_ld with
 * is_bf16 = 0, f32 key / value gradients): every f32 operand element of a block's tiles is split into an IEEE-half pair while the
 * tile is staged and every product is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_f16 (K20's arithmetic, K4's split mode), with
 * one power-of-two scale PER TILE found in registers between the loads and the LDS stores.  head_dim 16 / 32 / 64, ld_kv % 4 == 0,
 * 16-byte aligned tensors (mbv_attn_split_supported; else MBV_ERR_UNSUPPORTED and the caller keeps the exact-f32 form). */
int mbv_attn_split_supported(int32_t heads, int32_t head_dim, int32_t ld_kv);
int mbv_attn_split_fwd_ld(const float* q, const float* k, const float* v, int32_t ld_kv, const uint8_t* blocked, int32_t batch,
                          int32_t num_queries, int32_t num_keys, int32_t heads, int32_t head_dim, float* out, float* lse,
                          void* workspace, size_t workspace_bytes, void* stream);
int mbv_attn_split_bwd_ld(const float* q, const float* k, const float* v, int32_t ld_kv, const uint8_t* blocked, const float* out,
                          const float* grad_out, const float* lse, int32_t batch, int32_t num_queries, int32_t num_keys,
                          int32_t heads, int32_t head_dim, float* grad_q, float* grad_k, float* grad_v, int32_t ld_grad_kv,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * K17 — 16-bit (bf16 / fp16) MFMA GEMMs of the token-major Linear layers, with the element-wise work around them
 * fused into the epilogue.  dtype: 0 = bf16, 1 = fp16 (inputs; accumulation is f32).
 * Replaces the cuBLAS/ATen GEMMs behind nn.Linear in WindowMSA.qkv / .proj (mask_bev/models/networks/swin/swin.py:
 * 89-116), the mmcv FFN of SwinBlock (swin.py:347-377: Linear -> GELU -> Linear), PatchEmbed / PatchMerging
 * (swin.py:579-586, 611), the Linears of the pixel decoder and the transformer decoder
 * (mask_bev/models/head/mask_bev_panoptic_head.py:119-175) and their autograd backward.
 * Every matrix is row-major with leading dimension ld* (elements, multiples of 8; pointers 16-byte aligned);
 * `batch` independent problems are `stride_*` elements apart.  Shapes the kernels do not take return
 * MBV_ERR_UNSUPPORTED (callers use the library GEMM for those).
 *
 *   mbv_gemm16_nt   out (m, n) = act(x (m, k) . w (n, k)^T + bias);  act: 0 none, 1 ReLU, 2 GELU (erf form);
 *                   out_pre (optional, act != 0) receives the pre-activation; out / out_pre are 16-bit or f32.
 *   mbv_gemm16_nn   out (m, k) = act'(aux) * (g (m, n) . w (n, k));  act: 0 none, 1 ReLU' with aux = the activation
 *                   output, 2 GELU' with aux = the pre-activation (aux (m, k) 16-bit, ld = ldaux, batch stride of
 *                   out); colsum (k) f32 (optional) += column sums of the stored out (the bias gradient of the
 *                   Linear in front of the activation; needs `workspace` of mbv_gemm16_nn_workspace_bytes).
 *   mbv_gemm16_tn   accumulate != 0: dw (n, k) f32 += g (m, n)^T . x (m, k), the sum over m split over `splits`
 *                   workgroups per tile (0 = choose).  With a `workspace` of mbv_gemm16_tn_workspace_bytes (dw
 *                   contiguous, batch 1) the parts are stored and added by their owner thread (no atomics, bit-
 *                   reproducible); without it they add with f32 atomics (dw is the parameter arena's gradient);
 *                   accumulate == 0: dw = g^T . x stored once (16-bit or f32).
 */
int mbv_gemm16_supported(int32_t layout, int64_t m, int64_t n, int64_t k);

int mbv_gemm16_nt(const void* x, const void* w, const float* bias, void* out, void* out_pre, int64_t m, int64_t n,
                  int64_t k, int64_t ldx, int64_t ldw, int64_t ldo, int32_t dtype, int32_t out_f32, int32_t act,
                  int32_t batch, int64_t stride_x, int64_t stride_w, int64_t stride_o, void* stream);

/* acc (m, n) f32 += x (m, k) . w (n, k)^T with the sum over k split over `splits` workgroups per tile (0 = choose)
 * that add with f32 atomics: few-row products with a long contraction — d(mask_embed) = d(logits) . mask_feature^T of
 * torch.einsum('bqc,bchw->bqhw') (mask_bev/models/networks/mask2former_head/mask2former_head.py:459), 1000 x 256
 * outputs over 16 384 pixels per sample. */
int mbv_gemm16_nt_acc(const void* x, const void* w, float* acc, int64_t m, int64_t n, int64_t k, int64_t ldx,
                      int64_t ldw, int64_t ldacc, int32_t dtype, int32_t splits, int32_t batch, int64_t stride_x,
                      int64_t stride_w, int64_t stride_acc, void* stream);

size_t mbv_gemm16_nn_workspace_bytes(int64_t m, int64_t k, int32_t batch);

int mbv_gemm16_nn(const void* g, const void* w, void* out, const void* aux, float* colsum, int64_t m, int64_t n,
                  int64_t k, int64_t ldg, int64_t ldw, int64_t ldo, int64_t ldaux, int32_t dtype, int32_t out_f32,
                  int32_t act, int32_t batch, int64_t stride_g, int64_t stride_w, int64_t stride_o, void* workspace,
                  size_t workspace_bytes, void* stream);

/* mbv_gemm16_nn with the bias gradient's reduction left to the caller: `parts` (mbv_gemm16_nn_part_rows(m, k, batch), k)
 * f32, contiguous, 16-byte aligned, parts_bytes >= mbv_gemm16_nn_workspace_bytes(m, k, batch), receives one partial
 * column-sum row per 64 output rows (every element written); the column sum is their sum over the rows.  A backward pass
 * hands the rows of all its fused data gradients to ONE mbv_colsum_accum_group launch at its end instead of a small
 * reduction launch behind every GEMM (same reference lines as mbv_gemm16_nn: the fc1 bias gradient of mmcv's FFN,
 * mask_bev/models/networks/swin/swin.py:347-355). */
int64_t mbv_gemm16_nn_part_rows(int64_t m, int64_t k, int32_t batch);

int mbv_gemm16_nn_parts(const void* g, const void* w, void* out, const void* aux, float* parts, size_t parts_bytes,
                        int64_t m, int64_t n, int64_t k, int64_t ldg, int64_t ldw, int64_t ldo, int64_t ldaux,
                        int32_t dtype, int32_t out_f32, int32_t act, int32_t batch, int64_t stride_g, int64_t stride_w,
                        int64_t stride_o, void* stream);

size_t mbv_gemm16_tn_workspace_bytes(int64_t m, int64_t n, int64_t k);

int mbv_gemm16_tn(const void* g, const void* x, void* dw, int64_t m, int64_t n, int64_t k, int64_t ldg, int64_t ldx,
                  int64_t lddw, int32_t dtype, int32_t accumulate, int32_t out_f32, int32_t splits, int32_t batch,
                  int64_t stride_g, int64_t stride_x, int64_t stride_dw, void* workspace, size_t workspace_bytes,
                  void* stream);

/* d(coarse map) of `F.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=False)` — the adjoint K18's fused
 * FPN step owes its added map (ATen upsample_bilinear2d_backward): grad_out (planes, h, w) → grad_in (planes, in_h, in_w), any
 * MBV_DT_* storage types; gather form, no atomics, every output written once. */
int mbv_upsample_bilinear_bwd(const void* grad_out, int32_t grad_dtype, int64_t planes, int32_t h, int32_t w, int32_t in_h,
                              int32_t in_w, void* grad_in, int32_t in_dtype, void* stream);

/* K18 — GroupNorm of NCHW maps fused with its surroundings in mmcv's ConvModule (conv -> GroupNorm(32) [-> ReLU]) as
 * the pixel decoder builds it (mask_bev/models/head/mask_bev_panoptic_head.py:119-123 -> mmdet MSDeformAttnPixelDecoder
 * input_convs / lateral_convs / output_convs) and the FPN step  lateral + F.interpolate(previous, bilinear,
 * align_corners=False)  between them.  x (batch, channels, h, w) in x_dtype (MBV_DT_*), h*w % 4 == 0, 16-byte aligned;
 *   y = GroupNorm(x; groups, gamma, beta, eps)  [+ up-sampled `add` (batch, channels, add_h, add_w), w % 4 == 0]  [ReLU]
 * stored in y_dtype; mean / rstd (batch * groups) f32 are saved for the backward; statistics in f64 (biased variance).
 * `add` together with relu is MBV_ERR_UNSUPPORTED: the backward gates on GroupNorm(x) alone, not on the sum.
 * Backward: dx in dx_dtype, dgamma / dbeta (channels) stored or (accumulate != 0) added to; the ReLU gate is recomputed
 * from x with the forward's arithmetic; the gradient of `add` is the up-sampling's backward of dy (left to the caller).
 * plane_sums: batch * channels * 2 floats of scratch. */
int mbv_groupnorm_supported(int32_t channels, int32_t groups, int32_t h, int32_t w);
size_t mbv_groupnorm_workspace_bytes(int64_t batch, int32_t channels, int32_t groups, int32_t h, int32_t w);
int mbv_groupnorm_fwd(const void* x, int32_t x_dtype, int64_t batch, int32_t channels, int32_t h, int32_t w,
                      int32_t groups, const float* gamma, const float* beta, float eps, const void* add,
                      int32_t add_dtype, int32_t add_h, int32_t add_w, int32_t relu, void* y, int32_t y_dtype, float* mean,
                      float* rstd, void* workspace, size_t workspace_bytes, void* stream);
int mbv_groupnorm_bwd(const void* dy, int32_t dy_dtype, const void* x, int32_t x_dtype, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, int64_t batch, int32_t channels, int32_t h,
                      int32_t w, int32_t groups, int32_t relu, void* dx, int32_t dx_dtype, float* dgamma, float* dbeta,
                      int32_t accumulate, float* plane_sums, void* stream);

/* The weight gradients of `count` Linears in one GEMM launch (+ one parts-add launch) per 48 of them:
 *   dw[i] (n[i], k[i]) f32, contiguous  +=  g[i] (m[i], n[i])^T . x[i] (m[i], k[i])          for i < count.
 * Replaces the per-layer weight-gradient GEMMs of autograd's Linear backward (the same layers as above): a weight
 * gradient is nobody's input, so the caller collects the (g, x, dw) triples of a backward pass and issues them together
 * at its end — a 192 x 192 ... 2304 x 768 output alone cannot fill 256 CUs without cutting the token sum into slivers,
 * the tiles of all layers together do.  Every array argument is a HOST array of length count; g / x are 16-bit
 * (`dtype`), ld* in elements (multiples of 8), pointers 16-byte aligned, m[i] == 0 entries are skipped.  Token sums
 * deeper than the work-item depth are cut into parts stored in `workspace` (mbv_gemm16_tn_group_workspace_bytes) and
 * added to dw by their owner thread: no atomics, bit-reproducible. */
size_t mbv_gemm16_tn_group_workspace_bytes(const int64_t* m, const int64_t* n, const int64_t* k, int32_t count);

int mbv_gemm16_tn_group(const void* const* g, const void* const* x, float* const* dw, const int64_t* m, const int64_t* n,
                        const int64_t* k, const int64_t* ldg, const int64_t* ldx, int32_t count, int32_t dtype,
                        void* workspace, size_t workspace_bytes, void* stream);

/* mbv_gemm16_tn_group with the AdamW update of a weight in the epilogue of its gradient's product.
 * mbv_adam_dev: the hyper-parameters of one parameter group in DEVICE memory (64 bytes, 4-byte aligned) — read when the
 *   launch RUNS, so a launch captured in a graph follows the learning-rate schedule and the step count.
 * mbv_adam_args_write: fills a block for update `step` (1-based; the bias corrections are computed on the host exactly as
 *   mbv_adamw_step computes them) with a one-thread launch on `stream`.  shadow_kind = MBV_DT_BF16 / MBV_DT_F16 (0: unused).
 * mbv_gemm16_tn_group_adam: as mbv_gemm16_tn_group; adam (HOST array of length count) holds for every entry a DEVICE
 *   mbv_adam_dev block or null.  An entry with a block whose token sum is ONE work item (m[i] <= 4096: its tile is the whole
 *   gradient) and whose dw[i] = grad + o lies inside the arena gradient [grad, grad + arena_numel) with o a multiple of 8
 *   does not touch dw[i]: its owner reads param / exp_avg / exp_avg_sq at o, applies mbv_adamw_step's arithmetic
 *   (grad_scale 1, no loss scaling) with the gradient from its accumulators and writes them back, with the 16-bit shadow
 *   (nullable).  All four arenas 16-byte aligned.  fused (HOST, out, length count) is 1 for the entries that did so; every
 *   other entry — no block, or a deeper token sum — accumulates into dw[i] as in mbv_gemm16_tn_group.  The CALLER keeps a
 *   fused destination out of the step's mbv_adamw_step and never hands one destination to two entries. */
typedef struct mbv_adam_dev {
  float lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2_sqrt;
  int32_t decoupled, shadow_kind;
  int32_t pad[7];
} mbv_adam_dev;

int mbv_adam_args_write(void* dev_block, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                        int32_t decoupled, int32_t shadow_kind, void* stream);

int mbv_gemm16_tn_group_adam(const void* const* g, const void* const* x, float* const* dw, const int64_t* m,
                             const int64_t* n, const int64_t* k, const int64_t* ldg, const int64_t* ldx, int32_t count,
                             int32_t dtype, void* workspace, size_t workspace_bytes, const void* const* adam, float* grad,
                             float* param, float* exp_avg, float* exp_avg_sq, void* shadow, int64_t arena_numel,
                             int32_t* fused, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K19— row-local stage chains of the transformer decoder's query side (csrc/rowchain.hip).
 * Replaces, per decoder layer, the few-row Linear / LayerNorm / ReLU / add launches between two attention calls of
 * mask_bev/models/networks/mask2former_head/mask2former_head.py:535-560 (mmdet Mask2FormerTransformerDecoderLayer:
 * cross-attn out-proj + LN, self-attn projections, out-proj + LN, FFN + LN) and the prediction-head MLPs of :428-472.
 * A workgroup owns 16 token rows and runs `num_stages` stages over them; activations stay in LDS slots
 * (mbv_rowchain_slots() slots of 16 x 256 f32) between stages.  Stage operations:
 *   MBV_RC_LOAD    dst <- rows of p0 (dtype = flags & 3, row stride ld) [+ f32 p1 at row (r % q_mod), stride ld2];
 *                  p0 == NULL: the base operand is slot `src` (then p1 is required).  Rows >= `rows` load as zeros.
 *   MBV_RC_STORE   rows of p0 <- src (dtype = flags & 3, stride ld); MBV_RC_ACCUM: p0 += src (f32; in a split launch only with an owner — BAD_ARG otherwise).
 *   MBV_RC_GEMM    dst = act((ACCUM ? dst : 0) + src (16 x k) . W^T + bias), W = p0 (n, k) row-major with row stride ld in
 *                  the program's weight dtype, bias = p1 f32 or NULL; MBV_RC_RELU; MBV_RC_MASK: result zeroed where
 *                  slot src2 <= 0 (ReLU backward).  f32 weights: exact f32 MFMA; 16-bit weights: activations rounded to
 *                  that type, f32 accumulation.  n <= 256, k <= 256, k % 16 (f32) / 32 (16-bit) == 0, dst != src.
 *                  MBV_RC_FRAG (16-bit): p0 is a fragment-major copy (mbv_fragment_group) positioned at the stage's first
 *                  (tile, block) and ld = its 32-column blocks per tile row (one load instruction = 8 full cache lines
 *                  instead of 16 half lines).  The FFN stage's weights are always fragment-major (ld / ld2 likewise).
 *   MBV_RC_LN      dst = LayerNorm(src [+ src2]) * p0 + p1 (src2 = -1: none); MBV_RC_SAVE_SUM: src <- the sum;
 *                  p2 (nullable): (rows, 2) f32 <- (mean, rstd).
 *   MBV_RC_LN_BWD  dst = d(sum) given src = d(output), src2 = the sum, p0 = gamma, p2 = stats; p1 (nullable):
 *                  (blocks, 2 n) f32 <- this block's partial d(gamma) | d(beta).
 *   MBV_RC_ADD     dst = src + src2.      MBV_RC_COLSUM  p0[block * ld + c] = sum over the block's rows of src.
 *   MBV_RC_FFN     (16-bit weights) the MLP pair with the hidden dimension cut into 256-wide chunks owned by the waves in
 *                  parallel: forward dst = relu(src . W1^T + b1) . W2^T with W1 = p0 (k x n, stride ld), b1 = p1, W2 = p2
 *                  (n x k, stride ld2); MBV_RC_MASK = backward: dst = ((src . p0^T) * (act > 0)) . p2^T with p0 = W2^T,
 *                  p2 = W1^T.  n = embed width (<= 256, % 32), k = hidden width (% 256); src2 = first of 5 scratch slots.
 *                  Directly followed by an MBV_RC_FFN_IO descriptor: p0 = hidden activations (rows x k f32, stride ld;
 *                  written forward, read backward), p1 = d(hidden) out (backward), p2 = (blocks, ld2) column partials of
 *                  d(hidden) (backward, nullable).  The output bias is left to the caller (e.g. a following LN's operand).
 *   MBV_RC_SUM     dst = sum over j < k of p0[j * ld2 + row * ld + c] (f32): the parts a split launch stored.
 * Split launches (mbv_rowchain_run_split, split = S > 1): S consecutive workgroups share a 16-row block, so that a
 * 400-row decoder layer occupies S x 25 CUs instead of 25.  A stage whose flags bits 8..15 hold v > 0 runs only in
 * workgroup v - 1 of its row block, every other stage in all S (redundantly: loads, the cheap products and norms).
 * MBV_RC_FFN | MBV_RC_SLICE (k == 256 S): workgroup j computes the hidden units [256 j, 256 j + 256) and leaves its
 * PARTIAL output in dst (workgroup 0 adds the output bias p1 of the descriptor; p2 is a K-MAJOR fragment copy and
 * n % 16 == 0); MBV_RC_STORE | MBV_RC_SPLIT writes to
 * p0 + j * ld2 elements.  A following launch adds the parts with MBV_RC_SUM — in part order, so the result does not
 * depend on timing.  Per-block partial outputs (MBV_RC_COLSUM, LN_BWD's p1, the descriptor's p2) are indexed by ROW
 * block in either form.
 * Data gradients dX = dY . W are MBV_RC_GEMM stages against transposed weight copies (mbv_transpose_group).
 * The program is copied into the kernel arguments (<= mbv_rowchain_max_stages() stages): nothing is retained. */
#define MBV_RC_LOAD 0
#define MBV_RC_STORE 1
#define MBV_RC_GEMM 2
#define MBV_RC_LN 3
#define MBV_RC_LN_BWD 4
#define MBV_RC_ADD 5
#define MBV_RC_COLSUM 6
#define MBV_RC_FFN 7
#define MBV_RC_FFN_IO 8
#define MBV_RC_SUM 9
#define MBV_RC_ACCUM 4
#define MBV_RC_RELU 8
#define MBV_RC_MASK 16
#define MBV_RC_SAVE_SUM 32
#define MBV_RC_SLICE 64  /* FFN stages */
#define MBV_RC_SPLIT 64  /* STORE stages */
#define MBV_RC_FRAG 128
#define MBV_RC_OWNER(j) (((j) + 1) << 8) /* stage of workgroup j of a split launch only */
#define MBV_TR_MAX 96
typedef struct MbvRowStage {
  int32_t op;
  int16_t dst, src, src2, reserved;
  int32_t n, k, flags, ld, ld2;
  const void* p0;
  const void* p1;
  const void* p2;
} MbvRowStage;
int mbv_rowchain_max_stages(void);
int mbv_rowchain_slots(void);
int mbv_rowchain_run(const MbvRowStage* stages, int32_t num_stages, int32_t rows, int32_t q_mod, float eps,
                     int32_t wdtype, void* stream);
int mbv_rowchain_run_split(const MbvRowStage* stages, int32_t num_stages, int32_t rows, int32_t q_mod, float eps,
                           int32_t wdtype, int32_t split, void* stream);
/* Fragment-major copies of 16-bit weight matrices for the 16 x 16 x 32 MFMA B operand: for the logical (rows, cols) matrix
 * W, dst[((t * (cols / 32) + kb) * 64 + lane) * 8 + j] = W[t * 16 + lane % 16][kb * 32 + 8 * (lane / 16) + j], rows padded
 * with zeros to a multiple of 16; transposed[i] & 1: W[r][c] = src[c * ld + r] (the data-gradient operand), else
 * src[r * ld + c].  transposed[i] & 2: k-major block order — block (t, kb) at (kb * ceil(rows / 16) + t) instead of
 * (t * (cols / 32) + kb) — the second weight of an MBV_RC_SLICE stage.  cols % 32 == 0.  dst holds
 * ceil(rows / 16) * 16 * cols elements. */
int mbv_fragment_group(const void* const* src, void* const* dst, const int32_t* rows, const int32_t* cols,
                       const int32_t* ld, const int32_t* transposed, int32_t n, void* stream);
/* dst[i] = src[i], bytes[i] bytes each: the pieces of several small concatenations (the k / v rows of three decoder layers'
 * packed in_proj parameters, mask2former_head.py:535-560 → nn.MultiheadAttention) in one launch. */
int mbv_copy_group(const void* const* src, void* const* dst, const int64_t* bytes, int32_t n, void* stream);
/* dst[i] (cols, rows) = transpose of src[i] (rows, cols), n matrices of elem_size 2 or 4 bytes, <= MBV_TR_MAX per launch. */
int mbv_transpose_group(const void* const* src, void* const* dst, const int32_t* rows, const int32_t* cols, int32_t n,
                        int32_t elem_size, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K20 — f32 GEMMs on the 16-bit matrix pipe (csrc/gemm_f32s.hip): every f32 operand element is split at staging time into
 * an IEEE-half pair  x 2^e = hi + lo  (22 significant bits) and the product is hi.hi + hi.lo + lo.hi with f32
 * accumulation (error <= 2^-22 sum|a||b| + K 2^-37 max|a| max|b|: the level of an f32 dot product; the dropped lo.lo
 * term is 2^-22 relative).  Replaces, in the reference-precision (fp32) step, the f32 library GEMMs behind nn.Linear
 * forward / backward of the token-major layers: Swin qkv / proj / FFN / patch merging
 * (/root/reference: mask_bev/models/networks/swin/swin.py:89-116, 347-355, 611-616) and the pixel decoder's Linears
 * (mask_bev/models/head/mask_bev_panoptic_head.py:119-146) — `precision=32` in train_mask_bev.py:96.
 * All matrices f32, row-major, ld* in elements (multiples of 4), pointers 16-byte aligned, n and k multiples of 8.
 * amax_*: absmax RECORDS — 64 consecutive device words (256 bytes) whose maximum is the BITS of max|operand| or of an upper
 * bound of it (mbv_f32_absmax_group, or a K20 product that max-combined its outputs into the record: amax_out here; 64 slots, and a
 * workgroup adds only when its maximum exceeds what its slot already holds: a few atomics per launch) —
 * from which the kernel derives the power of two that puts the operand's largest magnitude in [2^13, 2^14); a bound up
 * to 2^4 too large costs nothing (the full-accuracy window is 18 binades deep); NULL = unscaled (operands whose magnitudes lie
 * within [2^-3, 2^15] then keep full accuracy, smaller elements lose one bit per binade).  `act`: 0 none, 1 ReLU,
 * 2 GELU (erf form); out_pre (optional) receives the pre-activation.  Batched: `batch` products with element strides. */
int mbv_gemm32s_supported(int32_t layout, int64_t m, int64_t n, int64_t k);

/* max|x| of `count` f32 tensors (rows[i], cols[i]) with row stride ld[i] (cols % 4 == 0), as the BITS of the maximum,
 * max-combined into the 64-word record at out[i] (slot = workgroup mod 64): the record must hold zeros (or earlier partial
 * maxima of the same tensor) when the launch starts.  Every array argument is a HOST array of length count; one launch per 64 tensors. */
int mbv_f32_absmax_group(const float* const* x, const int64_t* rows, const int64_t* cols, const int64_t* ld,
                         uint32_t* const* out, int32_t count, void* stream);

/* Absmax BOUNDS of LayerNorm outputs without a pass over them: y = xhat gamma + beta with |xhat| <= sqrt(C - 1), so word 0 of
 * records[i] (64 words, cleared by the caller once) receives the bits of sqrt(c[i]) max|gamma[i]| + max|beta[i]| (beta[i] may be
 * NULL) — ~ 3x above the true maximum of a 65 536 x 192 map, well inside the 18 binades a K20 operand keeps at full precision.
 * One workgroup per LayerNorm, 96 per launch; HOST arrays of length count. */
int mbv_ln_bound_group(const float* const* gamma, const float* const* beta, const int32_t* c, uint32_t* const* records,
                       int32_t count, void* stream);

/* out (m, n) = act(x (m, k) . w (n, k)^T + bias)                                   (nn.Linear forward) */
int mbv_gemm32s_nt(const float* x, const float* w, const float* bias, float* out, float* out_pre, int64_t m, int64_t n,
                   int64_t k, int64_t ldx, int64_t ldw, int64_t ldo, const uint32_t* amax_x, const uint32_t* amax_w,
                   uint32_t* amax_out, int32_t act, int32_t batch, int64_t stride_x, int64_t stride_w, int64_t stride_o,
                   void* stream);

/* out (m, k) = g (m, n) . w (n, k)                                                 (nn.Linear data gradient) */
int mbv_gemm32s_nn(const float* g, const float* w, float* out, int64_t m, int64_t n, int64_t k, int64_t ldg, int64_t ldw,
                   int64_t ldo, const uint32_t* amax_g, const uint32_t* amax_w, uint32_t* amax_out, int32_t batch,
                   int64_t stride_g, int64_t stride_w, int64_t stride_o, void* stream);

/* dw (n, k) contiguous += g (m, n)^T . x (m, k)                                     (nn.Linear weight gradient)
 * The token sum is cut into parts that are stored to `workspace` (mbv_gemm32s_tn_workspace_bytes) and added into dw by
 * their owner thread: no atomics, bit-reproducible. */
size_t mbv_gemm32s_tn_workspace_bytes(int64_t m, int64_t n, int64_t k);
int mbv_gemm32s_tn_acc(const float* g, const float* x, float* dw, int64_t m, int64_t n, int64_t k, int64_t ldg, int64_t ldx,
                       const uint32_t* amax_g, const uint32_t* amax_x, void* workspace, size_t workspace_bytes,
                       void* stream);

/* The 4 x 4 non-overlapping patch projection of the backbone (mmdet PatchEmbed = Conv2d(C, E, 4, stride 4) on the encoder's
 * (B, C, h, w) f32 pseudo-image; /root/reference: mask_bev/models/networks/swin/swin.py:579-586) on K20 WITHOUT materialising
 * the (tokens, 16 C) row matrix: element (token, k' = c 16 + dy 4 + dx) of the rows is image element (b, c, 4 oy + dy, 4 ox + dx),
 * gathered (forward, weight gradient) or scattered (image gradient) by the GEMM's own 16-byte operand pieces.  Replaces, in fp32
 * compute, MIOpen's convolution forward / backward (0.73 + 1.78 ms per step at 512 x 512, batch 4).  weight (E, 16 C) = the
 * (E, C, 4, 4) parameter as it lies in memory; out (B * h/4 * w/4, E) token-major; w % 128 == 0, h % 4 == 0, C even, E % 8 == 0. */
int mbv_patch_embed32_supported(int64_t batch, int64_t channels, int64_t h, int64_t w, int64_t embed);
int mbv_patch_embed32_fwd(const float* image, const float* weight, const float* bias, float* out, int64_t batch,
                          int64_t channels, int64_t h, int64_t w, int64_t embed, const uint32_t* amax_image,
                          const uint32_t* amax_w, void* stream);
int mbv_patch_embed32_bwd_image(const float* d_out, const float* weight, float* d_image, int64_t batch, int64_t channels,
                                int64_t h, int64_t w, int64_t embed, const uint32_t* amax_g, const uint32_t* amax_w,
                                void* stream);
size_t mbv_patch_embed32_bwd_weight_workspace_bytes(int64_t batch, int64_t channels, int64_t h, int64_t w, int64_t embed);
int mbv_patch_embed32_bwd_weight(const float* d_out, const float* image, float* d_weight, int64_t batch, int64_t channels,
                                 int64_t h, int64_t w, int64_t embed, const uint32_t* amax_g, const uint32_t* amax_image,
                                 void* workspace, size_t workspace_bytes, void* stream);


/* The weight gradients of `count` f32 Linears in ONE K20 launch (+ one parts-add launch) per 48 of them:
 * dw[i] (n[i], k[i]) f32, contiguous  +=  g[i] (m[i], n[i])^T . x[i] (m[i], k[i]);  the dw[i] of one call must not overlap.
 * A weight gradient is nobody's input: the Linears of a backward pass hand theirs over and the pass issues them together at its
 * end (fp32 compute; the 16-bit modes' mbv_gemm16_tn_group).  Few-row products (the decoder's 400 query rows: a 256 x 256 ...
 * 2048 x 256 output is 4 ... 32 tiles) fill the chip together; token-major ones (1 024 - 65 536 tokens) are cut into ranges of
 * ~ 4 096 tokens instead of the ~ 40 slivers each needs alone.  One range: the tile is added to dw in place by its owner
 * workgroup; several: partial tiles go to `workspace` (mbv_gemm32s_tn_group_workspace_bytes; 16-byte aligned) and are added by
 * their owner — no atomics, bit-reproducible.  amax_g[i] / amax_x[i]: absmax records of the operands (NULL array or entry =
 * unscaled).  Replaces, in fp32 compute, mbv_wgrad_small_f32_group (exact-f32 MFMA + atomics) for shapes with n, k multiples
 * of 8, and the per-layer mbv_gemm32s_tn_acc launches.  HOST arrays of length count. */
size_t mbv_gemm32s_tn_group_workspace_bytes(const int64_t* m, const int64_t* n, const int64_t* k, int32_t count);
int mbv_gemm32s_tn_group(const float* const* g, const float* const* x, float* const* dw, const int64_t* m, const int64_t* n,
                         const int64_t* k, const int64_t* ldg, const int64_t* ldx, const uint32_t* const* amax_g,
                         const uint32_t* const* amax_x, int32_t count, void* workspace, size_t workspace_bytes, void* stream);

/* The pixel decoder's 3 x 3 convolution in-tree (fp32 compute; replaces MIOpen's f32 convolution forward / backward-data /
 * backward-weight for /root/reference: mask_bev/models/head/mask_bev_panoptic_head.py:119-146 — mmdet
 * MSDeformAttnPixelDecoder.output_convs: ConvModule(256, 256, 3, padding 1, bias off) + GroupNorm + ReLU on the (B, 256, 128, 128)
 * map).  The map is turned once into a zero-bordered channels-last ROWS buffer — (mbv_conv_rows(B, H, W), C): G = W + 3 guard
 * rows, then the (B, H + 2, W + 2) padded positions, then G guard rows; everything but the interior pixels zero — on which the
 * convolution is ONE token-major K20 product over k = (tap, channel): the row of position m for tap t = 3 dy + dx is row
 * m + (dy - 1)(W + 2) + (dx - 1) of the same buffer (a scalar offset per K-step, no im2col).
 *   mbv_conv_pad_rows:   dst rows (cleared by the caller) <- interior pixels of src (B, C, H, W); elem_size 4 (f32) or 2
 *   mbv_conv_unpad_rows: dst (B, C, H, W) <- interior pixels of the rows buffer src
 *   mbv_conv3x3_gemm32s: out_rows (rows buffer, cout channels; its interior positions hold the result) from rows (C channels)
 *                        and wm (cout, 9 C) f32 with wm[co][t C + ci] = weight[co][ci][dy][dx].  The DATA gradient is the same call
 *                        on the output gradient's rows with wm[ci][t cout + co] = weight[co][ci][2 - dy][2 - dx]; the WEIGHT
 *                        gradient is nine entries of mbv_gemm32s_tn_group (g = the output gradient's rows, x = rows shifted by
 *                        the tap).  C % 32 == 0, cout % 8 == 0, 16-byte aligned buffers; amax_*: absmax records (NULL = unscaled). */
int64_t mbv_conv_rows(int64_t batch, int64_t H, int64_t W);
int mbv_conv_pad_rows(const void* src, void* dst, int64_t batch, int64_t C, int64_t H, int64_t W, int32_t elem_size, void* stream);
int mbv_conv_unpad_rows(const void* src, void* dst, int64_t batch, int64_t C, int64_t H, int64_t W, int32_t elem_size,
                        void* stream);
int mbv_conv3x3_gemm32s(const float* rows, const float* wm, float* out_rows, int64_t batch, int64_t H, int64_t W, int64_t C,
                        int64_t cout, const uint32_t* amax_rows, const uint32_t* amax_w, uint32_t* amax_out, void* stream);
/* the 16-bit compute modes' form (K17; dtype 0 = bf16, 1 = fp16; out_rows 16-bit or f32): the same buffers and weight layout */
int mbv_conv3x3_gemm16(const void* rows, const void* wm, void* out_rows, int64_t batch, int64_t H, int64_t W, int64_t C,
                       int64_t cout, int32_t dtype, int32_t out_f32, void* stream);

/* The fp32 FFN's backward in one K20 launch: out (m, k) = act'(pre (m, k)) * (g (m, n) . w (n, k)) — the data gradient of the
 * output layer times the activation's derivative (act: 1 ReLU, 2 erf-GELU) — and, into `parts`
 * ((mbv_gemm32s_nn_part_rows(m, 1), k) f32, every element written), the partial column sums of `out`: their sum over the rows is
 * the bias gradient of the input layer.  Replaces the f32 library GEMM + mbv_act_bwd_colsum pass of mmcv FFN's backward
 * (/root/reference: mask_bev/models/networks/swin/swin.py:347-355). */
int64_t mbv_gemm32s_nn_part_rows(int64_t m, int32_t batch);
int mbv_gemm32s_nn_act(const float* g, const float* w, float* out, const float* pre, float* parts, size_t parts_bytes,
                       int64_t m, int64_t n, int64_t k, int64_t ldg, int64_t ldw, int64_t ldo, int64_t ldpre,
                       const uint32_t* amax_g, const uint32_t* amax_w, uint32_t* amax_out, int32_t act, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K21 — instances of one decoder output at inference (csrc/instances.hip).
 * Replaces the host loops `c = cls.argmax(); if c > 0: sigmoid(F.interpolate(mask, (ny, nx), 'bilinear',
 * align_corners=False)) > 0.5` of mask_bev/evaluation/kitti_eval.py:27-44 and mask_bev/mask_bev_module.py:286-294, with no
 * (B, Q, ny, nx) intermediate.  Class convention: index 0 = empty, > 0 = object.
 *
 * mbv_select_queries: cls (rows, classes) in f32 / bf16 / fp16 (cls_dtype: MBV_DT_*), classes <= 256.  Per row, in f32:
 *   label = first argmax (torch's tie rule), score = softmax(cls)[label] (max-subtracted),
 *   keep = label > 0 && score >= score_threshold.  label (rows) i32, score (rows) f32, keep (rows) u8 {0, 1}.
 *
 * mbv_extract_masks: logits (batch, num_queries, h, w) f32, score / keep (batch * num_queries) as above; BEV grid H x W with
 *   H*W <= 1024*1024.  Every pixel is interpolated with upsample_bilinear2d's align_corners=False arithmetic (as K15);
 *   a pixel is SET when v > 0 (sigmoid(v) > 0.5).  Outputs, each may be NULL:
 *   masks_packed (batch * num_queries, mbv_packed_mask_words(H, W)) u32: every map, mbv_pack_binary_masks layout;
 *   areas (batch, num_queries) i32: set pixels;  mask_scores (batch, num_queries) f32: mean of sigmoid(v) over the set
 *   pixels, 0 for an empty mask;  instance_map (batch, H, W) i32: the kept query with a set bit maximising
 *   score[q] * sigmoid(v_q), ties to the smaller q, -1 where there is none.
 *   areas / mask_scores need `workspace` (mbv_extract_masks_workspace_bytes; per-tile partial sums, reduced in a second
 *   launch in a fixed order: deterministic).  No memset, no atomics on floats: every output element is written by a kernel.
 *   batch * num_queries == 0 returns MBV_OK before any pointer is checked (with batch > 0 and num_queries == 0 a non-NULL
 *   instance_map is filled with -1); MBV_ERR_UNSUPPORTED when a tile's logit rows
 *   exceed 64 KB of LDS (w > 8192). */
int mbv_select_queries(const void* cls, int32_t cls_dtype, int64_t rows, int32_t classes, float score_threshold,
                       int32_t* label, float* score, uint8_t* keep, void* stream);
size_t mbv_extract_masks_workspace_bytes(int32_t batch, int32_t num_queries, int32_t h, int32_t w, int32_t H, int32_t W);
int mbv_extract_masks(const float* logits, const float* score, const uint8_t* keep, int32_t batch, int32_t num_queries,
                      int32_t h, int32_t w, int32_t H, int32_t W, uint32_t* masks_packed, int32_t* areas,
                      float* mask_scores, int32_t* instance_map, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K22 — SemanticKITTI scene → instance-id map (csrc/rasterize.hip): the input of K14, made on the device.
 * Replaces: SemanticKittiRasterizer.get_mask_around (mask_bev/datasets/semantic_kitti/semantic_kitti_rasterizer.py:41-94;
 * numpy + one cv2.morphologyEx pair per instance on the host) and with it the reference's `.npy` mask cache.
 *
 * points        (n_points, stride) f32 (points_f64 = 0) or f64 (points_f64 = 1), x, y, z first, stride 3 or 4; scans
 *               concatenated.  f64 is the reference's aggregated scene in the world frame, passed through as it is.
 * inst          (n_points) i32 instance id per point, 0 = no instance; valid ids are 1 … 65535 (SemanticKITTI's 16 bits)
 * scan_offsets  (n_scans + 1) i32; transforms (n_scans, 4, 4) f64 row-major, scan → centre-scan frame, last row 0 0 0 1
 *               (the caller checks it; only the upper 3 x 4 block is read)
 * centre_inst   (n_centre) i32.  n_centre < 0 (`remove_unseen = False`, :80): the present instances are the ids with at
 *               least one kept point.  n_centre >= 0 (:73-78): they are the non-zero ids with >= max(min_points, 1) labels in
 *               the whole centre scan; a present instance with no kept point paints nothing.
 * geometry      a point is KEPT iff lo < c < hi strictly on all three axes of the transformed point (:59-61; NaN / inf
 *               never are); cell ix = floor((x - x_lo) / voxel_size), iy likewise (:66-67), all in f64 with one rounding
 *               per operation (the transform is ((m0 x + m1 y) + m2 z) + m3, no contraction).  nx, ny are the caller's
 *               int((hi - lo) / voxel_size); a kept point whose cell index reaches nx or ny is dropped.
 * morph_kernel  odd, 1 … 31: every present instance's occupancy is closed, then opened, with a k x k square (:71, :87-88).
 *               Border rule (cv2 BORDER_CONSTANT with morphologyDefaultBorderValue): outside the grid a cell counts as
 *               set for an erosion and as clear for a dilation.
 * instance_map  (nx, ny) i32, 0 = background: the layout of the reference's mask cache and of K14's input.
 *               OVERLAPS: the reference paints in the iteration order of a Python set of numpy.uint32 (hash order, neither
 *               ascending nor stable); here THE HIGHEST ID WINS on a cell that several closed-and-opened instances
 *               claim, independent of point order.  Where no two instances share a cell the map equals the reference's.
 * status        device i32, written by phase 1: bit 0 = more than max_instances present instances (the max_instances
 *               smallest ids are rasterised), bit 1 = an id outside 0 … 65535 was met (those points are skipped).
 * phases        bit 0 = K22a (id table, occupancy bits and cell bounding boxes into `workspace`), bit 1 = K22b
 *               (morphology + paint from `workspace`); 3 = the whole call.  Split only for measurements.
 * workspace     mbv_rasterize_workspace_bytes(nx, ny, max_instances) bytes, 256-byte aligned; 0 = bad geometry
 *               (nx, ny >= 1, nx * ny <= 2^26, 1 <= max_instances <= 65535).  MBV_ERR_UNSUPPORTED when a row band of
 *               the widest window cannot hold its halo: 8192 / ceil(ny / 32) - 8 * (k / 2) < 1 (ny > 2176 with k = 31).
 *               `inst` must be 16-byte aligned.
 *
 * mbv_rasterize_paint is K22b alone on caller-given data: occupancy (n_slots_max, nx, ceil(ny / 32)) u32, bit b of word w
 * of row ix = cell (ix, 32 w + b), bits at iy >= ny clear; bbox (n_slots_max, 4) i32 = inclusive cell bounds xmin, ymin,
 * xmax, ymax of the set bits (xmax < 0: nothing to paint); slot_ids (n_slots_max) i32 > 0; *n_slots (device i32) <=
 * n_slots_max slots are painted.  It zeroes instance_map first.
 */
size_t mbv_rasterize_workspace_bytes(int32_t nx, int32_t ny, int32_t max_instances);
int mbv_rasterize(const void* points, int32_t points_f64, int32_t stride, const int32_t* inst, int64_t n_points,
                  const int32_t* scan_offsets, int32_t n_scans, const double* transforms, const int32_t* centre_inst,
                  int64_t n_centre, double x_lo, double x_hi, double y_lo, double y_hi, double z_lo, double z_hi,
                  double voxel_size, int32_t nx, int32_t ny, int32_t morph_kernel, int32_t min_points,
                  int32_t max_instances, int32_t phases, int32_t* instance_map, int32_t* status, void* workspace,
                  size_t workspace_bytes, void* stream);
int mbv_rasterize_paint(const uint32_t* occupancy, const int32_t* bbox, const int32_t* slot_ids, const int32_t* n_slots,
                        int32_t n_slots_max, int32_t nx, int32_t ny, int32_t morph_kernel, int32_t* instance_map,
                        void* stream);

/* K34 — mbv_rasterize for a whole batch on a scene bank that stays on the device (scene_bank.SceneBank): the labelled
 * points of a sequence, every scan in its own frame.  A sample's scene is a list of SEGMENTS of the bank, each with the
 * transform that takes its scan into the sample's frame; the bank is read in place, nothing is copied or reordered, and
 * the number of launches depends neither on the number of segments nor on `batch`.
 *
 * points, inst    the bank: (n_bank, 3) f32 and (n_bank) i32, both 16-byte aligned
 * seg_start       (n_seg) i64 first bank point, seg_count (n_seg) i32 points of each segment; the segments of sample 0
 *                 first, then sample 1's, ... in the order in which mbv_rasterize would get the scans.  The caller checks
 *                 0 <= seg_start and seg_start + seg_count <= n_bank; the kernels also never read beyond n_bank.
 * transforms      (n_seg, 4, 4) f64 row-major, as in mbv_rasterize
 * chunks          (n_chunks, 4) i32, 16-byte aligned, made on the host: segment, first point inside the segment, sample, 0.
 *                 One workgroup bins the points [first, first + chunk_points) of the segment (fewer at its end), so every
 *                 point of a workgroup has one transform; chunk_points is a multiple of 4.  Every point of every segment
 *                 must lie in exactly one chunk, whose sample is the one the segment belongs to.
 * centre_start    (batch) i64, centre_count (batch) i32: sample b's centre_inst is inst[centre_start[b] : centre_start[b] +
 *                 centre_count[b]]; centre_count[b] < 0 = remove_unseen off for that sample (n_centre < 0 there)
 * instance_maps   (batch, nx, ny) i32; status (batch) i32, the bits of mbv_rasterize per sample.
 * Map b and status[b] are bit-equal to what mbv_rasterize gives for the concatenation of sample b's segments in table
 * order with sample b's transforms and that centre_inst: every rule above holds, the same device functions run.  A sample
 * without segments, or without a kept point, gets an all-zero map.  batch = 0 returns MBV_OK before anything is checked.
 * geometry, morph_kernel, min_points, max_instances, phases: as in mbv_rasterize.
 * workspace       mbv_rasterize_bank_workspace_bytes(batch, nx, ny, max_instances) bytes, 256-byte aligned; 0 = bad
 *                 geometry or batch outside 1 ... 65535.
 */
size_t mbv_rasterize_bank_workspace_bytes(int32_t batch, int32_t nx, int32_t ny, int32_t max_instances);
int mbv_rasterize_bank(const float* points, const int32_t* inst, int64_t n_bank, const int64_t* seg_start,
                       const int32_t* seg_count, int32_t n_seg, const double* transforms, const int32_t* chunks,
                       int32_t n_chunks, int32_t chunk_points, const int64_t* centre_start, const int32_t* centre_count,
                       int32_t batch, double x_lo, double x_hi, double y_lo, double y_hi, double z_lo, double z_hi,
                       double voxel_size, int32_t nx, int32_t ny, int32_t morph_kernel, int32_t min_points,
                       int32_t max_instances, int32_t phases, int32_t* instance_maps, int32_t* status, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K23 — training augmentations of scans and instance maps (csrc/augment.hip).
 * Replaces: Flip, ShufflePoints, RandomRotate, DecimatePoints, JitterPoints, RandomDropPoints of
 * mask_bev/augmentations/semantic_kitti_mask_augmentations.py:44-161 (numpy + cv2.warpAffine on the host, per sample).
 * The per-sample decisions (which transforms fire, the angle, the seed) are drawn on the host; the device runs them.
 *
 * points        (n_points, dim) f32, dim 3 or 4 (x, y, z[, intensity]); the scans of a batch concatenated
 * scan_offsets  (batch + 1) i32, ascending, scan_offsets[batch] = n_points; 1 <= batch <= 4096, n_points < 2^28
 * records       (batch) records of 656 bytes, 8-byte aligned, one per scan, little endian, no padding beyond what is named:
 *                 u32 seed_lo, u32 seed_hi   the sample's 64-bit seed
 *                 i32 n_ops                  0 ... 8 ops, run in order
 *                 i32 flags                  bit 0: the scan's output order is that of the order hash (a shuffle or a
 *                                            decimate was drawn); otherwise the scan keeps its input order
 *                 8 x op (80 bytes each):    i32 code, u32 arg, f64 p[9]
 *               op codes: 0 none; 1 linear, p[0..3] = a00 a01 a10 a11; 2 jitter, p[0] = magnitude, p[1..4] = std of
 *               x y z intensity, p[5..8] = max_delta of x y z intensity (+inf = no clip); 3 drop, arg = T;
 *               4 shuffle (sets nothing on a point: flags bit 0 carries it); 5 decimate, arg = k >= 1;
 *               6 global noise, p[0] = scale, p[1..3] = translation of x y z (kitti_mask_augmentations.py:196-217).
 * the ops       The value of a point lives in f32 between ops.  f64 arithmetic has one rounding per operation, no
 *               contraction.
 *                 linear   x' = (f32)(a00 * (f64)x + a01 * (f64)y), y' = (f32)(a10 * (f64)x + a11 * (f64)y), both from the
 *                          old x, y; z, intensity untouched.
 *                 jitter   per component c < dim: d = std_c * (f64)n_c, clipped to [-max_delta_c, max_delta_c];
 *                          v_c = (f32)((f64)v_c + magnitude * d); then, dim = 4, intensity clamped to [0, 1] in f32.
 *                 drop     the point is kept iff (draw(slot, idx, 0, 0) >> 8) >= T, T = ceil(p * 2^24) clamped to 0 ... 2^24.
 *                 global noise   v_c = (f32)((f64)v_c * scale + t_c) for c = x, y, z; intensity untouched.
 * the draws     with pcg(v): s = v * 747796405 + 2891336453; w = ((s >> ((s >> 28) + 4)) ^ s) * 277803737;
 *               pcg = (w >> 22) ^ w (all u32, wrapping):
 *                 stream(slot)            = pcg(seed_lo ^ pcg(seed_hi + slot * 0x9E3779B9))
 *                 draw(slot, idx, c, j)   = pcg(stream(slot) + (idx * 8 + c * 2 + j))
 *               slot = the op's position in the list (0 ... 7; 8 = the order hash), idx = the point's ORIGINAL index within
 *               its scan, c = component, j = 0 / 1.  A result therefore depends neither on the launch shape nor on what
 *               other scans share the batch.  The standard normal of (slot, idx, c), all in f32 with the full-precision
 *               logf / sqrtf / cosf:  u1 = ((draw(.., 0) >> 8) + 1) * 2^-24, u2 = (draw(.., 1) >> 8) * 2^-24,
 *               n = sqrtf(-2 * logf(u1)) * cosf(6.283185307179586f * u2);  |n| <= 5.77.
 * mode          0: no point is removed or moved; drop / shuffle / decimate ops are ignored; no workspace needed.
 *               1: drops only: the kept points of every scan in input order (count, scan, scatter: stable compaction).
 *               2: order and selection by one stable radix sort (batch <= 63 and n_points < 2^26 are required).  Key of
 *                  a kept point = scan << 26 | (draw(8, idx, 0, 0) >> 6) when flags bit 0 is set, else scan << 26 | idx; a
 *                  dropped point has the key batch << 26.  Ties keep input order: a shuffle is uniform up to the
 *                  ~n^2 / 2^27 expected pairs of equal 26-bit hashes (107 at 120 000 points), which stay in input order.
 *                  The key's hash bits do not depend on the batch, so a scan comes out the same alone or beside others.  Of the m
 *                  survivors of a scan the first keep are written, keep = m passed through ceil(keep / k) once per
 *                  decimate op, in op order: a uniform random subset in random order, the reference's pc[randperm][::k]
 *                  in distribution.  A drop counts wherever it stands in the list: all drops act before the decimates.
 *               The caller passes the smallest mode that covers the ops of the batch.
 * out           (n_points, dim) f32: the output scans concatenated, the first out_offsets[batch] rows are written
 * out_offsets   (batch + 1) i32, out_counts (batch) i32: written on the device in every mode
 * workspace     mbv_augment_workspace_bytes(n_points, batch, mode) bytes (0 = bad arguments), 256-byte aligned.
 * MBV_ERR_UNSUPPORTED: n_points >= 2^28, or mode 2 with n_points >= 2^26 or batch > 63.  No atomics: the output is a pure function of
 * the inputs.
 *
 * mbv_warp_instance_maps — the cached-map path: maps (batch, nx, ny) i32 → out (batch, nx, ny) i32 (out != maps), mats
 * (batch, 4) f64 = a00 a01 a10 a11 of every sample's composed matrix A (flips and rotations in op order, original →
 * augmented; orthogonal, so its inverse is its transpose); cx = -x_lo / voxel_size, cy = -y_lo / voxel_size: the cell
 * coordinate of the origin.  For every output cell, in f64, one rounding per operation:
 *   du = (ix + 0.5) - cx;  dv = (iy + 0.5) - cy;  su = (a00 * du + a10 * dv) + cx;  sv = (a01 * du + a11 * dv) + cy;
 *   out[ix, iy] = maps[floor(su), floor(sv)], 0 where that lies outside the grid.
 * A flip on a symmetric range is exactly the reference's mask[::-1, :] / mask[:, ::-1] (:52, :55); on an asymmetric range
 * it mirrors about the origin's cell, as the flipped points do, and cells from outside the grid arrive as 0.  A rotation is
 * nearest-neighbour about the origin; the reference's cv2.warpAffine(INTER_NEAREST) turns about (sx / 2, sy / 2) in
 * integer-centred pixel coordinates, half a cell away: parity with OpenCV is not pinned by any test.
 */
size_t mbv_augment_workspace_bytes(int64_t n_points, int32_t batch, int32_t mode);
int mbv_augment_points(const float* points, int32_t dim, int64_t n_points, const int32_t* scan_offsets, int32_t batch,
                       const void* records, int32_t mode, float* out, int32_t* out_offsets, int32_t* out_counts,
                       void* workspace, size_t workspace_bytes, void* stream);
int mbv_warp_instance_maps(const int32_t* maps, const double* mats, int32_t batch, int32_t nx, int32_t ny, double cx,
                           double cy, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K24 — KITTI / Waymo box tables → instance-id maps (csrc/box_rasterize.hip): the input of K14 for the box datasets.
 * Replaces: the paint loop of KittiRasterizer.get_mask (mask_bev/datasets/kitti/kitti_rasterizer.py:45-56) and of
 * WaymoRasterizer.get_mask (mask_bev/datasets/waymo/waymo_rasterizer.py:38-45): one cv2.drawContours(..., -1) per box on
 * the host.  The corners are made on the host (rasterize.box_vertices: the reference's f64 expressions and np.intp).
 *
 * vertices      (n_boxes, 4, 2) i32, 16-byte aligned: v0 .. v3 of every box in cell coordinates (px, py), px along x.
 *               |coordinate| <= 2^20; a box with a vertex beyond that paints nothing.
 * ids           (n_boxes) i32: the value a box paints
 * frame_offsets (batch + 1) i32 on the device, ascending from 0; frame b owns rows frame_offsets[b] .. frame_offsets[b + 1]
 *               - 1, frame_offsets[batch] = n_boxes.  An empty frame is valid.  Rows outside 0 .. frame_offsets[batch]
 *               are never read.
 * maps          (batch, nx, ny) i32, ny contiguous: the layout of K14's input.  EVERY cell is written: 0 where no box of
 *               the frame holds it, else the id of the LAST box in table order that does (the reference's overwrite).
 * the fill rule A cell (px, py) belongs to a box iff it is in I or in L; cells outside the grid are dropped.
 *                 I  the integer point lies inside or on the closed quadrilateral: on an edge (cross product 0, inside
 *                    the edge's bounding box), or a ray towards +x crosses an odd number of edges: edge a → b is crossed
 *                    iff (ay > py) != (by > py) and cross = (bx - ax)(py - ay) - (by - ay)(px - ax) is > 0 for by > ay,
 *                    < 0 for by < ay.  64-bit products; either vertex order; a folded quadrilateral fills even-odd.
 *                 L  the point is on the line between two consecutive vertices (v3 → v0 included): dx = bx - ax,
 *                    dy = by - ay, n = max(|dx|, |dy|), the points (ax + floor((2 i dx + n) / (2 n)),
 *                    ay + floor((2 i dy + n) / (2 n))), i = 0 .. n; n = 0: the single point.
 *               All arithmetic is integer: the map is a pure function of the table.  Parity with OpenCV's fill is NOT
 *               pinned by any test: drawContours draws the outline with its own line iterator and fills spans in 16-bit
 *               fixed point, so tie cells on an edge may differ.
 * One launch, no workspace, no host synchronisation, nothing to pre-zero.  MBV_ERR_BAD_ARG: a null pointer, batch outside
 * 1 .. 65535, nx or ny < 1, nx * ny > 2^26, nx > 16 * 65535, vertices not 16-byte aligned; nothing is launched.
 */
int mbv_rasterize_boxes(const int32_t* vertices, const int32_t* ids, const int32_t* frame_offsets, int32_t batch,
                        int32_t nx, int32_t ny, int32_t* maps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K25 — oriented box of a bit-packed BEV mask (csrc/box_fit.hip).
 * Stands where mask_to_pred (mask_bev/evaluation/kitti_eval.py:27-45) takes cv2.minAreaRect of the largest contour on the
 * host.  Here ALL set cells of a mask count and the box is the MOMENT-AXIS box; equality with minAreaRect is not pinned
 * by any test (OpenCV is not a dependency).
 *
 * packed        (num_maps, mbv_packed_mask_words(H, W)) u32, mbv_pack_binary_masks layout: pixel y * W + x; H * W <= 2^20.
 *               Bits at and beyond H * W are not read as cells.
 * rows          (num_rows) i32: the maps to fit; a row outside 0 .. num_maps - 1 counts as an empty mask.
 * n             (num_rows) i32: set cells.
 * moments       (num_rows, 5) i64: Σx, Σy, Σx², Σy², Σxy over the set cells, x and y the integer cell indices; exact.
 * boxes         (num_rows, 5) f32: cx, cy, dx, dy, theta in cell units; all 0 for a row with n == 0.
 *                 cx = Σx / n, cy = Σy / n (the centroid).
 *                 theta = atan2(2 m11, m20 - m02) / 2 with m20 = n Σx² - (Σx)², m02 = n Σy² - (Σy)², m11 = n Σxy - Σx Σy
 *                 formed in i64 (exact) and only then converted to f64; theta = 0 when m11 = 0 and m20 = m02.
 *                 dx = max u - min u + |cos theta| + |sin theta| with u = x cos theta + y sin theta over the set cells,
 *                 dy the same with v = y cos theta - x sin theta: the extent of the cells' centres plus the support of
 *                 the unit cell, so an axis-aligned a x b block of cells gives exactly (a, b).
 *               f64 arithmetic, one rounding per operation, one rounding to f32 at the store.
 * One workgroup per row, two sweeps over its words; integer sums and min / max only, so the result is deterministic.
 * MBV_ERR_BAD_ARG: a null pointer (with num_rows > 0), H or W < 1, H * W > 2^20, num_maps < 1 with rows to fit.
 */
int mbv_fit_boxes(const uint32_t* packed, int64_t num_maps, int32_t H, int32_t W, const int32_t* rows, int32_t num_rows,
                  int32_t* n, int64_t* moments, float* boxes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K30a — the largest 8-connected component of a bit-packed mask (csrc/mask_components.hip).
 * K30b — the minimum-area rectangle of the set cells of a bit-packed mask (csrc/min_area_rect.hip).
 * Together what mask_to_pred (mask_bev/evaluation/kitti_eval.py:27-45) does with cv2.findContours + cv2.minAreaRect: the
 * tightest rectangle around the largest blob of a mask.  K30b is over ALL set cells of the map it is given; the component
 * logic lives in K30a alone and the two compose (K30a's output is K30b's input).
 * Not reproduced: the reference picks the contour by cv2.contourArea (the polygon area through the border pixels'
 * centres), which cannot be restated without OpenCV (not a dependency); K30a picks by the NUMBER OF CELLS.  OpenCV's own
 * floating-point rectangle arithmetic is not restated either: K30b's choice of the rectangle is exact integer arithmetic.
 *
 * Common to both:
 * packed        (num_maps, mbv_packed_mask_words(H, W)) u32, mbv_pack_binary_masks layout: pixel y * W + x is bit p % 32 of
 *               word p / 32, maps are not row-aligned.  Bits at and beyond H * W are garbage and never cells.
 * rows          (num_rows) i32, any order, repeats allowed; a row outside 0 .. num_maps - 1 counts as an empty map.
 * 1 <= H, W <= 1024, anything else is MBV_ERR_BAD_ARG, as are a null pointer or num_maps < 1 with rows to do.
 * num_rows == 0 returns MBV_OK without a launch.  One workgroup per listed row, one launch, no host readback, no device
 * allocation, every loop bounded by construction: capturable into a HIP graph.  Integer work only up to the box's store,
 * so the results are deterministic.
 *
 * K30a.  Connectivity is 8-neighbour (as findContours traces foreground).  The kept component is the one with the most
 * cells; among components of equal size the one that contains the lowest raster index y * W + x wins.
 * out_packed    (num_rows, words) u32: the kept component in the same layout; bits at and beyond H * W are 0.
 * n             (num_rows) i32: cells of the kept component (0 for an empty map, with out_packed all 0).
 * components    (num_rows) i32: number of components of the map.
 * workspace     mbv_largest_component_workspace_bytes(H, W, num_rows) bytes (0 for small grids: two row-aligned planes of
 *               the cells' bounding box live in LDS when they fit 16 KiB each, in the workspace otherwise);
 *               MBV_ERR_WORKSPACE when it is smaller.  Nothing to pre-zero.
 *
 * K30b.  The points are the integer cell coordinates (x, y); everything that selects the rectangle is integer arithmetic.
 * n             (num_rows) i32: set cells.
 * hull          (num_rows) i32: vertices of the STRICTLY convex hull (collinear points dropped): 0 for an empty map, 1 for a
 *               single cell, 2 for collinear cells.
 * boxes         (num_rows, 5) f32: cx, cy, dx, dy, theta in cell units; all 0 for an empty map; [x, y, 1, 1, 0] for one cell.
 *   For each hull edge direction e = (ex, ey) the rectangle through the points with a side along e has the area
 *   (max - min of p . e) (max - min of p x e) / |e|^2, p x e = ex py - ey px: a ratio of integers; areas are compared
 *   exactly by cross-multiplication.  The smallest area wins.  Among edges of exactly equal area: rotate e by multiples of
 *   90 degrees to the canonical form ex > 0, -ex < ey <= ex and take the smallest |ey| / ex (cross-multiplied), then
 *   ey >= 0.  Edges with the same canonical direction give the same rectangle.  Collinear cells: the direction of the
 *   segment, canonicalised.
 *   theta = atan2(ey, ex) of the canonical direction, in (-pi/4, pi/4].  With u = p . e / |e| and v = p x e / |e|:
 *   dx = max u - min u + |cos theta| + |sin theta|, dy the same with v (K25's unit-cell support: an axis-aligned a x b
 *   block of cells gives exactly (a, b) and rasterize.boxes_from_cells applies unchanged); the centre is
 *   uc = (max u + min u) / 2, vc likewise, cx = uc cos theta - vc sin theta, cy = uc sin theta + vc cos theta.
 *   f64 arithmetic, one rounding per operation, one rounding to f32 at the store.
 */
int64_t mbv_largest_component_workspace_bytes(int32_t H, int32_t W, int32_t num_rows);
int mbv_largest_component(const uint32_t* packed, int64_t num_maps, int32_t H, int32_t W, const int32_t* rows,
                          int32_t num_rows, uint32_t* out_packed, int32_t* n, int32_t* components, void* workspace,
                          int64_t workspace_bytes, void* stream);
int mbv_min_area_boxes(const uint32_t* packed, int64_t num_maps, int32_t H, int32_t W, const int32_t* rows, int32_t num_rows,
                       int32_t* n, int32_t* hull, float* boxes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K26 — rotated-box overlap over ragged frames (csrc/rotate_iou.hip).
 * Stands where rotate_iou_gpu_eval (mask_bev/evaluation/rotate_iou.py) is called per part of the validation set.
 *
 * boxes         (n_boxes, 5) f32, qboxes (n_qboxes, 5) f32: x, y, dx, dy, angle.  The corners are those of
 *               rasterize.box_vertices: centre ± (dx / 2) d ± (dy / 2) d_bar, d = (cos angle, sin angle),
 *               d_bar = (-sin angle, cos angle): the angle turns COUNTER-clockwise (the reference's kernel turns clockwise).
 * box_offsets, qbox_offsets   (frames + 1) i32 on the device, ascending from 0 to n_boxes / n_qboxes.
 * pair_offsets  (frames + 1) i64 on the device: pair_offsets[f + 1] - pair_offsets[f] = n_f * k_f, pair_offsets[frames] =
 *               total_pairs.
 * criterion     -1: intersection / union; 0: intersection / area of the box; 1: / area of the query box; 2: the intersection.
 * overlaps      (total_pairs) f32: frame f's (n_f, k_f) matrix, k_f contiguous, at pair_offsets[f].  Exactly 0 where the
 *               rectangles do not meet in a polygon of positive area.
 * One thread per pair: the first rectangle, expressed in the second one's axes, is clipped against its four half-planes
 * (Sutherland-Hodgman), then the shoelace area.  f32 throughout.  Offsets that point outside the tables read nothing.
 * MBV_ERR_BAD_ARG: a null pointer, frames < 1, a criterion outside -1 .. 2; MBV_ERR_UNSUPPORTED: more than 2^39 pairs.
 */
int mbv_rotate_iou(const float* boxes, int64_t n_boxes, const float* qboxes, int64_t n_qboxes, const int32_t* box_offsets,
                   const int32_t* qbox_offsets, const int64_t* pair_offsets, int32_t frames, int64_t total_pairs,
                   int32_t criterion, float* overlaps, void* stream);

/* K26b — the same for boxes with a height: (n, 7) f32 x, y, z, dx, dy, dz, angle with z the BOTTOM face (the `boxes` of
 * batch.kitti_labels_to_velodyne, K28's membership rule); offsets, pair layout, criterion and error codes as K26.  The
 * overlap is inter = inter_bev * max(0, min(z + dz) - max(z)), divided by  -1: vol_a + vol_b - inter;  0: vol_a;  1: vol_b;
 * 2: 1  (vol = |dx dy dz|): the reference's d3_box_overlap_kernel with z_center = 1, moved to a z-up frame.  Exactly 0 where
 * the BEV polygons do not meet or the z-intervals do not overlap (touching faces included). */
int mbv_rotate_iou_3d(const float* boxes, int64_t n_boxes, const float* qboxes, int64_t n_qboxes, const int32_t* box_offsets,
                      const int32_t* qbox_offsets, const int64_t* pair_offsets, int32_t frames, int64_t total_pairs,
                      int32_t criterion, float* overlaps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K27 — KITTI statistics of all frames and score thresholds (csrc/kitti_stats.hip): the protocol's inner loop,
 * compute_statistics_jit / fused_compute_statistics of mask_bev/evaluation/kitti_eval.py:266-443 for metric == 1 (BEV).
 * DontCare regions and the orientation score (AOS) belong to the image-box metric: out of scope.
 *
 * overlaps      K26's output with the DETECTIONS as the first table: frame f's (d_f, g_f) matrix at pair_offsets[f].
 * dt_offsets, gt_offsets (frames + 1) i32, pair_offsets (frames + 1) i64, on the device.
 * ignored_gt    (n_gt) i32: 0 counted, 1 ignored at this difficulty (or a neighbouring class), -1 another class.
 * ignored_dt    (n_dt) i32: 0 counted, 1 ignored, -1 another class.  dt_scores (n_dt) f32.
 * min_overlap   a match needs (double)overlap > min_overlap.
 * thresholds    (num_thresholds) f32; with compute_fp a detection with score < threshold does not exist.
 * compute_fp    0: the highest-scoring candidate is matched, no false positives are counted (the pass that collects the
 *               scores get_thresholds consumes: num_thresholds = 1); 1: the candidate of largest overlap is matched, ignored
 *               detections only as a last resort, false positives counted.  The rules are written out in the kernel file.
 * stats         (num_thresholds, 3) i64: tp, fp, fn summed over the frames; zeroed by the call, exact.
 * tp_scores     (n_gt) f32 and tp_flags (n_gt) i32, both or neither: for threshold 0, per ground truth whether it was a
 *               true positive and the score of its detection (0 otherwise); every entry of a well-formed frame is written.
 * workspace     mbv_kitti_statistics_workspace_bytes(n_dt, num_thresholds) bytes: the per-thread "assigned" flags.
 * One thread per (frame, threshold), a serial greedy loop; integer atomics on `stats`.  A frame whose offsets point outside
 * the tables is left out.  MBV_ERR_BAD_ARG: a null pointer, frames < 1, num_thresholds outside 1 .. 65535.
 */
size_t mbv_kitti_statistics_workspace_bytes(int64_t n_dt, int32_t num_thresholds);
int mbv_kitti_statistics(const float* overlaps, const int64_t* pair_offsets, const int32_t* dt_offsets,
                         const int32_t* gt_offsets, int32_t frames, int64_t n_dt, int64_t n_gt, int64_t n_pairs,
                         const int32_t* ignored_gt, const int32_t* ignored_dt, const float* dt_scores, double min_overlap,
                         const float* thresholds, int32_t num_thresholds, int32_t compute_fp, int64_t* stats,
                         float* tp_scores, int32_t* tp_flags, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K28 — KITTI object augmentations: per-object perturbation and ground-truth pasting (csrc/object_augment.hip).
 * Replaces the per-point halves of BoxNoise and ObjectSample (mask_bev/augmentations/kitti_mask_augmentations.py:227-323):
 * mmdet3d's points_in_rbbox and points_transform_ (every point against every box, numba on a DataLoader worker) and the
 * numpy mask / concatenate that removes the scene points inside pasted boxes and appends the pasted points.  The decisions
 * of a frame (which bank entries are pasted, the noise each box takes: object_augment.py) are made on the host.  Parity
 * with mmdet3d itself is not pinned by any test: the rules below are the specification.
 *
 * points         (n_points, dim) f32, dim 3 or 4; the scans of a batch concatenated
 * scan_offsets   (batch + 1) i32 on the device, ascending, scan_offsets[batch] = n_points; 1 <= batch <= 4096
 * box_table      (n_boxes, 14) f64, 8-byte aligned, the rows of all scans concatenated; one row per box:
 *                  0 cx, 1 cy, 2 cz (the BOTTOM face), 3 l / 2, 4 w / 2, 5 h     l along the yaw direction, w across it
 *                  6 cos theta, 7 sin theta                                      centre and theta BEFORE the noise
 *                  8 cos r, 9 sin r, 10 tx, 11 ty, 12 tz                          the box's noise: a turn about its centre, a shift
 *                  13 flags (0 .. 3 as an f64): bit 0 = scene points inside are removed (a pasted box),
 *                                               bit 1 = points inside are moved
 *                The host supplies the cosines and sines; the kernels call no transcendental function.  Pasted boxes stand
 *                last in a scan's rows, in paste order.
 * box_offsets    (batch + 1) i32 on the device, ascending from 0, box_offsets[batch] = n_boxes.  Rows outside the table
 *                are never read.
 * max_boxes      the largest number of rows one scan owns, as the caller states it: no scan is given more than this many of
 *                its rows.  More than 128: MBV_ERR_UNSUPPORTED.
 * bank_points    (n_bank_points, 4) f32: the points of all bank samples (object_augment.ObjectBank), resident on the device
 * paste_segments (n_segments, 2) i32: first bank row and number of rows of every pasted sample, grouped by scan
 * paste_offsets  (batch + 1) i32: scan b owns the segments paste_offsets[b] .. paste_offsets[b + 1] - 1; n_segments <= 65535
 * n_paste_points the sum of the segments' rows as the caller states it.  A segment is clipped to the bank, and the segments
 *                together to n_paste_points: nothing is read outside the bank or written outside `out`.
 * out            (n_points + n_paste_points, dim) f32, of which the first out_offsets[batch] rows are written;
 *                n_points + n_paste_points < 2^28, else MBV_ERR_UNSUPPORTED
 * out_offsets    (batch + 1) i32, out_counts (batch) i32: written on the device
 * workspace      mbv_object_augment_workspace_bytes(n_points, batch, n_segments) bytes (0 = bad arguments), 256-byte aligned
 *
 * The rules.  f64 arithmetic, one rounding per operation, no contraction; (x, y, z) a point's f32 values taken to f64.
 *   membership   dx = x - cx; dy = y - cy; lx = cos theta * dx + sin theta * dy; ly = cos theta * dy - sin theta * dx;
 *                inside iff |lx| < l / 2 and |ly| < w / 2 and 0 < z - cz < h.  All strict: a point on a face is outside.
 *   scene point  inside ANY of its scan's rows with bit 0: removed.  Otherwise the FIRST row in table order that holds it
 *                and has bit 1 moves it:
 *                  x' = (f32)(((cos r * dx - sin r * dy) + cx) + tx)
 *                  y' = (f32)(((sin r * dx + cos r * dy) + cy) + ty)
 *                  z' = (f32)(z + tz)
 *                intensity untouched.  A box whose search found no free place has bit 1 and the identity noise: it still
 *                claims its points from the rows behind it, as points_transform_ does.
 *   pasted point never removed; moved by the same first-row rule, so a pasted object follows its own perturbed box.  A
 *                dim = 3 batch takes the bank's first three columns.
 *   output       per scan: the kept scene points in input order, then every segment's points in paste order.
 * Count, scan, scatter; no atomics: the output is a pure function of the inputs and a scan comes out the same alone or
 * beside others.
 *
 * mbv_points_in_boxes — index (n_points) i32: the first of the n_boxes rows of box_table (same layout; columns 8 .. 13 are
 * not read) that holds the point by the membership rule, or -1.  ObjectBank.build cuts its samples with it.
 */
size_t mbv_object_augment_workspace_bytes(int64_t n_points, int32_t batch, int32_t n_segments);
int mbv_object_augment(const float* points, int32_t dim, int64_t n_points, const int32_t* scan_offsets, int32_t batch,
                       const double* box_table, const int32_t* box_offsets, int64_t n_boxes, int32_t max_boxes,
                       const float* bank_points, int64_t n_bank_points, const int32_t* paste_segments,
                       const int32_t* paste_offsets, int32_t n_segments, int64_t n_paste_points, float* out,
                       int32_t* out_offsets, int32_t* out_counts, void* workspace, size_t workspace_bytes, void* stream);
int mbv_points_in_boxes(const float* points, int32_t dim, int64_t n_points, const double* box_table, int32_t n_boxes,
                        int32_t* index, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K29 — COCO mask AP: the per-image part of the `map_metric` slot, torchmetrics MeanAveragePrecision(iou_type='segm')
 * (mask_bev/mask_bev_module.py:85-94, fed at mask_bev/models/head/mask_bev_panoptic_head.py:87-96), which evaluates every
 * image with pycocotools' COCOeval.evaluateImg at `compute`.  Parity with those packages is not pinned (neither is
 * installed); the plain-loop statement of the protocol is oracle/metrics_oracle.py.
 *
 * K29a mbv_pairwise_mask_overlap — popcounts of N images' bit-packed masks (mbv_pack_binary_masks layout, tail bits zero):
 *   pred_words (N * Q, words) u32, gt_words (N * G, words) u32, words = mbv_packed_mask_words of the grid
 *   inter      (N, Q, G) i32   sum over the words of popc(pred & gt)
 *   pred_area  (N, Q) i32, gt_area (N, G) i32   set bits of every row
 *   Integer work, exact.  Q, G <= 1024 and words <= 2^26, else MBV_ERR_UNSUPPORTED.  N * Q * G == 0: MBV_OK whatever the
 *   pointers are; `inter` is not touched, and an area table is written only where it has rows and was given with its words.
 *   Nothing but the three outputs is written.
 *
 * K29b mbv_coco_match — COCOeval.evaluateImg for every image, class 0 .. num_labels-1, area range and IoU threshold at once:
 *   inter, pred_area, gt_area as above; scores (N, Q) f32; pred_labels (N, Q) i32, gt_labels (N, G) i32 (a label outside
 *   0 .. num_labels-1 takes no part); iou_thrs (T) f64; area_ranges (A, 2) f64 = [lo, hi] closed; T * A <= 64; max_det >= 1.
 *   Per (image, class): the detections of that label in descending score, ties in index order, the first max_det of them;
 *   a ground truth is ignored iff its area is outside the range; iou = (double)inter / (double)(pred_area + gt_area - inter),
 *   0 for an empty union, compared in f64 with the thresholds as given; a detection tries the free, not ignored ground
 *   truths of its class in index order and the ignored ones only if it found nothing, every comparison `iou >= best` with
 *   best starting at min(threshold, 1 - 1e-10); matched to an ignored ground truth, or unmatched with its own area outside
 *   the range: the detection is ignored.
 *   rank    (N, Q) i32   position in the score order of the class; 2^30 past max_det or without a label in range
 *   matched (N, Q) i64, ignored (N, Q) i64   bit a * T + t: area range a, threshold t
 *   npig    (N, num_labels, A) i32   ground truths of the class that are not ignored
 *   Q, G <= 1024, num_labels <= 65536, else MBV_ERR_UNSUPPORTED.  N == 0: MBV_OK.  Every index comes from the sizes: values
 *   that disagree with them change results, never addresses. */
int mbv_pairwise_mask_overlap(const uint32_t* pred_words, const uint32_t* gt_words, int32_t N, int32_t Q, int32_t G,
                              int64_t words, int32_t* inter, int32_t* pred_area, int32_t* gt_area, void* stream);
int mbv_coco_match(const int32_t* inter, const int32_t* pred_area, const int32_t* gt_area, const float* scores,
                   const int32_t* pred_labels, const int32_t* gt_labels, int32_t N, int32_t Q, int32_t G, int32_t num_labels,
                   const double* iou_thrs, int32_t T, const double* area_ranges, int32_t A, int32_t max_det, int32_t* rank,
                   int64_t* matched, int64_t* ignored, int32_t* npig, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K31 — lift the predicted BEV instances to the points of the scans (csrc/point_lift.hip): per-point query labels, the
 * points of every query and the z-extent of those points.  The reference has no counterpart: its mask_to_pred writes a
 * height of 0.
 *
 * points        (total_points, point_dim) f32, point_dim 3 or 4, the scans concatenated as K1 takes them
 * scan_offsets  (batch + 1) i32 on the device, ascending from 0 to total_points
 * x_min .. gz, prefilter   the voxel geometry of K1 (see its entry above)
 * instance_map  (batch, gy, gx) i32 from K21: row = y-cell, column = x-cell; -1 = none.  A value outside
 *               [-1, num_queries) counts as -1 and is never used as an index.
 * num_queries   <= 1024 (else MBV_ERR_UNSUPPORTED);  z_bins 1 .. 256;  0 <= q_lo <= q_hi <= 1
 * point_query   (total_points) i32: the query that owns the point's BEV cell, or -1.  The cell is computed exactly as K1
 *               computes it (f32 subtract, IEEE f32 divide, floorf, the rejection on all three axes, the strict pre-filter
 *               under `prefilter`): a point K1 would drop gets -1.
 * counts        (batch, num_queries) i32: lifted points per query
 * z_extent      (batch, num_queries, 4) f32: z_min, z_max, z_lo, z_hi of a query's points; four zeros without a point.
 *               With bw = (z_max - z_min) / (float)z_bins of the GEOMETRY, bin(z) = clamp((int)floorf((z - z_min) / bw), 0,
 *               z_bins - 1), rank(q) = clamp((int64)floorf(q * (float)(n - 1)), 0, n - 1) and k(r) the first bin whose
 *               cumulative count exceeds r:  z_lo = z_min + (float)k(rank(q_lo)) * bw,  z_hi = z_min + (float)(k(rank(q_hi))
 *               + 1) * bw, each clamped into [z_min, z_max] of the query's own points.  f32 and integer operations only, one
 *               rounding per operation.
 * workspace     the byte count the _workspace_bytes entry returns (0 for sizes out of range): the encoded extremes and the
 *               (batch, num_queries, z_bins) i32 histogram.
 * Every element of the three outputs is written; nothing has to be pre-set.  Three launches (initialise; one thread per
 * point, blocks of 256, grid.y = batch, per-block LDS aggregation flushed with integer atomics; finalise), integer atomics
 * only: bit-deterministic.  No host synchronisation.
 * batch * num_queries == 0: MBV_OK, a non-NULL point_query filled with -1.  total_points == 0: MBV_OK, non-NULL counts and
 * z_extent filled with zeros.  MBV_ERR_BAD_ARG: a null pointer, point_dim other than 3 or 4, a grid size < 1, z_bins or the
 * quantiles out of range;  MBV_ERR_UNSUPPORTED: num_queries > 1024, batch > 65535, total_points >= 2^31 - 1;
 * MBV_ERR_WORKSPACE: a workspace that is too small.
 */
size_t mbv_lift_instances_workspace_bytes(int32_t batch, int32_t num_queries, int32_t z_bins);
int mbv_lift_instances(const float* points, int32_t point_dim, int64_t total_points, const int32_t* scan_offsets,
                       int32_t batch, float x_min, float y_min, float z_min, float x_max, float y_max, float z_max, float vx,
                       float vy, float vz, int32_t gx, int32_t gy, int32_t gz, int32_t prefilter, const int32_t* instance_map,
                       int32_t num_queries, int32_t z_bins, float q_lo, float q_hi, int32_t* point_query, int32_t* counts,
                       float* z_extent, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K35 — a ground height for every BEV cell from the scan itself, and K31's lift restricted to the returns above it
 * (csrc/point_lift.hip, built with -ffp-contract=off; the numpy restatement of the words below is tests/ground_ref.py).
 * A BEV mask is a footprint: K31 labels the road returns inside it too.  K35a estimates the ground under every cell as the
 * lowest return nearby, K35b keeps a point's query only when the point stands clear of that height.
 *
 * K35a — mbv_ground_map.  points, point_dim, total_points, scan_offsets, batch, x_min .. gz, prefilter: as in K31.
 * radius        cells, 0 .. 32;  z_floor f32, may be -inf
 * A point TAKES PART iff K1's cell rule accepts it — the arithmetic of K31's point_query, the same device function: separate
 * IEEE f32 subtract and divide, floorf, the rejection on all three axes, the strict pre-filter first under `prefilter`; NaN
 * fails every compare — and, in addition, z >= z_floor (a NaN z_floor lets no point take part).
 * cell_min      (batch, gy, gx) f32, row = y-cell, column = x-cell (the layout of instance_map): the minimum z of the points
 *               that take part in the cell, +inf for a cell without one.  The minimum is taken on the order-preserving u32
 *               encoding of K31 (negative numbers: all bits flipped; others: the sign bit set) with integer atomicMin, so
 *               -0.0 < +0.0 and the result does not depend on the order of the points.
 * ground        (batch, gy, gx) f32: the minimum — on the same encoding — of cell_min over cy' in [max(0, cy - radius),
 *               min(gy - 1, cy + radius)] and cx' likewise; +inf when the whole window is empty.  radius = 0: ground ==
 *               cell_min.
 * workspace     the byte count the _workspace_bytes entry returns (0 for sizes out of range): two (batch, gy, gx) u32 planes,
 *               the encoded cell minima and their row-window minima.
 * Every element of both outputs and of the workspace is written by a kernel; nothing has to be pre-set.  Four launches
 * whatever the batch (initialise; one thread per point, integer atomicMin; the window minimum along x; along y), three
 * when total_points == 0 (both maps are +inf then).  The two window passes work on tiles of 64 x 16 and 64 x 64 cells staged
 * in LDS with a halo of `radius` cells: no cell is read from memory more than once per tile that needs it.  16-byte accesses
 * when gx is a multiple of 4 and the outputs and the workspace are 16-byte aligned, dword accesses otherwise (one condition
 * for every path).  Bit-deterministic.  No host synchronisation, no allocation.
 * batch == 0: MBV_OK, nothing is written.  MBV_ERR_UNSUPPORTED: radius > 32, batch > 65535, total_points >= 2^31 - 1, gx or
 * gy > 65536;  MBV_ERR_BAD_ARG: a negative size, radius < 0, point_dim other than 3 or 4, a grid size < 1, a null output,
 * null points or scan_offsets with total_points > 0;  MBV_ERR_WORKSPACE: a workspace that is too small.
 *
 * K35b — mbv_lift_instances_ground: K31 with a ground map.  All arguments of mbv_lift_instances, and
 * ground        (batch, gy, gx) f32, K35a's (or any map of that layout)
 * clearance, max_height   f32; max_height may be +inf
 * q is found exactly as in K31.  With g = ground[b][cy][cx] the point KEEPS q iff  z > g + clearance  and
 * z <= g + max_height, each sum one rounded f32 addition; otherwise it gets -1.  There are no special cases: g = +inf (an
 * empty window) fails the first compare, a NaN anywhere fails both.
 * counts, z_extent        K31's, over the kept points only
 * z_ground      (batch, num_queries) f32: the minimum of g over the kept points of the query, on the integer encoding; 0
 *               for a query without a kept point.
 * The device code is K31's: one kernel body, instantiated with and without the ground.  Launches, determinism, the cases
 * batch * num_queries == 0 and total_points == 0 (z_ground: zeros) and the error codes are K31's; ground and z_ground must
 * not be null when there is work.
 *
 * Not pinned: the defaults of the host API (a window of 1.6 m, a clearance of 0.3 m) rest on geometry — half a car's width
 * plus slack; above road noise and the 8 cm a window minimum loses on a 5 % slope, below a sill — not on measurement.  One
 * return below the road (a multipath reflection) pulls the ground down over its whole window; z_floor is the only defence.
 */
size_t mbv_ground_map_workspace_bytes(int32_t batch, int32_t gx, int32_t gy);
int mbv_ground_map(const float* points, int32_t point_dim, int64_t total_points, const int32_t* scan_offsets, int32_t batch,
                   float x_min, float y_min, float z_min, float x_max, float y_max, float z_max, float vx, float vy, float vz,
                   int32_t gx, int32_t gy, int32_t gz, int32_t prefilter, int32_t radius, float z_floor, float* cell_min,
                   float* ground, void* workspace, size_t workspace_bytes, void* stream);
size_t mbv_lift_instances_ground_workspace_bytes(int32_t batch, int32_t num_queries, int32_t z_bins);
int mbv_lift_instances_ground(const float* points, int32_t point_dim, int64_t total_points, const int32_t* scan_offsets,
                              int32_t batch, float x_min, float y_min, float z_min, float x_max, float y_max, float z_max,
                              float vx, float vy, float vz, int32_t gx, int32_t gy, int32_t gz, int32_t prefilter,
                              const int32_t* instance_map, int32_t num_queries, int32_t z_bins, float q_lo, float q_hi,
                              const float* ground, float clearance, float max_height, int32_t* point_query, int32_t* counts,
                              float* z_extent, float* z_ground, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K36 — BEV frames of scans, predicted instances, tracks and boxes, composed on the device (csrc/render.hip, built with
 * -ffp-contract=off for K36a's cell rule; the plain-loop restatement of the words below is tests/render_ref.py).
 *
 * K36a — mbv_cell_counts.  points, point_dim, total_points, scan_offsets, batch, x_min .. gz, prefilter: as in K31.
 * counts        (batch, gy, gx) i32, row = y-cell, column = x-cell (the layout of instance_map): the points of the scan that
 *               K1's cell rule accepts in the cell — the device function K31 and K35 decide with (csrc/point_cell.hpp).
 * Two launches (zero the table; one thread per point, an integer atomic add), one when total_points == 0.  The result does
 * not depend on the order of the points.  No workspace, no host synchronisation.
 * batch == 0: MBV_OK, nothing is written.  MBV_ERR_UNSUPPORTED: batch > 65535, total_points >= 2^31 - 1, gx or gy > 65536;
 * MBV_ERR_BAD_ARG: a negative size, point_dim other than 3 or 4, a grid size < 1, null counts, null points or scan_offsets
 * with total_points > 0.
 *
 * K36b — mbv_render_bev.  image (batch, H, W, 3) u8 with H = gy * scale, W = gx * scale, scale in 1 .. 8, H and W at most
 * 4096; 4-byte aligned.  Every table below may be null (its layer is then skipped) except image.  Colours passed by value
 * are packed r | g << 8 | b << 16.  For pixel (py, px) of scan b the cell is (cy, cx) = (py / scale, px / scale); the layers
 * apply in this order, in integer arithmetic only:
 *   1. density    c = counts[b][cy][cx] (0 without counts);  level = min(bit_length(max(c, 0)), 15);
 *                 rgb = density_lut[level], density_lut (16, 3) u8.  Without density_lut: rgb = (0, 0, 0), and counts must
 *                 be null.
 *   2. instances  q = instance_map[b][cy][cx], (batch, gy, gx) i32; drawn only for 0 <= q < num_queries.
 *                 id = id_table[b][q] with id_table (batch, num_queries) i32, else q.
 *                 col = palette[id % palette_size] for id >= 0 (palette (palette_size, 3) u8), untracked_rgb for id < 0.
 *                 per channel rgb = (rgb * (256 - alpha) + col * alpha + 128) >> 8, alpha in 0 .. 256.
 *   3. contour    v = gt_map[b][cy][cx], (batch, gy, gx) i32.  The pixel takes gt_rgb iff v != gt_background and at least
 *                 one of the pixels (py, px - 1), (py, px + 1), (py - 1, px), (py + 1, px) lies in a cell whose value is not
 *                 v; a neighbour outside the image counts as gt_background.  A one-pixel inner outline at any scale.
 *   4. boxes      rows box_offsets[b] .. box_offsets[b + 1] - 1 (clamped into [0, num_boxes]; box_offsets (batch + 1) i32) of
 *                 box_corners (num_boxes, 4, 2) i32, (x, y) per corner in HALF-PIXEL units — round(2 * scale * c) of a cell
 *                 coordinate c, made on the host — in order, later rows win.  line in 1 .. 32, half-pixel units.  With the
 *                 pixel centre P = (2 px + 1, 2 py + 1) the pixel takes box_rgb[r] ((num_boxes, 3) u8) iff P is within
 *                 line / 2 of one of the four segments corner k -> corner (k + 1) % 4, decided exactly in 64-bit integers:
 *                 u = B - A, v = P - A, d = u.v, L = u.u;  d <= 0: 4 |v|^2 <= line^2;  d >= L: 4 |P - B|^2 <= line^2;
 *                 otherwise 4 cross(u, v)^2 <= line^2 L (the left side as an unsigned 64-bit number: it can pass 2^63).
 *                 A box with a corner coordinate outside [-16384, 16384] is not drawn and counts in skipped[b] — the bound
 *                 keeps cross^2 below 2^62.  A box whose four corners are equal is a dot of diameter `line`.
 * flip_rows != 0: pixel row py is written to image row H - 1 - py (y up); the layers do not change.
 * skipped       (batch) i32 or null: the boxes of the scan outside the coordinate bound; written for every scan, 0 without
 *               boxes.
 * One launch.  A lane composes four consecutive pixels of the flat (batch * H * W) pixel run and stores them as three dwords,
 * so a row length that is no multiple of 4 bytes needs no scalar head or tail; a workgroup owns 128 x 8 pixels of one scan,
 * stages the scan's boxes in LDS in chunks of mbv_render_box_chunk() rows and rejects each by its bounding box, grown by
 * `line`, against the tile.  No dense (batch, queries, gy, gx) tensor, no workspace, no host synchronisation.
 * batch == 0: MBV_OK, nothing is written.  MBV_ERR_UNSUPPORTED: H or W > 4096, batch > 65535, num_boxes >= 2^31 - 1;
 * MBV_ERR_BAD_ARG: a grid size < 1, scale outside 1 .. 8, a negative size, a null or unaligned image, counts without
 * density_lut, an instance_map without palette (or palette_size < 1, num_queries < 0, alpha outside 0 .. 256), box_corners
 * (with num_boxes > 0) without box_rgb or box_offsets or with line outside 1 .. 32.
 *
 * Not pinned: any speed; profiles/k36 holds what was measured.
 */
int32_t mbv_render_box_chunk(void);
int mbv_cell_counts(const float* points, int32_t point_dim, int64_t total_points, const int32_t* scan_offsets, int32_t batch,
                    float x_min, float y_min, float z_min, float x_max, float y_max, float z_max, float vx, float vy, float vz,
                    int32_t gx, int32_t gy, int32_t gz, int32_t prefilter, int32_t* counts, void* stream);
int mbv_render_bev(int32_t batch, int32_t gx, int32_t gy, int32_t scale, int32_t flip_rows, const int32_t* counts,
                   const uint8_t* density_lut, const int32_t* instance_map, int32_t num_queries, const int32_t* id_table,
                   const uint8_t* palette, int32_t palette_size, int32_t alpha, uint32_t untracked_rgb, const int32_t* gt_map,
                   int32_t gt_background, uint32_t gt_rgb, const int32_t* box_corners, const uint8_t* box_rgb,
                   const int32_t* box_offsets, int64_t num_boxes, int32_t line, uint8_t* image, int32_t* skipped, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K32 — panoptic quality of point or BEV instances (csrc/panoptic.hip): per frame the tp / fp / fn, the IoU sums and the
 * confusion of the SemanticKITTI panoptic protocol, PanopticEval.addBatchPanoptic of semantic-kitti-api's eval_np.py,
 * restated, not repaired.  Parity with that package is not pinned (it is not installed); the numpy restatement in its own
 * formulation is tests/panoptic_ref.py.
 *
 * Elements are the points (or BEV cells) of `frames` frames concatenated.
 * pred_query    (total) i32: the query that owns the element (K31's point_query, K21's flattened instance_map), -1 for
 *               none.  A value outside [0, P) counts as -1 and is never used as an index.
 * gt_word       (total) u32 in the `.label` layout: semantic id in the low, instance id in the high 16 bits
 * frame_offsets (frames + 1) i32 on the device; frame f owns the elements frame_offsets[f] .. frame_offsets[f + 1] - 1,
 *               clamped into [0, total]
 * query_class   (frames, P) i32: the class of every query; a value outside [1, C) turns the query's elements into class 0
 *               with no instance
 * class_lut     (lut_len) i32: semantic id -> class in [0, C), -1 = ignored.  A semantic id >= lut_len, or a table value
 *               outside [-1, C), is ignored and never used as an index.
 * C             classes: 0 = everything else, 1 .. C-1 the thing classes; C <= 16.  P <= 1024.  max_gt in 1 .. 1024: the
 *               ground-truth segments a frame may hold.  min_points >= 0.
 *
 * An ignored element takes part in nothing: it does not count towards the area of the prediction it lies under.
 *   ground-truth segment  the non-ignored elements of a frame that share a thing class and a 16-bit instance id (id 0 is a
 *                         segment like any other); area = elements
 *   prediction segment    the non-ignored elements of a frame that share a query of a thing class; at least one element
 *   pair                  inter = elements in both, counted only where the two classes are equal;
 *                         union = gt_area + pred_area - inter;  iou = (double)inter / (double)union
 *   true positive         iff iou > 0.5 in f64 (inter = 2, union = 4 is none)
 *   per thing class       tp = such pairs, iou_sum = the sum of their IoUs in ascending order of the ground truth's key;
 *                         fn / fp = unmatched ground-truth / prediction segments of the class with area >= min_points
 *
 * frame_stats   (frames, C, 3) i32: tp, fp, fn; the row of class 0 is zeros (no stuff-style PQ)
 * frame_iou     (frames, C) f64: iou_sum
 * confusion     (frames, C, C) i64: [gt class][prediction class] over all non-ignored elements, class 0 included; the
 *               prediction's class is its query's class, else 0
 * n_gt          (frames) i32: the true number of ground-truth segments
 * gt_key        (frames, max_gt) i32: class << 16 | instance, ascending, -1 past the end;  gt_area (frames, max_gt) i32
 * pred_area     (frames, P) i32
 * A frame with n_gt > max_gt gets zeros in frame_stats and frame_iou; its confusion and pred_area stay valid, n_gt reports
 * it, and gt_key / gt_area hold its first max_gt segments.
 * workspace     the byte count the _workspace_bytes entry returns (0 for sizes out of range): per frame a presence bitmap of
 *               C * 65536 bits, its word-prefix counts, and the (max_gt, P) i32 pair table.
 * Every element of the seven outputs is written by the call, nothing has to be pre-set and nothing else is written.  Five
 * launches whatever the number of frames (initialise; mark, one thread per element; index, one workgroup per frame; count,
 * one thread per element with LDS tables per block; match, one workgroup per frame).  Integer atomics only and a fixed
 * order of the f64 sum: bit-deterministic.  No host synchronisation.
 * frames == 0: MBV_OK whatever the pointers are.  Empty frames are fine.  MBV_ERR_UNSUPPORTED: P > 1024, max_gt > 1024,
 * C > 16, frames > 65535, total >= 2^31 - 1;  MBV_ERR_BAD_ARG: a null pointer for a table that has elements, a negative
 * size, C < 1, max_gt < 1, min_points < 0;  MBV_ERR_WORKSPACE: a workspace that is too small.
 */
size_t mbv_panoptic_frames_workspace_bytes(int32_t frames, int32_t P, int32_t max_gt, int32_t C);
int mbv_panoptic_frames(const int32_t* pred_query, const uint32_t* gt_word, int64_t total, const int32_t* frame_offsets,
                        int32_t frames, const int32_t* query_class, int32_t P, const int32_t* class_lut, int32_t lut_len,
                        int32_t C, int32_t max_gt, int32_t min_points, int32_t* frame_stats, double* frame_iou,
                        int64_t* confusion, int32_t* n_gt, int32_t* gt_key, int32_t* gt_area, int32_t* pred_area,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K33a — the tracker step (csrc/track.hip): BEV instance maps of consecutive frames of ONE sequence are associated after
 * ego-motion compensation, so that an object keeps one global id.  Built with -ffp-contract=off; the numpy restatement of
 * the words below is tests/track_ref.py.  The motion model (K37, below) is off by default: in this step a moving object is
 * matched only while its footprints of consecutive frames overlap.
 *
 * Grid           H = ny rows, W = nx columns, the layout of Predictions.instance_map[b]; x_lo, y_lo, voxel f64.  Cell
 *                (iy, ix) has the centre x = x_lo + (ix + 0.5) * voxel, y = y_lo + (iy + 0.5) * voxel.
 * State          owned by the caller, on the device: state_map (H, W) i32, a local track index in [0, n_live) or -1;
 *                live_id (P) i32, the global id; live_seen (P) i32, the frame counter at the last match; counters (4) i32 =
 *                [n_live, next_id, frame, dropped].  A fresh tracker: the map filled with -1, the counters 0.  A stored
 *                n_live outside [0, P] is clamped into it.
 * One frame      instance_maps (F, H, W) i32: a query in [0, Q) or -1; any other value counts as -1 and is never used as
 *                an index.  prev_from_cur (F, 2, 3) f64 row-major on the device: m00 m01 m02 / m10 m11 m12.
 *                Q <= P <= 1024, H * W <= 1024 * 1024, min_iou f64, max_age >= 0, min_cells >= 1.
 *
 * 1. warp    for every current cell centre, in f64 with one rounding per operation:
 *            xp = (m00 * x + m01 * y) + m02, yp = (m10 * x + m11 * y) + m12, jx = floor((xp - x_lo) / voxel), jy likewise;
 *            warped[iy, ix] = state_map[jy, jx] when 0 <= jx < W and 0 <= jy < H, else -1 (NaN and inf fall under the
 *            else); a stored index outside [0, n_live) counts as -1.
 * 2. count   area_q[q] = cells of the instance map equal to q, area_t[t] = cells of warped equal to t, inter[q, t] = cells
 *            where both hold.  A query is present iff area_q[q] >= min_cells; the cells of a query that is not present
 *            count as empty from here on.
 * 3. match   greedy and exact.  Candidates: (q, t) with q present, inter > 0 and (double)inter / (double)union >= min_iou,
 *            union = area_q + area_t - inter (inter = 1, union = 2 at min_iou = 0.5 is one).  Order: IoU descending,
 *            compared as inter_a * union_b against inter_b * union_a in i64; ties to the smaller q, then the smaller t.
 *            Walk the order and take a pair when neither its q nor its t is taken.
 * 4. update  the new live list: the present queries in ascending q — a matched one inherits live_id[t], an unmatched one
 *            takes next_id and increments it; both get seen = frame.  Then the unmatched old tracks in ascending t: one
 *            with frame - live_seen[t] <= max_age is appended with its id and seen unchanged while the list holds fewer
 *            than P entries, otherwise dropped is incremented; older tracks vanish silently.  The new state_map of a cell:
 *            the new index of its present query, else the new index of its warped track if that track was appended, else
 *            -1 (a matched track's cells outside its query are released).  frame is incremented.  live_id and live_seen
 *            past the new n_live are -1.
 *
 * query_track    (F, Q) i32: the global id, -1 when the query is not present
 * track_map      (F, H, W) i32 or NULL: the global id on the cells of present queries, else -1
 * workspace      the byte count the _workspace_bytes entry returns (0 for sizes out of range): the warped map, the two area
 *                tables, the (Q, P) intersection table, a candidate list of Q * P pairs and two index tables.
 * mbv_track_frames steps through the F frames in order: four launches per frame (clear; count, one thread per cell with the
 * areas summed in LDS per block; match and update, ONE workgroup; paint, one thread per cell), enqueued on the stream, never
 * synchronised.  Integer atomics only: bit-deterministic.  Every element of query_track, track_map and of the new state is
 * written by the call; nothing has to be pre-set.
 * F == 0: MBV_OK whatever the pointers are.  MBV_ERR_UNSUPPORTED: Q > P, P > 1024, H * W > 1024 * 1024;  MBV_ERR_BAD_ARG: a
 * null pointer for a table that has elements, a negative size, min_cells < 1, max_age < 0;  MBV_ERR_WORKSPACE: a workspace
 * that is too small.
 */
size_t mbv_track_frames_workspace_bytes(int32_t H, int32_t W, int32_t Q, int32_t P);
int mbv_track_frames(const int32_t* instance_maps, const double* prev_from_cur, int32_t F, int32_t H, int32_t W, double x_lo,
                     double y_lo, double voxel, int32_t Q, int32_t P, double min_iou, int32_t max_age, int32_t min_cells,
                     int32_t* state_map, int32_t* live_id, int32_t* live_seen, int32_t* counters, int32_t* query_track,
                     int32_t* track_map, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K37 — the tracker step with a constant-velocity motion model and gated re-association (csrc/track.hip).  K33a's step with
 * a prediction in front of it and a second matching stage behind it; mbv_track_frames is unchanged and stays the default.
 * The numpy restatement of the words below is tests/track_motion_ref.py.  All f64 arithmetic takes one rounding per
 * operation, in the order written (-ffp-contract=off); division and rint only, no sqrt, no transcendental function.
 *
 * State          K33a's, and a motion record owned by the caller, on the device: pos (P, 2) f64, the centroid of every live
 *                track in metres, x then y, in the coordinates of the frame last processed; vel (P, 2) f64, metres per
 *                frame in the same coordinates — the ego motion is compensated, so this is motion over ground in sensor
 *                axes; motion_counters (2) i32 = [gated, reserved 0].  A fresh record is all zeros.
 * One frame      K33a's inputs, and cur_from_prev (F, 2, 3) f64 = n, the inverse of prev_from_cur = m (n00 n01 n02 / n10 n11
 *                n12); gain f64 in [0, 1]; gate f64 >= 0 in metres, 0 switches step 3b off; max_shift i32 >= 0 in cells.
 *
 * 0. advect  every live track t gets an integer cell shift sx = rint(vel[t].x / voxel), sy = rint(vel[t].y / voxel); if
 *            !(fabs(sx) <= max_shift && fabs(sy) <= max_shift), tested in f64 before any conversion, both are 0 (NaN and
 *            inf give 0).  moved (H, W) starts at -1; every cell (iy, ix) of state_map that holds t in [0, n_live) writes t
 *            to (iy + sy, ix + sx) when that lies inside the grid; where several tracks land on one cell the smallest t
 *            wins.  A pure integer translation leaves no holes.
 * 1 – 3.     K33a's warp, count and match word for word, reading moved instead of state_map.  The count also keeps
 *            sum_ix[q], sum_iy[q] (i64) over the cells of q; for a present query
 *            c_q.x = x_lo + ((double)sum_ix / (double)area_q + 0.5) * voxel, c_q.y = y_lo + ((double)sum_iy / (double)area_q
 *            + 0.5) * voxel.
 * 3b. gate   for every live t: a = pos[t] + vel[t]; pred[t].x = (n00 * a.x + n01 * a.y) + n02, pred[t].y = (n10 * a.x +
 *            n11 * a.y) + n12; velr[t].x = n00 * vel.x + n01 * vel.y, velr[t].y = n10 * vel.x + n11 * vel.y.  When gate > 0:
 *            candidates are the pairs (q, t) with q present and unmatched after step 3, t live and untaken, and
 *            d2 = dx * dx + dy * dy <= gate * gate, dx = c_q.x - pred[t].x, dy = c_q.y - pred[t].y (NaN fails the
 *            comparison).  Order: d2 ascending as f64; ties to the smaller q, then the smaller t.  Walk the order and take
 *            a pair when neither its q nor its t is taken.  motion_counters[0] += the pairs taken here.
 * 4. update  the live list, the ids, seen, dropped, state_map, track_map and query_track follow K33a's step 4 with warped
 *            from moved (so a coasting track's footprint coasts with it) and a pair of either stage counting as a match.
 *            The new list's entries: a present query matched to t: pos' = c_q, vel' = velr[t] + gain * (c_q - pred[t]) per
 *            component (subtract, multiply, add); a born query: pos' = c_q, vel' = 0; an appended unmatched track:
 *            pos' = pred[t], vel' = velr[t].  A component of vel' that is not finite is stored as 0.0.  pos and vel past
 *            the new n_live are 0.0.
 *
 * query_velocity (F, Q, 2) f64: vel' of a present query's track, 0.0 for a query that is not present
 * Identity       with gain = 0 and gate = 0 every velocity stays 0, every shift is 0 and moved == state_map on valid
 *                indices: query_track, track_map, state_map, live_id, live_seen and counters equal mbv_track_frames' bit
 *                for bit.
 * Limits         shifts are whole cells, so a coasting track's footprint drifts by up to half a cell per frame against its
 *                pos; step 3b can hand a lost track to another detection within gate of its prediction.
 * workspace      K33a's, the advected map, the two index sums, the shifts, and c_q, pred and velr.
 * mbv_track_frames_motion steps through the F frames in order, five launches per frame (clear, which also clears moved and
 * the index sums and computes the shifts; advect, one thread per cell, an unsigned atomicMin on a map of all-ones; count,
 * one thread per cell, the index sums per block in LDS and then 64-bit global integer atomics; match + gate + update, ONE
 * workgroup, the same mutual-best rounds under both orders; paint), enqueued on the stream, never synchronised.  Integer
 * atomics only: bit-deterministic.  Every output element and every element of the new state and motion record is written by
 * the call.  Every index comes from the sizes.
 * Error codes as mbv_track_frames; in addition MBV_ERR_BAD_ARG: gain outside [0, 1] or not finite, gate < 0 or not finite,
 * max_shift < 0, a null cur_from_prev or motion_counters, null pos / vel when P > 0, null query_velocity when Q > 0.
 */
size_t mbv_track_frames_motion_workspace_bytes(int32_t H, int32_t W, int32_t Q, int32_t P);
int mbv_track_frames_motion(const int32_t* instance_maps, const double* prev_from_cur, const double* cur_from_prev, int32_t F,
                            int32_t H, int32_t W, double x_lo, double y_lo, double voxel, int32_t Q, int32_t P, double min_iou,
                            int32_t max_age, int32_t min_cells, double gain, double gate, int32_t max_shift, int32_t* state_map,
                            int32_t* live_id, int32_t* live_seen, int32_t* counters, double* pos, double* vel,
                            int32_t* motion_counters, int32_t* query_track, int32_t* track_map, double* query_velocity,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K38 — BEV visibility maps and occlusion-aware track ageing.  K38a says which BEV cells a scan could observe at the height
 * one asks about; K38b is the first consumer: K37's tracker step in which a track that goes unmatched while most of its
 * footprint was out of sight does not age.  Both are opt-in; mbv_track_frames and mbv_track_frames_motion are unchanged.
 * The numpy restatements of the words below are tests/visibility_ref.py and tests/track_occlusion_ref.py.
 *
 * K38a — mbv_visibility_map (csrc/visibility.hip, built with -ffp-contract=off).  points, point_dim, total_points,
 * scan_offsets, batch, x_min .. gz, prefilter: as in K31 / K35a / K36a.
 * origin_cx, origin_cy   i32: the sensor's cell, made on the host; it may lie outside the grid; |value| <= 2^20
 * origin_z, z_top        f32, in the scan's frame: the sensor's height and the roof height of the objects one asks about
 * vis           (batch, gy, gx) u8, row = y-cell, column = x-cell (the layout of instance_map): bit 0 PASSED, bit 1 HIT.
 *               Every element is written.
 *
 * 1. targets    a cell is a target iff at least one point TAKES PART in it: K1's cell rule, the device function of K31 / K35a
 *               / K36a (csrc/point_cell.hpp), the strict pre-filter first under `prefilter`.  Its z_end is the minimum z of
 *               those points on K31's order-preserving u32 encoding (so -0.0 < +0.0): K35a's cell_min with radius 0 and no
 *               floor, the same pass (csrc/cell_min.hpp).  A target cell gets HIT.
 * 2. ray        for a target (ty, tx): dx = tx - origin_cx, dy = ty - origin_cy, n = max(|dx|, |dy|).  Sample k in [0, n) is
 *               the cell (origin_cy + floor_div(2 * k * dy + n, 2 * n), origin_cx + floor_div(2 * k * dx + n, 2 * n)), in
 *               64-bit integers, floor_div rounding towards minus infinity.  n = 0 has no samples; the target's own cell
 *               (k = n) is none.  Samples outside the grid are skipped.
 * 3. height     sample k certifies its cell iff  (z_end - origin_z) * (float)k <= (z_top - origin_z) * (float)n,  each side
 *               one f32 subtraction and one f32 multiplication, in that order; a NaN fails.  Certified cells get PASSED.
 * In words: a beam marks the part of its path on which it ran at or below z_top.  Close to a roof-mounted sensor that part
 * is empty: the beams are still above the roofs there.
 *
 * workspace     the byte count the _workspace_bytes entry returns (0 for sizes out of range): one (batch, gy, gx) u32 plane,
 *               the encoded cell minima.
 * Four launches whatever the batch (initialise; one thread per point, integer atomicMin; the rays; the HIT bit).  The rays: a
 * block of 256 threads owns 256 consecutive cells, scans the ray lengths of its targets in LDS and walks the samples of all
 * of them with consecutive lanes on consecutive samples, so rays of 0 and of 700 cells load the lanes alike; a certified
 * cell takes a plain store of the byte 1, and the HIT bit is added by the one thread that owns the cell in the last launch.
 * Integer atomics and idempotent stores only: the result does not depend on the order of points or rays.  No host
 * synchronisation, no allocation.
 * batch == 0: MBV_OK, nothing is written.  total_points == 0: vis is all zeros (one fill; no workspace is needed).
 * MBV_ERR_UNSUPPORTED: batch > 65535, total_points >= 2^31 - 1, gx or gy > 65536;  MBV_ERR_BAD_ARG: a negative size,
 * point_dim other than 3 or 4, a grid size < 1, |origin_cx| or |origin_cy| > 2^20, null vis, null points or scan_offsets with
 * total_points > 0;  MBV_ERR_WORKSPACE: a workspace that is too small.
 * Limits        z_top is absolute in the sensor frame, not relative to K35's ground; returns outside the grid cast no rays;
 *               one ray per cell, to its lowest return; the blind ring next to the sensor is neither PASSED nor HIT.
 *
 * K38b — mbv_track_frames_occluded (csrc/track.hip): mbv_track_frames_motion with
 * visibility          (F, H, W) u8 or NULL: K38a's map of every frame (any non-zero byte counts as seen)
 * live_held           (P) i32 state: the frames a live track has been held since its last match; a fresh tracker: zeros
 * occlusion_counters  (2) i32 state = [held, reserved 0]
 * hold_num, hold_den  i32, 0 < hold_num <= hold_den: the share of a footprint that must be hidden
 * max_hold            i32 >= 0: the most frames in a row a track is held
 * and these additions to K37's steps:
 * 2. count   also hidden[t] = the cells where warped == t and visibility[f][iy][ix] == 0 (0 for every t without a map).
 * 4. update  an unmatched old track t, in ascending t, is OCCLUDED iff visibility != NULL and area_t[t] > 0 and
 *            (int64)hidden[t] * hold_den >= (int64)area_t[t] * hold_num and live_held[t] < max_hold.  An occluded track takes
 *            seen' = live_seen[t] + 1 and held' = live_held[t] + 1, and occlusion_counters[0] is incremented; otherwise
 *            seen' = live_seen[t] and held' = live_held[t].  The age test frame - seen' <= max_age, the capacity rule and
 *            dropped are K33a's with seen'; an appended track stores seen' and held'.  Matched and born entries get
 *            held' = 0; live_held past the new n_live is 0.  pos and vel of a held track follow K37's "appended unmatched
 *            track" line: it coasts.
 * Identity   with visibility == NULL or max_hold == 0 no track is ever occluded: every output and every state element equals
 *            mbv_track_frames_motion's bit for bit and live_held stays all 0; with gain = gate = 0 in addition they equal
 *            mbv_track_frames'.
 * Limits     a track in the blind ring next to the sensor, or anywhere no beam passed below z_top, counts as hidden and is
 *            held up to max_hold frames; nothing is claimed about LSTQ on real data.
 * workspace  K37's and the hidden table.  Five launches per frame, K37's: the count and match kernels are the third
 * instantiation of the same two templates (hidden is summed per block in LDS, then integer global atomics).  Integer
 * atomics only: bit-deterministic.  Every output element and every element of the new state is written by the call.
 * Error codes as mbv_track_frames_motion; in addition MBV_ERR_BAD_ARG: hold_num < 1, hold_num > hold_den, max_hold < 0, null
 * occlusion_counters, null live_held when P > 0.
 */
size_t mbv_visibility_map_workspace_bytes(int32_t batch, int32_t gx, int32_t gy);
int mbv_visibility_map(const float* points, int32_t point_dim, int64_t total_points, const int32_t* scan_offsets,
                       int32_t batch, float x_min, float y_min, float z_min, float x_max, float y_max, float z_max, float vx,
                       float vy, float vz, int32_t gx, int32_t gy, int32_t gz, int32_t prefilter, int32_t origin_cx,
                       int32_t origin_cy, float origin_z, float z_top, uint8_t* vis, void* workspace, size_t workspace_bytes,
                       void* stream);
size_t mbv_track_frames_occluded_workspace_bytes(int32_t H, int32_t W, int32_t Q, int32_t P);
int mbv_track_frames_occluded(const int32_t* instance_maps, const double* prev_from_cur, const double* cur_from_prev,
                              const uint8_t* visibility, int32_t F, int32_t H, int32_t W, double x_lo, double y_lo,
                              double voxel, int32_t Q, int32_t P, double min_iou, int32_t max_age, int32_t min_cells,
                              double gain, double gate, int32_t max_shift, int32_t hold_num, int32_t hold_den,
                              int32_t max_hold, int32_t* state_map, int32_t* live_id, int32_t* live_seen, int32_t* live_held,
                              int32_t* counters, double* pos, double* vel, int32_t* motion_counters,
                              int32_t* occlusion_counters, int32_t* query_track, int32_t* track_map, double* query_velocity,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K33b — tube association (csrc/track.hip): the S_assoc term of LSTQ (Aygün et al., 4D Panoptic LiDAR Segmentation) over a
 * whole sequence, from per-element track ids and `.label` words.  Parity with semantic-kitti-api's 4D evaluator is not
 * pinned (it is not installed); the restatement is tests/track_ref.py.
 *
 * mbv_tube_accumulate adds `total` elements (points or cells) to tables that persist on the device; the caller zeroes them once.
 * pred_track    (total) i32: the global track id, -1 (or any negative value) = none
 * gt_word       (total) u32 in the `.label` layout; class_lut / lut_len / C exactly as in K32 (-1 = ignored, C <= 16)
 * id_limit I    (1 .. 65536) and max_tracks T (1 .. 2^20), with (C - 1) * I * T < 2^31 - 1
 * An ignored element takes part in nothing.  A ground-truth tube is a thing class c >= 1 with an instance id in [1, I); its
 * row is r = (c - 1) * I + inst; instance id 0 is no tube.
 * gt_size       ((C - 1) * I) i64 += 1 for every element of the tube
 * pred_size     (T) i64 += 1 for every non-ignored element with 0 <= p < T, class-agnostic
 * pair          ((C - 1) * I, T) i32 += 1 where both hold
 * overflow      (2) i64: [0] += non-ignored thing elements with an instance id >= I; [1] += non-ignored elements with a
 *               track id >= T
 * The two size tables are summed in LDS per block where they have at most 4096 entries.  total == 0: MBV_OK.
 *
 * mbv_tube_scores, one workgroup per row: with g = gt_size[r] > 0,
 *   assoc[r] = (sum over p ascending with pair > 0 of (double)tpa * ((double)tpa / (double)(g + pred_size[p] - tpa))) / (double)g
 * summed in that fixed order, one rounding per operation; otherwise assoc[r] = 0.
 * assoc         ((C - 1) * I) f64;  class_assoc (C) f64: the sum of the class's rows with g > 0 in ascending order (class 0:
 *               0);  class_tubes (C) i32: those rows' number.
 * Neither synchronises.  MBV_ERR_UNSUPPORTED beyond the limits, total >= 2^31 - 1;  MBV_ERR_BAD_ARG: a null table that has
 * elements, a negative size, C < 1, I < 1, T < 1.
 */
int mbv_tube_accumulate(const int32_t* pred_track, const uint32_t* gt_word, int64_t total, const int32_t* class_lut,
                        int32_t lut_len, int32_t C, int32_t id_limit, int32_t max_tracks, int64_t* gt_size, int64_t* pred_size,
                        int32_t* pair, int64_t* overflow, void* stream);
int mbv_tube_scores(const int64_t* gt_size, const int64_t* pred_size, const int32_t* pair, int32_t C, int32_t id_limit,
                    int32_t max_tracks, double* assoc, double* class_assoc, int32_t* class_tubes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K39 — tracked BEV footprints fused over time in a rolling world grid (csrc/fuse.hip, built with -ffp-contract=off).  The
 * tracker (K33a / K37 / K38b) remembers which id an object has; K39a remembers where its cells were: per-cell evidence in a
 * world-anchored store that scrolls by whole cells, so memory is never re-sampled.  Opt-in; nothing else changes.  The numpy
 * restatement of the words below is tests/fuse_ref.py.  All f64 arithmetic takes one rounding per operation, in the order
 * written: (a * x + b * y) + c and (p - lo) / v.
 *
 * K39a — mbv_fuse_frames.
 * Grid           K33a's: H rows, W columns, x_lo, y_lo, voxel = v f64; H * W <= 1024 * 1024; Q <= 1024.
 * State          owned by the caller, on the device, for ONE sequence: owner (S, S) i32, the global track id that owns a store
 *                cell, -1 for none; count (S, S) i32, its evidence in [0, cap]; window (4) i64 = [wx0, wy0, frames, reserved
 *                0].  A fresh state: window all zeros; owner and count may hold anything (frames == 0 clears them).  S is
 *                even, (S - 4)^2 >= H^2 + W^2 (S >= ceil(hypot(H, W)) + 4: the rotated grid fits whatever the heading) and
 *                S <= 8192.
 * World frame    the sensor frame of the first frame after a reset.  World cell (gx, gy) = (floor(X / v), floor(Y / v)) as
 *                i64 lives at store[gy mod S][gx mod S], the mathematical mod; the window is gx in [wx0, wx0 + S), gy in [wy0,
 *                wy0 + S).  Store cell (sy, sx) under a corner (wx0, wy0) represents gx = wx0 + ((sx - wx0) mod S), gy likewise.
 * One frame      instance_maps (F, H, W) i32: the query per cell, a value outside [0, Q) means none; query_track (F, Q) i32
 *                from the tracker, < 0: the query is not present; world_from_cur = m and cur_from_world = n (F, 2, 3) f64
 *                row-major, inverses of each other; visibility (F, H, W) u8 or NULL (K38a's, non-zero = seen);
 *                query_velocity (F, Q, 2) f64 or NULL (K37's); cap >= 1, hit >= 1, miss >= 0, min_count >= 1 i32;
 *                static_speed f64 >= 0.
 * Moving         query q is MOVING iff query_velocity != NULL and vx * vx + vy * vy > static_speed * static_speed (a NaN on
 *                either side fails: not moving).
 *
 * 1. window  (cx, cy) = (x_lo + (W * 0.5) * v, y_lo + (H * 0.5) * v); X = (m00 * cx + m01 * cy) + m02, Y likewise;
 *            wx0' = floor(X / v) - S / 2, wy0' = floor(Y / v) - S / 2.  The frame is INVALID iff any of the twelve entries of m
 *            and n is not finite or !(|X / v| < 2^40 && |Y / v| < 2^40): state and window stay untouched, fused_ids and
 *            fused_queries of the frame are -1.  Otherwise a store cell is cleared (owner -1, count 0) iff frames == 0 or the
 *            world cell it represents under (wx0', wy0') differs from the one under (wx0, wy0).
 * 2. update  one gather per store cell, its world cell (gx, gy) under the new corner: x = ((double)gx + 0.5) * v, y likewise;
 *            xs = (n00 * x + n01 * y) + n02, ys = (n10 * x + n11 * y) + n12; fx = floor((xs - x_lo) / v), fy = floor((ys - y_lo)
 *            / v).  Unless 0 <= fx < W and 0 <= fy < H (NaN and inf fail): hold.  Else q = instance_maps[f][fy][fx]:
 *              q in [0, Q) and MOVING                         hold
 *              q in [0, Q), g = query_track[f][q] >= 0, owner == g    count = min(count + hit, cap)
 *              ...                                 owner != g    count -= hit; if count <= 0: owner = g, count = hit
 *              no detection (q outside [0, Q) or g < 0), cell seen (visibility == NULL or visibility[f][fy][fx] != 0)
 *                                                             count -= miss; if count <= 0: owner = -1, count = 0
 *              no detection, cell not seen                    hold
 *            (count is stepped in 64-bit integers and stored as i32.)
 * 3. read    one gather per sensor cell (iy, ix), q = instance_maps[f][iy][ix]: if q in [0, Q) is MOVING and query_track[f][q]
 *            >= 0, fused_ids = that id and fused_queries = q.  Otherwise x = x_lo + (ix + 0.5) * v, y likewise, X = (m00 * x +
 *            m01 * y) + m02, Y likewise, gx = floor(X / v), gy = floor(Y / v); if wx0' <= gx < wx0' + S and wy0' <= gy <
 *            wy0' + S (compared in f64; NaN and inf fail) and the store cell has owner >= 0 and count >= min_count: fused_ids =
 *            owner and fused_queries = the smallest q in [0, Q) that is not MOVING with query_track[f][q] == owner, -1 when
 *            there is none.  Otherwise both are -1.  Then window = [wx0', wy0', frames + 1, 0].
 *
 * fused_ids      (F, H, W) i32;  fused_queries (F, H, W) i32 or NULL.  Every element is written.
 * Identity       with cap = hit = miss = min_count = 1, no visibility, no velocity, identity poses and x_lo, y_lo multiples
 *                of v, fused_ids equals mbv_track_frames' track_map on maps whose present queries are the ones with an id.
 * Limits         moving objects are passed through, not accumulated; both gathers are nearest-cell, so a footprint seen
 *                under a turning ego loses and gains border cells; the id of a track that died persists under cells nobody
 *                sees until the window leaves them; z is ignored.
 * mbv_fuse_frames steps through the F frames in order, two launches per frame (window + update, one thread per store cell;
 * read-out, one thread per sensor cell with the frame's Q ids in LDS; its first thread writes the window, which no other
 * thread of that launch reads), enqueued on the stream, never synchronised, no workspace.  No atomics: both steps are pure
 * gathers, bit-deterministic.  Every index comes from the sizes: a bad pose, id or stored value changes results, never
 * addresses (a stored corner is the call's own: |wx0|, |wy0| < 2^41).
 * F == 0 or H * W == 0: MBV_OK, nothing is written.  MBV_ERR_UNSUPPORTED: S odd, too small or > 8192, Q > 1024, H * W >
 * 1024 * 1024;  MBV_ERR_BAD_ARG: a negative size, cap < 1, hit < 1, miss < 0, min_count < 1, !(static_speed >= 0), voxel not
 * finite or <= 0, a null pointer other than visibility, query_velocity, fused_queries (query_track may be null when Q == 0).
 *
 * K39b — mbv_masks_from_map: a map of query indices back to the masks every consumer of masks_packed reads.
 * maps           (F, H, W) i32: a query in [0, Q) per cell; any other value sets nothing
 * masks_packed   (F * Q, mbv_packed_mask_words(H, W)) u32, mbv_pack_binary_masks layout, row f * Q + q: bit (y * W + x) is
 *                (maps[f][y][x] == q); tail bits zero
 * areas          (F, Q) i32: the set bits of every row
 * Three launches: two fills (masks_packed, areas), then one thread per pixel — a wave ballots every distinct query of its 64
 * pixels and its first lane stores the two words of that query's row (a word of a row has one writer: plain stores) and
 * counts the query's cells in an LDS table that is flushed once per block (integer atomicAdd).
 * Every element of both outputs is written.  F == 0 or Q == 0: MBV_OK, nothing is written.  MBV_ERR_UNSUPPORTED: Q > 1024,
 * F > 65535, H * W > 1024 * 1024;  MBV_ERR_BAD_ARG: a negative size, H < 1 or W < 1, a null pointer.
 */
int mbv_fuse_frames(const int32_t* instance_maps, const int32_t* query_track, const double* world_from_cur,
                    const double* cur_from_world, const uint8_t* visibility, const double* query_velocity, int32_t F, int32_t H,
                    int32_t W, int32_t S, double x_lo, double y_lo, double voxel, int32_t Q, int32_t cap, int32_t hit,
                    int32_t miss, int32_t min_count, double static_speed, int32_t* owner, int32_t* count, int64_t* window,
                    int32_t* fused_ids, int32_t* fused_queries, void* stream);
int mbv_masks_from_map(const int32_t* maps, int32_t F, int32_t H, int32_t W, int32_t Q, uint32_t* masks_packed, int32_t* areas,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * K40 — LAMB and (Nesterov) SGD over the flat parameter arena (csrc/optim_flat.hip, built with -ffp-contract=off; the
 * arithmetic has one definition, csrc/adam.hpp).  Replaces: torch_optimizer.Lamb and torch.optim.SGD built by
 * MaskBevModule.configure_optimizers (mask_bev/mask_bev_module.py:141-151).  Like K11 every pass streams the arena once with
 * 16 B per lane, folds the 16-bit shadow refresh and the gradient clear in, allocates nothing, never synchronises with the
 * host and can be captured in a graph.  All f32 arena arrays are 16-byte aligned, `shadow` (nullable) 8-byte aligned with
 * shadow_dtype = MBV_DT_BF16 / MBV_DT_F16.  grad is multiplied by grad_scale first; loss_scale / skip_flag / applied_steps
 * are K11's device scalars (all nullable): grad is divided by *loss_scale on the fly, and a non-zero *skip_flag means the
 * gradient held inf / nan — parameters, optimizer state and shadow stay as they are and the gradient is cleared.
 *
 * LAMB, per parameter tensor (torch_optimizer 0.3.0 Lamb.step):
 *   m = b1 m + (1 - b1) g        v = b2 v + (1 - b2) g g        u = m / (sqrt(v) + eps) + weight_decay p   (if weight_decay != 0)
 *   wn = min(||p||, clamp_value)   un = ||u||   trust = 1 if wn == 0 or un == 0 else wn / un
 *   p -= lr * bias_correction * trust * u,   bias_correction = sqrt(1 - b2^t) / (1 - b1^t) with debias, else 1
 * The per-tensor norms come from a CHUNK TABLE the caller builds once and keeps on the device: every parameter's padded
 * arena range [off, off + round_up(numel, 64)) cut into chunks of at most 4096 elements, a parameter's chunks consecutive,
 * no chunk straddling two parameters; `chunks` holds n_chunks records (16-byte aligned), `param_chunks` n_params pairs
 * (chunk_begin, chunk_end) of i32 (8-byte aligned).  start and len are multiples of 4, 0 < len <= 4096; a record that breaks
 * this or reaches past n (the arena's element count) is skipped.  Padding elements must be zero in param, grad and both
 * moments; they stay zero.  c0 <= c1 select the chunk range [c0, c1) of a launch (a run of parameter groups that share
 * hyper-parameters).  beta1 / beta2 are f64 so that 1 - beta is rounded to f32 once, from the value the caller means (0.001
 * for 0.999, where 1.0f - 0.999f is 1.3e-5 off) — what torch does with the Python scalar.
 * mbv_lamb_moments: reads param, grad, exp_avg, exp_avg_sq; writes exp_avg, exp_avg_sq and u OVER grad (the gradient buffer
 *   is the stash: mbv_lamb_apply clears it); partials (2, n_chunks) f32 receives, per chunk, the sum of p^2 (row 0) and of
 *   u^2 (row 1), each reduced by one block in a fixed order — no float atomics, so the sums are bit-reproducible.  On a set
 *   skip flag it changes nothing.
 * mbv_lamb_trust: trust[i] (n_params f32) from the partials of parameter i, summed in a fixed order in f64, one block per
 *   parameter.  After a skipped moments pass its output is meaningless (and unused).
 * mbv_lamb_apply: reads param, u (in grad) and trust[param of chunk]; writes param, shadow and zeroes grad.  step >= 1 is the
 *   1-based update count for debias (computed on the host in f64); with debias and applied_steps given, t = *applied_steps + 1
 *   instead.  On a set skip flag it only zeroes grad.
 * mbv_sgd_step: ONE pass over n elements, torch/optim/sgd.py's single-tensor order:
 *   g += weight_decay p (if != 0);  buf = momentum buf + (1 - dampening) g;  g = g + momentum buf if nesterov else buf;
 *   p -= lr g;  shadow refreshed; zero_grad=1 clears grad.  momentum_buf starts at zero, which equals torch's first-step
 *   `buf = g` exactly when dampening == 0.  On a set skip flag only zero_grad is honoured.
 * MBV_ERR_BAD_ARG: a null pointer other than the nullable ones, a misaligned array, a negative size, c0 < 0, c1 < c0,
 *   c1 > n_chunks, step < 1, a beta outside [0, 1), a shadow whose dtype is neither MBV_DT_BF16 nor MBV_DT_F16.
 */
typedef struct mbv_lamb_chunk {
  int64_t start;  /* first arena element of the chunk */
  int32_t len;    /* elements */
  int32_t param;  /* index of its parameter, in arena layout order */
} mbv_lamb_chunk;

int mbv_lamb_moments(const float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                     const mbv_lamb_chunk* chunks, int32_t n_chunks, int32_t c0, int32_t c1, float* partials, double beta1,
                     double beta2, float eps, float weight_decay, float grad_scale, const float* loss_scale,
                     const int32_t* skip_flag, void* stream);
int mbv_lamb_trust(const float* partials, int32_t n_chunks, const int32_t* param_chunks, int32_t n_params,
                   float clamp_value, float* trust, void* stream);
int mbv_lamb_apply(float* param, float* grad, void* shadow, int32_t shadow_dtype, int64_t n, const mbv_lamb_chunk* chunks,
                   int32_t n_chunks, int32_t c0, int32_t c1, const float* trust, int32_t n_params, float lr, double beta1,
                   double beta2, int32_t debias, int64_t step, const int32_t* applied_steps, const int32_t* skip_flag,
                   void* stream);
int mbv_sgd_step(float* param, float* grad, float* momentum_buf, void* shadow, int32_t shadow_dtype, int64_t n, float lr,
                 float momentum, float dampening, float weight_decay, int32_t nesterov, float grad_scale, int32_t zero_grad,
                 const float* loss_scale, const int32_t* skip_flag, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K41 — gradient clipping by global norm for the flat optimizers (csrc/optim_flat.hip).  Replaces:
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2), which Lightning's Trainer(gradient_clip_val=...) runs
 * between backward and optimizer.step().  Two launches measure the norm of the gradient the optimizer will apply,
 * g * grad_scale / *loss_scale, and leave ONE device float, loss_scale / clip_coefficient, which mbv_adamw_step,
 * mbv_adamw_step_ranges, mbv_lamb_moments and mbv_sgd_step take as their `loss_scale` argument: the gradient buffer is never
 * rewritten.  No atomics, no host synchronisation, nothing allocated; both can be captured in a graph.
 *
 * mbv_grad_norm_partials: start / len are HOST arrays of count <= 8 element ranges of the arena gradient `grad` (n elements,
 *   16-byte aligned); starts and lengths are multiples of 4, ranges lie inside [0, n).  Every range is cut into chunks of 4096
 *   elements (the last one shorter); the chunks of range r follow those of range r - 1.  partials (n_partials f64, 8-byte
 *   aligned) receives per chunk the sum of (double)g * (double)g: each thread accumulates its float4s in f64, one block reduces
 *   a chunk in a fixed order — the result does not depend on the grid and is bit-reproducible; a gradient element whose square
 *   overflows f32 is summed right.  n_partials must equal the sum of ceil(len[r] / 4096).  Padding elements inside a range are
 *   summed: they must be zero (ParameterArena's are).
 * mbv_grad_clip_coef: range_chunks is a HOST array of count + 1 chunk boundaries into partials (range_chunks[0] = 0,
 *   non-decreasing, range_chunks[count] = n_partials).  One block sums every range and the total in f64 in a fixed order, then
 *     L = loss_scale ? *loss_scale : 1      total = sqrt(sum) * grad_scale / L      coef = min(1, max_norm / (total + 1e-6))
 *   (all f64 from the f32 inputs; torch's rule) and writes rec (16 f32, 4-byte aligned):  rec[0] = L / coef, rec[1] = total,
 *   rec[2] = coef, rec[3 + r] = sqrt(sum of range r) * grad_scale / L, the rest zero.  max_norm = +inf measures and never
 *   clips: coef is exactly 1 and rec[0] exactly L.  A NaN total gives a NaN coefficient, as torch's.  loss_scale is K11's
 *   device scalar (nullable).
 * n == 0 or count == 0: MBV_OK (mbv_grad_clip_coef then writes norm 0, coefficient 1).  MBV_ERR_UNSUPPORTED: count > 8, more
 *   than 2^31 - 1 chunks;  MBV_ERR_BAD_ARG: a null or misaligned pointer (other than loss_scale), a negative size, a range
 *   outside the arena, a start or length that is no multiple of 4, n_partials or range_chunks that do not match,
 *   max_norm <= 0 or NaN.
 */
int mbv_grad_norm_partials(const float* grad, int64_t n, const int64_t* start, const int64_t* len, int32_t count,
                           double* partials, int32_t n_partials, void* stream);
int mbv_grad_clip_coef(const double* partials, int32_t n_partials, const int32_t* range_chunks, int32_t count, float max_norm,
                       float grad_scale, const float* loss_scale, float* rec, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K43 — averaged weights over the flat arena (csrc/optim_flat.hip).  Replaces: mmengine's EMAHook / timm's ModelEmaV2
 * (torch._foreach_lerp_ over every parameter plus a host-side decay warm-up) and SWA's equal-weight mean
 * (torch.optim.swa_utils.AveragedModel).  `avg` is one more f32 buffer the size of the arena.  No host synchronisation,
 * nothing allocated, capturable in a graph: the counters live in a 16-byte device record and advance on the device.
 *
 * mbv_weight_average_update: TWO launches on `stream`.
 *   tick (one thread), with u = state->updates, c = state->calls:
 *     applied = applied_steps ? (*applied_steps != state->seen) : true;   if applied_steps: state->seen = *applied_steps
 *       (applied_steps is K11's count of applied updates, LossScaler's: mbv_loss_scale_update does not advance it on an
 *       overflowed step, and has already cleared the overflow flag when this runs)
 *     w = 0;  if applied: c += 1; if c % every == 0:
 *       MBV_AVERAGE_MEAN:  w = 1.0f / (float)(u + 1)
 *       MBV_AVERAGE_EMA:   d = warmup ? min(decay, (float)(1 + u) / (float)(10 + u)) : decay;   w = 1.0f - d
 *       u += 1
 *     state->weight = w        (f32 throughout, the divides correctly rounded)
 *   stream (k_sgd's frame: 16-byte non-temporal accesses, grid-stride, ragged tail), every element of [0, n):
 *     w == 0: nothing is read or written;   w == 1: avg = param;   else avg = avg + w * (param - avg), three f32 roundings,
 *     no contraction.  Reads param and avg, writes avg: at most 12 B per element.  param is never written.
 *   The first update of a mean (u = 0) and of an EMA with decay 0 has w = 1: avg takes param bit for bit.
 * mbv_weight_average_swap: param[i] <-> avg[i], and shadow[i] = bf16 / half (RNE) of the new param[i] when shadow is given:
 *   one pass, 16 B per element + 2 B.  Bits are moved: two calls restore param, avg and the shadow exactly.
 * n == 0: MBV_OK, nothing launched (the record does not advance).  MBV_ERR_BAD_ARG: a null param, avg or state, param == avg,
 *   n < 0, param or avg not 16-byte aligned, state or applied_steps not 4-byte aligned, decay outside [0, 1) or NaN, every < 1,
 *   a mode other than the two, a shadow that is not 8-byte aligned or whose dtype is neither MBV_DT_BF16 nor MBV_DT_F16.
 */
#define MBV_AVERAGE_EMA 0
#define MBV_AVERAGE_MEAN 1
typedef struct mbv_weight_average_state {
  int32_t updates; /* u: averaging updates applied */
  int32_t calls;   /* c: applied optimizer steps seen */
  int32_t seen;    /* *applied_steps at the last call */
  float weight;    /* w of the last call; 0 = it did nothing */
} mbv_weight_average_state;

int mbv_weight_average_update(const float* param, float* avg, int64_t n, mbv_weight_average_state* state,
                              const int32_t* applied_steps, int32_t mode, float decay, int32_t warmup, int32_t every,
                              void* stream);
int mbv_weight_average_swap(float* param, float* avg, void* shadow, int32_t shadow_dtype, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K42 — reconciling the kept queries of one decoder output with each other (csrc/resolve.hip): greedy mask NMS and
 * Mask2Former's overlap filter (`panoptic_postprocess`: the per-pixel argmax over the kept queries, a segment dropped when it
 * wins less than OVERLAP_THRESHOLD of its own mask).  The reference's consumers keep every `argmax > 0` query
 * (mask_bev/mask_bev_module.py:286-294, mask_bev/evaluation/kitti_eval.py:27-44).  Integer arithmetic only (comparisons in
 * int64), per frame, no host synchronisation, no workspace, capturable in a graph.  Thresholds are ratios num / den with
 * 1 <= num <= den <= 65535.
 *
 * The rule, between K21a / K21b and their consumers:
 *   N  candidates = queries with keep set, in descending f32 score, ties to the smaller q.  Walking that order, a candidate
 *      not yet suppressed is a survivor; a survivor i suppresses every later, not yet suppressed candidate j with
 *      labels[i] == labels[j] (only with same_label), union = area_i + area_j - inter_ij > 0 and
 *      inter_ij * den >= num * union (equality suppresses): suppressed_by[j] = i, -1 for everybody else;
 *      keep1 = keep & (suppressed_by < 0).  Not transitive: a suppressed candidate suppresses nobody.
 *   M  mbv_extract_masks again on the same logits with keep1, for instance_map only.
 *   F  owned[q] = cells of that map equal to q (0 for q outside keep1); a q of keep1 is dropped iff owned[q] < min_cells or
 *      owned[q] * den < num * areas[q]; one pass, not iterated; the cells of a dropped query become -1 and are not handed to
 *      the next best query.  keep2 is the final keep.
 *   X  (optional) mbv_masks_from_map of the filtered map: disjoint masks, areas == owned on kept queries.
 *
 * K42a mbv_mask_self_overlap — words (B * Q, nwords) u32, mbv_pack_binary_masks layout with tail bits zero, row b * Q + q;
 *   keep (B, Q) u8; inter (B, Q, Q) i32: inter[b][i][j] = popcount(row i & row j) where both are kept — symmetric, the
 *   diagonal is a kept mask's own popcount — and 0 wherever either is not kept.  Rows that are not kept are never read.
 *   Two launches: a fill of inter, then one workgroup per (32 x 32 tile of the frame's KEPT rows in ascending q, tile pairs
 *   with row tile <= column tile only; 512 words of the contraction).  The kept count exists only on the device: the grid
 *   is sized from Q and a workgroup whose tile lies beyond the kept rows leaves after reading keep.  The 64 rows of a pair
 *   of tiles stream through LDS 128 words at a time (16-byte loads where nwords and the base allow), popcounts are taken 64
 *   bits at a time, and the splits of the contraction are joined with integer atomics into both triangles: exact, so
 *   their order does not matter.
 * K42b mbv_mask_nms — stage N from K42a's table (areas = its diagonal), scores (B, Q) f32, labels (B, Q) i32, keep (B, Q)
 *   u8 → keep_out (B, Q) u8 and suppressed_by (B, Q) i32.  One workgroup per frame: the order by counting in LDS, then the
 *   walk, the later candidates tested in parallel between barriers.  A score that does not order (NaN) is skipped by the walk
 *   and stays kept.  keep_out may be keep.
 * K42c mbv_overlap_filter — stage F: instance_map (B, H, W) i32 in and out, areas (B, Q) i32, keep (B, Q) u8 (keep1) →
 *   owned (B, Q) i32, keep_out (B, Q) u8.  num == 0 leaves only the min_cells test.  Three launches: a fill of owned, a
 *   per-workgroup cell histogram in LDS flushed with integer atomics for the queries of keep, then the decision per
 *   workgroup in LDS and the rewrite of its cells: a cell whose value is in [0, Q) and not in keep_out becomes -1 (a query
 *   outside keep included), any other value stays.  keep_out must not be keep: other workgroups still read it.
 * Every element of every output is written by a kernel.  Indices come from the sizes: a label, score or map value out of
 * range changes results, never addresses.
 * B * Q == 0: MBV_OK before any pointer is looked at, nothing is written.  MBV_ERR_UNSUPPORTED: Q > 1024, B > 65535,
 * nwords > 32768, H * W > 1024 * 1024;  MBV_ERR_BAD_ARG: a null pointer, a negative size, H < 1 or W < 1, min_cells < 0, a
 * ratio outside 1 <= num <= den <= 65535 (K42c: 0 <= num).
 */
int mbv_mask_self_overlap(const uint32_t* words, const uint8_t* keep, int32_t B, int32_t Q, int64_t nwords, int32_t* inter,
                          void* stream);
int mbv_mask_nms(const int32_t* inter, const float* scores, const int32_t* labels, const uint8_t* keep, int32_t B, int32_t Q,
                 int32_t num, int32_t den, int32_t same_label, uint8_t* keep_out, int32_t* suppressed_by, void* stream);
int mbv_overlap_filter(int32_t* instance_map, const int32_t* areas, const uint8_t* keep, int32_t B, int32_t H, int32_t W,
                       int32_t Q, int32_t num, int32_t den, int32_t min_cells, int32_t* owned, uint8_t* keep_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MASKBEV_HIP_H_ */
