/*
 * ver_ops.h -- C ABI of the MI355X (gfx950) kernels for VER's 2D->3D lifting path.
 *
 * Drop-in boundary.  The reference (DefaultRui/VLN-VER) is pure Python; the only native
 * entry points on its hot path are two symbols of the third-party mmcv-full 1.4.0 `_ext`
 * library, loaded at
 *   projects/mmdet3d_plugin/bevformer/modules/multi_scale_deformable_attn_function.py:11-12
 * and called at :118-124 (forward) and :150-160 (backward).  `ver_msda_forward` /
 * `ver_msda_backward` below are exactly those two calls with torch tensors replaced by raw
 * device pointers + sizes.  The remaining entry points replace Python/torch code of the
 * reference that sits on the same path (file:line cited per function) with fused kernels.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - buffers are dense, row-major, in the index order written in the comment;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it
 *     (no allocation, no synchronisation, no global state besides the last-error string);
 *   - return value: 0 on success, negative VER_E* on failure; `ver_last_error()` returns a
 *     thread-local description of the last failure;
 *   - dtype: fp32 everywhere (the reference forces fp32 on this op:
 *     multi_scale_deformable_attn_function.py:93 `custom_fwd(cast_inputs=torch.float32)`),
 *     except `value_dtype` where noted (VER_F32 = 0, VER_BF16 = 1: value stored as bf16).
 *     Arithmetic on VER_BF16 value: fp32 everywhere EXCEPT the forward gather's point
 *     accumulation, which is packed fp16 over the <= 8 points of a (voxel, head, corner) and
 *     fp32 after the corner fold -- range and precision contract at `ver_sca_forward`.
 */
#ifndef VER_OPS_H
#define VER_OPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VER_ABI_VERSION 31

#define VER_OK            0
#define VER_EINVAL       -1   /* bad argument (null pointer, non-positive size, ...) */
#define VER_EUNSUPPORTED -2   /* shape outside what the fused kernels are built for   */
#define VER_ELAUNCH      -3   /* HIP reported an error at launch                      */

#define VER_F32  0
#define VER_BF16 1

#define VER_I32  0            /* index dtypes (ver_occ_targets) */
#define VER_I64  1

int         ver_abi_version(void);
const char* ver_last_error(void);

/* ---------------------------------------------------------------------------------------
 * mmcv op boundary: ext_module.ms_deform_attn_forward(value, value_spatial_shapes,
 *   value_level_start_index, sampling_locations, attention_weights, im2col_step)
 *   (multi_scale_deformable_attn_function.py:118-124).
 *
 *   value       f32 [B, num_keys, heads, head_dim]
 *   shapes_hw   i64 [levels, 2]   (h, w) per level            (device, like the reference)
 *   level_start i64 [levels]
 *   loc         f32 [B, Nq, heads, levels, points, 2]   (x, y) normalised to [0,1]
 *   attn_w      f32 [B, Nq, heads, levels, points]
 *   out         f32 [B, Nq, heads*head_dim]              (written, need not be zeroed)
 * out[b,q,h,:] = sum_{l,p} attn_w * bilinear(value_l[b,:,h,:], x = loc_x*W-0.5, y = loc_y*H-0.5),
 * zero outside the map.  `im2col_step` of the reference only batches launches and has no
 * numerical effect; it is accepted and ignored.
 */
int ver_msda_forward(const float* value, const int64_t* shapes_hw, const int64_t* level_start,
                     const float* loc, const float* attn_w, float* out,
                     int B, int num_keys, int heads, int head_dim, int levels, int points,
                     int Nq, int im2col_step, void* stream);

/* ext_module.ms_deform_attn_backward(value, shapes, level_start, loc, attn_w, grad_output,
 *   grad_value, grad_sampling_loc, grad_attn_weight, im2col_step)
 *   (multi_scale_deformable_attn_function.py:150-160).  As in the reference the three
 *   gradient buffers are caller-allocated and ZERO-INITIALISED by the caller (:146-148);
 *   grad_value is accumulated with atomics, grad_loc / grad_attn_w are written.
 */
int ver_msda_backward(const float* value, const int64_t* shapes_hw, const int64_t* level_start,
                      const float* loc, const float* attn_w, const float* grad_out,
                      float* grad_value, float* grad_loc, float* grad_attn_w,
                      int B, int num_keys, int heads, int head_dim, int levels, int points,
                      int Nq, int im2col_step, void* stream);

/* 3-D (trilinear) twin used by the detection decoder: the reference's in-tree
 *   voxel_multi_scale_deformable_attn_pytorch(value, value_spatial_shapes, sampling_locations,
 *   attention_weights) (bevformer/modules/voxel_temporal_self_attention.py:275-335), called from
 *   VoxelCustomMSDeformableAttention.forward (bevformer/modules/voxel_decoder.py:312-313).
 *   shapes_dhw i64 [levels,3] = (D,H,W); loc f32 [B,Nq,heads,levels,points,3] = (x,y,z) in [0,1];
 *   flat key index = (z*H + y)*W + x; 5-D grid_sample semantics (pixel = loc*size - 0.5, zeros).
 *   Gate: a sample contributes -- to out and to every gradient -- only if -1 < pixel < size on EVERY axis (strict both
 *   ways; a NaN fails it).  This differs from grid_sample in one point per axis only: at a pixel coordinate of exactly -1
 *   the corner at 0 has weight 0, so out, grad_value and grad_attn_w are 0 either way, but grid_sample returns a non-zero
 *   location gradient there and these kernels return 0.  The 2-D op above follows mmcv's rule, which is the same strict gate.
 *   (tests/test_msda_forms_cpu.py holds both halves: equality with grid_sample elsewhere, its non-zero gradient at -1.)
 *   Gradient buffers of the backward are caller-allocated and ZERO-INITIALISED: grad_value is accumulated into with
 *   atomics, grad_loc / grad_attn_w are written for every sample (0 outside the gate).
 */
int ver_msda3d_forward(const float* value, const int64_t* shapes_dhw, const int64_t* level_start,
                       const float* loc, const float* attn_w, float* out,
                       int B, int num_keys, int heads, int head_dim, int levels, int points,
                       int Nq, void* stream);
int ver_msda3d_backward(const float* value, const int64_t* shapes_dhw, const int64_t* level_start,
                        const float* loc, const float* attn_w, const float* grad_out,
                        float* grad_value, float* grad_loc, float* grad_attn_w,
                        int B, int num_keys, int heads, int head_dim, int levels, int points,
                        int Nq, void* stream);

/* ---------------------------------------------------------------------------------------
 * Hit table: the per-viewpoint visibility structure shared by the three encoder layers.
 *   uv        f32 [B, Ncam, Nq, D, 2]  projected, normalised pixel coords (NOT clamped)
 *   vis       u8  [B, Nq]              bit c set <=> camera c sees voxel n (any anchor)
 *   vis_list  i32 [B, Ncam, Nq]        ascending voxel ids seen by camera c  (= the reference's
 *                                      `indexes[c]`, spatial_cross_attention.py:139-141)
 *   vis_cnt   i32 [B, Ncam]
 *   zero_list i32 [B, Nq]              ascending voxel ids NOT seen by exactly one camera: their
 *                                      output rows are zero-filled before the gather (unseen ->
 *                                      stay zero; seen by several cameras -> atomically summed)
 *   zero_cnt  i32 [B]
 *   fwd_list  i32 [B, Ncam, Nq]        work order of ver_sca_forward for camera c: the voxels ONLY camera c
 *                                      sees from the front (ascending), the voxels it shares with other
 *                                      cameras from the back (fwd_list[Nq-1], fwd_list[Nq-2], ...)
 *   fwd_cnt   i32 [B, Ncam, 2]         {#only-this-camera, #shared}; their sum is vis_cnt
 */

/* VoxelFormerEncoder.get_reference_points('3d') + point_sampling
 *   (bevformer/modules/voxel_encoder.py:54-83, 119-195) for B viewpoints at once, followed
 *   by the list construction above (replaces the per-camera nonzero() host syncs of
 *   spatial_cross_attention.py:139-142).  D = 1 (the reference never produces more anchors).
 *   world2pixel f32 [B, Ncam, 4, 4] row-major; origin f32 [B, 3];
 *   pc_range: HOST pointer to 6 floats (xmin,ymin,zmin,xmax,ymax,zmax);
 *   flat voxel index n = k*H*W + j*W + i.
 */
int ver_project_points(const float* world2pixel, const float* origin, const float* pc_range,
                       int B, int Ncam, int bev_z, int bev_h, int bev_w,
                       float img_w, float img_h,
                       float* uv, uint8_t* vis, int32_t* vis_list, int32_t* vis_cnt,
                       int32_t* zero_list, int32_t* zero_cnt, int32_t* fwd_list, int32_t* fwd_cnt,
                       void* stream);

/* Same lists from a caller-supplied mask in the reference's layout
 *   bev_mask u8/bool [Ncam, B, Nq, D]  (spatial_cross_attention.py:87,139-141,170).
 */
int ver_hits_from_mask(const uint8_t* bev_mask, int B, int Ncam, int Nq, int D,
                       uint8_t* vis, int32_t* vis_list, int32_t* vis_cnt,
                       int32_t* zero_list, int32_t* zero_cnt, int32_t* fwd_list, int32_t* fwd_cnt,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused multi-view gather = the body of SpatialCrossAttention.forward between the three
 * input projections and output_proj (spatial_cross_attention.py:139-173 together with
 * MSDeformableAttention3D.forward :345-398): per-camera re-batching, softmax over the
 * points, location arithmetic, bilinear sampling, scatter-add over cameras and division by
 * the camera count -- without padded rows or host syncs.  Rows of voxels seen by exactly one
 * camera are plain stores; rows seen by several cameras are zero-filled first and accumulated
 * with fp32 atomic adds, so the result is bitwise reproducible run to run as long as no voxel is
 * seen by more than two cameras (with three or more the last bit depends on the add order).
 *
 *   value   f32|bf16 [B, Ncam, map_h*map_w, heads, head_dim]   value_proj output
 *   offsets f32 [B, Nq, heads, points, 2]     sampling_offsets output, in pixels (one level)
 *   logits  f32 [B, Nq, heads, points]        attention_weights output, PRE-softmax
 *   slots   f32 [B, Nq, heads*head_dim]       (written; every row, unseen voxels get zeros)
 * slots[b,n] = (1/max(1,#cams seeing n)) * sum_{c sees n} sum_p softmax(logits)[p] *
 *              bilinear(value[b,c], uv[b,c,n,p%D] + offsets[n,p]/(map_w,map_h))
 * Supported: one feature level; head_dim in {8,16,32,64,96,128}; points in {4,8}; D | points;
 *   one (camera, head) value tile must fit the 160 KiB LDS: map_h*map_w*head_dim*4 <= 160 KiB
 *   in forward (<= 80 KiB keeps two workgroups per CU), twice that tile in backward.
 * Arithmetic and numerical contract, by value_dtype:
 *   VER_F32   fp32 throughout (<= 2e-5 against the fp32 reference formula).
 *   VER_BF16  with points == 8 and head_dim % 32 == 0 (the vocc.py shape) the staged tile is converted to fp16 in LDS
 *             and the <= 8 products weight * value of one (voxel, head, corner) are accumulated with packed fp16 FMAs;
 *             the corner fold result is converted to fp32 once and the camera sum / division are fp32.
 *             RANGE: the bf16 -> fp16 conversion is exact for |value| in [6.1e-5, 65504]; larger magnitudes SATURATE at
 *             +-65504 (round toward zero: no inf is produced, NaN stays NaN), smaller ones truncate into the fp16
 *             subnormals (absolute error < 6e-8); sample weights below ~6e-8 flush to zero.
 *             PRECISION: ~5e-4 of the partial sums (max |delta| 3.7e-3 at |slots| <= 1.2, 1e-3 relative L2 against
 *             fp32 accumulation of the same bf16 values; the north star's bf16 bound is 1e-2).
 *             The exact form of the contract is a VER_F32 value: fp32 tiles, fp32 accumulation, <= 2e-5.
 *             Other shapes always use fp32 arithmetic.
 * flags: 0, or VER_SCA_ROWS_PREZEROED -- the caller has already zero-filled the rows `zero_list` names
 *   (`ver_sca_zero_rows(zero_list, zero_cnt, slots, B, Nq, heads*head_dim, side_stream)`, ordered before this call by
 *   an event): the fill depends on the hit table only, so it can run under the projections that precede the gather
 *   instead of in front of it.
 */
#define VER_SCA_ROWS_PREZEROED 1
/*        VER_SCA_VALUE_HEAD_MAJOR (ver_sca_forward and ver_sca_backward): `value` is laid out
 *   [heads, B, Ncam, map_h*map_w, head_dim] instead of the reference's [B, Ncam, map_h*map_w, heads, head_dim]: a (camera,
 *   head) tile is then ONE contiguous block of HBM (every 1-KB LDS-DMA request covers 8 whole 128-byte lines, none shared
 *   with another head's workgroup).  Only where `ver_sca_head_major_supported(...)` returns 1 (bf16 tiles, 8 points,
 *   head_dim % 32 == 0, 14x14 maps: the vocc.py shape); `grad_value` of ver_sca_backward keeps the REFERENCE layout
 *   either way (the weight gradient of value_proj reads it as a plain [rows, heads*head_dim] matrix).
 */
#define VER_SCA_VALUE_HEAD_MAJOR 2
/*        VER_SCA_GRAD_SLOTS_BF16 (ver_sca_backward): `grad_slots` is bf16 [B, Nq, heads*head_dim] -- what the GEMM behind the
 *   gather hands back under bf16 autocast -- and is used as it is, one bf16 term per element (the fp32 form is split into
 *   bf16 hi + lo), whatever the camera count: the division by the count is done in fp32, on the sampling weight, so the three
 *   gradients equal bit for bit those of the fp32 form on the same rows wherever no voxel is seen by more than two cameras
 *   (with more, grad_offsets / grad_logits depend on the order of the atomic adds either way, as the slots do); only where
 *   ver_sca_backward_grad_dtype(...) == VER_BF16, with grad_value_dtype = VER_BF16.
 */
#define VER_SCA_GRAD_SLOTS_BF16 4
int ver_sca_head_major_supported(int value_dtype, int head_dim, int points, int map_h, int map_w);
int ver_sca_zero_rows(const int32_t* zero_list, const int32_t* zero_cnt, float* slots, int B, int Nq, int row_floats,
                      void* stream);
int ver_sca_forward(const void* value, int value_dtype, const float* offsets, const float* logits,
                    const float* uv, const uint8_t* vis, const int32_t* vis_list,
                    const int32_t* vis_cnt, const int32_t* zero_list, const int32_t* zero_cnt,
                    const int32_t* fwd_list, const int32_t* fwd_cnt,
                    float* slots,
                    int B, int Ncam, int Nq, int D, int heads, int head_dim, int points,
                    int map_h, int map_w, int flags, void* stream);

/* Gradient of ver_sca_forward.
 *   grad_slots   f32 [B, Nq, heads*head_dim]
 *   grad_value   f32 | bf16 [B, Ncam, map_h*map_w, heads, head_dim]  (written in full); grad_value_dtype = VER_F32
 *                always works, VER_BF16 only where ver_sca_backward_grad_dtype() says so (the matrix-core path
 *                rounds its fp32 accumulators once, instead of a separate cast pass over the tensor)
 *   grad_offsets f32 [B, Nq, heads, points, 2]                (written in full)
 *   grad_logits  f32 [B, Nq, heads, points]                   (written in full; softmax bwd fused)
 * None of the outputs needs to be zeroed by the caller.
 */
int ver_sca_backward_grad_dtype(int value_dtype, int head_dim, int points, int map_h, int map_w);
int ver_sca_backward(const void* value, int value_dtype, const float* offsets, const float* logits,
                     const float* uv, const uint8_t* vis, const int32_t* vis_list,
                     const int32_t* vis_cnt, const int32_t* fwd_list, const int32_t* fwd_cnt,
                     const void* grad_slots,
                     void* grad_value, int grad_value_dtype, float* grad_offsets, float* grad_logits,
                     int B, int Ncam, int Nq, int D, int heads, int head_dim, int points,
                     int map_h, int map_w, int flags, void* stream);

/* ---------------------------------------------------------------------------------------
 * Data movement of the even-lattice coarse-to-fine upsample: the reference's three
 * ConvTranspose3d(768,768,(3,5,5),s=(1,2,2),p=(2,4,4),d=(2,2,2),op=(0,1,1))
 * (dense_heads/voxelformer_occupancy_head.py:251-258, applied at :560) are evaluated as
 * im2col + GEMM over the channels-last data lattice.
 *   src  f32|bf16 [B, Z, H, W, C]            channels-last lattice
 *   col  f32|bf16 [B*Z*H*W, ntaps, C]        col[(b,z,y,x), t, :] = src[b, z+dz_t, y+dy_t, x+dx_t, :]
 *                                             (zero outside the lattice)
 *   taps HOST pointer to ntaps*(dz,dy,dx) int32 offsets, ntaps <= 80
 * ver_lattice_col2im is the adjoint (gradient of im2col), in gather form (no atomics).
 */
int ver_lattice_im2col(const void* src, void* col, const int* taps, int ntaps,
                       int B, int Z, int H, int W, int C, int dtype, void* stream);
int ver_lattice_col2im(const void* grad_col, void* grad_src, const int* taps, int ntaps,
                       int B, int Z, int H, int W, int C, int dtype, void* stream);

/* Generalised lattice gather / scatter used by the parity-class upsample layers.  Rows enumerate
 * (b, zr < Zr, y, x); tap t reads the source position (zr + dz_t, y + dy_t, x + dx_t) of a lattice
 * with Zs z-layers (zero outside) into col[r * col_stride + col_offset[t] .. + C) (elements; offsets
 * and stride multiples of 16 bytes; columns between tap blocks are left untouched unless `const_rows` fills them);
 * ntaps <= 64.  Source layouts (`layout`):
 *   0 plain [B,Zs,H,W,C]      1 planar: four planes [B,Zs,H/2,W/2,C], plane 2*pm+pn = positions
 *   (2y'+pm, 2x'+pn) of the combined (H, W) lattice      2 z-split [B,2,H,W,2,C] (Zs = 4): element
 *   (b,z,y,x) at row (b, z&1, y, x), channel block z>>1      3 planar z-split: four planes of layout 2.
 * scatter is the adjoint (gather form, no atomics): grad_src is overwritten in the source's layout.
 * Limits: the gather takes any C (whole 16-byte vectors); the scatter gives a lane one 16-byte vector of one position and
 * REFUSES (VER_EUNSUPPORTED) more than 256 vectors per position, C > 2048 bf16 / 1024 f32 channels.
 */
/* const_rows (may be NULL): [Zr*H*W][const_blocks][const_width] elements, the constant-pattern blocks of one viewpoint's
 * rows; the gather copies them to columns const_offset[0 .. const_blocks) of every viewpoint (whole 16-byte vectors).
 */
int ver_lattice_gather(const void* src, void* col, const int* taps, const long* col_offset, long col_stride,
                       int ntaps, int B, int Zr, int Zs, int H, int W, int C, int layout, int dtype,
                       const void* const_rows, const long* const_offset, int const_blocks, int const_width, void* stream);
int ver_lattice_scatter(const void* grad_col, void* grad_src, const int* taps, const long* col_offset,
                        long col_stride, int ntaps, int B, int Zr, int Zs, int H, int W, int C, int layout, int dtype,
                        void* stream);

/* Layout changes of the coarse-to-fine head (LDS-tiled transposes):
 *   ver_convt_weight_forward : ConvTranspose3d weight f32 [pairs = Ci*Co][3*5*5] (the reference's
 *       parameter layout, head:251-258) -> correlation taps [75][pairs] in `dtype`, tap (a,b,c) =
 *       weight[.., 2-a, 4-b, 4-c];  _backward: gradient of the taps -> f32 gradient of the weight.
 *   ver_lattice_transpose    : even lattice channels-last (one of the four layouts of
 *       ver_lattice_gather) <-> channel-first rows cf[b*cf_stride + ((c*Z + z)*H + y)*W + x]
 *       (to_channel_first != 0: channels_last is read; else it is written).  Any C, cf_stride >= C Z H W and alignment of
 *       the element type are taken (16-byte channel vectors and 8-byte position vectors where everything is whole and
 *       aligned, element by element otherwise); a row of 128 channels x (W + 1) positions must fit 64 KB of LDS: W <= 255
 *       bf16, W <= 127 f32, wider lattices are REFUSED (VER_EUNSUPPORTED).
 */
int ver_convt_weight_forward(const float* weight, void* taps, long pairs, int dtype, void* stream);
int ver_convt_weight_backward(const void* grad_taps, float* grad_weight, long pairs, int dtype, void* stream);
/*   ver_convt_weight_backward_blocks : the same adjoint taken straight from the weight gradients of a lattice layer's class
 *       GEMMs (no reference counterpart: the reference's ConvTranspose3d backward, head:251-258 through autograd): tap t
 *       is the fp32 sum of up to two [ci x co] blocks of `blocks` (row pitch `ld` elements, `dtype`) at element offsets
 *       block_offsets[2t], block_offsets[2t+1] (device int64 [75][2], -1 = none) plus prev_bias[ci] * grad_v[t*co + co']
 *       (both `dtype`, or both NULL) -> grad_weight f32 [ci*co][75], taps flipped as above.  bf16 with even co and ld:
 *       the offsets must be even too (4-byte loads; the layers' offsets row * ld + {0, co} are). */
int ver_convt_weight_backward_blocks(const void* blocks, const long* block_offsets, long ld, const void* prev_bias,
                                     const void* grad_v, float* grad_weight, int ci, int co, int dtype, void* stream);
/*   ver_convt_weight_forward_blocks (ABI 29): the forward twin -- the f32 ConvTranspose3d weight [ci*co][75] written STRAIGHT
 *       into the weight matrices the class GEMMs of a lattice layer read: tap t's [ci x co] block goes to element offsets
 *       block_offsets[2t], block_offsets[2t+1] (-1 = none) of `blocks` (row pitch ld, `dtype`): its "lower half" / "upper
 *       half" slots in the class-stacked [sum K_c, 2 co] matrix.  Replaces ver_convt_weight_forward + a concatenation with the
 *       constant rows + one row gather per parity class (dense_heads/upsample.py).  Even co / ld / offsets.
 *   ver_blocks_vec_forward / _backward (ABI 29): a row vector through every [ci x ncols] block of such a stacked matrix:
 *       vec[b][col] = sum_ci x[ci] * blocks[(block_rows[b] + ci) * ld + col]   (the previous layer's bias seen through every
 *       tap, head:251-258's bias-valued odd positions: v = b_prev^T K[t] for all taps in one pass over the bf16 weights),
 *       grad_x[ci] = sum_b sum_col blocks[(block_rows[b] + ci) * ld + col] * grad_vec[b][col].  x, grad_vec f32.  Both write
 *       PARTIAL results that the caller adds up in order (no atomics, bitwise reproducible): vec is f32 [8][nblocks][ncols]
 *       (8 slices of ci), grad_x f32 [nblocks][ci] (one row per block).  block_rows: device int64 [nblocks]. */
int ver_convt_weight_forward_blocks(const float* weight, const long* block_offsets, long ld, void* blocks, int ci, int co,
                                    int dtype, void* stream);
int ver_blocks_vec_forward(const void* blocks, const long* block_rows, int nblocks, long ld, int ci, int ncols, const float* x,
                           float* vec, int dtype, void* stream);
int ver_blocks_vec_backward(const void* blocks, const long* block_rows, int nblocks, long ld, int ci, int ncols,
                            const float* grad_vec, float* grad_x, int dtype, void* stream);
int ver_lattice_transpose(void* channels_last, void* channel_first, long cf_stride, int B, int Z, int H, int W,
                          int C, int layout, int to_channel_first, int dtype, void* stream);
/*   ver_lattice_rows : ver_lattice_transpose and ver_run_gather / _scatter (below) in ONE pass, bf16: the lattice
 *       (channels-last, one of the four layouts) <-> the gathered operand rows of occ_proj's GEMMs, when the runs of the
 *       raw .view (head:564) tile the flat channel-first lattice periodically: flat = k*quarter + row*period + off, the
 *       segment j with seg_off[j] <= off < seg_off[j] + seg_len[j] (host tables, nseg <= 8, the segments cover the
 *       period in order) is a pattern group whose rows live at rows[seg_base[j] + (b*seg_rows[j] + row)*seg_pitch[j]
 *       + k*seg_len[j] + (off - seg_off[j])] (elements).  to_rows != 0: the lattice is read; else it is written.
 *       Limits (refused otherwise): period <= 4096, a multiple of 4 like every seg_len / seg_pitch / seg_base; quarter a
 *       multiple of period and of H*W and a divisor of C Z H W; seg_rows[j] * period == quarter; seg_pitch[j] >=
 *       (C Z H W / quarter) * seg_len[j]; W % 4 == 0, C % 8 == 0, W <= 252; the lattice below 2^31 elements. */
int ver_lattice_rows(void* channels_last, void* rows, long quarter, int period, int nseg, const int* seg_off,
                     const int* seg_len, const long* seg_base, const int* seg_pitch, const int* seg_rows, int B, int Z,
                     int H, int W, int C, int layout, int to_rows, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused LayerNorm(128) + ReLU of the occupancy MLP (`occ_branches`, layers 1-2 and 4-5:
 * dense_heads/voxelformer_occupancy_head.py:241-248, applied at :580 to 504 000 rows per
 * viewpoint): y = relu((x - mean) * rstd * gamma + beta), eps as nn.LayerNorm (1e-5).
 *   x, y, grad_y, grad_x  f32|bf16 [N, 128]   (dtype = VER_F32 | VER_BF16; statistics in fp32)
 *   gamma, beta, grad_gamma, grad_beta f32 [128];  mean, rstd f32 [N] (written by forward)
 * backward writes grad_x in full and the two parameter gradients (zeroed inside).
 */
int ver_ln_relu_forward(const void* x, const float* gamma, const float* beta, void* y,
                        float* mean, float* rstd, long N, int W, float eps, int dtype, void* stream);
int ver_ln_relu_backward(const void* x, const void* grad_y, const float* gamma, const float* beta,
                         const float* mean, const float* rstd, void* grad_x,
                         float* grad_gamma, float* grad_beta, long N, int W, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Sigmoid focal loss of the occupancy term (dense_heads/voxelformer_occupancy_head.py:977-989 ->
 * mmdet 2.14 `FocalLoss(use_sigmoid=True)` / py_sigmoid_focal_loss, configured at
 * projects/configs/verformer/vocc.py:190-195), weight=None:
 *   logits f32|bf16 [N, C] (C % 8 == 0), target int64 [N] in [0, C] (C = background)
 *   forward : partial[b] = sum of the elementwise loss over the elements workgroup b visited,
 *             b < ver_focal_loss_blocks(N, C); the caller adds the partials (and applies
 *             loss_weight / avg_factor).  A target outside [0, C] (F.one_hot raises on it in the
 *             reference) makes the sum NaN and ORs 1 into *bad_labels (device int32, may be NULL;
 *             never cleared by the kernel): a caller that cleans NaNs out of its losses, as the
 *             head does, can still be loud about it without a synchronisation per step
 *   backward: grad[n,c] = scale[0] * d loss[n,c] / d logits[n,c]   (scale: device scalar; grad in
 *             the logits' dtype)
 *   arithmetic: fp32 per element.  f32 logits: log1p / exact division (1e-4 parity with the reference's
 *             fp32 formulas).  bf16 logits: the hardware exp2 / log2 / reciprocal (1 ulp each; exp(-|x|)
 *             below 2^-126 flushes to zero) -- the error stays far below the bf16 rounding of the inputs
 *             and of the gradient that is written back
 */
int ver_focal_loss_blocks(long N, int C);
int ver_focal_loss_forward(const void* logits, const int64_t* target, float* partial, long N, int C,
                           float gamma, float alpha, int dtype, int32_t* bad_labels, void* stream);
/*   forward_grad: the forward pass that ALSO writes the unscaled gradient d loss[n,c] / d logits[n,c] (logits' dtype) to
 *             `grad`, which may be the logits buffer itself -- for steps that need the loss and its gradient, not the logits */
int ver_focal_loss_forward_grad(const void* logits, const int64_t* target, float* partial, void* grad, long N, int C,
                                float gamma, float alpha, int dtype, int32_t* bad_labels, void* stream);
/* ... with the labels as bytes (C <= 254; ABI 28): what a caller that permutes and counts its labels as bytes hands over */
int ver_focal_loss_forward_grad_u8(const void* logits, const uint8_t* target, float* partial, void* grad, long N, int C,
                                   float gamma, float alpha, int dtype, int32_t* bad_labels, void* stream);
int ver_focal_loss_backward(const void* logits, const int64_t* target, const float* scale, void* grad,
                            long N, int C, float gamma, float alpha, int dtype, void* stream);
/*   class weights (the `_cw` twins; head:1417-1425 `weight=weights[gt_occupancy]` of loss_only_occupancy -> mmdet's
 *             `loss * weight.view(-1, 1)`): class_weight f32 [C + 1] on the device, one factor per label value in [0, C]
 *             (index C = the empty / background label); every element of row n is multiplied by class_weight[target[n]]:
 *               forward sum = sum_n class_weight[t_n] * sum_c loss[n, c]
 *               gradient    = class_weight[t_n] * d loss[n, c] / d logits[n, c]   (no gradient to the table)
 *             The caller's avg_factor stays the UNWEIGHTED count of occupied voxels, as in the reference.  A label
 *             outside [0, C] never indexes the table (factor 0); the sum is NaN and *bad_labels is raised as above.
 *             Same arguments and checks as the twins, plus C + 1 <= 256 (VER_EUNSUPPORTED otherwise: the table is
 *             staged on chip) and class_weight != NULL when N > 0 (VER_EINVAL).  A table of ones gives the forward
 *             twins' partials and gradients bit for bit.  N == 0: VER_OK, nothing is launched
 *             (ver_focal_loss_forward_cw then leaves `partial` as the caller zero-filled it). */
int ver_focal_loss_forward_cw(const void* logits, const int64_t* target, const float* class_weight, float* partial,
                              long N, int C, float gamma, float alpha, int dtype, int32_t* bad_labels, void* stream);
int ver_focal_loss_forward_grad_cw(const void* logits, const int64_t* target, const float* class_weight, float* partial,
                                   void* grad, long N, int C, float gamma, float alpha, int dtype, int32_t* bad_labels,
                                   void* stream);
int ver_focal_loss_forward_grad_u8_cw(const void* logits, const uint8_t* target, const float* class_weight, float* partial,
                                      void* grad, long N, int C, float gamma, float alpha, int dtype, int32_t* bad_labels,
                                      void* stream);
int ver_focal_loss_backward_cw(const void* logits, const int64_t* target, const float* class_weight, const float* scale,
                               void* grad, long N, int C, float gamma, float alpha, int dtype, void* stream);
/*   byte labels for the separate forward and backward passes (additive to ABI 31): ver_focal_loss_forward / _backward and
 *             their `_cw` twins with target uint8 [N], as ver_focal_loss_forward_grad_u8 takes it -- for a caller whose
 *             labels are bytes already (the row-order labels ver_occ_targets writes) and who keeps the logits, so that no
 *             int64 [N] copy of the labels is made in front of the loss.  The same kernels instantiated for the label
 *             type: the same arithmetic per element, the same partial layout (ver_focal_loss_blocks), the same NaN sum and
 *             *bad_labels flag for a label outside [0, C] (255, a wrapped -1, among them), hence partials and gradients
 *             that equal the int64 entries' on the widened labels bit for bit.  Arguments and checks as the int64 entries',
 *             plus C <= 254 (VER_EINVAL: the classes and the empty label fit a byte; the `_cw` forms' C + 1 <= 256 with
 *             C % 8 == 0 implies it).  N == 0 as the int64 entries: the `_cw` forms and the backward launch nothing. */
int ver_focal_loss_forward_u8(const void* logits, const uint8_t* target, float* partial, long N, int C,
                              float gamma, float alpha, int dtype, int32_t* bad_labels, void* stream);
int ver_focal_loss_backward_u8(const void* logits, const uint8_t* target, const float* scale, void* grad,
                               long N, int C, float gamma, float alpha, int dtype, void* stream);
int ver_focal_loss_forward_u8_cw(const void* logits, const uint8_t* target, const float* class_weight, float* partial,
                                 long N, int C, float gamma, float alpha, int dtype, int32_t* bad_labels, void* stream);
int ver_focal_loss_backward_u8_cw(const void* logits, const uint8_t* target, const float* class_weight, const float* scale,
                                  void* grad, long N, int C, float gamma, float alpha, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * y = LayerNorm(residual + dropout(a)): how both branches of the reference's VoxelFormerLayer end
 * (voxel_encoder.py:344-464 with operation_order cross_attn - norm - ffn - norm; SpatialCrossAttention.forward
 * returns `dropout(output_proj(slots)) + residual`, spatial_cross_attention.py:173-176; mmcv FFN returns
 * `identity + dropout(layers(x))`; a LayerNorm over C = embed_dims follows), one pass each way.
 *   a [N,C] f32 or bf16 (a_dtype), residual f32 [N,C], gamma / beta f32 [C]; C in {256, 512, 768, 1024}
 *   dropout: element i is kept iff hash(seed[0], i) < 1 - p_drop (seed: device int64; the backward pass recomputes
 *            the decision -- no mask tensor), kept values scaled by 1 / (1 - p_drop); p_drop = 0: no dropout, seed
 *            may be NULL.  (The reference's nn.Dropout draws from torch's generator: same distribution, different
 *            stream; parity vectors are taken in eval mode.)
 *   forward : y f32 [N,C], y_bf16 (optional, NULL to skip: the copy the next Linear reads under bf16 autocast),
 *             mean, rstd f32 [N]
 *   backward: grad_y f32 (+ grad_y_bf16, optional: the gradient that arrived through y_bf16) ->
 *             grad_a (a's dtype), grad_residual f32, grad_gamma / grad_beta f32 [C] (zeroed inside)
 *   non-finite inputs (tests/test_row_kernels_gpu.py pins this):
 *     forward : a NaN in residual, or in a KEPT element of a, makes that row's y, y_bf16, mean and rstd NaN and leaves every
 *             other row bit for bit as it would be without it.  A DROPPED element of a is never multiplied: it contributes
 *             exactly 0 whatever it holds, a NaN or an infinity included (torch's dropout, mask * a, would propagate it).
 */
int ver_add_ln_forward(const void* a, int a_dtype, const float* residual, const float* gamma, const float* beta,
                       const int64_t* seed, float p_drop, float eps, float* y, void* y_bf16, float* mean,
                       float* rstd, long N, int C, void* stream);
/*     backward: the same rows (it reads the forward's NaN mean / rstd) have NaN grad_residual and NaN grad_a in their kept
 *             elements; grad_a of a dropped element is exactly 0 in every row, those included; grad_gamma is NaN in every
 *             channel (each sums over that row), grad_beta (a sum of grad_y alone) stays finite; every other row's grad_a
 *             and grad_residual are bit for bit as without the NaN. */
int ver_add_ln_backward(const float* grad_y, const void* grad_y_bf16, const void* a, int a_dtype,
                        const float* residual, const float* gamma, const float* mean, const float* rstd,
                        const int64_t* seed, float p_drop, void* grad_a, float* grad_residual, float* grad_gamma,
                        float* grad_beta, long N, int C, void* stream);
/*   y = dropout(relu(x)): the hidden activation of the layer's FFN (mmcv FFN: Linear - ReLU - Dropout - Linear), the
 *   same hash for the keep decision.  backward: grad_x = y > 0 ? grad_y / (1 - p_drop) : 0 (needs y only).
 *   n elements (a multiple of 4), dtype VER_F32 / VER_BF16; y may alias x.
 *   special values: the gate is the fp32 comparison x > 0, so +-0, negative values and NaN give y = 0; +inf stays +inf, and a
 *   finite x whose product with 1 / (1 - p_drop) leaves the fp32 range becomes +inf.  Denormals are NOT flushed (the
 *   library is built with fp32 denormals on): a kept positive denormal x gives the denormal y = x / (1 - p_drop), in fp32
 *   and in bf16, and the backward, whose only gate is y > 0, passes its gradient -- grad_x != 0 exactly where y != 0.  A
 *   build that flushes denormals would close the gate for them in both passes alike; callers must not rely on either
 *   (tests/test_row_kernels_gpu.py asserts the agreement of the two passes, not the fate of a denormal).
 */
int ver_relu_dropout_forward(const void* x, void* y, const int64_t* seed, float p_drop, long n, int dtype, void* stream);
int ver_relu_dropout_backward(const void* y, const void* grad_y, void* grad_x, float p_drop, long n, int dtype,
                              void* stream);

/* ---------------------------------------------------------------------------------------
 * Run copies between the channel-first even lattice and the rows of the gathered `occ_proj` operand
 * (the reference's raw `.view(bs, Z, X, Y, C)` + `permute(0,2,3,1,4).flatten(3)` of the upsampled volume,
 * dense_heads/voxelformer_occupancy_head.py:564-570, restricted to the columns that are not constants).
 * A row (sample b, member i of a row group) is `runs` contiguous runs of `run_len` elements of sample b's image
 * starting at run_start[i*runs + k], followed by n_aug single elements image[aug_idx[i*n_aug + j]]:
 *   gather : rows[(b*n_rows + i)*row_elems + ...] <- image[b*image_stride + ...]       (forward operand)
 *   scatter: image[b*image_stride + run_start[..] + o] <- rows[(b*n_rows + i)*row_elems + k*run_len + o]
 *            (backward: every image element is written by exactly one row)
 * dtype VER_F32 / VER_BF16; run_len, run starts, image_stride and row_elems multiples of 8 bytes.
 */
int ver_run_gather(const void* image, long image_stride, const int32_t* run_start, const int32_t* aug_idx,
                   void* rows, int B, int n_rows, int runs, int run_len, int n_aug, int row_elems, int dtype,
                   void* stream);
int ver_run_scatter(const void* rows, void* image, long image_stride, const int32_t* run_start, int B,
                    int n_rows, int runs, int run_len, int row_elems, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused occupancy MLP = the reference's `occ_branches` Sequential
 * (dense_heads/voxelformer_occupancy_head.py:241-248; applied at :580):
 *   Linear(128,128) LayerNorm ReLU Linear(128,128) LayerNorm ReLU Linear(128,16)
 * bf16 operands, fp32 accumulation / LayerNorm statistics (the arithmetic of the reference's
 * layers under bf16 autocast); the hidden activations never leave the registers.
 *   pack    : W1, W2 f32 [128,128], W3 f32 [16,128] (nn.Linear layout [out,in]) -> `image`
 *             (ver_occ_mlp_image_bytes() bytes, 16-byte aligned): MFMA weight fragments
 *   vectors : f32 [ver_occ_mlp_vector_floats()] = b1 gamma1 beta1 b2 gamma2 beta2 (128 each) b3 (16)
 *   forward : x bf16 [N,128] -> logits bf16 [N,16]
 *   flags   : bit 0 = first Linear.  Clear: the first Linear has been folded into the producer of x (two Linears in a row compose:
 *             `occ_proj` :571 feeds `occ_branches[0]` :580 with nothing in between), x is ITS output and the chain
 *             starts at the first LayerNorm; W1 / b1 of image / vectors are ignored, grad_a1 may be NULL,
 *             grad_x = d loss / d x is then the gradient w.r.t. that output, and no dW1 is to be formed.
 *             Bit 1 = VER_OCC_MLP_CENTERED: the caller has
 *             centred the weights and biases of both hidden Linears over their OUTPUT axis (W <- W - mean_o W,
 *             b <- b - mean b; with bit 0 clear the centring of Linear 1 sits in the producer of x), so every
 *             LayerNorm input has zero row mean and the kernel skips the mean pass.  LayerNorm is invariant to a
 *             per-row constant: LN(Wx + b) = LN(PWx + Pb), P = I - 11^T/128 -- the same function of the parameters;
 *             the caller maps the gradients of the centred parameters back through P (autograd does).
 */
#define VER_OCC_MLP_CENTERED 2
long ver_occ_mlp_image_bytes(void);
int ver_occ_mlp_vector_floats(void);
int ver_occ_mlp_pack(const float* W1, const float* W2, const float* W3, void* image, void* stream);
int ver_occ_mlp_forward(const void* x, const void* image, const float* vectors, void* logits,
                        long N, int width, int classes, float eps, int flags, void* stream);
/*   the same, also writing the reciprocal standard deviation of both LayerNorms per row (ABI 24):
 *     rstd f32 [N, 2]  (may be NULL: plain forward).  ver_occ_mlp_backward_fused_stats reads it back, so that its two
 *     recomputed LayerNorm-forward steps need no statistics (elementwise; VER_OCC_MLP_CENTERED rows only).
 */
int ver_occ_mlp_forward_stats(const void* x, const void* image, const float* vectors, void* logits, float* rstd,
                              long N, int width, int classes, float eps, int flags, void* stream);
/*   backward (first_linear: zero or not, as bit 0 of the forward's flags; no centred form): re-computes the forward from x, then
 *     grad_x  bf16 [N,128]                      d loss / d x
 *     grad_a1, grad_a2 bf16 [N,128]             gradients w.r.t. the outputs of Linear 1 / Linear 2
 *     h1      bf16 [N,128]                      input of Linear 2 (post-ReLU activation)
 *     param_grads f32 [6*128 + 16*128 + 16]     d gamma1, d beta1, d b1, d gamma2, d beta2, d b2, then
 *                                               d W3 [16,128] and d b3 [16] (accumulated in-kernel); zeroed inside
 *   grad_a*, h1 are stored in FRAGMENT feature order: column 32t + 8g + j of a row holds feature
 *   32t + (j < 4 ? 4g + j : 16 + 4g + j - 4); the caller forms dW2 = grad_a2^T h1, dW1 = grad_a1^T x
 *   from them and un-permutes.
 */
int ver_occ_mlp_backward(const void* x, const void* grad_logits, const void* image, const float* vectors,
                         void* grad_x, void* grad_a1, void* grad_a2, void* h1,
                         float* param_grads, long N, int width, int classes, float eps, int first_linear,
                         void* stream);
/*   backward, folded first Linear (first_linear = 0), EVERYTHING accumulated in the kernel (ABI 22): reads x and
 *   grad_logits, writes grad_x; no side tensors.  W2 f32 [128,128], W3 f32 [16,128] are the raw nn.Linear weights
 *   (no image), `vectors` as above (b1 is ignored).
 *     param_grads f32 [6*128 + 16*128 + 16 + 128*128]   d gamma1, d beta1, (unused), d gamma2, d beta2, d b2, then
 *                                               d W3 [16,128], d b3 [16], d W2 [128,128] -- natural order; zeroed inside
 *   flags: 0 or VER_OCC_MLP_CENTERED (the forward ran centred: W2 / b2 passed here are the centred ones, the recomputed
 *   LayerNorm-forward steps skip the mean pass).
 *   grad_scale: NULL, or a DEVICE scalar that multiplies grad_logits as it is read (the gradient of the loss sum that
 *   `ver_focal_loss_forward_grad` left unscaled: the training loss then needs no backward pass over the logits).
 *   Always accepted: one kernel serves every combination of flags, grad_scale and rstd.
 */
int ver_occ_mlp_backward_fused(const void* x, const void* grad_logits, const float* W2, const float* W3,
                               const float* vectors, void* grad_x, float* param_grads, long N, int width,
                               int classes, float eps, const float* grad_scale, int flags, void* stream);
/*   the same with the statistics ver_occ_mlp_forward_stats saved (rstd f32 [N, 2], may be NULL; used with
 *   VER_OCC_MLP_CENTERED only, ignored otherwise) */
int ver_occ_mlp_backward_fused_stats(const void* x, const void* grad_logits, const float* W2, const float* W3,
                                     const float* vectors, const float* rstd, void* grad_x, float* param_grads, long N,
                                     int width, int classes, float eps, const float* grad_scale, int flags, void* stream);
/*   the same with REPRODUCIBLE parameter gradients (additive to ABI 31): the two entries above add every workgroup's share of
 *   param_grads with float atomics, so their last bits follow the arrival order and differ from run to run.  Here workgroup w
 *   adds into its own zeroed slab, slabs f32 [workgroups][6*width + classes*width + classes + width*width] (scratch, at least
 *   ver_occ_mlp_backward_fused_slab_bytes(N) bytes, 4-byte aligned), and one more launch sums the slabs in a fixed order into
 *   param_grads: the same inputs give the same bits.  grad_x is the same kernel's and was reproducible already.  Two more
 *   launches (zeroing the slabs, the sum: 19.7 MB each way at 256 workgroups) on a kernel of milliseconds. */
long ver_occ_mlp_backward_fused_slab_bytes(long N);
int ver_occ_mlp_backward_fused_slabs(const void* x, const void* grad_logits, const float* W2, const float* W3,
                                     const float* vectors, const float* rstd, void* grad_x, float* param_grads, float* slabs,
                                     long slab_bytes, long N, int width, int classes, float eps, const float* grad_scale,
                                     int flags, void* stream);

/* ---------------------------------------------------------------------------------------
 * Occupancy post-processing: VoxelFormerOccupancyHead.get_occupancy_prediction, focal-loss branch
 * (dense_heads/voxelformer_occupancy_head.py:1505-1540): sigmoid, the threshold as an extra last
 * ("empty") column, arg-max, sparse (voxel index, class) pairs of the occupied voxels.
 *   logits     f32|bf16 [N, C]  (C % 8 == 0, 16-byte aligned)
 *   block_work i32 [ver_occ_predict_blocks(N)]   scratch
 *   pairs      i64 [N, 2] capacity; rows [0, *count) are written: (row index, class), ascending row index
 *   count      i64 device scalar: number of occupied rows
 * Semantics of torch.argmax: the first of equal maxima wins (so a class probability EQUAL to the threshold is
 * occupied), NaN counts as the maximum.  Sigmoid is evaluated in fp32 (1 / (1 + exp(-x))).
 */
long ver_occ_predict_blocks(long N);
int  ver_occ_predict(const void* logits, int dtype, long N, int C, float threshold, int32_t* block_work,
                     int64_t* pairs, int64_t* count, void* stream);

/* ---------------------------------------------------------------------------------------
 * Occupancy IoU / mIoU confusion matrix (ABI 30): the numpy `bincount` of the reference's
 * SSCMetrics.add_batch (datasets/occupancy_metrics.py) fed by MP3DDataset.evaluate_occ_iou
 * (mp3docc_dataset.py:485-584), for T thresholds in one pass over the logits.
 *   logits      f32|bf16 [samples * rows_per_sample, C]   (16-byte aligned, C % 8 == 0, 8 <= C <= 32)
 *   labels      u8 [samples * rows_per_sample], same row order; a value >= C + 1 is ignored (the
 *               reference's `gt < n_cl`: pass invalid / invisible voxels as 255)
 *   thresholds  HOST f32 [num_thresholds], 1 <= num_thresholds <= 8 (copied into the kernel arguments:
 *               a captured launch keeps them)
 *   hist        i64 [samples, num_thresholds, K, K], K = C + 1; row = label, column = prediction,
 *               column C = empty.  ACCUMULATED (+=): zero it once at allocation; nothing is cleared here.
 * The prediction of a row under threshold t is the class ver_occ_predict gives with that threshold
 * (fp32 sigmoid, first of equal maxima, NaN as the maximum, class C when thr_t > every probability).
 * rows_per_sample == 0 or samples == 0: nothing is launched, hist is unchanged.
 */
int  ver_occ_confusion(const void* logits, int dtype, long rows_per_sample, int samples, int C, const uint8_t* labels,
                       const float* thresholds, int num_thresholds, int64_t* hist, void* stream);

/* ---------------------------------------------------------------------------------------
 * The same two results WITHOUT the logits: the classification runs in the epilogue of the fused MLP forward kernel
 * (csrc/ver_occ_mlp.hip), on the bf16 logits ver_occ_mlp_forward would have stored -- they never reach memory.
 *   x, image, vectors, width, classes, eps, flags: as ver_occ_mlp_forward (flags bit 0 = first Linear, bit 1 =
 *               VER_OCC_MLP_CENTERED; x and image 16-byte aligned; another width / class count: VER_EUNSUPPORTED)
 * ver_occ_mlp_confusion: labels, rows_per_sample, samples, thresholds (HOST array, copied into the kernel arguments: a
 *   captured launch keeps them), num_thresholds (1 to 8) and hist (8-byte aligned, ACCUMULATED, never cleared) as
 *   ver_occ_confusion; sample s owns rows [s, s + 1) * rows_per_sample of x.  CONTRACT: it adds to hist exactly what
 *   ver_occ_mlp_forward followed by ver_occ_confusion on its bf16 logits adds.  rows_per_sample == 0 or samples == 0:
 *   nothing is launched, no pointer is looked at, hist is unchanged.
 * ver_occ_mlp_classes: cls u8 [N] = threshold_class(row_argmax(logits of the row), threshold): the class
 *   ver_occ_predict pairs with the row, `classes` (16) for an empty row; prob f32 [N] or NULL = the probability of the best
 *   class (row_argmax's pb, bit for bit).  N == 0: nothing is launched.
 * One launch each, no memset node, no allocation, no host read.
 */
int ver_occ_mlp_confusion(const void* x, const void* image, const float* vectors, const uint8_t* labels,
                          long rows_per_sample, int samples, const float* thresholds, int num_thresholds,
                          int64_t* hist, int width, int classes, float eps, int flags, void* stream);
int ver_occ_mlp_classes(const void* x, const void* image, const float* vectors, uint8_t* cls, float* prob,
                        long N, float threshold, int width, int classes, float eps, int flags, void* stream);

/* ---------------------------------------------------------------------------------------
 * Weight gradient of the head's GEMM layers with ROWS on the contraction axis (ABI 24):
 *     out[Ka, N] = A[M, Ka]^T G[M, N]
 * A = the operand of the forward GEMM (tap matrix of a lattice layer / gathered occ_proj rows), G = the gradient of
 * its output; replaces the `a.t() @ g` of dense_heads/upsample.py::rows_tn, i.e. the d(weight) of the reference's
 * ConvTranspose3d stack and occ_proj (voxelformer_occupancy_head.py:251-258, :560, :571) as autograd forms it.
 *   a          bf16 [M, lda]  (the first Ka columns are used; a column range of a wider matrix is passed by pointer)
 *   g          bf16 [M, ldg]  (first N columns)
 *   out        bf16 | f32 [Ka, ldo]  (out_dtype VER_BF16 | VER_F32), written
 *   workspace  f32 [splits, Ka, N]: the row axis is split into `splits` chunks (0: ver_wgrad_tn_splits), every
 *              chunk's product stays fp32 until the chunks are added up (no bf16 rounding of partial sums)
 * Requirements: a, g 16-byte aligned, lda % 8 == 0, ldg % 8 == 0, N % 4 == 0, ldo % 4 == 0; any M (M = 0: zeros).
 * flags: 0 (slabs per phase and the prefetch distance are constants of ver_wgrad.hip).
 */
int  ver_wgrad_tn_splits(long M, int Ka, int N);
/*   the same choice knowing the widest row pitch ld = max(lda, ldg) in elements (ABI 29): a row chunk has to stay inside the
 *   4-GiB range of a buffer offset, so wide rows need more chunks than the default cap of 45 000 rows assumes */
int  ver_wgrad_tn_splits_ld(long M, int Ka, int N, long ld);
long ver_wgrad_tn_workspace(long M, int Ka, int N, int splits);
int  ver_wgrad_tn(const void* a, long lda, const void* g, long ldg, long M, int Ka, int N, void* out, long ldo,
                  int out_dtype, int splits, int flags, void* workspace, long workspace_bytes, void* stream);
/*   the same product with the IMPLICIT tap matrix of ver_gemm_nn_segments as A (ABI 29): out[Ka, N] = A^T g, A's columns =
 *   the segments in order (taps int [nseg][3]: (dz, dy, dx) = C columns, (-1 - k, 0, 0) = the cw columns of pattern block k of
 *   cst), rows = the cells of the combined (H, W) lattice, M = B 2 H W.  Segment widths must be multiples of 64 (a wave's
 *   64-column LDS-DMA piece lies inside one segment): C % 64 == 0, cw % 64 == 0.  16 <= 2 H W <= 2 048 rows per viewpoint
 *   (four per-wave offset tables of 2 H W ints sit next to the 128-KiB ring: 160 KiB, all of a CU's LDS, at 2 048), the source
 *   lattice below 2 GiB (the forward, ver_gemm_nn_taps / _segments / _planes, has no bound on 2 H W).
 *   ver_wgrad_tn_segments_splits: the row-chunk count for `splits` = 0 (sizes the workspace f32 [splits][Ka][N]). */
int  ver_wgrad_tn_segments(const void* lattice, int layout, int B, int H, int W, int C, const int* taps, int nseg, const void* cst,
                           int ncst, int cw, const void* g, long ldg, int N, void* out, long ldo, int out_dtype, int splits,
                           void* workspace, long workspace_bytes, void* stream);
int  ver_wgrad_tn_segments_splits(int B, int H, int W, long Ka, int N, long ldg);

/* Forward product of the same layers (ABI 24):  c[M, N] = a[M, K] w[K, N] (+ bias[N]), bf16 in, fp32 accumulation, bf16 out.
 * Replaces the `torch.mm(a_mat[:, c0:c1], w, out=...)` / `addmm` of dense_heads/upsample.py and the `a @ wa.t()` of
 * occ_proj_lattice.py (with wa.t() materialised as [K, N]) -- the reference's ConvTranspose3d / occ_proj forward
 * (voxelformer_occupancy_head.py:560, :571) on the even lattice.
 *   a    bf16 [M, lda] (first K columns; K contiguous)      w  bf16 [K, ldw] (first N columns; N contiguous)
 *   bias f32 [N] or NULL                                     c  bf16 [M, ldc] (first N columns written)
 * Requirements: K % 32 == 0, K >= 64, a / w 16-byte aligned, lda % 8 == 0, ldw % 8 == 0; any M, N.  flags: 0.
 */
int  ver_gemm_nn(const void* a, long lda, const void* w, long ldw, const float* bias, void* c, long ldc, long M, int K,
                 int N, int flags, void* stream);
/*   the same product cut into K slices (ABI 29) for SKINNY operands -- the 450- and 1 800-row tap matrices of a
 *   one-viewpoint step (vocc.py:222 samples_per_gpu = 1) give 12-42 output tiles, a fraction of the chip: every slice's
 *   partial tile stays fp32 in `workspace` (f32 [splits][M][N]) and one pass adds them up, adds the bias and rounds once.
 *   ver_gemm_nn_splits: the slice count the library would pick (1: no workspace needed).  Needs N % 4 == 0, ldc % 4 == 0. */
/*   the same product with an IMPLICIT operand (ABI 29): the tap matrix of a Z = 4 lattice layer is never written -- row r of
 *   the product is cell (b, zl, y, x) of the combined (H, W) lattice (r = ((b 2 + zl) H + y) W + x; M = B 2 H W), its K axis
 *   `ntaps` blocks of C channels, block t = the channel vector of cell (zl + dz, y + dy, x + dx) of the source lattice
 *   (taps int [ntaps][3] = (dz in {0, 2}, dy, dx), HOST memory; zeros outside) -- what ver_lattice_gather would have copied,
 *   read straight from the lattice by the kernel's LDS-DMA.  layout: 0 plain [B,4,H,W,C], 2 z-split, 3 planar z-split (as
 *   ver_lattice_gather).  w bf16 [ntaps*C, ldw].  rowpos f32 [2 H W][N] or NULL: added to row r by its position r % (2 H W)
 *   (the constant-pattern columns of the explicit tap matrix times their weight rows); bias f32 [N] or NULL.
 *   Requirements: C % 32 == 0, ntaps <= 64, the source lattice below 2 GiB. */
int  ver_gemm_nn_taps(const void* lattice, int layout, int B, int H, int W, int C, const int* taps, int ntaps, const void* w,
                      long ldw, const float* rowpos, const float* bias, void* c, long ldc, int N, void* stream);
/*   ... with constant-pattern segments between the tap blocks: a taps entry (-1 - k, 0, 0) stands for the `cw` columns of
 *   block k of cst bf16 [2 H W][ncst][cw], which depend on the row's position r % (2 H W) only (the 0/1 patterns of the
 *   bias-valued odd input positions and the ones column of dense_heads/upsample.py's class layout
 *   [P00 | G1 | P10 | G2 | P11 | G3 | G4 | P01]); w then has sum-of-segment-widths rows, in segment order: the explicit
 *   tap matrix's column ranges and class weight matrices as they are.  cw % 32 == 0. */
int  ver_gemm_nn_segments(const void* lattice, int layout, int B, int H, int W, int C, const int* taps, int ntaps,
                          const void* cst, int ncst, int cw, const void* w, long ldw, const float* rowpos, const float* bias,
                          void* c, long ldc, int N, void* stream);
/*   ... reading its tap blocks from SEVERAL source lattices of one shape, plane_elems elements apart (tap t from plane
 *   tap_plane[t], host int [ntaps]; each plane below 2 GiB): d(input) of a lattice layer as ONE gather-form product over the four
 *   class planes of the output gradient, d_e[cell] = sum over (class, tap, half) of g_class[cell - tap] W^T -- no explicit
 *   d(tap matrix), no ver_lattice_scatter (the reference's ConvTranspose3d backward-data, head:251-258 through autograd). */
int  ver_gemm_nn_planes(const void* lattice, int layout, int B, int H, int W, int C, long plane_elems, int nplanes,
                        const int* tap_plane, const int* taps, int ntaps, const void* cst, int ncst, int cw, const void* w,
                        long ldw, const float* rowpos, const float* bias, void* c, long ldc, int N, void* stream);
int  ver_gemm_nn_splits(long M, int K, int N);
int  ver_gemm_nn_splitk(const void* a, long lda, const void* w, long ldw, const float* bias, void* c, long ldc, long M, int K,
                        int N, int splits, void* workspace, long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Gradient clipping by the global L2 norm + AdamW, one call per step (ABI 27).  Replaces, for fp32 parameters, the
 * optimizer step the reference configures: mmcv OptimizerHook(grad_clip=dict(max_norm=..., norm_type=2)) in front of
 * torch.optim.AdamW (projects/configs/verformer/vocc.py:268-274) -- torch.nn.utils.clip_grad_norm_ (coefficient
 * min(1, max_norm / (norm + 1e-6))) followed by AdamW (decoupled weight decay, amsgrad off, bias corrections of `step`).
 *   table        device array of 4 * n_tensors pointers: parameters | gradients | exp_avg | exp_avg_sq (all f32, same sizes)
 *   sizes        device long [n_tensors]: elements per tensor
 *   chunk_tensor, chunk_index   device int [n_chunks]: the tensor of every chunk of `chunk_elems` elements (a multiple of 4)
 *                and the chunk's index inside that tensor
 *   partial      device float [n_chunks] scratch; norm_out: device float receiving the gradient norm BEFORE clipping, or NULL
 *   max_norm <= 0: no clipping.  Gradients are read, not rewritten.  step = 1 for the first update. */
int ver_clip_adamw_step(void* const* table, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                        int n_tensors, int n_chunks, int chunk_elems, float* partial, float* norm_out, float max_norm,
                        float lr, float beta1, float beta2, float eps, float weight_decay, long step, void* stream);

/* The same step with PER-TENSOR hyper-parameters and update counts (ABI 29; several parameter groups -- vocc.py:260-267
 * `paramwise_cfg` gives img_backbone its own lr -- and parameters that received their first gradient at different steps;
 * torch.optim.AdamW tracks `step` per parameter), everything the launch reads resident on the device so that a captured
 * hipGraph of the step replays correctly:
 *   hyper   device float [n_tensors][6] = lr, beta1, beta2, eps, weight_decay, (unused) of tensor t
 *   steps   device int   [n_tensors]    = updates applied to tensor t so far; this call adds 1 to every entry and uses the
 *                                         new value in the bias corrections 1 - beta^step
 * The clip norm is global over all tensors, as in clip_grad_norm_; a non-finite norm gives a NaN factor (torch.clamp). */
int ver_clip_adamw_step_tensors(void* const* table, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                                const float* hyper, int* steps, int n_tensors, int n_chunks, int chunk_elems, float* partial,
                                float* norm_out, float max_norm, void* stream);

/* Gradient exchange through ONE flat buffer (added under ABI 31; data-parallel training without DistributedDataParallel's
 * bucket hooks, so that the step can live in captured hipGraphs: graph A ends in ver_grad_pack, one eager all-reduce of
 * `flat` follows, graph B is ver_clip_adamw_step_flat -- vln-ver_amd/ddp.py GradExchange).
 *   offsets      device long [n_tensors]: first element of tensor t inside `flat`; every offset a multiple of 8 elements,
 *                tensors in order and not overlapping (running sum of the sizes, each rounded up to 8)
 *   flat         device buffer, 16-byte aligned, f32 | bf16 (flat_dtype = VER_F32 | VER_BF16)
 *   sizes, chunk_tensor, chunk_index, n_tensors, n_chunks, chunk_elems: the chunk tables of ver_clip_adamw_step above
 *
 * ver_grad_pack: flat[offsets[t] + i] = g_t[i] * scale for every tensor, one launch.
 *   table        device array of n_tensors pointers: the f32 gradients, each at least 4-byte aligned (16-byte aligned ones
 *                move 16 bytes per lane and store, any other -- a view into a bucket -- goes element by element)
 *   scale        1 / world size for a mean of the ranks' gradients; the product is formed in fp32
 *   VER_F32: the product is stored as computed.  VER_BF16: it is rounded ONCE, to nearest-even; a NaN is stored as the
 *   quiet NaN 0x7fc0, +-inf stay +-inf, a finite product past the largest bf16 becomes +-inf (round-to-nearest).
 *   The elements of `flat` between the tensors (the padding up to the next multiple of 8) are never written. */
int ver_grad_pack(const void* const* table, const long* sizes, const long* offsets, const int* chunk_tensor,
                  const int* chunk_index, int n_tensors, int n_chunks, int chunk_elems, float scale, void* flat,
                  int flat_dtype, void* stream);

/* ver_clip_adamw_step_flat: ver_clip_adamw_step_tensors with the gradient of tensor t read from flat + offsets[t] in
 * flat_dtype (bf16 widened to fp32 on load) instead of through the table.
 *   table        keeps its [4][n_tensors] layout (parameters | gradients | exp_avg | exp_avg_sq); the gradient row is NOT read
 * Every result -- parameters, both moments, `steps`, norm_out -- is bit for bit what ver_clip_adamw_step_tensors gives on
 * 16-byte-aligned f32 gradient tensors holding the same values: both are one kernel body over two gradient loaders, so the
 * order of the sum of squares (lane i of 256 takes elements 4(i + 256k) .. +3, the tail element by element, the block sum,
 * the in-order sum of the partials in every workgroup) is the same. */
int ver_clip_adamw_step_flat(void* const* table, const long* sizes, const long* offsets, const int* chunk_tensor,
                             const int* chunk_index, const float* hyper, int* steps, const void* flat, int flat_dtype,
                             int n_tensors, int n_chunks, int chunk_elems, float* partial, float* norm_out, float max_norm,
                             void* stream);

/* ---------------------------------------------------------------------------------------
 * Hungarian target assignment (ABI 31): a batch of rectangular linear sum assignment problems, with the semantics of
 * `scipy.optimize.linear_sum_assignment(cost[p, :, :ncols[p]])` as the reference calls it per (decoder layer, sample) at
 * core/bbox/assigners/hungarian_assigner_3d.py:129 (detection boxes) and :165 (room layout) -- on the device, so that the
 * targets of a training step need no device -> host round trip and can be part of a captured graph.
 *   cost   f32 [P, R, Ccap]  (row pitch Ccap; columns >= ncols[p] of problem p are never read)
 *   ncols  i32 device [P]    valid columns of problem p, 0 <= ncols[p] <= Ccap
 *   match  i32 [P, R]        written in full: the column assigned to row r, or -1
 *   bad    i32 device scalar or NULL: 1 is ORed in when a problem holds a NaN or -inf among its valid entries, or has no
 *          finite assignment (scipy raises on both), or its ncols lies outside [0, Ccap]; that problem's rows are all -1.
 *          Never cleared by the kernel.
 * min(R, ncols[p]) rows are matched and the total cost is minimal; either side may be the longer one.  +inf entries are
 * legal ("this pair is forbidden").  Shortest augmenting paths (Jonker-Volgenant / Crouse 2016, scipy's algorithm) on the
 * orientation with fewer rows, duals and path costs in fp64 and in scipy's order of operations: with fp32 costs and a UNIQUE
 * optimum the result is scipy's, index for index.  Among several optima of equal total cost the choice may differ from
 * scipy's (tie rule of a search step: smallest path cost, then an unassigned column, then the lowest index).
 * One wavefront per problem (csrc/ver_assign.hip).  Supported: 1 <= R <= 1024, 0 <= Ccap <= 1024 (VER_EUNSUPPORTED beyond),
 * any P >= 0; P == 0 launches nothing, ncols[p] == 0 gives all -1.  One kernel launch, no memset node, no allocation.
 */
int ver_lsa_solve(const float* cost, const int32_t* ncols, int32_t* match, int32_t* bad,
                  int P, int R, int Ccap, void* stream);

/* ---------------------------------------------------------------------------------------
 * Detection mAP / mAR on the device (additive to ABI 31): rotated 3-D box IoU and the per-image matching of the indoor
 * protocol the reference evaluates detections with (MP3DDataset.evaluate, mp3docc_dataset.py:304-384, calling
 * datasets/indoor_eval.py:196 with iou_thr = (0.10, 0.25, 0.5, 0.75)).
 * Box format everywhere: f32 [.., 7] = (x, y, z_bottom, dx, dy, dz, yaw) -- what the head's _to_box_type produces and
 * LiDARInstance3DBoxes(..., origin=(0.5, 0.5, 0)) holds (box_type_3d = 'LiDAR', vocc.py:238).
 *
 * ver_box3d_overlaps: mmdet3d's BaseInstance3DBoxes.overlaps(mode='iou') as indoor_eval.py:102 calls it
 * (`pred_cur.overlaps(pred_cur, gt_cur)`: height overlap times the rotated BEV intersection), batched.
 *   a    f32 [S, Acap, 7]          b    f32 [S, Bcap, 7]
 *   na   i32 device [S] or NULL    nb   i32 device [S] or NULL   valid boxes of sample s; NULL: every slot is valid;
 *                                                                counts outside [0, cap] are clamped
 *   iou  f32 [S, Acap, Bcap], written in full; slots beyond the counts get 0
 *     h   = max(0, min(za + dza, zb + dzb) - max(za, zb))
 *     bev = area of the intersection of the rotated rectangles (x, y, dx, dy, yaw)
 *     o   = bev * h,    iou = o / max(dxa dya dza + dxb dyb dzb - o, 1e-8)
 * OUR DEFINITION where the reference's behaviour is undefined: a box with a non-finite entry or a dimension <= 0 overlaps
 * nothing -- IoU 0, never NaN (so does a pair whose volumes leave the fp32 range).
 * One launch, no memset node, no allocation, no host read.  S, Acap or Bcap == 0 launches nothing.
 */
int ver_box3d_overlaps(const float* a, const int32_t* na, const float* b, const int32_t* nb, float* iou,
                       int S, int Acap, int Bcap, void* stream);

/* ver_det_match: the per-image half of eval_det_cls (indoor_eval.py:54-143) for a batch in one launch.
 *   pred_boxes f32 [S, Pcap, 7], pred_labels i32 [S, Pcap], pred_scores f32 [S, Pcap], pred_valid u8 [S, Pcap]
 *   gt_boxes   f32 [S, Gcap, 7], gt_labels   i32 [S, Gcap], ngt i32 device [S] (clamped to [0, Gcap])
 *   thresholds HOST f32 [num_thresholds], 1 <= num_thresholds <= 8 (copied into the kernel arguments, as ver_occ_confusion)
 *   iou_max f32, gt_index i32, tp_bits u8: [S, Pcap], written in full
 *   npos    i64 [num_classes], ACCUMULATED and never cleared: npos[c] += valid ground truths of class c in the batch
 * For a valid prediction d of sample s with label c: gt_index = the ground truth of class c of the same sample with the
 * largest IoU (the first of equal maxima, the reference's `iou > iou_max`; a NaN never wins), iou_max = that IoU; without a
 * candidate gt_index = -1 and iou_max = 0.  Bit t of tp_bits is set iff iou_max > thresholds[t] (strict, as in the
 * reference) and no other valid prediction d' of the sample has the same gt_index, iou_max[d'] > thresholds[t] and goes
 * before d in the evaluation order: score descending, then slot ascending.  That is the reference's sequential "mark the
 * ground truth as detected" loop -- a later prediction whose best ground truth is taken is a false positive, it does not
 * fall back to its second best; the loop's `det` flags are per image and the global score order restricted to an image is
 * that image's score order, so the flags are resolved per sample, in parallel.
 * Predictions with pred_valid == 0 or a label outside [0, num_classes) match nothing (gt_index -1, tp_bits 0); ground
 * truths with a label outside the range are neither counted nor matched.  Only same-class pairs are clipped.
 * One workgroup per sample (csrc/ver_boxiou.hip).  Supported: 1 <= Pcap <= 1024, 0 <= Gcap <= 1024, Pcap * Gcap <= 16 384
 * (VER_EUNSUPPORTED beyond); S == 0 launches nothing; Gcap == 0 or ngt[s] == 0: every valid prediction is a false positive.
 * One launch, no memset node, no allocation, no host read.
 */
int ver_det_match(const float* pred_boxes, const int32_t* pred_labels, const float* pred_scores,
                  const uint8_t* pred_valid, const float* gt_boxes, const int32_t* gt_labels, const int32_t* ngt,
                  const float* thresholds, int num_thresholds, float* iou_max, int32_t* gt_index,
                  uint8_t* tp_bits, int64_t* npos, int num_classes, int S, int Pcap, int Gcap, void* stream);

/* ---------------------------------------------------------------------------------------
 * Detection set loss on the device (additive to ABI 31; csrc/ver_setloss.hip): with ver_lsa_solve between the first and the
 * second, these three take the decoder's outputs of ALL layers and samples to the matching costs, the per-layer focal and L1
 * sums and their gradients -- what the head's _assignment_costs, _targets_from_match and _losses_from_targets (and autograd
 * behind them) do in about fifty small torch launches (loss_single of the reference, head:903-976, per decoder layer).
 * Shared operands:
 *   cls          f32 | bf16 [L, B, Q, C] class logits (cls_dtype = VER_F32 | VER_BF16), or NULL: the room-layout form
 *                (assign(..., layout=True), head:760-841), regression terms alone; gt_labels may then be NULL too
 *   box          f32 [L, B, Q, box_ld] box codes, row pitch box_ld
 *   gt           f32 [B, Gcap, 9]      gravity centre, dims, yaw, velocity; rows >= counts[b] are padding, never read
 *   gt_labels    i64 [B, Gcap]
 *   counts       i32 device [B]        valid boxes of sample b (clamped to [0, Gcap])
 * n = normalize_bbox(gt) = (cx, cy, log w, log l, cz, log h, sin yaw, cos yaw, vx, vy).
 *
 * ver_det_costs: cost f32 [L, B, Q, Gcap], WRITTEN IN FULL; columns g >= counts[b] get 0.  For a valid column
 *     cost = w_cls * (pos - neg)[gt_labels[b, g]] + w_reg * sum_{k<8} |box_k - n_k|
 *     p = sigmoid(logit) in fp32;  pos = -log(p + eps) alpha (1 - p)^gamma;  neg = -log(1 - p + eps) (1 - alpha) p^gamma
 *   (FocalLossCost + BBox3DL1Cost as HungarianAssigner3D.assign states them); non-finite entries of n count as 0, as the
 *   nan_to_num of _assignment_costs does.  1 - p is formed without a subtraction (from exp(-|logit|)), so the cost stays
 *   finite and accurate where the fp32 torch chain's 1 - p has rounded to 0.  A label outside [0, C) in a valid column gives
 *   a NaN cost (the solver then flags the problem).  box_ld >= 8.
 *   One workgroup per (layer, sample); one launch, no memset node, no allocation, no host read; an empty dimension (L, B, Q
 *   or Gcap == 0) launches nothing.  Supported: Q, Gcap <= 1024 (the solver's limits), C <= 64; VER_EUNSUPPORTED beyond.
 *
 * ver_det_set_loss_forward: match i32 [L, B, Q] as ver_lsa_solve writes it; code_weights f32 [10]; sums f32 [2, L] and
 *   npos i32 [L], both WRITTEN, not accumulated.  Row (l, b, q): label = gt_labels[b, match] when match >= 0, else C
 *   (background, an all-zero one-hot).
 *     sums[0, l] = sum over the layer's rows and C logits of the sigmoid focal loss, losses.sigmoid_focal_loss element for
 *                  element: bce_with_logits(x, t) (alpha t + (1 - alpha)(1 - t)) pt^gamma, fp32 arithmetic (log1pf, IEEE
 *                  division) on bf16 logits too; 0 in the layout form
 *     sums[1, l] = sum of keep * code_weights[k] * |box_k - n_k| over k < 10, keep = matched AND all ten n_k finite (the
 *                  rows the reference drops by boolean indexing)
 *     npos[l]    = rows with match >= 0, whatever keep says
 *   The sums are bit-reproducible from run to run: one workgroup per layer, a fixed reduction order, no float atomics.
 *   A match outside [-1, counts[b]), or a matched label outside [0, C), makes that layer's two sums NaN and ORs 1 into
 *   `bad` (i32 device scalar or NULL; never cleared here); the other layers are unaffected.  box_ld >= 10.
 *   One launch, no memset node, no allocation, no host read.  L == 0 launches nothing.
 *
 * ver_det_set_loss_backward: the same operands; scale f32 DEVICE [2, L]; grad_cls in the dtype of cls [L, B, Q, C] (NULL in
 *   the layout form); grad_box f32 [L, B, Q, box_ld]; both WRITTEN IN FULL.
 *     grad_cls   = scale[0, l] * d focal / d logit
 *     grad_box_k = scale[1, l] * keep * code_weights[k] * sign(box_k - n_k), sign(0) = 0; 0 for k >= 10 and rows not kept
 *   The per-row terms are recomputed, nothing is saved by the forward.  A layer whose scale entry is exactly 0 gets exact
 *   zeros, even where its logits or codes are NaN; a row the forward flags counts as background / not kept.  One launch.
 */
int ver_det_costs(const void* cls, int cls_dtype, const float* box, int box_ld, const float* gt,
                  const int64_t* gt_labels, const int32_t* counts, float* cost, int L, int B, int Q, int C, int Gcap,
                  float w_cls, float alpha, float gamma, float eps, float w_reg, void* stream);
int ver_det_set_loss_forward(const void* cls, int cls_dtype, const float* box, int box_ld, const int32_t* match,
                             const float* gt, const int64_t* gt_labels, const int32_t* counts,
                             const float* code_weights, float* sums, int32_t* npos, int32_t* bad, int L, int B, int Q,
                             int C, int Gcap, float alpha, float gamma, void* stream);
int ver_det_set_loss_backward(const void* cls, int cls_dtype, const float* box, int box_ld, const int32_t* match,
                              const float* gt, const int64_t* gt_labels, const int32_t* counts,
                              const float* code_weights, const float* scale, void* grad_cls, float* grad_box, int L,
                              int B, int Q, int C, int Gcap, float alpha, float gamma, void* stream);

/* ---------------------------------------------------------------------------------------
 * Detection decoding on the device (additive to ABI 31; csrc/ver_decode.hip): the reference's NMSFreeCoder.decode
 * (core/bbox/coders/nms_free_coder.py:9-122: sigmoid, top-k over the flattened [Q * C] scores, label = index % C, query =
 * index / C, denormalize_bbox of core/bbox/util.py:4-55, centre-range and score masks) for a whole batch in fixed shapes,
 * with the bottom-centre shift of the head's _to_box_type (head:1466-1471) -- what stands between the decoder's outputs and
 * ver_det_match.  In place of the torch chain of NMSFreeCoder.decode_padded + head.get_bboxes_padded.
 *   cls          f32 | bf16 [B, Q, C] class logits of ONE decoder layer (cls_dtype = VER_F32 | VER_BF16), or NULL: the
 *                layout form below
 *   box          f32 [B, Q, box_ld] normalised codes (cx, cy, log w, log l, cz, log h, sin, cos[, vx, vy]), row pitch box_ld
 *   codes        8 or 10 (with the velocity), codes <= box_ld
 *   center_range HOST f32[6] (x, y, z lower ends, then the upper ends; copied into the kernel arguments)
 *   out_boxes f32 [B, K, codes - 1], out_scores f32 [B, K], out_labels i32 [B, K], out_valid u8 [B, K], out_query i32 [B, K]
 *                or NULL: all written in full
 * SELECTION.  Slot j of sample b holds the j-th entry of the sample's Q * C logits in this order: LOGIT DESCENDING, FLAT INDEX
 * q * C + c ASCENDING AMONG EQUAL LOGITS.  A NaN logit comes after every number; -0.0 equals +0.0; bf16 logits are widened
 * to fp32 first (exact).  The fp32 sigmoid 1 / (1 + exp(-x)) is non-decreasing in x, so the K first entries of this order
 * always are one of the top-k sets `topk` over the sigmoid scores may return, in a score-descending order -- the only one
 * wherever the K + 1 best scores are distinct.  Where `topk` has a choice (torch promises no order among equal values, and
 * under bf16 autocast equal logits are the rule) the choice is stated here: the lower flat index.  That also covers
 * saturation: every logit above about 17 scores exactly 1.0 in fp32, and such slots are still ordered by their logits.
 * PER SLOT.  idx = the selected flat index:  score = sigmoid(logit) in fp32;  label = idx % C;  query = idx / C (the reference's
 * bbox_index);  box = (cx, cy, cz, exp(log w), exp(log l), exp(log h), atan2(sin, cos)[, vx, vy]) of that query's codes.
 *   flags & 1: z = cz - h / 2 (bottom centre);   flags & 2: score_threshold is in force.
 *   valid = the gravity centre lies inside center_range (six inclusive comparisons, before the z shift)
 *           AND (flags & 2 == 0 OR score > score_threshold) AND the logit is not a NaN (OUR DEFINITION: torch sorts a NaN
 *           first).  Boxes, scores and labels are written for the invalid slots too.
 * LAYOUT FORM (cls == NULL; LayoutCoder.decode, layout_coder.py): K == Q and slot j is query j; scores and labels are written
 * as 0, valid is the range test alone; cls_dtype and C are not looked at.
 * One workgroup per sample: a bitonic sort of 64-bit (order word, flat index) keys in LDS, then one thread per slot.
 * Supported: 0 <= K <= min(Q * C, 1024), Q * C <= 16 384 (VER_EUNSUPPORTED beyond; K > Q * C is VER_EINVAL); B == 0 or K == 0
 * launches nothing.  One launch, no memset node, no allocation, no host read.
 */
int ver_det_decode(const void* cls, int cls_dtype, const float* box, int box_ld, float* out_boxes, float* out_scores,
                   int32_t* out_labels, uint8_t* out_valid, int32_t* out_query, const float* center_range,
                   float score_threshold, int flags, int B, int Q, int C, int K, int codes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Occupancy targets on the device (additive to ABI 31; csrc/ver_targets.hip): the dataset's sparse occupancy annotation of a
 * whole batch -> one byte label per voxel and the number of occupied voxels, in place of the reference's per-sample
 * `gt_occupancy = full(voxel_num, classes); gt_occupancy[idx] = cls` on an int64 volume (head:1322-1326, :1404-1408) and of
 * the label volume of MP3DDataset.evaluate_occ_iou (mp3docc_dataset.py:500-514).
 *   pairs           i32 | i64 [n_total][2] (flat voxel index, class) of all samples, one after the other (pair_dtype =
 *                   VER_I32 | VER_I64; aligned to one pair); may be NULL when n_total == 0
 *   offsets         i32 device [bs + 1]: sample b owns pairs [offsets[b], offsets[b+1]); clamped into [0, n_total];
 *                   an empty sample is legal
 *   invalid         i32 | i64 [n_invalid] flat voxel indices (invalid_dtype), invalid_offsets i32 device [bs + 1]; both may
 *                   be NULL when n_invalid == 0: the evaluation form
 *   row_table       i32 [voxel_num / zdim][3] = (group offset, group n_rows, index within the group) of every lattice
 *                   position q, or NULL.  The label of sample b, voxel v = z * rows + q (rows = voxel_num / zdim; the
 *                   reference's (Z, X, Y) order) is byte (bs * off[q] + b * n[q] + loc[q]) * zdim + z -- the group-major row
 *                   order the occupancy GEMMs leave their rows in (dense_heads/occ_proj_lattice.py) -- and byte
 *                   b * voxel_num + v with a NULL table.  The table does not depend on bs.  A table entry that points
 *                   outside the buffer writes nothing and counts in bad[0].
 *   labels          u8 [bs * voxel_num], 4-byte aligned and ALLOCATED ROUNDED UP to a multiple of 4 bytes; written in full,
 *                   whatever it held (the padding bytes too)
 *   count           i32 [bs + 1], written: occupied voxels of every sample, then their total
 *   bad             i32 [2], written (see below)
 * SEMANTICS.  Every voxel starts as `classes` (empty).  A pair (v, c) with 0 <= v < voxel_num and 0 <= c < classes sets voxel
 * v of its sample to c; c == classes names the empty label and writes nothing; any other pair is skipped and counted in bad[0]
 * (the reference raises there).  With distinct voxel indices per sample the result is the reference's, byte for byte.
 * OUR DEFINITION where the reference's is undefined (a voxel listed several times: on a GPU its index_put_ leaves the winner
 * open, on the CPU the last pair stays): the LARGEST class stays, whatever the order of the pairs.  bad[1] = the number of
 * pairs (c < classes) whose voxel ends up with another class than theirs -- the listings that lost; 0 exactly when no voxel
 * is listed with two different classes, and independent of the order of the pairs.  Repeats of one class count nothing.
 * count[b] counts the voxels of sample b that left the empty state, each once: (labels < classes).sum() per sample before
 * the invalid pass, exact under repeats.
 * Invalid voxels are set to 255 after all pairs, in a later kernel of the same call, and override any pair; out-of-range
 * entries count in bad[0].  count stays the pairs' count (the evaluation never reads it).
 * Per-byte read-modify-write = a 32-bit compare-and-swap on the aligned word holding the byte (relaxed, agent scope).  Four
 * launches at most (fill, pairs, verify, invalid), the fill being a kernel: no memset node, no allocation, no host read --
 * the call can be captured.  Supported: bs * voxel_num < 2^31, classes < 255, voxel_num % zdim == 0, bs < 65 536
 * (VER_EUNSUPPORTED beyond); bs == 0 returns 0 and launches nothing.
 */
int ver_occ_targets(const void* pairs, int pair_dtype, const int32_t* offsets, long n_total, const void* invalid,
                    int invalid_dtype, const int32_t* invalid_offsets, long n_invalid, const int32_t* row_table,
                    uint8_t* labels, int32_t* count, int32_t* bad, long voxel_num, int zdim, int classes, int bs,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * Decoder 3-D deformable attention from the raw Linear outputs (additive to ABI 31; csrc/ver_dattn3d.hip): the reference's
 * VoxelCustomMSDeformableAttention.forward between its three input Linears and output_proj
 * (bevformer/modules/voxel_decoder.py:234-337) around voxel_multi_scale_deformable_attn_pytorch
 * (voxel_temporal_self_attention.py:275-335) -- ver_msda3d_* with the softmax over the points and the sampling-location
 * arithmetic inside the kernel, as ver_sca_* are to ver_msda_*.
 *   value        f32 | bf16 [B, num_keys, heads, head_dim]     output of value_proj (value_dtype: 0 f32, 1 bf16)
 *   shapes_dhw   i64 device [levels, 3] = (D, H, W);  level_start i64 device [levels]      as for ver_msda3d_forward
 *   ref          f32 [B, Nq, levels, 3]                        (x, y, z) in [0, 1]
 *   offsets      f32 | bf16 [B, Nq, heads, levels, points, 3]  raw Linear output (q_dtype)
 *   logits       f32 | bf16 [B, Nq, heads, levels*points]      pre-softmax (q_dtype, the same as offsets)
 *   out          f32 | bf16 [B, Nq, heads*head_dim]            written in full (out_dtype)
 * All arithmetic is fp32, bf16 operands are widened first:
 *   w   = softmax(logits) over the levels*points entries of a (query, head), the maximum subtracted
 *   loc = ref[b,q,l] + offsets[b,q,h,l,p] / (W_l, H_l, D_l)          (the division, then the add)
 *   out[b,q,h,:] = sum_{l,p} w * trilinear(value_l, loc)             (exactly ver_msda3d_forward's sampling: pixel =
 *                  loc*size - 0.5, zeros outside, flat key (z*H + y)*W + x)
 * ver_dattn3d_backward takes the same operands plus grad_out [B, Nq, heads*head_dim] in out_dtype and WRITES IN FULL, whatever
 * the buffers held (the caller zeroes nothing):
 *   grad_value   value_dtype, as value.  No float atomics: every cell is summed in fp32 by one wave in ascending (query,
 *                level, point, corner) order and rounded once -- the same inputs give the same bits on every run
 *   grad_offsets q_dtype, as offsets  = grad_loc / (W, H, D)
 *   grad_logits  q_dtype, as logits   = w * (g_w - sum(w * g_w)), the softmax backward;  g_w and grad_loc are
 *                ver_msda3d_backward's grad_attn_w and grad_loc
 *   grad_ref     f32 [B, Nq, levels, 3] or NULL (not wanted): grad_loc summed over the heads (ascending), then the points,
 *                in that fixed order
 * One launch forward, two backward; no memset node, no allocation, no host read, no workspace: the calls can be captured.
 * B == 0 or Nq == 0: VER_OK, nothing is launched and no pointer is looked at.  Another null pointer: VER_EINVAL.
 * Supported (VER_EUNSUPPORTED beyond; ver_dattn3d_supported answers 1 / 0 for a shape without touching the device):
 * levels*points <= 32, head_dim <= 128, heads <= 64, and B*Nq*heads and B*heads*ceil(num_keys/64) below 2^31.  The level
 * geometry lives on the device and is not validated: sum(D*H*W) must equal num_keys (keys are clamped into the volume for
 * reads and dropped for writes, so a wrong geometry gives wrong numbers, not a fault).
 */
int ver_dattn3d_supported(int B, int num_keys, int heads, int head_dim, int levels, int points, int Nq);
int ver_dattn3d_forward(const void* value, int value_dtype, const int64_t* shapes_dhw, const int64_t* level_start,
                        const float* ref, const void* offsets, const void* logits, int q_dtype, void* out, int out_dtype,
                        int B, int num_keys, int heads, int head_dim, int levels, int points, int Nq, void* stream);
int ver_dattn3d_backward(const void* value, int value_dtype, const int64_t* shapes_dhw, const int64_t* level_start,
                         const float* ref, const void* offsets, const void* logits, int q_dtype, const void* grad_out,
                         int out_dtype, void* grad_value, void* grad_offsets, void* grad_logits, float* grad_ref,
                         int B, int num_keys, int heads, int head_dim, int levels, int points, int Nq, void* stream);

/* ---------------------------------------------------------------------------------------
 * Decoder self-attention between the input projections and out_proj (additive to ABI 31; csrc/ver_mha.hip): what
 * torch.nn.MultiheadAttention (the mmcv MultiheadAttention wrapper of vocc.py's DetrTransformerDecoderLayer, called with
 * need_weights=True) runs between its in-projection Linears and out_proj -- head transposes, q scaling, bmm, softmax,
 * dropout, bmm, transpose back -- without the head-averaged weights nobody reads.  No masks.
 *   q            f32 | bf16 [Nq, B, heads*head_dim]   row pitch ldq: ELEMENTS between consecutive (n, b) rows, so q and k
 *   k, v         as q       [Nk, B, heads*head_dim]   (pitches ldk, ldv) may be column halves of one [N, B, 2C] GEMM output
 *   seed         i64 device [1]                       may be NULL when p_drop == 0
 *   out          as q       [Nq, B, heads*head_dim]   dense, written in full
 *   lse          f32        [B, heads, Nq]            the row's max + log(sum exp), saved for the backward
 * All arithmetic outside the matrix products is fp32:
 *   S[i,j]  = (q_i . k_j) / sqrt(head_dim)            the scale on the fp32 product, not on a rounded q
 *   P       = softmax_j(S), the row maximum subtracted
 *   Pd[i,j] = keep(idx, seed) ? P[i,j] / (1 - p_drop) : 0,   idx = ((b*heads + h)*Nq + i)*Nk + j;  keep, thresh and scale
 *             are ver_add_ln_forward's (the murmur finaliser, thresh = (uint32_t)((1.0f - p_drop) * 16777216.0f))
 *   out[i,b,h,:] = sum_j Pd[i,j] * v[j,b,h,:]
 * bf16 operands: the products run on v_mfma_f32_16x16x32_bf16 with fp32 accumulators; P / Pd and dS are rounded to bf16
 * (RNE) only as MFMA operands; ragged sizes are padded in LDS.  fp32 operands: fp32 VALU products.
 * ver_mha_backward takes the same operands plus grad_out (dense, operand dtype), lse, seed and p_drop, recomputes S and P
 * from q, k and lse with the same keep decisions, and WRITES IN FULL grad_q, grad_k, grad_v (operand dtype, pitches ldgq,
 * ldgk, ldgv: grad_q and grad_k may be the halves of one [N, B, 2C] buffer):
 *   dV = Pd^T dO;  dPd = dO V^T;  dP = keep ? dPd / (1 - p) : 0;  dS = P * (dP - sum_j(dP * P));
 *   dQ = dS K / sqrt(hd);  dK = dS^T Q / sqrt(hd)
 * One workgroup owns a whole (b, head): no float atomics, no workspace, nothing for the caller to zero; every gradient
 * element is written exactly once in a fixed summation order -- the same inputs give the same bits on every run, and a
 * sample's result does not depend on B or on its place in the batch (apart from idx under dropout).
 * One launch forward, one backward; no memset node, no allocation, no host read: both calls can be captured.
 * B == 0 or Nq == 0: VER_OK, nothing is launched and no pointer is looked at.  Nk == 0 with Nq > 0, another null pointer, a
 * dtype other than 0 (f32) / 1 (bf16), or a q / k / v / grad_out that is not 16-byte aligned: VER_EINVAL.
 * Supported (VER_EUNSUPPORTED beyond, the message names the limit; ver_mha_supported answers 1 / 0 for a shape, for both
 * dtypes and both directions, without touching the device): 1 <= Nq, Nk <= 128; head_dim a multiple of 8 up to 128; every
 * pitch a multiple of 8 and at least heads*head_dim; B*heads < 2^31; 0 <= p_drop < 1.
 */
int ver_mha_supported(int B, int heads, int head_dim, int Nq, int Nk);
int ver_mha_forward(const void* q, const void* k, const void* v, int dtype, long ldq, long ldk, long ldv,
                    const int64_t* seed, float p_drop, void* out, float* lse, int B, int heads, int head_dim, int Nq, int Nk,
                    void* stream);
int ver_mha_backward(const void* q, const void* k, const void* v, int dtype, long ldq, long ldk, long ldv,
                     const void* grad_out, const float* lse, const int64_t* seed, float p_drop, void* grad_q, void* grad_k,
                     void* grad_v, long ldgq, long ldgk, long ldgv, int B, int heads, int head_dim, int Nq, int Nk,
                     void* stream);

/* ---------------------------------------------------------------------------------------
 * Occupancy pairs from byte labels (additive to ABI 31; csrc/ver_pairs.hip): the inverse of ver_occ_targets, and the tail of
 * VoxelFormerOccupancyHead.get_occupancy_prediction (head:1535-1540: idx = where(cls < C); stack(idx, cls[idx])) in fixed
 * shapes -- the class bytes of a batch become per-sample sparse (voxel index, class) pairs with offsets, the layout
 * ver_occ_targets takes, without a host read of the pair count.
 *   labels       u8 [bs * voxel_num]: with row_table == NULL in the reference's (Z, X, Y) voxel order (byte b * voxel_num + v);
 *                with a table in the group-major row order of the occupancy GEMMs, the byte of (sample b, voxel v) being where
 *                ver_occ_targets puts it (see there).  A table entry that points outside the buffer reads as empty.
 *   row_table    i32 [voxel_num / zdim][3] or NULL, as for ver_occ_targets
 *   pairs        i32 | i64 [capacity][2] (pair_dtype = VER_I32 | VER_I64; aligned to one pair; may be NULL when capacity == 0):
 *                (voxel index within the sample, class) of every occupied voxel, ascending within a sample, sample after
 *                sample.  Only the first min(total, capacity) pairs are written; what lies behind them is left as it was.
 *   offsets      i32 [bs + 1], written: exclusive prefix sums of the per-sample counts, each clamped to `capacity` -- sample b
 *                owns pairs [offsets[b], offsets[b+1]), and no slice reaches past the buffer
 *   count        i32 [bs + 2], written: the true occupied count of every sample, their true total, then 1 when the total
 *                exceeded `capacity` and 0 when not (written, not ORed)
 *   block_work   i32 [ver_occ_pairs_blocks(bs, voxel_num)] scratch; a workgroup covers ver_occ_pairs_block_size() consecutive
 *                voxels of one sample
 *   flags        bit 0: add b * voxel_num to the voxel index -- the index over the flattened batch
 * A byte < classes is an occupied voxel; `classes` (empty) and anything above (255 = invalid) produce nothing.  Integer
 * results: bit-exact.  Three launches (block counts, one scan, ordered compaction), plain vector stores, no memset node, no
 * allocation, no host read: the call can be captured.  bs == 0 or voxel_num == 0: VER_OK, nothing is launched and no pointer
 * is looked at.  Supported: bs * voxel_num < 2^31 (so flattened indices fit int32 pairs too), classes < 255,
 * voxel_num % zdim == 0, bs < 65 536, capacity < 2^31 (VER_EUNSUPPORTED beyond); negative sizes, zdim < 1, classes < 1, an
 * unknown dtype or flag, a null or misaligned pointer: VER_EINVAL.
 */
long ver_occ_pairs_block_size(void);
long ver_occ_pairs_blocks(int bs, long voxel_num);
int  ver_occ_pairs(const uint8_t* labels, const int32_t* row_table, void* pairs, int pair_dtype, int32_t* offsets,
                   int32_t* count, int32_t* block_work, long capacity, long voxel_num, int zdim, int classes, int bs,
                   int flags, void* stream);

/* ---------------------------------------------------------------------------------------
 * A batch out of a device-resident viewpoint store, by index (additive to ABI 31; csrc/ver_fetch.hip).  The reference keeps
 * the feature maps it has read in a host dict (detectors/voxelformer.py:317-325) and re-reads the occupancy annotation on
 * every step; here the whole split lives in device memory and a step's batch is gathered straight into the static buffers
 * of a captured step, the only host -> device traffic being the index vector.
 *   index        i32 [bs], device memory: read by the kernels, never by the host.  A value outside [0, V) makes an EMPTY
 *                sample: zero feature and camera rows, count 0, no pairs; nothing is read outside the store.
 * Four groups, each may be absent (all of its pointers NULL):
 *  features      feat_store f32 | bf16 [V, ncam, row] -> feat_out [ncam, bs, row], same dtype (feat_dtype = VER_F32 |
 *                VER_BF16): a pure copy, bit for bit, with 64-bit element offsets and the widest access (16, 8, 4 or 2 bytes)
 *                that divides the row bytes and both base addresses; any row >= 1 works (row == 0 copies nothing).
 *  cameras       w2p_store f32 [V, ncam, 4, 4] -> w2p_out [bs, ncam, 4, 4];  origin_store f32 [V, 3] -> origin_out [bs, 3]
 *  boxes         box_store f32 [V, store_cap, box_dim], label_store i64 [V, store_cap], count_store i32 [V] ->
 *                box_out f32 [bs, out_cap, box_dim], label_out i64 [bs, out_cap], count_out i32 [bs] (a PaddedGts): the first
 *                min(count, out_cap) rows of a sample are copied and count_out[b] is that minimum; columns at or past it are
 *                left as they were.  box_store / label_store may be NULL when store_cap == 0, box_out / label_out when
 *                out_cap == 0.  (A stored count is read as clamped to [0, store_cap].)
 *  pairs         CSR: pair_store i32 [pair_total][2], pair_offsets i64 [V + 1] -> offsets_out i32 [bs + 1], pairs_out i32
 *                [pair_capacity][2] (the views of a PackedOccGts): offsets are the exclusive prefix sums of the fetched
 *                lengths, each clamped to pair_capacity; the pairs of sample b are copied in order into
 *                [offsets[b], offsets[b+1]); pairs past the capacity are dropped; what lies behind the live pairs is left as
 *                it was.  pair_store may be NULL when pair_total == 0, pairs_out when pair_capacity == 0.  (CSR bounds are
 *                read as clamped to [0, pair_total] and never descending.)
 *   status       i32 [4], written in full by every call (never ORed, no zeroing needed): [0] samples whose index was outside
 *                [0, V); [1] samples whose box count exceeded out_cap; [2] 1 if the pairs overflowed pair_capacity, else 0;
 *                [3] the true pair total, saturated at 2^31 - 1.  Words of an absent group are 0.
 * At most four launches (a one-workgroup scan of the bs lengths, then the copies of the present groups), plain vector
 * stores, no memset node, no allocation, no host read: the call can be captured, and a replay after the index buffer changed
 * fetches the new batch.  ver_fetch_pair_tile(): the output pair slots one workgroup of the pair copy covers.
 * bs == 0: VER_OK, nothing is launched and no pointer is looked at.  Negative sizes, an unknown dtype, a null index or
 * status, a null or misaligned pointer of a present group (features: one element; pairs and labels: 8 bytes; else 4):
 * VER_EINVAL.  bs >= 65 536, ncam >= 65 536 or pair_capacity >= 2^31: VER_EUNSUPPORTED.
 */
long ver_fetch_pair_tile(void);
int  ver_fetch_batch(const int32_t* index, int bs, long V, int ncam, const void* feat_store, void* feat_out, int feat_dtype,
                     long row, const float* w2p_store, const float* origin_store, float* w2p_out, float* origin_out,
                     const float* box_store, const int64_t* label_store, const int32_t* count_store, float* box_out,
                     int64_t* label_out, int32_t* count_out, int store_cap, int out_cap, int box_dim,
                     const int32_t* pair_store, const int64_t* pair_offsets, long pair_total, int32_t* offsets_out,
                     int32_t* pairs_out, long pair_capacity, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VER_OPS_H */
