/*
 * smot_emm.h — C ABI of libsmot_emm.so, the MI355X (gfx950) implementation of the SiamMOT
 * EMM tracker-head hot path.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * amazon-science/siam-mot root; [UPSTREAM] = facebookresearch/maskrcnn-benchmark, the
 * reference's un-vendored native substrate).
 *
 * Conventions:
 *   - all tensors are contiguous fp32, NCHW (the *_typed_* entry points at the end also take fp16 / bf16
 *     feature MAPS); boxes are fp32 xyxy pixels; device pointers unless the parameter is documented as
 *     a HOST array;
 *   - the caller owns every buffer (outputs and workspaces included); nothing is allocated,
 *     nothing persists between calls, no host synchronisation happens inside;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: 0 on success, a negative SMOT_ERR_* for argument/shape errors, or a positive
 *     hipError_t if the launch failed; smot_last_error() gives a message for the calling thread.
 *     The Python host layer turns non-zero into RuntimeError (the reference's native ops raise
 *     RuntimeError through TORCH_CHECK).
 */
#ifndef SMOT_EMM_H
#define SMOT_EMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* smot_stream_t; /* hipStream_t */

#define SMOT_OK 0
#define SMOT_ERR_BAD_ARG (-1)      /* null pointer, non-positive size, inconsistent shapes */
#define SMOT_ERR_UNSUPPORTED (-2)  /* legal in the reference but not implemented here (documented per call) */

#define SMOT_MAX_LEVELS 8
#define SMOT_MAX_IMAGES 64          /* images per call of the batched head (smot_emm_*_batched_fwd) and solver */
/* ABI history.
 * 10: the image of smot_emm_tower_pack grew (fp32 image + three-part bf16 image: ask smot_emm_tower_pack_floats), an image
 *     packed by a version-9 library is too short for this one; smot_emm_tower_form added.  (9: order-hint entries of 528 floats)
 * 11: smot_frame_args grew by the six carry_* pointers and carry_src_row0 / carry_rows / carry_dst_row0 (SMOT_STAGE_CARRY);
 *     smot_track_solve_carry_fwd and smot_memory_carry_fwd added.
 * 12: order-hint entries of 536 floats — behind the tables every entry carries the by-roi record the consumer VERIFIES against
 *     its own boxes / search regions, and entry 0 the list's status word; the geometry stamp includes the level's scale;
 *     smot_emm_track_fwd writes NaN rows when the verification fails; record word 6 of the solver became a bit field;
 *     smot_emm_order_hint_status added.
 * 13: the second image of smot_emm_tower_pack is the TWO-part fp16 image (C/32 + 1 rotated blocks of 8192 floats per
 *     16-channel tile) followed by a four-word header {largest |w| bits, 2^-ku, 0, 0}: ask smot_emm_tower_pack_floats — an
 *     image packed by a version-12 library has another size and layout; smot_emm_tower_form returns 3 at every track count
 *     (one form); smot_emm_predictor_fwd may use the head of its `logits` output as scratch before it writes the logits;
 *     smot_sr_xcorr_fused_fwd / smot_emm_track_fwd correlate on the matrix cores (no signature change: responses equal
 *     smot_xcorr_dw_fwd's to rounding, not bit for bit).
 * 14: smot_emm_track_batched_fwd / smot_emm_extract_cache_batched_fwd and SMOT_MAX_IMAGES added (several images per
 *     call); existing entry points unchanged.
 *     Added since without a new version (every existing symbol, struct and layout unchanged; a host layer asks for the
 *     symbols it needs): the _typed_ entry points, smot_rpn_proposals_*, smot_box_detect_post_*, and the box head over
 *     several images: smot_roi_align_levels_batched_typed_fwd, smot_box_detect_post_batched_ws_bytes,
 *     smot_box_detect_post_batched_fwd; the frames of several cameras in one call: smot_preprocess_batch_fwd; the track
 *     solver over several images: smot_track_solve_batched_fwd; the RPN head and anchors: smot_rpn_head_*,
 *     smot_rpn_anchors_fwd; the feature pyramid: smot_fpn_packed_floats, smot_fpn_pack, smot_fpn_ws_bytes, smot_fpn_fwd;
 *     the DLA backbone body: smot_dla_packed_floats, smot_dla_pack, smot_dla_ws_bytes, smot_dla_fwd and its operators alone:
 *     smot_dla_conv_packed_floats, smot_dla_conv3x3_fwd, smot_dla_conv3x3_form, smot_dla_conv1x1_fwd, smot_dla_stem_ws_bytes, smot_dla_stem_fwd;
 *     the body with split operands: smot_dla_split_packed_floats, smot_dla_split_pack, smot_dla_split_fwd,
 *     smot_dla_conv_split_packed_floats, smot_dla_conv3x3_split_fwd, smot_dla_conv3x3_split_form;
 *     the bodies of either block type: smot_dla_net_*, smot_dla_conv1x1_res_fwd; the bodies in half compute mode:
 *     smot_dla_half_packed_floats, smot_dla_half_pack, smot_dla_half_fwd, smot_dla_conv_half_packed_floats,
 *     smot_dla_conv3x3_half_fwd, smot_dla_conv3x3_half_form, smot_dla_conv1x1_half_fwd; the feature pyramid and the RPN head
 *     in half compute mode: smot_fpn_half_packed_floats, smot_fpn_half_pack, smot_fpn_half_fwd,
 *     smot_rpn_head_half_packed_floats, smot_rpn_head_half_pack, smot_rpn_head_half_fwd; the bodies in half compute mode with
 *     the maps between layers stored in the compute type: smot_dla_half_storage_ws_bytes, smot_dla_half_storage_fwd,
 *     smot_dla_conv3x3_half_storage_fwd, smot_dla_conv1x1_half_storage_fwd.
 */
#define SMOT_ABI_VERSION 14

/* ABI version of the loaded library (checked by the host layer at load time). */
int smot_abi_version(void);

/* Build flavour of the loaded library.  bit 0 = measurement build (libsmot_emm_debug.so, compiled with
 * -DSMOT_DEBUG): kernel A/B switches and timing ablations exist and smot_debug_set_knob() is exported.  The
 * product library (libsmot_emm.so) returns 0: it reads no environment variable and contains no switch that
 * changes which kernel runs or what it computes. */
int smot_build_info(void);

#ifdef SMOT_DEBUG
/* Measurement library only: set one A/B or ablation switch by its SMOT_* name (csrc/knobs.h), value spelled as
 * the environment variable would be.  The environment itself is read once, when the library is loaded. */
int smot_debug_set_knob(const char* name, const char* value);
/* Measurement library only: smot_sr_xcorr_fused_fwd (Rx = 30, Rz = 15, sampling_ratio = 2) WITH an order hint (see
 * smot_emm_track_fwd below), for phase traces and A/B runs of that kernel alone. */
int smot_debug_sr_xcorr_fused_hint_fwd(const float* const* feats, const int* heights, const int* widths,
                                       const int* pad_cells, const float* scales, int num_levels, int C,
                                       const float* boxes, const float* sr, const float* templates, int N,
                                       float* resp, const float* order_hint, smot_stream_t stream);
/* Measurement library only: smot_linear_rows_fwd's layer on up to smot_box_refine_batched_max_rows() rows, in the form
 * smot_box_refine_batched_typed_fwd runs it (row blocks of 128 in the same two launches) — for the test that row r equals,
 * bit for bit, what smot_linear_rows_fwd gives for it in any call of at most 128 rows.  K % 4 == 0. */
long long smot_debug_linear_rows_blocks_ws_floats(int M, int K, int N);
int smot_debug_linear_rows_blocks_fwd(const float* x, int M, int K, const float* W, const float* bias, int N, int relu,
                                      float* ws, float* y, int ldy, smot_stream_t stream);
#endif

/* Message describing the last non-zero return on the calling thread ("" if none). */
const char* smot_last_error(void);

/*
 * FPN-level-routed ROIAlign with VIRTUAL zero padding.
 *
 * Replaces: SRPooler.forward (siammot/modelling/track_head/EMM/sr_pool.py:53-91) =
 *   LevelMapper [UPSTREAM modeling/poolers.py] + 4x torch.nonzero + per-level
 *   ROIAlign.forward -> _C.roi_align_forward(input, rois, spatial_scale, pooled_h, pooled_w,
 *   sampling_ratio) [UPSTREAM csrc/cuda/ROIAlign_cuda.cu, layers/roi_align.py], AND the
 *   TrackUtils.pad_feature zero-padding (track_head/track_utils.py:87-107) that precedes it in
 *   EMM.forward (EMM/track_core.py:49): level l is treated as if padded by pad_cells[l] zero
 *   cells on every side, without materialising the padded map.
 *
 *   feats[l]      device [1, C, heights[l], widths[l]]   (HOST array of num_levels device pointers)
 *   heights, widths, pad_cells, scales : HOST arrays [num_levels]
 *   rois          device [R,4]  boxes that are pooled, in PADDED-image pixels (xyxy)
 *   level_boxes   device [R,4]  boxes whose area picks the level (the TEMPLATE boxes in the
 *                 reference; pass rois again for the template pooler / a plain Pooler)
 *   out           device [R, C, out_h, out_w]
 *   levels_out    device [R] int32 or NULL: the level chosen per roi (diagnostics/tests)
 *
 * num_levels == 1 skips the level mapping (sr_pool.py:70-71).
 * Level rule: floor(4 + log2(sqrt(area)/224 + 1e-6)) clamped to
 *   [-log2(scales[0]), -log2(scales[L-1])], area with the upstream +1 convention.
 * SMOT_ERR_UNSUPPORTED: sampling_ratio <= 0 (adaptive grid) or > 4.
 */
int smot_roi_align_levels_fwd(const float* const* feats, const int* heights, const int* widths,
                              const int* pad_cells, const float* scales, int num_levels, int C,
                              const float* rois, const float* level_boxes, int R,
                              int out_h, int out_w, int sampling_ratio,
                              float* out, int32_t* levels_out, smot_stream_t stream);

/*
 * Single-level ROIAlign with upstream's native signature (SURVEY.md §8(b) "Native boundary").
 *
 * Replaces: [UPSTREAM] maskrcnn_benchmark._C.roi_align_forward(Tensor input, Tensor rois, float spatial_scale,
 *   int pooled_h, int pooled_w, int sampling_ratio) -> Tensor, the call inside layers/roi_align.py::ROIAlign.forward
 *   that the reference reaches through SRPooler (EMM/sr_pool.py:28-31,89) and the box head's Pooler
 *   (box_head/box_head.py:46): legacy (non-"aligned") ROIAlign, sampling_ratio x sampling_ratio samples per bin.
 *
 *   input   device [num_images, C, H, W] contiguous
 *   rois5   device [R,5] = (image index, x1, y1, x2, y2), the tensor convert_to_roi_format builds (sr_pool.py:40-51);
 *           the image index is honoured (a row whose index is outside [0, num_images) pools to zeros — upstream reads
 *           out of bounds there)
 *   out     device [R, C, pooled_h, pooled_w], caller-allocated
 *   pad_cells  0 for upstream's behaviour; > 0 treats the map as zero-padded by that many cells on every side
 *           (TrackUtils.pad_feature, track_utils.py:87-107) with rois in padded coordinates, without the padded copy.
 * SMOT_ERR_UNSUPPORTED: sampling_ratio <= 0 (adaptive grid) or > 4.  The reference-side monkey patch is in
 * INTEGRATION.md §2.
 */
int smot_roi_align_fwd(const float* input, int num_images, int C, int H, int W, int pad_cells,
                       const float* rois5, int R, float spatial_scale, int pooled_h, int pooled_w,
                       int sampling_ratio, float* out, smot_stream_t stream);

/*
 * Search-region boxes from template boxes.
 *
 * Replaces: TrackUtils.update_boxes_in_pad_images + TrackUtils.extend_bbox
 *   (track_head/track_utils.py:109-135, :62-85) as called by EMM.extract_cache
 *   (EMM/track_core.py:94-95).  search_expansion = SEARCH_REGION - 1 (track_utils.py:260).
 *   boxes device [N,4] -> sr device [N,4] (padded-image coordinates).
 */
int smot_search_region_fwd(const float* boxes, int N, float pad_pixels, float search_expansion,
                           float min_search_wh, float* sr, smot_stream_t stream);

/*
 * Depthwise (per-track x per-channel) valid cross-correlation.
 *
 * Replaces: xcorr_depthwise(x, kernel) (EMM/xcorr.py:37-46; F.conv2d with groups = N*C).
 *   x [N,C,Rx,Rx], z [N,C,Rz,Rz] -> out [N,C,Ho,Ho], Ho = Rx-Rz+1,
 *   out[n,c,i,j] = sum_{u,v} x[n,c,i+u,j+v] * z[n,c,u,v]   (u-major, v-minor fp32 FMA chain).
 * Algorithmic HBM bytes: 4*N*C*(Rx^2 + Rz^2 + Ho^2).
 */
int smot_xcorr_dw_fwd(const float* x, const float* z, float* out, int N, int C, int Rx, int Rz,
                      smot_stream_t stream);

/*
 * Search-region pooling fused with the cross-correlation (the [N,C,Rx,Rx] tensor stays on chip).
 *
 * Replaces, in EMM.forward (EMM/track_core.py:49-53): pad_feature -> SRPooler(sr) -> xcorr_depthwise.
 *   Arguments as smot_roi_align_levels_fwd (rois = sr, level_boxes = boxes) and smot_xcorr_dw_fwd
 *   (z = templates [N,C,rz,rz]); resp [N,C,Ho,Ho].  x_debug: NULL, or a [N,C,rx,rx] buffer that
 *   receives the pooled planes (tests).  The pooling is separable (fp32-rounding-level differences to ROIAlign).  Since
 *   ABI 13 the correlation runs on the matrix cores (two-part fp16 operands of power-of-two-scaled planes, fp32
 *   accumulation): responses equal smot_xcorr_dw_fwd on the pooled planes to ROUNDING — within 6e-7 * sum |x||z| of an
 *   fp64 correlation on everything measured (worst 5.8e-7 over 1,950 random launches; the fp32 FMA chain of
 *   smot_xcorr_dw_fwd itself: 1.3e-6 on the same planes) — not bit for bit any more.  A pooled plane or a
 *   template that holds an inf / NaN gives an ALL-NaN response plane (smot_xcorr_dw_fwd: NaN / inf in the outputs whose
 *   window covers the value; behind the towers' GroupNorm both are a NaN track).
 * SMOT_ERR_UNSUPPORTED unless rx == 30, rz == 15, sampling_ratio == 2 (35 / 7: smot_sr_xcorr_gather_fwd; otherwise the two
 * unfused calls).
 */
int smot_sr_xcorr_fused_fwd(const float* const* feats, const int* heights, const int* widths,
                            const int* pad_cells, const float* scales, int num_levels, int C,
                            const float* boxes, const float* sr, const float* templates, int N,
                            int rx, int rz, int sampling_ratio,
                            float* resp, float* x_debug, smot_stream_t stream);

/*
 * The same for the reference's second yaml family (DLA_34_FPN_EMM_AOT.yaml: rx == 35, rz == 7, sampling_ratio == 2): the
 * generic ROIAlign kernel's gathers and the row-patch correlation in one kernel — responses bit-identical to
 * smot_roi_align_levels_fwd + smot_xcorr_dw_fwd; the [N,C,35,35] tensor stays on chip.  SMOT_ERR_UNSUPPORTED otherwise.
 */
int smot_sr_xcorr_gather_fwd(const float* const* feats, const int* heights, const int* widths,
                             const int* pad_cells, const float* scales, int num_levels, int C,
                             const float* boxes, const float* sr, const float* templates, int N, int rx, int rz,
                             int sampling_ratio, float* resp, smot_stream_t stream);

/*
 * EMM prediction tower + heads.
 *
 * Replaces: EMMPredictor.forward (EMM/feature_extractor.py:62-69): cls_tower / reg_tower =
 *   conv3x3(C->C, pad 1, no bias) + GroupNorm(gn_groups, eps, affine) + ReLU
 *   [UPSTREAM make_conv3x3(use_gn=True, use_relu=True)], then cls (C->2), center (C->1) on the
 *   cls tower and reg (C->4, followed by ReLU) on the reg tower, each conv3x3 + bias.
 *   Weight pointers are the reference state_dict tensors as they are (OIHW, contiguous):
 *   predictor.{cls_tower.0.weight, cls_tower.1.weight, cls_tower.1.bias, reg_tower.0.weight,
 *   reg_tower.1.weight, reg_tower.1.bias, cls.weight, cls.bias, center.weight, center.bias,
 *   reg.weight, reg.bias}.
 *
 *   resp      [N, C, Ho, Ho]
 *   tower_ws  [N, 2C, Ho, Ho] caller-owned workspace (cls tower in channels [0,C), reg in [C,2C))
 *   logits    [N, 7, Ho, Ho]  channel order: cls0, cls1, center, reg_l, reg_t, reg_r, reg_b
 * Requires C % gn_groups == 0.
 *
 *   tower_packed: optional (may be NULL) output of smot_emm_tower_pack for the SAME tower weights: the
 *   Winograd F(2x2,3x3)-transformed tower filters in the order the matrix-core kernel consumes them.
 *   With it (and Ho == 16) the towers run as a Winograd convolution on the matrix cores — 2.25x fewer
 *   multiplies, results equal to the direct convolution up to fp32 rounding order; without it the direct
 *   fp32 kernel runs.  For C % 32 == 0 (a power of two, <= 512) the transform-domain GEMMs run on fp16 matrix
 *   instructions with every fp32 operand as TWO fp16 parts of a power-of-two-scaled value (weights: scaled and
 *   split once into the second image; a track's response: scaled by 2^kv chosen from its planes' largest
 *   |response| and split in registers; three of the four part products, fp32 accumulation, the scales taken
 *   out exactly afterwards): the logits' error against an fp64 evaluation equals the fp32 form's, at every
 *   track count (one form: a track's logits do not depend on how many tracks the call has).  Other channel
 *   counts with C % 16 == 0 run the fp32 matrix instructions on the fp32 image.
 *   The plane maxima come from the pooling + correlation kernel inside smot_emm_track_fwd; a stand-alone call
 *   computes them with one small launch into the head of `logits` (N*C floats) before the logits are written.
 *   It is a pure function of the two tower weight tensors: recompute it whenever they change (the Python
 *   layer keys it on the tensors' versions).
 */
/* floats of the packed image: 2*C*C*16 (fp32 image; C % 16 == 0, else 0 = no packed path), plus for C % 32 == 0 the
 * two-part fp16 image, (2*C/16) * (C/32 + 1) * 8192, and its four-word header */
long long smot_emm_tower_pack_floats(int C);
/* which form of the packed towers N tracks get (reporting: bench.py, tools/): 0 = none (the direct kernel: C not a power
 * of two, C % 32 != 0, C > 512 or a response map other than 16 x 16 / 29 x 29), 1 = one 16-channel tile per workgroup
 * (fp32; measurement library only since ABI 13), 2 = two tiles (fp32), 3 = two tiles, two-part fp16 operands */
int smot_emm_tower_form(int N, int C, int Ho);
int smot_emm_tower_pack(const float* cls_tower_w, const float* reg_tower_w, int C, float* packed,
                        smot_stream_t stream);

int smot_emm_predictor_fwd(const float* resp, int N, int C, int Ho,
                           const float* cls_tower_w, const float* cls_gn_w, const float* cls_gn_b,
                           const float* reg_tower_w, const float* reg_gn_w, const float* reg_gn_b,
                           const float* cls_w, const float* cls_b,
                           const float* center_w, const float* center_b,
                           const float* reg_w, const float* reg_b,
                           int gn_groups, float gn_eps, const float* tower_packed,
                           float* tower_ws, float* logits, smot_stream_t stream);

/*
 * Fused bicubic x`up` up-sampling + location grid + response decode + argmax.
 *
 * Replaces, in EMM.forward (EMM/track_core.py:69-77): 3x F.interpolate(scale_factor=16,
 *   mode='bicubic'), get_locations (:184-225) and decode_response (:101-135, with
 *   get_scale_penalty :138-152 and get_cosine_window_penalty :155-162).  The up-sampled planes
 *   and the [N, G*G, 2] location tensor are never materialised.
 *
 *   logits  [N,7,Ho,Ho] (layout of smot_emm_predictor_fwd)
 *   sr      [N,4] search regions (padded-image coords),  boxes [N,4] template boxes
 *   hann    [G] the 1-D window, G = up*Ho (host layer passes torch.hann_window(G), periodic)
 *   cand_ws [N * smot_emm_decode_ws_floats(Ho, up)] fp32 workspace, 8-byte aligned
 *   bb [N,4], conf [N]; idx [N] int64 flat argmax index (y*G+x) or NULL
 *   rx, rz : search / template pooler resolutions (Ho must equal rx-rz+1; rz odd)
 *   one_minus_sigma and sigma are passed separately so the host can form 1-sigma in double as
 *   the reference does.
 *   clip_w, clip_h : image size for the clamp of wrap_results_to_boxlist (track_core.py:177-178:
 *   BoxList.clip_to_image, x in [0,w-1], y in [0,h-1]; the reference discards the filtered copy, so
 *   boxes are clamped, never removed); pass clip_w <= 0 for INPUT.AMODAL (no clamp).
 * NaN scores win the argmax and ties go to the lowest index (torch.argmax on CPU).
 */
int smot_emm_decode_fwd(const float* logits, const float* sr, const float* boxes, const float* hann,
                        int N, int Ho, int up, int rx, int rz, float pad_pixels,
                        float one_minus_sigma, float sigma, int use_centerness,
                        float clip_w, float clip_h,
                        float* cand_ws, float* bb, float* conf, int64_t* idx, smot_stream_t stream);

/* fp32 elements of decode workspace needed PER TRACK. */
int smot_emm_decode_ws_floats(int Ho, int up);

/*
 * Greedy IoU non-maximum suppression.
 *
 * Replaces [UPSTREAM] _C.nms(dets, scores, thresh) as reached through boxlist_nms from the solver
 *   (track_head/track_solver.py:22), the RPN post-processor (operator_patch/rpn_patch.py:53) and the box
 *   post-processor (box_head/inference.py:174).
 *   boxes_sorted [n,4] xyxy, ALREADY sorted by descending score (the host layer sorts, as upstream's wrapper
 *   does); IoU with the upstream +1 convention; box j is dropped when a kept earlier box i has
 *   IoU(i,j) > thresh.  keep [n] bytes (1 = kept), in the sorted order.  mask_ws: smot_nms_ws_bytes(n)
 *   bytes, 8-byte aligned.  n <= 8192.
 */
long long smot_nms_ws_bytes(int n);
int smot_nms_fwd(const float* boxes_sorted, int n, float thresh, void* mask_ws, unsigned char* keep,
                 smot_stream_t stream);

/*
 * Frame pre-processing: uint8 RGB HWC frame -> fp32 CHW network input in one launch.
 *
 * Replaces the CPU chain of demos/demo_inference.py:74-82 and build_augmentation.py:52-66 / image_augmentation.py:21-50:
 *   PIL.Image.resize((OW, OH), BILINEAR) -> ToTensor -> Normalize(mean, std, to_bgr255) [UPSTREAM transforms.py].
 *   Bit-exact with Pillow's 8-bit resampler: the caller supplies Pillow's per-axis tables (device memory),
 *   bounds [O,2] int32 = (first input index, tap count) and coeffs [O,k] int32 = weights quantised to 22
 *   fractional bits (an axis that keeps its size: (i,1) and 1<<22).  max_tile_rows = the largest number of
 *   input rows any 8 consecutive output rows touch.  mean3 / std3: HOST arrays, indexed by OUTPUT channel
 *   (after the optional BGR swap, as upstream applies them).  out [3, OH, OW].
 */
int smot_preprocess_fwd(const unsigned char* frame, int H, int W,
                        const int* xbounds, const int* xcoeffs, int kx,
                        const int* ybounds, const int* ycoeffs, int ky,
                        int OH, int OW, int max_tile_rows,
                        const float* mean3, const float* std3, int to_bgr255,
                        float* out, smot_stream_t stream);

/*
 * The frames of several cameras in one call: num_images uint8 RGB HWC frames, each of its own input size and anywhere on
 * the device, -> one [num_images, 3, OH, OW] network input of ONE output size, in ceil(num_images / 16) launches (image =
 * blockIdx.z; the per-image values travel in the kernel-argument block).  Resampling, ToTensor and Normalize are
 * smot_preprocess_fwd's, operation for operation: with out_type SMOT_FEAT_F32, image b is bit for bit what that call
 * gives on frame b.
 *
 *   frames, H, W, xbounds, xcoeffs, kx, ybounds, ycoeffs, ky, max_tile_rows
 *                HOST arrays of length num_images; entry b describes image b as smot_preprocess_fwd's arguments of the
 *                same names do (the tables are device memory, made for H[b] x W[b] -> OH x OW; images of one input size
 *                may share theirs).
 *   mean3, std3  HOST arrays, indexed by OUTPUT channel; to_bgr255 as in smot_preprocess_fwd; one set per call.
 *   out_type     SMOT_FEAT_F32, SMOT_FEAT_F16 or SMOT_FEAT_BF16 (defined below), optionally OR'ed with
 *                SMOT_FEAT_CHANNELS_LAST: the element type and the layout of `out`.  A half output is the fp32 result
 *                followed by exactly one round-to-nearest-even conversion (bit for bit `fp32_result.to(dtype)`).
 *   out          without the layout flag [num_images, 3, OH, OW] contiguous: out[((b*3+c)*OH+y)*OW+x]; with it the same
 *                tensor in channels-last memory: out[((b*OH+y)*OW+x)*3+c].  Aligned to its element size.
 *
 * Before the first launch, and without touching the device: SMOT_ERR_BAD_ARG for num_images outside [1, SMOT_MAX_IMAGES],
 * a null pointer (array or entry), a non-positive size, an out_type outside {0, 1, 2, 16, 17, 18} or a misaligned out;
 * SMOT_ERR_UNSUPPORTED for an image whose max_tile_rows * 384 bytes exceed 64 KiB of LDS (the message names the image).
 * Deterministic; no atomics, no workspace.
 */
int smot_preprocess_batch_fwd(int num_images, const unsigned char* const* frames, const int* H, const int* W,
                              const int* const* xbounds, const int* const* xcoeffs, const int* kx,
                              const int* const* ybounds, const int* const* ycoeffs, const int* ky,
                              const int* max_tile_rows, int OH, int OW,
                              const float* mean3, const float* std3, int to_bgr255,
                              void* out, int out_type, smot_stream_t stream);

/*
 * Instrumentation (bench.py roofline leg): between _begin and _end every smot_xcorr_dw_fwd and
 * smot_sr_xcorr_fused_fwd launch — direct or inside smot_emm_track_fwd — is issued through hipExtLaunchKernel with a
 * start / stop event pair of its own (events are created in _begin, outside any timed region; at most max_launches
 * pairs): the elapsed time between the two is the kernel's duration as rocprofv3 reports it (round 1 recorded two
 * marker events AROUND the launch: that span ran 2.5-3.5 us longer).  _end synchronises the events and returns the
 * summed kernel durations and the number of launches timed.  Not thread-safe; one timing session at a time.
 */
int smot_xcorr_timer_begin(int max_launches);
int smot_xcorr_timer_end(double* total_ms, int* launches);
/* Same mechanism per slot, timing every `stride`-th launch only: 0 = the cross-correlation kernels (what the two
 * calls above use, stride 1), 1 = the tower kernel of smot_emm_predictor_fwd / smot_emm_track_fwd. */
/* Phase trace: while buf != NULL every workgroup of the tower kernels, of the pooling / correlation kernels, of the
 * decode and of the solver kernel writes s_memtime stamps to buf[item*8 + 0..7] (device memory, 8 int64 per
 * workgroup of the launch grid; tower: start, main loop begin/end, output exchange done, GroupNorm done, end;
 * pooling: start, tables done, templates staged, pooling done, end, after the workgroup assignment).  NULL switches
 * it off. */
void smot_debug_trace(long long* buf);
int smot_kernel_timer_begin(int slot, int max_launches, int stride);
int smot_kernel_timer_end(int slot, double* total_ms, int* launches);
/* Median span (microseconds) of `reps` EMPTY marker-event brackets on `stream` (kept for tools that still time with
 * markers; bench.py no longer needs it). */
int smot_kernel_timer_bracket_overhead(smot_stream_t stream, int reps, double* median_us);
/* An empty kernel of workgroups x threads inside timer slot 0's event bracket (bench.py's
 * `roofline.empty_launch_event_bracket_us`): 4.1 us on MI355X whatever the grid — the BRACKET's floor, an upper bound on the
 * fixed cost of a dispatch (the packet's own timestamps under rocprofv3 give 0.8-1.5 us for the same empty kernel). */
int smot_dispatch_floor_fwd(int workgroups, int threads, smot_stream_t stream);

/*
 * One-call halves of a frame pair (same kernels, one FFI crossing each).
 *
 * smot_emm_track_fwd replaces the inference branch of EMM.forward (EMM/track_core.py:28-79):
 *   pad_feature (virtual) + SRPooler on the search regions -> xcorr_depthwise -> EMMPredictor ->
 *   bicubic x`up` + get_locations + decode_response -> clip of wrap_results_to_boxlist.
 *   boxes     [N,4] template boxes (pick the FPN level, scale penalty), sr [N,4] search regions
 *   templates [N,C,rz,rz] (track memory), predictor_params: HOST array of 13 device pointers: the 12 parameters in
 *   the order cls_tower.0.weight, cls_tower.1.weight, cls_tower.1.bias, reg_tower.0.weight,
 *   reg_tower.1.weight, reg_tower.1.bias, cls.weight, cls.bias, center.weight, center.bias,
 *   reg.weight, reg.bias, followed by a 13th entry: the smot_emm_tower_pack image of the tower weights
 *   or NULL (see smot_emm_predictor_fwd).   ws: smot_emm_track_ws_floats(N,C,rx,rz) floats, 16-byte aligned.
 *   Remaining arguments as in the per-operator calls above.
 *
 * smot_emm_extract_cache_fwd replaces EMM.extract_cache (EMM/track_core.py:81-98): template pooling
 *   on the un-padded maps (boxes pick level and roi) + search regions for the next frame.
 *
 * order_hint (optional, may be NULL everywhere): a scheduling side channel between the two halves, no part of the
 *   reference's interface.  A hint made from exactly the boxes / search regions it is passed with changes no result
 *   (bit-identical outputs with and without, tests/test_hip_parity.py); a hint made from OTHER boxes gives wrong
 *   results — see the last sentences.  The pooling + correlation kernel of
 *   smot_emm_track_fwd balances the chip by handing its workgroups the rois in cost order (wide search windows
 *   first); ranking them costs every workgroup ~3 us of start-up latency.  The extraction that CREATES those rois
 *   can rank them once: given a buffer of smot_emm_order_hint_floats(N, rz, sampling_ratio) floats (32-byte
 *   aligned; 0 = this shape / count writes no hint: pass NULL), smot_emm_extract_cache[_masked]_fwd writes
 *   SMOT_HINT_FLOATS dwords per roi — {search region x1,y1,x2,y2, FPN level (int32 bits), roi index (int32 bits),
 *   0, 0 | ymin, ymax, xmin, xmax of the touched window, pad cells / H / W / scale of the level the tables stand for |
 *   y sample table 64 x {row byte offset lo, hi, weight lo, hi} | x sample table 64 x {window column lo, hi, weight lo,
 *   hi} | by-roi record (8 dwords, see below)}, entry k = the roi of rank k; the tables (ABI 9) are the FINISHED sample tables of the roi's 30x30 search-region
 *   pooling in the next frame (zero-pad int(pad_pixels * scale) cells, same map sizes), so that a consumer workgroup
 *   copies them instead of building them (a geometry stamp that does not match the consumer's level makes it rebuild
 *   them) — and smot_emm_track_fwd given that buffer TOGETHER WITH exactly the `boxes`
 *   and `sr` of the same extraction (same N, same row order, same maps geometry) reads one entry per workgroup
 *   instead of ranking.  For the masked form the hint covers the first *n_valid rows.
 *   VERIFIED, not trusted (ABI 12): behind the tables, entry x carries the by-roi record of roi x — {its search region,
 *   its FPN level, the number of rois the list ranks, a status word, 0} — and the consuming kernel compares every record with
 *   ITS sr[x] (bit for bit), the level it derives from ITS boxes[x] and ITS N (one workgroup per roi, loads that travel
 *   beside the entry's own: no cost on the kernel's chain).  The list is a permutation of the rois it was made from by
 *   construction, so a list that passes describes exactly these rois.  One that does not (other boxes, another row
 *   order, another count or level geometry) raises the status word of entry 0 (SMOT_HINT_STATUS_WORD; the buffer is
 *   therefore IN/OUT for smot_emm_track_fwd), and the same call's decode kernel then writes NaN into every row of `bb`
 *   and `conf`: a stale hint is reported (NaN rows; smot_emm_order_hint_status; bit 1 of the solver's record word 6),
 *   never silently used.  Indices are clamped, so nothing is read out of range either way.
 */
#define SMOT_HINT_FLOATS 536
#define SMOT_HINT_STATUS_WORD 534   /* dword index (in the buffer, i.e. of entry 0) of the list's status word */
/* Copies the status word of an order hint to *status_host (pinned or pageable host memory) on `stream`: 0 = every head that
 * was given this hint found it describing its rois; non-zero = one did not (and wrote NaN rows).  Asynchronous: valid once
 * the stream has been synchronised. */
int smot_emm_order_hint_status(const float* order_hint, int* status_host, smot_stream_t stream);
long long smot_emm_order_hint_floats(int N, int rz, int sampling_ratio);

long long smot_emm_track_ws_floats(int N, int C, int rx, int rz);

int smot_emm_track_fwd(const float* const* feats, const int* heights, const int* widths,
                       const int* pad_cells, const float* scales, int num_levels, int C,
                       const float* boxes, const float* sr, const float* templates, int N,
                       int rx, int rz, int sampling_ratio,
                       const float* const* predictor_params, int gn_groups, float gn_eps,
                       const float* hann, int up, float pad_pixels,
                       float one_minus_sigma, float sigma, int use_centerness,
                       float clip_w, float clip_h,
                       float* ws, float* bb, float* conf, int64_t* idx, const float* order_hint,
                       smot_stream_t stream);

int smot_emm_extract_cache_fwd(const float* const* feats, const int* heights, const int* widths,
                               const float* scales, int num_levels, int C,
                               const float* boxes, int N, int rz, int sampling_ratio,
                               float pad_pixels, float search_expansion, float min_search_wh,
                               float* templates, float* sr, float* order_hint, smot_stream_t stream);

/* EMM.extract_cache over a CAPACITY of boxes of which the first *n_valid (device int32, e.g. &record[1] of
 * smot_track_solve_fwd) are real: rows >= *n_valid are skipped on the device, their outputs stay unwritten.  Lets
 * the tracker enqueue the template extraction before the host has read the solver's counts (Rz = 15 or 7,
 * sampling_ratio = 2 only). */
int smot_emm_extract_cache_masked_fwd(const float* const* feats, const int* heights, const int* widths,
                                      const float* scales, int num_levels, int C,
                                      const float* boxes, int capacity, const int* n_valid, int rz,
                                      int sampling_ratio, float pad_pixels, float search_expansion,
                                      float min_search_wh, float* templates, float* sr, float* order_hint,
                                      smot_stream_t stream);

/*
 * The two halves of a frame pair over a BATCH of images in one set of launches (several video streams on one device).
 * Arguments as in the single-image twins, plus num_images and row_start, a HOST array of num_images + 1 ints:
 *   feats[l]  points at [num_images, C, H_l, W_l] contiguous maps; all images share one map size per level;
 *   the rows of image b are [row_start[b], row_start[b+1]) of boxes / sr / templates / the outputs (N = row_start[num_images]);
 *   1 <= num_images <= SMOT_MAX_IMAGES, row_start[0] == 0, row_start non-decreasing: anything else is SMOT_ERR_BAD_ARG
 *   before any launch.  Images without rows and N == 0 are legal.
 * The rows of image b get exactly what the single-image call gives on that image's maps with those rows (bit for bit).
 * ws: smot_emm_track_ws_floats(N, C, rx, rz) floats.  clip_w / clip_h are the one image size of the batch.  An order hint
 * of a batched extraction describes its rows whatever the split: the sample tables in it are relative to the image, and
 * the consuming kernel takes the image of a row from ITS row_start.  Hints cover at most 256 rows, as for one image.
 */
int smot_emm_track_batched_fwd(const float* const* feats, const int* heights, const int* widths,
                               const int* pad_cells, const float* scales, int num_levels, int C,
                               const float* boxes, const float* sr, const float* templates, int N,
                               int rx, int rz, int sampling_ratio,
                               const float* const* predictor_params, int gn_groups, float gn_eps,
                               const float* hann, int up, float pad_pixels,
                               float one_minus_sigma, float sigma, int use_centerness,
                               float clip_w, float clip_h,
                               float* ws, float* bb, float* conf, int64_t* idx, const float* order_hint,
                               smot_stream_t stream, int num_images, const int* row_start);

int smot_emm_extract_cache_batched_fwd(const float* const* feats, const int* heights, const int* widths,
                                       const float* scales, int num_levels, int C,
                                       const float* boxes, int N, int rz, int sampling_ratio,
                                       float pad_pixels, float search_expansion, float min_search_wh,
                                       float* templates, float* sr, float* order_hint, smot_stream_t stream,
                                       int num_images, const int* row_start);

/*
 * Box-head post-processing of the propagated tracks + the score average of _refine_tracks, one launch, no host sync.
 *
 * Replaces, when every proposal is a track (ids >= 0 and labels given — what CombinedROIHeads._refine_tracks passes to
 * the box head, siammot/modelling/roi_heads.py:60-84): PostProcessor.forward / filter_results
 * (siammot/modelling/box_head/inference.py:46-185: soft-max, BoxCoder.decode [UPSTREAM modeling/box_coder.py], track
 * rows keep their label's probability + 1, clip_to_image(remove_empty=False), per-class grouping) and
 * roi_heads.py:66-82 (score = (box-head score + matching score + 1) / 2, or the box-head score alone for TRACKTOR).
 *
 *   head_out   device [N, ld]: columns [0, K) = FPNPredictor.cls_score logits, [K, K + 4*KR) = bbox_pred deltas
 *              (KR = K, or 2 with CLS_AGNOSTIC_BBOX_REG: the last four columns are used, inference.py:67-68)
 *   boxes      device [N,4] xyxy proposals (the boxes EMM.forward propagated); labels / ids device [N] int64;
 *   track_conf device [N] matching scores in [0, 1] (the + 1 band is applied inside)
 *   wx..wh     BBOX_REG_WEIGHTS; xform_clip = log(1000/16); clip_w / clip_h = image size, 0 = INPUT.AMODAL
 *   out_*      device [N,4] / [N] / [N] int64 / [N] int64: exactly N rows, grouped by label in ascending order, input
 *              order inside a label (the order the reference's per-class loop produces); like the reference the
 *              matching scores are taken in INPUT order and the box-head scores in OUTPUT order (roi_heads.py:66,70).
 * Preconditions (checked by the host wrapper, not here): SCORE_THRESH < 1 (a track row scores p + 1 and is never
 * dropped), labels in [1, K).  N <= smot_box_refine_post_max_rows().
 */
int smot_box_refine_post_max_rows(void);
int smot_box_refine_post_fwd(const float* head_out, int ld, int num_classes, int reg_classes,
                             const float* boxes, const int64_t* labels, const int64_t* ids, const float* track_conf,
                             int N, float wx, float wy, float ww, float wh, float xform_clip,
                             float clip_w, float clip_h, int tracktor,
                             float* out_boxes, float* out_scores, int64_t* out_ids, int64_t* out_labels,
                             smot_stream_t stream);

/*
 * The whole box-head refinement of the propagated tracks behind one call (six launches, no host synchronisation: the
 * K-slice sums of fc7 and of cls_score | bbox_pred are added by their consumers while they load; eight launches when the
 * head is wider than 64 columns or fc7's width is not a multiple of 64).
 *
 * Replaces: CombinedROIHeads._refine_tracks (siammot/modelling/roi_heads.py:60-84) = ROIBoxHead.forward on the
 *   propagated boxes as proposals (box_head/box_head.py:46-50: [UPSTREAM] Pooler 7x7 -> fc6 -> ReLU -> fc7 -> ReLU ->
 *   cls_score / bbox_pred -> PostProcessor, box_head/inference.py:46-185) + the score average (roi_heads.py:66-82).
 *   feats / heights / widths / scales: the FPN levels as in smot_roi_align_levels_fwd (the level of a roi is picked by
 *   the roi itself, no padding); pooled = POOLER_RESOLUTION (7; 15 and 30 also run), sampling_ratio 2;
 *   fc6_w [dim6, C*pooled^2], fc7_w [dim7, dim6], cls_w [num_classes, dim7], reg_w [4*reg_classes, dim7] (+ biases) as
 *   the state_dict holds them; the remaining arguments as smot_box_refine_post_fwd.
 *   ws: device fp32 [smot_box_refine_ws_floats(...)], 16-byte aligned.   N <= 128.
 * SMOT_ERR_UNSUPPORTED: another pooler shape or layer widths that are not multiples of 4 (use the stage-wise entries).
 */
long long smot_box_refine_ws_floats(int N, int C, int pooled, int dim6, int dim7, int num_classes, int reg_classes);
int smot_box_refine_fwd(const float* const* feats, const int* heights, const int* widths, const float* scales,
                        int num_levels, int C, int pooled, int sampling_ratio, const float* boxes,
                        const int64_t* labels, const int64_t* ids, const float* track_conf, int N,
                        const float* fc6_w, const float* fc6_b, int dim6, const float* fc7_w, const float* fc7_b, int dim7,
                        const float* cls_w, const float* cls_b, int num_classes,
                        const float* reg_w, const float* reg_b, int reg_classes,
                        float wx, float wy, float ww, float wh, float xform_clip, float clip_w, float clip_h, int tracktor,
                        float* ws, float* out_boxes, float* out_scores, int64_t* out_ids, int64_t* out_labels,
                        smot_stream_t stream);

/*
 * y = act(x W^T + b) on a handful of rows: the box head's linear layers for the propagated tracks.
 *
 * Replaces: [UPSTREAM] FPN2MLPFeatureExtractor.fc6 / fc7 (+ ReLU) and FPNPredictor.cls_score / bbox_pred as
 *   ROIBoxHead.forward calls them (siammot/modelling/box_head/box_head.py:46-50) from
 *   CombinedROIHeads._refine_tracks (roi_heads.py:60-84), where x has one row per propagated track.
 *   x device [M, K] (M <= smot_linear_rows_max_rows(), K % 4 == 0, 16-byte aligned), W device [N, K] as
 *   torch.nn.Linear stores it, bias device [N] or NULL, relu 0/1, ws device fp32 [smot_linear_rows_ws_floats(M, K, N)]
 *   (16-byte aligned scratch for the split-K partial sums), y device [M, ldy] (ldy >= N: several layers can write
 *   column blocks of one row-major buffer).  Two launches (split-K partial products on the fp32 matrix cores, then the
 *   slice-ordered sum + bias + ReLU); deterministic.  SMOT_ERR_UNSUPPORTED: K % 4 != 0.
 */
int smot_linear_rows_max_rows(void);
long long smot_linear_rows_ws_floats(int M, int K, int N);
int smot_linear_rows_fwd(const float* x, int M, int K, const float* W, const float* bias, int N, int relu,
                         float* ws, float* y, int ldy, smot_stream_t stream);

/*
 * Track solver: one launch for a frame's TrackSolver.forward + pool transitions + active-row filter.
 *
 * Replaces TrackSolver.forward (siammot/modelling/track_head/track_solver.py:36-108: score banding of active
 * tracks :63-69, class-agnostic NMS at IoU 0.5 over detections + dormant + active boxes :22/:71 [UPSTREAM
 * boxlist_nms -> _C.nms], band removal :30-31, start / inactive / resume decisions :78-92, id writes :94-103),
 * the TrackPool transitions they trigger (track_head/track_utils.py:157-236: resume_track, start_track,
 * suspend_track, expire_tracks, increment_frame) and TrackHead._get_track_targets (track_head/track_head.py:99-110).
 * The reference synchronises with the host once per BOX here; this call never does.
 *
 *   det_* / trk_*  the frame's boxes in two segments (the detector's boxes; the boxes the tracker propagated —
 *                  either may be empty): boxes [n,4] xyxy, scores [n] (IN/OUT: banded in place as the reference
 *                  does), ids [n] int64 (-1 = no track), labels [n] int64 (may be NULL: 1).
 *                  trk_score_bias is added to the propagated scores first (the +1 of roi_heads.py:67 when no box
 *                  head refines them; 0 if they are already in the (1,2] band).
 *   pool_state     device int32 [8 + 3*pool_capacity], PERSISTENT between frames: word 0 max_id (-1 for a fresh
 *                  pool), word 1 frame_idx, word 2 n_active, word 3 n_dormant, word 4 the number of act_* rows the
 *                  last call wrote (A: a device-resident count, e.g. the n_valid of
 *                  smot_emm_extract_cache_masked_fwd), words 5-7 reserved (0); then the
 *                  active ids [pool_capacity], the dormant ids [pool_capacity] and the frame each dormant id was
 *                  last active in [pool_capacity].  Read and rewritten by every call.
 *   out_*          kept rows in ascending original order (boxes [M,4], scores back in [0,1], ids with new ids
 *                  started and inactive ones set to -1, labels); M = n_det + n_trk rows of capacity each.
 *   act_*          the rows of the output whose id is active after the update (the next frame's track targets).
 *   record         int32 [8 + 4*M + 3*pool_capacity], DEVICE memory or device-accessible pinned HOST memory (the
 *                  kernel's stores then land in host memory directly and the caller needs no copy, only an event
 *                  behind this launch): K (kept), A (active rows), max_id, frame_idx,
 *                  n_active, n_dormant, flags (bit 0: id table overflow; bit 1, ABI 12: a propagated track came in with a NaN
 *                  score — what a head writes whose order hint failed its verification, see order_hint; bit 2, ABI 12: no id
 *                  started, resumed, was suspended or expired in this frame — the three tables stand; bits 8 and up: the number of
 *                  ids that were resumed AND suspended in this frame and are still dormant — they are the LAST entries of
 *                  the dormant table), M; kept
 *                  original row [M]; kept id [M]; active-row id
 *                  [M]; snapshot of the three pool tables.  The only thing the host has to read back.  frame_idx
 *                  (word 3, always >= 1) is stored last, behind a system-scope fence: a host polling a pinned
 *                  record it zeroed before the launch finds the record complete once word 3 is non-zero.
 * At most smot_track_solve_max_boxes() boxes / ids per call (one workgroup); more -> SMOT_ERR_UNSUPPORTED.
 */
int smot_track_solve_max_boxes(void);
int smot_track_solve_fwd(const float* det_boxes, float* det_scores, const int64_t* det_ids,
                         const int64_t* det_labels, int n_det,
                         const float* trk_boxes, float* trk_scores, const int64_t* trk_ids,
                         const int64_t* trk_labels, int n_trk, float trk_score_bias,
                         float track_thresh, float start_thresh, float resume_thresh, float nms_thresh,
                         int max_dormant_frames, int* pool_state, int pool_capacity,
                         float* out_boxes, float* out_scores, int64_t* out_ids, int64_t* out_labels,
                         float* act_boxes, int64_t* act_ids, int64_t* act_labels, float* act_scores,
                         int* record, smot_stream_t stream);

/*
 * The same launch carrying the dormant tracks' rows of the track memory (track_head/track_head.py:77-97; the stand-alone
 * form is smot_memory_carry_fwd, below): rows carry_src_row0 .. carry_src_row0 + carry_rows - 1 of the memory the frame's
 * head ran on (carry_* arrays: templates [*, row_floats], boxes / sr [*,4], ids / labels int64, scores) go behind the rows
 * this launch leaves active.  Boxes, ids, labels and scores are appended to act_* behind the count the launch determines
 * (always the right place).  Templates and search regions are copied by extra workgroups beside the solver's one — they
 * add nothing to the launch's duration but cannot know that count: they write to rows carry_dst_row0 .. of next_templates /
 * next_sr (capacity n_det + n_trk rows; the masked template extraction fills rows 0 .. count-1 of the same buffers
 * afterwards), the CALLER'S GUESS of the count; a caller whose guess turns out wrong (record word 1 != carry_dst_row0)
 * copies again with smot_memory_carry_fwd.  row_floats % 4 == 0, 16-byte aligned arrays.  carry_rows == 0: plain
 * smot_track_solve_fwd.
 */
int smot_track_solve_carry_fwd(const float* det_boxes, float* det_scores, const int64_t* det_ids,
                               const int64_t* det_labels, int n_det,
                               const float* trk_boxes, float* trk_scores, const int64_t* trk_ids,
                               const int64_t* trk_labels, int n_trk, float trk_score_bias,
                               float track_thresh, float start_thresh, float resume_thresh, float nms_thresh,
                               int max_dormant_frames, int* pool_state, int pool_capacity,
                               float* out_boxes, float* out_scores, int64_t* out_ids, int64_t* out_labels,
                               float* act_boxes, int64_t* act_ids, int64_t* act_labels, float* act_scores,
                               int* record,
                               const float* carry_templates, const float* carry_boxes, const float* carry_sr,
                               const int64_t* carry_ids, const int64_t* carry_labels, const float* carry_scores,
                               int carry_src_row0, int carry_rows, int carry_dst_row0,
                               float* next_templates, float* next_sr, int row_floats, smot_stream_t stream);

/*
 * The track solver for the images (cameras) of a call: smot_track_solve_fwd on num_images independent frames, each with its
 * own pool, in ONE launch per 16 images that have rows (ABI 14, additive).
 *
 * Replaces num_images calls of smot_track_solve_fwd — num_images single-workgroup launches that run one after the other on
 * one compute unit each — for callers that run the batched head (smot_emm_track_batched_fwd) over several video streams.
 * Every image gets one workgroup of the same solver; image b's results are bit for bit those of smot_track_solve_fwd on
 * image b's arguments.  Workgroups share nothing.
 *
 *   layout    every argument of smot_track_solve_fwd as a HOST array of num_images entries, in that entry's order: entry b
 *             of each array is image b's argument (det_labels[b] / trk_labels[b] may be NULL: 1).  Thresholds, nms_thresh
 *             and max_dormant_frames are per image: cameras may be configured differently.  The arrays are read during the
 *             call only — the per-image arguments travel in the launches' kernel arguments, nothing is kept.
 *   empty     an image with n_det[b] + n_trk[b] == 0 gets no workgroup: its pool_state, outputs and record are neither read
 *             nor written (its pointers may be NULL), as a caller of the single entry skips such a frame (the reference
 *             does neither expire_tracks nor increment_frame for it).  A call in which no image has rows returns 0 and
 *             launches nothing.
 *   record    record[b]: int32 [8 + 4*M_b + 3*pool_capacity[b]] as smot_track_solve_fwd writes it, word 3 last behind a
 *             system-scope fence; the segments may lie back to back in one allocation (one host copy for all images).
 *   limits    1 <= num_images <= SMOT_MAX_IMAGES.  No dormant-row carry in this form (smot_track_solve_carry_fwd is
 *             single-image).  The images' buffers must not overlap; the call checks what would make two workgroups race.
 *
 * Before the first launch and before any per-image pointer is dereferenced, with a message that names the image:
 * SMOT_ERR_BAD_ARG for num_images outside [1, SMOT_MAX_IMAGES], a null array, a negative count, and — for an image with rows
 * — the null-pointer and 16-byte alignment conditions of smot_track_solve_fwd, or the same pool_state or the same record as
 * an earlier image with rows; SMOT_ERR_UNSUPPORTED for an image with more than smot_track_solve_max_boxes() rows or a
 * larger pool_capacity.  A call that returns an error has launched nothing.
 */
int smot_track_solve_batched_fwd(int num_images,
                                 const float* const* det_boxes, float* const* det_scores, const int64_t* const* det_ids,
                                 const int64_t* const* det_labels, const int* n_det,
                                 const float* const* trk_boxes, float* const* trk_scores, const int64_t* const* trk_ids,
                                 const int64_t* const* trk_labels, const int* n_trk, const float* trk_score_bias,
                                 const float* track_thresh, const float* start_thresh, const float* resume_thresh,
                                 const float* nms_thresh, const int* max_dormant_frames,
                                 int* const* pool_state, const int* pool_capacity,
                                 float* const* out_boxes, float* const* out_scores, int64_t* const* out_ids,
                                 int64_t* const* out_labels, float* const* act_boxes, int64_t* const* act_ids,
                                 int64_t* const* act_labels, float* const* act_scores,
                                 int* const* record, smot_stream_t stream);

/*
 * One tracking frame behind ONE call (or two): the launches of smot_emm_track_fwd (3) [+ smot_box_refine_fwd (8)] +
 * smot_track_solve_fwd (1) + smot_emm_extract_cache_masked_fwd (1) enqueued back to back on `stream`.
 *
 * Replaces the inference branch of CombinedROIHeads.forward from `self.track(...)` on
 * (siammot/modelling/roi_heads.py:38-50): TrackHead.forward_inference -> EMM.forward (track_head.py:37-46),
 * _refine_tracks (roi_heads.py:60-84), cat_boxlist + TrackSolver.forward (track_solver.py:36-108),
 * TrackHead.get_track_memory -> EMM.extract_cache on the rows the solver leaves active (track_head.py:54-75,99-110).
 * Every field is an argument of one of the four entry points above and means what it means there; the outputs of a
 * stage are the inputs of the next (the propagated boxes / scores feed the refinement or the solver, the solver's
 * act_boxes and pool_state[4] feed the masked template extraction).  n_trk == 0 skips the head and the refinement
 * (first frame, or an empty memory); refine == 0 skips the refinement (the solver then applies trk_score_bias = 1).
 * SMOT_STAGE_CARRY (with SMOT_STAGE_SOLVE; never part of stages == 0) makes the solver's launch carry the dormant rows
 * of the track memory the head ran on (the carry_* fields: smot_track_solve_carry_fwd; next_templates / next_sr are the
 * destination buffers, row_floats = C * rz * rz).  ORDERING CONTRACT of the carried templates / search regions: they are
 * written to rows [carry_dst_row0, carry_dst_row0 + carry_rows) of next_templates / next_sr BEFORE the active count A is
 * known; when carry_dst_row0 < A the masked extraction of the same frame (SMOT_STAGE_EXTRACT, enqueued behind the solver
 * on the same stream) overwrites rows 0 .. A-1 afterwards and never writes rows >= A — so a wrong guess leaves garbage
 * only in rows the caller re-copies (record word 1 != carry_dst_row0 -> smot_memory_carry_fwd).  A caller that runs the
 * two launches on different streams, or the extraction first, must not use SMOT_STAGE_CARRY.
 * `stages` selects what this call enqueues (0 = everything): a frame is a serial chain — host work before the first
 * launch, the kernels, the record, host bookkeeping — so a caller whose argument preparation is not free calls once
 * with SMOT_STAGE_HEAD as soon as the head's arguments stand (fields of later stages are not read) and a second time
 * with the remaining stages while the head runs (siammot_amd.track_head.TrackingLoop does).
 * The host reads `record` (pinned host memory) as with smot_track_solve_fwd.  Plain C struct: pointers first, then
 * 32-bit fields, no padding; inside each group the fields that change from frame to frame are contiguous (a binding
 * that keeps the block between frames rewrites two short ranges per call).
 */
#define SMOT_STAGE_HEAD 1
#define SMOT_STAGE_REFINE 2
#define SMOT_STAGE_SOLVE 4
#define SMOT_STAGE_EXTRACT 8
#define SMOT_STAGE_CARRY 16     /* with SMOT_STAGE_SOLVE: smot_track_solve_carry_fwd on the carry_* fields */
typedef struct smot_frame_args {
    /* ---- fixed while the video's geometry and the model stand ---- */
    /* FPN levels (HOST arrays of num_levels entries, as in smot_roi_align_levels_fwd; the entries of `feats` are
     * this frame's maps — the array itself can stay where it is) */
    const float* const* feats;
    const int* heights;
    const int* widths;
    const int* pad_cells;        /* search-region pooling (virtual padding) */
    const float* scales;
    const float* const* predictor_params;   /* HOST array of 13 device pointers (smot_emm_track_fwd) */
    const float* hann;
    const float* fc6_w; const float* fc6_b; const float* fc7_w; const float* fc7_b;   /* box head (refine != 0) */
    const float* cls_w; const float* cls_b; const float* reg_w; const float* reg_b;
    int* pool_state;
    /* ---- this frame: the head (SMOT_STAGE_HEAD reads up to trk_conf) ---- */
    float* head_ws;              /* smot_emm_track_ws_floats(n_trk, C, rx, rz) */
    const float* tpl_boxes;      /* [n_trk,4] track memory of the previous frame */
    const float* sr;             /* [n_trk,4] */
    const float* templates;      /* [n_trk,C,rz,rz] */
    const float* order_hint;     /* order hint of exactly these rows (smot_emm_track_fwd) or NULL */
    const int64_t* trk_ids;      /* [n_trk] */
    const int64_t* trk_labels;   /* [n_trk] */
    float* trk_boxes;            /* [n_trk,4] out: propagated boxes */
    float* trk_conf;             /* [n_trk]   out: matching scores */
    /* ---- this frame: refinement, detections, solver, next memory ---- */
    float* refine_ws;            /* smot_box_refine_ws_floats(...) */
    float* ref_boxes;            /* [n_trk,4] out */
    float* ref_scores;           /* [n_trk]   out */
    int64_t* ref_ids;            /* [n_trk]   out */
    int64_t* ref_labels;         /* [n_trk]   out */
    const float* det_boxes; float* det_scores; const int64_t* det_ids; const int64_t* det_labels;
    float* out_boxes; float* out_scores; int64_t* out_ids; int64_t* out_labels;
    float* act_boxes; int64_t* act_ids; int64_t* act_labels; float* act_scores;
    int* record;
    /* next frame's memory (capacity n_det + n_trk rows; the first pool_state[4] are written) */
    float* next_templates;
    float* next_sr;
    float* next_order_hint;      /* smot_emm_order_hint_floats(n_det + n_trk, rz, sampling_ratio) floats or NULL */
    /* dormant rows carried by the solver's launch (SMOT_STAGE_CARRY; smot_track_solve_carry_fwd) */
    const float* carry_templates; const float* carry_boxes; const float* carry_sr;
    const int64_t* carry_ids; const int64_t* carry_labels; const float* carry_scores;
    /* ---- sizes and scalars: per frame first ---- */
    int n_trk, stages, n_det;
    int num_levels, C;
    int rx, rz, sampling_ratio, gn_groups, up, use_centerness;
    int refine, box_pooled, box_sampling_ratio, dim6, dim7, num_classes, reg_classes, tracktor;
    int max_dormant_frames, pool_capacity;
    int carry_src_row0, carry_rows, carry_dst_row0;
    float track_thresh, start_thresh, resume_thresh;
    float gn_eps, pad_pixels, one_minus_sigma, sigma, clip_w, clip_h;
    float box_wx, box_wy, box_ww, box_wh, box_xform_clip;
    float nms_thresh, search_expansion, min_search_wh;
} smot_frame_args;

int smot_track_frame_fwd(const smot_frame_args* args, smot_stream_t stream);

/*
 * Dormant rows of the track memory, carried on the device.
 *
 * Replaces: TrackHead._update_memory_with_dormant_track (track_head/track_head.py:77-97: torch.cat of the templates +
 *   two cat_boxlist calls per frame).  A dormant track's (template, search region, box, id, label, score) never changes
 *   while it is dormant and is a row of the memory the frame's head just ran on: D rows `rows[j]` (host array, indices
 *   into the source memory of `src_rows_total` rows) are copied to rows dst_row0 + j of the destination buffers
 *   (`dst_capacity` rows each; templates [*, row_floats], boxes / sr [*,4], ids / labels int64 [*], scores [*]).
 *   dst_row0_dev != NULL: the first destination row is read from that device word instead (the solver's pool state
 *   word 4 = the number of active rows: a launch enqueued before the host has read the frame's record); rows at or
 *   beyond dst_capacity are then dropped.  D <= smot_memory_carry_max_rows().  Pure copies (bit-exact).
 */
int smot_memory_carry_max_rows(void);
int smot_memory_carry_fwd(const float* src_templates, const float* src_boxes, const float* src_sr,
                          const int64_t* src_ids, const int64_t* src_labels, const float* src_scores,
                          int src_rows_total, float* dst_templates, float* dst_boxes, float* dst_sr,
                          int64_t* dst_ids, int64_t* dst_labels, float* dst_scores, int dst_capacity,
                          const int* rows, int D, int dst_row0, const int* dst_row0_dev, int row_floats,
                          smot_stream_t stream);

/*
 * fp16 / bf16 FEATURE MAPS (a PyTorch backbone under torch.autocast or .half()).
 *
 * Every entry point above that reads the FPN maps has a `_typed_` twin that takes the maps as `const void*` and their
 * element type `feat_type`; every other argument, and its order, is the twin's.  Only the MAPS have a type: boxes,
 * templates / track memory, weights, workspaces, order hints and all outputs stay fp32.
 *
 * The contract: for T in {fp16, bf16}, a call on maps of element type T returns BIT FOR BIT what the same call returns
 * on the maps converted to fp32 (T -> fp32 is exact; the kernels convert in registers right behind each load — fp16
 * subnormals are kept — and every later instruction is the fp32 kernel's).  This holds for every output: pooled planes,
 * responses, templates, search regions, order hints (an order hint holds no map data and no element size: one written
 * from half maps and one written from their fp32 upcast are the same bytes, and a consumer of either type accepts
 * either), boxes, scores, arg-max indices, solver records.  No fp32 copy of a map is made.
 *
 * SMOT_FEAT_F32 through a typed entry point runs the fp32 kernels (it IS the untyped call).  Any other `feat_type` is
 * SMOT_ERR_BAD_ARG with a message that names the value, before any launch and before any pointer is looked at.
 *
 *   smot_emm_track_typed_fwd          the batched signature; one image = num_images 1, row_start {0, N}
 *   smot_emm_extract_cache_typed_fwd  the batched signature plus n_valid: NULL, or the masked form's device count
 *                                     (smot_emm_extract_cache_masked_fwd: N is then the capacity), legal with
 *                                     num_images == 1 only (SMOT_ERR_BAD_ARG otherwise)
 *   smot_track_frame_typed_fwd        args->feats[l] are read as maps of `feat_type` (the struct is unchanged)
 */
#define SMOT_FEAT_F32 0
#define SMOT_FEAT_F16 1
#define SMOT_FEAT_BF16 2

/*
 * CHANNELS-LAST FEATURE MAPS (a backbone run with .to(memory_format=torch.channels_last): [B, C, H, W] tensors whose
 * memory is [B, H, W, C]).
 *
 * SMOT_FEAT_CHANNELS_LAST is a LAYOUT flag OR'ed into the `feat_type` of the `_typed_` entry points: the legal values are
 * {0, 1, 2, 16, 17, 18}; every other value (3, 19, 32, -1, ...) is SMOT_ERR_BAD_ARG as above.  With the flag, every level
 * of the call is read as [num_images, H_l, W_l, C] — cell (img, c, y, x) at element ((img * H_l + y) * W_l + x) * C + c —
 * and must be 16-byte aligned (SMOT_ERR_BAD_ARG otherwise), with C % 8 == 0 (SMOT_ERR_UNSUPPORTED otherwise: pass NCHW maps).  The untyped symbols
 * stay NCHW fp32.
 *
 * The contract: a call on channels-last maps returns, for EVERY output, exactly the bits the same call returns on the
 * NCHW copy of the maps — pooled planes, responses, templates, search regions, order hints, boxes, scores, arg-max
 * indices, ids / labels, solver records.  The kernels read the channel runs of a pixel (8 channels = 32 bytes of fp32,
 * 16 of fp16 / bf16) and repeat the NCHW kernels' arithmetic in the NCHW kernels' order; no NCHW copy of a map is made.
 * An order hint holds no layout: one written from channels-last maps is the same bytes as one written from the NCHW
 * copy, and a head of either layout accepts either (its row offsets stay bytes of an fp32 NCHW row; the channels-last
 * kernels rescale them where they use them).  Everything but the maps stays fp32-contiguous.
 *
 *   honour the flag:   smot_roi_align_levels_typed_fwd, smot_roi_align_typed_fwd, smot_sr_xcorr_fused_typed_fwd (30 / 15,
 *                      x_debug included), smot_emm_extract_cache_typed_fwd (plain, hinted, masked, batched),
 *                      smot_emm_track_typed_fwd (one image and batched, hinted; every shape but 35 / 7),
 *                      smot_box_refine_typed_fwd, smot_track_frame_typed_fwd (all stages)
 *   SMOT_ERR_UNSUPPORTED with the flag (for N > 0):  smot_sr_xcorr_gather_typed_fwd, and the 35 / 7 shape through
 *                      smot_emm_track_typed_fwd / smot_track_frame_typed_fwd — callers pass the NCHW copy there
 */
#define SMOT_FEAT_CHANNELS_LAST 16

int smot_roi_align_levels_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                    const int* pad_cells, const float* scales, int num_levels, int C,
                                    const float* rois, const float* level_boxes, int R,
                                    int out_h, int out_w, int sampling_ratio,
                                    float* out, int32_t* levels_out, smot_stream_t stream);

/* smot_roi_align_levels_typed_fwd over a BATCH of images (the box head's pooler for several cameras): feats[l] points at
 * [num_images, C, H_l, W_l] maps (channels-last with the flag: [num_images, H_l, W_l, C]), the rois of image b are rows
 * [row_start[b], row_start[b+1]) of rois / level_boxes / out / levels_out (R = row_start[num_images]); num_images and
 * row_start (a HOST array) are checked as for smot_emm_*_batched_fwd, before any launch.  The rows of image b are bit for
 * bit what the single-image call returns on that image's maps with those rows — the separable 7 / 15 / 30 kernel and the
 * generic kernel alike.  Images without rois and R == 0 are legal. */
int smot_roi_align_levels_batched_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                            const int* pad_cells, const float* scales, int num_levels, int C,
                                            const float* rois, const float* level_boxes, int R,
                                            int out_h, int out_w, int sampling_ratio,
                                            float* out, int32_t* levels_out, smot_stream_t stream,
                                            int num_images, const int* row_start);

int smot_roi_align_typed_fwd(const void* input, int feat_type, int num_images, int C, int H, int W, int pad_cells,
                             const float* rois5, int R, float spatial_scale, int pooled_h, int pooled_w,
                             int sampling_ratio, float* out, smot_stream_t stream);

int smot_sr_xcorr_fused_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                  const int* pad_cells, const float* scales, int num_levels, int C,
                                  const float* boxes, const float* sr, const float* templates, int N,
                                  int rx, int rz, int sampling_ratio, float* resp, float* x_debug,
                                  smot_stream_t stream);

int smot_sr_xcorr_gather_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                   const int* pad_cells, const float* scales, int num_levels, int C,
                                   const float* boxes, const float* sr, const float* templates, int N,
                                   int rx, int rz, int sampling_ratio, float* resp, smot_stream_t stream);

int smot_emm_track_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                             const int* pad_cells, const float* scales, int num_levels, int C,
                             const float* boxes, const float* sr, const float* templates, int N,
                             int rx, int rz, int sampling_ratio,
                             const float* const* predictor_params, int gn_groups, float gn_eps,
                             const float* hann, int up, float pad_pixels,
                             float one_minus_sigma, float sigma, int use_centerness,
                             float clip_w, float clip_h,
                             float* ws, float* bb, float* conf, int64_t* idx, const float* order_hint,
                             smot_stream_t stream, int num_images, const int* row_start);

int smot_emm_extract_cache_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                     const float* scales, int num_levels, int C,
                                     const float* boxes, int N, int rz, int sampling_ratio,
                                     float pad_pixels, float search_expansion, float min_search_wh,
                                     float* templates, float* sr, float* order_hint, smot_stream_t stream,
                                     int num_images, const int* row_start, const int* n_valid);

int smot_box_refine_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                              const float* scales, int num_levels, int C, int pooled, int sampling_ratio,
                              const float* boxes, const int64_t* labels, const int64_t* ids, const float* track_conf, int N,
                              const float* fc6_w, const float* fc6_b, int dim6, const float* fc7_w, const float* fc7_b, int dim7,
                              const float* cls_w, const float* cls_b, int num_classes,
                              const float* reg_w, const float* reg_b, int reg_classes,
                              float wx, float wy, float ww, float wh, float xform_clip, float clip_w, float clip_h,
                              int tracktor, float* ws, float* out_boxes, float* out_scores, int64_t* out_ids,
                              int64_t* out_labels, smot_stream_t stream);

int smot_track_frame_typed_fwd(const smot_frame_args* args, int feat_type, smot_stream_t stream);

/*
 * RPN PROPOSAL SELECTION (the NMS's third caller): reference operator_patch/rpn_patch.py:15-60 on
 * [UPSTREAM] RPNPostProcessor.forward / select_over_all_levels (inference only), for all images and FPN levels of a call in
 * one memset + nine launches (their number depends on neither num_images nor num_levels) and without a host synchronisation.
 *
 *   objectness[l]  [num_images, A_l, H_l, W_l] logits, regression[l] [num_images, 4 A_l, H_l, W_l] (channel of coordinate c
 *                  of anchor a: 4a + c), contiguous, all of element type `feat_type` (SMOT_FEAT_F32 / F16 / BF16; the layout
 *                  flag is SMOT_ERR_BAD_ARG).  A half call returns bit for bit what the call returns on the upcast tensors.
 *   num_anchors / heights / widths   host arrays [num_levels]: A_l, H_l, W_l
 *   anchors        HOST array [num_images * num_levels] (image-major) of DEVICE pointers to fp32 [A_l H_l W_l, 4] xyxy rows in
 *                  the reference's flattened order (h W + w) A + a; read in place.  At most 128 DISTINCT pointers per call
 *                  (upstream's generator shares one tensor per level among the images): SMOT_ERR_UNSUPPORTED beyond.
 *   image_wh       host array [num_images][2]: width, height of each image (the clip; ignored when `amodal`)
 *   per (image, level): the k = min(pre_nms_top_n, A H W) largest LOGITS in descending order, ties to the lower flat index
 *                  (= objectness.sigmoid().topk(k) wherever the selected sigmoid values are distinct); BoxCoder.decode with
 *                  weights (wx, wy, ww, wh), TO_REMOVE = 1, dw / dh clamped at xform_clip with NaN kept; unless `amodal`
 *                  the clamp to [0, W - 1] x [0, H - 1]; rows with a side x2 - x1 + 1 or y2 - y1 + 1 not >= min_size dropped;
 *                  greedy NMS (+1 IoU, suppressed when IoU > nms_thresh) in score order, first post_nms_top_n kept.
 *   per image:     num_levels > 1: the levels concatenated in level order, the min(fpn_post_nms_top_n, total) best by logit
 *                  in descending order, ties to the lower concatenated position.  num_levels == 1: upstream makes no
 *                  selection; the level's list is copied (pass its capacity as fpn_post_nms_top_n).
 *   outputs        out_boxes [num_images, fpn_post_nms_top_n, 4], out_objectness [num_images, fpn_post_nms_top_n] (the
 *                  sigmoid, evaluated for these rows only), out_count [num_images] int32; rows beyond the count are zero.
 *   capacities     num_images <= SMOT_MAX_IMAGES, num_levels <= SMOT_MAX_LEVELS, pre_nms_top_n <= 2048,
 *                  fpn_post_nms_top_n <= 2048 (SMOT_ERR_BAD_ARG beyond); SMOT_ERR_UNSUPPORTED for nms_thresh <= 0 and for
 *                  num_levels * min(post_nms_top_n, pre_nms_top_n) * 4 + 64 > 65536 (the merge keeps one key per level row
 *                  in LDS: 8 levels x 2048 rows do not fit, 8 x 2032 and 7 x 2048 do).
 *   ws             smot_rpn_proposals_ws_bytes(...) bytes (-1 for shapes the call refuses), 16-byte aligned.  Its largest
 *                  part is the NMS bitmask, NL * P * ceil(P / 64) * 8 bytes (2.6 MB at 4 x 5 x 1000; 268 MB at 64 x 8 x 2048).  Its head is part
 *                  of the contract — the per-level candidates, in 4-byte words, every section padded to a multiple of 4
 *                  words, NL = num_images * num_levels, P = pre_nms_top_n, row il = image * num_levels + level:
 *                      int32 count[NL]        candidates of the pair (k)
 *                      int32 index[NL][P]     their flat indices, sorted (best first)
 *                      float logit[NL][P]     their logits
 *                      float box[NL][P][4]    their decoded boxes BEFORE the clip
 *                  What follows is scratch.
 */
long long smot_rpn_proposals_ws_bytes(int num_images, int num_levels, const int* num_anchors, const int* heights,
                                      const int* widths, int pre_nms_top_n, int post_nms_top_n);
int smot_rpn_proposals_fwd(const void* const* objectness, const void* const* regression, int feat_type,
                           const int* num_anchors, const int* heights, const int* widths, int num_levels,
                           int num_images, const float* const* anchors, const float* image_wh,
                           int pre_nms_top_n, int post_nms_top_n, int fpn_post_nms_top_n, float nms_thresh,
                           float min_size, int amodal, float wx, float wy, float ww, float wh, float xform_clip,
                           void* ws, float* out_boxes, float* out_objectness, int32_t* out_count,
                           smot_stream_t stream);

/*
 * BOX-HEAD POST-PROCESSING OF THE DETECTIONS (csrc/box_detect.hip): the half of the post-processor
 * smot_box_refine_post_fwd leaves out — one image whose proposals are all detections (ids = -1: what the RPN hands over).
 * Replaces: PostProcessor.forward + filter_results (reference siammot/modelling/box_head/inference.py:46-191) — per
 * foreground class a nonzero, three mask gathers, `len(det) > 0`, an argsort, the NMS launch and its mask gather,
 * `trk_idx.any()` and two cat_boxlist: ~25 launches and three to four host synchronisations per class — by FOUR launches
 * and no memset (their number depends on neither M nor num_classes nor the count), without a host synchronisation and
 * deterministic to the bit.
 *
 *   head_out       [M, ld] device, the columns of smot_box_refine_post_fwd: [0, K) logits, [K, K + 4 KR) deltas; KR =
 *                  reg_classes = K, or 2 (class-agnostic regression: the last four columns are used)
 *   boxes          [M, 4] device, xyxy proposals
 *   count          DEVICE int32: rows >= *count do not exist and are never loaded (*count > M counts as M, < 0 as 0)
 *   semantics      soft-max over the K logits; for every class j in [1, K): BoxCoder.decode of class j's deltas with
 *                  weights (wx, wy, ww, wh), TO_REMOVE = 1, dw / dh clamped at xform_clip with NaN kept; the clamp to
 *                  [0, clip_w - 1] x [0, clip_h - 1] unless clip_w == 0 (amodal); candidates: rows with p_j > score_thresh
 *                  (a NaN score is none); greedy NMS (+1 IoU, suppressed when IoU > nms_thresh) in descending score
 *                  order, ties to the lower row.  Output: classes ascending, inside a class ASCENDING PROPOSAL ROW.
 *                  DETECTIONS_PER_IMG is not applied.
 *   outputs        capacity M * (K - 1) rows: out_boxes [cap, 4], out_scores [cap], out_labels [cap] int64, out_rows [cap]
 *                  int32 (the proposal row of the detection), out_count [K] int32 (word 0: total, words 1 .. K - 1: per
 *                  class); rows beyond the total are zero.
 *   capacities     1 <= M <= 2048, 2 <= num_classes <= 128 (SMOT_ERR_BAD_ARG beyond); SMOT_ERR_UNSUPPORTED for
 *                  nms_thresh <= 0.
 *   ws             smot_box_detect_post_ws_bytes(M, num_classes) bytes (-1 for shapes the call refuses), 16-byte aligned.
 *                  Its largest part is the NMS bitmask, (K - 1) * M * ceil(M / 64) * 8 bytes (12 KB at 300 rows x 2
 *                  classes; 67 MB at 2048 x 128).  All of it is scratch.
 */
long long smot_box_detect_post_ws_bytes(int M, int num_classes);
int smot_box_detect_post_fwd(const float* head_out, int ld, int num_classes, int reg_classes, const float* boxes,
                             const int32_t* count, int M, float wx, float wy, float ww, float wh, float xform_clip,
                             float clip_w, float clip_h, float score_thresh, float nms_thresh, void* ws,
                             float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* out_rows,
                             int32_t* out_count, smot_stream_t stream);

/*
 * The same over the images of a call (several cameras): still FOUR launches and no memset whatever num_images is — the
 * image is one more grid dimension of the same four kernels — without a host synchronisation or a global atomic.
 * Replaces: PostProcessor.forward over a list of images (inference.py:46-82 splits the rows per image and runs
 * filter_results on each).
 *
 *   rows           the rows of all images concatenated: head_out [M, ld], boxes [M, 4]; image b owns rows [row_start[b],
 *                  row_start[b+1]) — num_images and row_start (HOST array of num_images + 1 ints) as for
 *                  smot_emm_*_batched_fwd: SMOT_ERR_BAD_ARG before any launch for num_images outside [1, SMOT_MAX_IMAGES],
 *                  row_start[0] != 0, a decrease, or row_start[num_images] != M.  M_b = row_start[b+1] - row_start[b] may be
 *                  0 and is at most 2048 per image.
 *   count          DEVICE int32 [num_images]: image b has min(max(count[b], 0), M_b) rows that exist; the rest is never loaded
 *   clip_w/clip_h  the one image size of the call
 *   outputs        the detections of image b occupy rows [row_start[b] (K - 1), row_start[b+1] (K - 1)) of out_boxes /
 *                  out_scores / out_labels / out_rows — classes ascending, ascending proposal row inside a class, out_rows
 *                  RELATIVE to the image's first row, the tail of the segment zero; out_count [num_images, K]: per image
 *                  the total, then the per-class counts.
 *   contract       for every image every output equals BIT FOR BIT what smot_box_detect_post_fwd returns on that image's
 *                  rows alone (the same device text, arithmetic and NaN rules).
 *   ws             smot_box_detect_post_batched_ws_bytes(num_images, row_start, num_classes) bytes (-1 for a call the entry
 *                  refuses), 16-byte aligned: one segment per image, each laid out as the single-image call's workspace of
 *                  M_b rows (for one image the two byte counts are equal).  All of it is scratch.
 */
long long smot_box_detect_post_batched_ws_bytes(int num_images, const int* row_start, int num_classes);
int smot_box_detect_post_batched_fwd(const float* head_out, int ld, int num_classes, int reg_classes, const float* boxes,
                                     const int32_t* count, int M, float wx, float wy, float ww, float wh, float xform_clip,
                                     float clip_w, float clip_h, float score_thresh, float nms_thresh, void* ws,
                                     float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* out_rows,
                                     int32_t* out_count, smot_stream_t stream, int num_images, const int* row_start);

/*
 * BOX-HEAD REFINEMENT OF THE PROPAGATED TRACKS OF SEVERAL IMAGES (csrc/box_refine.hip): smot_box_refine_post_fwd and
 * smot_box_refine_typed_fwd over the cameras of a call.
 * Replaces: CombinedROIHeads._refine_tracks (reference siammot/modelling/roi_heads.py:60-84) called once per image.
 *
 *   rows           the rows of all images concatenated (head_out / boxes / labels / ids / track_conf and every output); image
 *                  b owns rows [row_start[b], row_start[b+1]) — num_images and row_start (HOST array of num_images + 1 ints)
 *                  as for smot_emm_*_batched_fwd.  Before any launch: SMOT_ERR_BAD_ARG for num_images outside
 *                  [1, SMOT_MAX_IMAGES], a null row_start, row_start[0] != 0, a decrease (the image is named in
 *                  smot_last_error()), row_start[num_images] != N, null pointers, a misaligned ws.  An image may have no rows;
 *                  a call in which none has returns 0 and launches nothing.
 *   feats          [num_images, C, H_l, W_l] per level, of element type and layout feat_type (SMOT_FEAT_*, as for
 *                  smot_box_refine_typed_fwd); one image size, one clip pair and one tracktor flag per call.
 *   outputs        image b's rows in ITS segment [row_start[b], row_start[b+1]): grouped by label inside the segment, input
 *                  order inside a label; the box-head score of OUTPUT row p of the segment is averaged with the matching
 *                  score of INPUT row p of the segment (roi_heads.py:66,70, per image).
 *   contract       for every image every output equals BIT FOR BIT what the single-image entry (smot_box_refine_post_fwd /
 *                  smot_box_refine_typed_fwd) returns on that image's maps and rows alone: the layers run
 *                  smot_linear_rows_fwd's kernels with one more grid dimension (row blocks of 128), and a row's sums do not
 *                  depend on the rows that share its launch.
 *   launches       smot_box_refine_post_batched_fwd: one (a workgroup per image).  smot_box_refine_batched_typed_fwd: eight
 *                  whatever num_images is (batched pooler, a partial-sum and a reduction launch per layer, post-processing),
 *                  no host synchronisation.
 *   limits         smot_box_refine_post_batched_fwd: smot_box_refine_post_max_rows() rows per image (SMOT_ERR_BAD_ARG).
 *                  smot_box_refine_batched_typed_fwd: SMOT_ERR_UNSUPPORTED for an image of more than 128 rows (named in the
 *                  message; alone it would not take the one-call path), for N > smot_box_refine_batched_max_rows() (1024)
 *                  and for the pooler shapes / layer widths smot_box_refine_fwd refuses.
 *   ws             device fp32 [smot_box_refine_batched_ws_floats(N, ...)] (N = all rows; 0 for a call the entry refuses),
 *                  16-byte aligned, all of it scratch: the pooled rows, the three layers' outputs and the largest layer's
 *                  K-slice sums — at the yaml head (C 128, 7x7, 1024-1024) 0.2 MB per row + 33 MB per 128 rows.
 */
int smot_box_refine_batched_max_rows(void);
long long smot_box_refine_batched_ws_floats(int N, int C, int pooled, int dim6, int dim7, int num_classes, int reg_classes);
int smot_box_refine_post_batched_fwd(const float* head_out, int ld, int num_classes, int reg_classes, const float* boxes,
                                     const int64_t* labels, const int64_t* ids, const float* track_conf, int N, float wx,
                                     float wy, float ww, float wh, float xform_clip, float clip_w, float clip_h, int tracktor,
                                     float* out_boxes, float* out_scores, int64_t* out_ids, int64_t* out_labels,
                                     smot_stream_t stream, int num_images, const int* row_start);
int smot_box_refine_batched_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                      const float* scales, int num_levels, int C, int pooled, int sampling_ratio,
                                      const float* boxes, const int64_t* labels, const int64_t* ids, const float* track_conf,
                                      int N, const float* fc6_w, const float* fc6_b, int dim6, const float* fc7_w,
                                      const float* fc7_b, int dim7, const float* cls_w, const float* cls_b, int num_classes,
                                      const float* reg_w, const float* reg_b, int reg_classes, float wx, float wy, float ww,
                                      float wh, float xform_clip, float clip_w, float clip_h, int tracktor, float* ws,
                                      float* out_boxes, float* out_scores, int64_t* out_ids, int64_t* out_labels,
                                      smot_stream_t stream, int num_images, const int* row_start);

/*
 * RPN HEAD (csrc/rpn_head.hip): [UPSTREAM] maskrcnn_benchmark RPNHead.forward — conv3x3 C -> C (pad 1) + bias + ReLU, then
 * the 1x1 heads cls_logits (C -> A) and bbox_pred (C -> 4A), the weights shared by all levels — for every image and every
 * FPN level of a call in ONE launch (its workgroups are (image, level, 8 x 16 tile of positions); their number is all that
 * depends on num_images and num_levels) and without a host synchronisation.  Both stages run on the fp32 matrix cores
 * (exact fp32 products, fp32 accumulation); the C-channel activation between them never leaves the chip.
 *
 *   feats[l]       [num_images, C, H_l, W_l], contiguous NCHW, all of element type `feat_type` (SMOT_FEAT_F32 / F16 / BF16).
 *                  A half call returns bit for bit what the call returns on the upcast maps (converted on load).  The
 *                  layout flag SMOT_FEAT_CHANNELS_LAST is SMOT_ERR_UNSUPPORTED: pass NCHW copies.
 *   heights/widths host arrays [num_levels]: H_l, W_l.  Maps are not padded: edge tiles and levels smaller than a tile are
 *                  masked on load and on store; the convolution's zero padding is virtual.
 *   packed         smot_rpn_head_packed_floats(C, A) floats, 16-byte aligned, written by smot_rpn_head_pack from upstream's
 *                  parameters: conv.weight [C, C, 3, 3], conv.bias [C], cls_logits.weight [A, C(, 1, 1)], cls_logits.bias
 *                  [A], bbox_pred.weight [4A, C(, 1, 1)], bbox_pred.bias [4A] (one launch on `stream`; pack again when a
 *                  parameter changes).
 *   outputs        objectness_out[l] [num_images, A, H_l, W_l], regression_out[l] [num_images, 4A, H_l, W_l] (channel of
 *                  coordinate c of anchor a: 4a + c): contiguous fp32 NCHW — what smot_rpn_proposals_fwd reads in place.
 *   contract       an output's value depends on its own image's map of its own level alone, with a summation order fixed
 *                  by (C, A): image i of a call equals the one-image call on it, level l the one-level call on it, bit for
 *                  bit; deterministic.  A NaN or infinite input cell makes non-finite exactly the outputs whose 3x3 window
 *                  covers it.
 *   capacities     C % 32 == 0, 32 <= C <= 512, 1 <= A, 5 A <= 64 (SMOT_ERR_UNSUPPORTED beyond, also for a level of 2^28
 *                  cells or more); 1 <= num_images <= SMOT_MAX_IMAGES, 1 <= num_levels <= SMOT_MAX_LEVELS, non-null
 *                  pointers, H_l, W_l >= 1 (SMOT_ERR_BAD_ARG).  smot_rpn_head_packed_floats returns -1 for an unsupported
 *                  (C, A).  Nothing is launched by a refused call.
 *
 * RPN ANCHORS: [UPSTREAM] AnchorGenerator.grid_anchors for all levels in one launch:
 *   out[l][(h W_l + w) A_l + a] = cell_anchors[l][a] + (w s_l, h s_l, w s_l, h s_l), one fp32 addition per coordinate (the
 *   shifts are exact), i.e. bit for bit upstream's broadcast sum.  cell_anchors / out: HOST arrays [num_levels] of DEVICE
 *   pointers to fp32 [A_l, 4] / [H_l W_l A_l, 4], 16-byte aligned; num_anchors / strides / heights / widths: host int arrays
 *   [num_levels].  SMOT_ERR_BAD_ARG for num_levels outside [1, SMOT_MAX_LEVELS], a null or misaligned pointer, a
 *   non-positive size; SMOT_ERR_UNSUPPORTED for a level that spans more than 2^24 pixels or 2^31 anchors in all.
 */
long long smot_rpn_head_packed_floats(int C, int A);
int smot_rpn_head_pack(const float* conv_w, const float* conv_b, const float* cls_w, const float* cls_b,
                       const float* bbox_w, const float* bbox_b, int C, int A, float* packed, smot_stream_t stream);
int smot_rpn_head_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths, int num_levels,
                      int num_images, int C, int A, const float* packed, float* const* objectness_out,
                      float* const* regression_out, smot_stream_t stream);
int smot_rpn_anchors_fwd(const float* const* cell_anchors, const int* num_anchors, const int* strides, const int* heights,
                         const int* widths, int num_levels, float* const* out, smot_stream_t stream);

/*
 * RPN HEAD, HALF COMPUTE: the head above with its 3x3 convolution on the 16-bit matrix instruction
 * (v_mfma_f32_16x16x32_f16 / _bf16).  Opt-in: the entry points above and their packed image are untouched.  The arguments are
 * the fp32 twins' plus `compute_type` (SMOT_FEAT_F16 or SMOT_FEAT_BF16; anything else, SMOT_FEAT_F32 included, is
 * SMOT_ERR_BAD_ARG, and smot_rpn_head_half_packed_floats returns -1 for it).
 *
 *   t   = relu(conv3x3(rnd(x), rnd(conv.weight), pad 1) + conv.bias)
 *   obj = conv1x1(t, cls_logits.weight) + bias,  reg = conv1x1(t, bbox_pred.weight) + bias
 *
 *   rnd            tensor.to(compute_type)'s rounding: round to nearest even, an fp16 value beyond 65,504 becomes +-inf.  A
 *                  map value is loaded, widened to fp32 and then rounded (an fp16 map in fp16 mode is exact); the filters are
 *                  rounded once by smot_rpn_head_half_pack.  Products are exact, the accumulation is fp32, and the bias /
 *                  ReLU epilogue is the fp32 mode's.
 *   the heads      t stays fp32 on the chip and the two 1x1 heads run on it exactly as in the fp32 mode: fp32 matrix
 *                  instruction, unrounded cls_logits / bbox_pred.  The mode is the 3x3's; there is no second, data-dependent
 *                  rounding.
 *   packed         smot_rpn_head_half_packed_floats(C, A, compute_type) floats, 16-byte aligned, written by
 *                  smot_rpn_head_half_pack: the rounded filters two to a dword, everything behind them (biases, the heads'
 *                  rows) fp32 as smot_rpn_head_pack lays it out.  An image serves its compute_type and no other mode.
 *   contract       the fp32 mode's: one launch for all images and levels, no host synchronisation; a summation order fixed by
 *                  (C, A): image i of a call equals the one-image call on it bit for bit; a NaN or infinite input cell (an
 *                  fp16-mode value beyond 65,504 included) makes non-finite exactly the outputs whose 3x3 window covers it.
 *   capacities     the fp32 mode's (C % 32 == 0 is the K step of the 16-bit instruction), also SMOT_ERR_UNSUPPORTED for a
 *                  level of 2^26 cells or more.  Validation, refusals and "nothing is launched by a refused call" as above.
 */
long long smot_rpn_head_half_packed_floats(int C, int A, int compute_type);
int smot_rpn_head_half_pack(const float* conv_w, const float* conv_b, const float* cls_w, const float* cls_b,
                            const float* bbox_w, const float* bbox_b, int C, int A, int compute_type, float* packed,
                            smot_stream_t stream);
int smot_rpn_head_half_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths, int num_levels,
                           int num_images, int C, int A, int compute_type, const float* packed,
                           float* const* objectness_out, float* const* regression_out, smot_stream_t stream);

/*
 * FEATURE PYRAMID (csrc/fpn.hip): [UPSTREAM] maskrcnn_benchmark FPN.forward with the top-down path resized bilinearly to
 * the lateral's size (the stage maps need not halve exactly) — backbone stage maps to the pyramid's maps for every image of
 * a call in num_levels + 1 launches (one lateral launch per level, coarsest first, then ONE launch for the 3x3 convolutions
 * of all levels and images) and without a host synchronisation.  All products run on the fp32 matrix cores (exact fp32
 * products, fp32 accumulation).
 *
 *   last[L-1] = conv1x1(x[L-1], inner_w) + inner_b
 *   last[l]   = conv1x1(x[l], inner_w) + inner_b + resize(last[l+1] -> (H_l, W_l))       l = L-2 .. 0
 *   P[l]      = conv3x3(last[l], layer_w, pad 1) + layer_b                               every l
 *   P[L]      = P[L-1][:, :, ::2, ::2]                                                   top_block = 1 (LastLevelMaxPool)
 *
 *   resize         torch's F.interpolate(size=, mode="bilinear", align_corners=False) in fp32: scale = float(in) /
 *                  float(out), src = scale * (dst + 0.5f) - 0.5f (0 where negative), i0 = (int)src, i1 = i0 + (i0 < in - 1),
 *                  w1 = src - i0, w0 = 1 - w1, value = h0 * (w0 v00 + w1 v01) + h1 * (w0 v10 + w1 v11), every operation
 *                  rounded on its own and all four products evaluated: a non-finite cell spreads as it does in torch.
 *   stages[l]      [num_images, in_channels[l], H_l, W_l], finest first, contiguous NCHW, all of element type `stage_type`
 *                  (SMOT_FEAT_F32 / F16 / BF16): a half call returns bit for bit what the call returns on the upcast maps.
 *                  The layout flag SMOT_FEAT_CHANNELS_LAST is SMOT_ERR_UNSUPPORTED.
 *   packed         smot_fpn_packed_floats(...) floats, 16-byte aligned, written by smot_fpn_pack (one launch on `stream`;
 *                  pack again when a parameter changes) from upstream's parameters, HOST arrays [num_levels] of DEVICE
 *                  pointers: inner_w[l] = fpn_inner{l+1}.weight [C, in_channels[l](, 1, 1)], inner_b[l] [C], layer_w[l] =
 *                  fpn_layer{l+1}.weight [C, C, 3, 3], layer_b[l] [C], all fp32.
 *   ws             smot_fpn_ws_bytes(...) bytes, 16-byte aligned, owned by the caller: the fp32 last[l] maps.
 *   out            HOST array of num_levels + top_block DEVICE pointers: out[l] [num_images, C, H_l, W_l], out[num_levels]
 *                  [num_images, C, (H + 1) / 2, (W + 1) / 2] of the coarsest level; contiguous NCHW of element type
 *                  `out_type` (SMOT_FEAT_F32, or F16 / BF16: the fp32 value rounded to nearest even, NaN kept).
 *   contract       an output's value depends on its own image alone, with a summation order fixed by (in_channels[l], C)
 *                  and the position: image i of a call equals the one-image call on it bit for bit; deterministic.
 *   capacities     C % 32 == 0, 32 <= C <= 512, in_channels[l] % 16 == 0, 16 <= in_channels[l] <= 2048
 *                  (SMOT_ERR_UNSUPPORTED beyond, also for a level of 2^31 / max(C, in_channels[l]) cells or more);
 *                  1 <= num_levels <= SMOT_MAX_LEVELS - 1, 1 <= num_images <= SMOT_MAX_IMAGES, non-null pointers at
 *                  their alignment, H_l, W_l >= 1, top_block 0 or 1 (SMOT_ERR_BAD_ARG).  smot_fpn_packed_floats returns
 *                  -1 for unsupported channel counts, smot_fpn_ws_bytes -1 for counts or sizes out of range.  Nothing is
 *                  launched by a refused call.
 */
long long smot_fpn_packed_floats(int num_levels, const int* in_channels, int C);
int smot_fpn_pack(const float* const* inner_w, const float* const* inner_b, const float* const* layer_w,
                  const float* const* layer_b, int num_levels, const int* in_channels, int C, float* packed,
                  smot_stream_t stream);
long long smot_fpn_ws_bytes(int num_levels, const int* heights, const int* widths, int num_images, int C);
int smot_fpn_fwd(const void* const* stages, int stage_type, const int* in_channels, const int* heights, const int* widths,
                 int num_levels, int num_images, int C, const float* packed, float* ws, void* const* out, int out_type,
                 int top_block, smot_stream_t stream);

/*
 * FEATURE PYRAMID, HALF COMPUTE: the pyramid above with both convolutions on the 16-bit matrix instruction
 * (v_mfma_f32_16x16x32_f16 / _bf16).  Opt-in: the entry points above and their packed image are untouched.  The arguments are
 * the fp32 twins' plus `compute_type` (SMOT_FEAT_F16 or SMOT_FEAT_BF16; anything else, SMOT_FEAT_F32 included, is
 * SMOT_ERR_BAD_ARG, and smot_fpn_half_packed_floats returns -1 for it).
 *
 *   last[l] = conv1x1(rnd(x[l]), rnd(inner_w)) + inner_b + resize(last[l+1] -> (H_l, W_l))    fp32, in the workspace
 *   P[l]    = conv3x3(rnd(last[l]), rnd(layer_w), pad 1) + layer_b                            stored in out_type
 *   P[L]    = P[L-1][:, :, ::2, ::2]                                                          stored with P[L-1]
 *
 *   rnd            tensor.to(compute_type)'s rounding: round to nearest even, an fp16 value beyond 65,504 becomes +-inf.  A
 *                  value is loaded, widened to fp32 and then rounded (an fp16 stage map in fp16 mode is exact); the filters
 *                  are rounded once by smot_fpn_half_pack.  Products are exact and the accumulation is fp32.  `last` is
 *                  kept in fp32 and rounded AGAIN when the 3x3 stage loads it: that second rounding is part of the mode.
 *                  The bias add, the bilinear sample (resize above, every operation rounded on its own, all four products)
 *                  and the stores are the fp32 mode's expressions.
 *   packed         smot_fpn_half_packed_floats(...) floats, 16-byte aligned, written by smot_fpn_half_pack: 16-bit operands
 *                  two to a dword, the biases fp32.  An image serves its compute_type and no other mode.
 *   ws             smot_fpn_ws_bytes(...) bytes as above: the mode's workspace is the fp32 mode's.
 *   contract       the fp32 mode's: num_levels + 1 launches, no host synchronisation; a summation order fixed by
 *                  (in_channels[l], C) and the position: image i of a call equals the one-image call on it bit for bit.  A
 *                  non-finite cell (an fp16-mode value beyond 65,504 included) reaches exactly the outputs that the fp32
 *                  mode's composition spreads it to.
 *   capacities     the fp32 mode's, plus in_channels[l] % 32 == 0 for every level (a K step is 32 channels):
 *                  SMOT_ERR_UNSUPPORTED beyond, naming the level; nothing is launched and the outputs are untouched.
 *                  Validation and refusals otherwise as above.
 */
long long smot_fpn_half_packed_floats(int num_levels, const int* in_channels, int C, int compute_type);
int smot_fpn_half_pack(const float* const* inner_w, const float* const* inner_b, const float* const* layer_w,
                       const float* const* layer_b, int num_levels, const int* in_channels, int C, int compute_type,
                       float* packed, smot_stream_t stream);
int smot_fpn_half_fwd(const void* const* stages, int stage_type, const int* in_channels, const int* heights,
                      const int* widths, int num_levels, int num_images, int C, int compute_type, const float* packed,
                      float* ws, void* const* out, int out_type, int top_block, smot_stream_t stream);

/*
 * DLA BACKBONE (csrc/dla.hip): [UPSTREAM] siammot/modelling/backbone/dla.py with DlaBasic blocks and maskrcnn_benchmark's
 * FrozenBatchNorm2d, inference — an image batch to the four stage maps x2 .. x5 (strides 4, 8, 16, 32) that smot_fpn_fwd
 * reads, without a host synchronisation or an allocation.  Every convolution runs on the fp32 matrix cores (exact fp32
 * products, fp32 accumulation) and has no bias; a frozen BN is y = x * scale + shift with scale = weight * rsqrt(running_var)
 * (no epsilon) and shift = bias - running_mean * scale, both computed by the caller; cbr = conv, BN, ReLU; cb = conv, BN.
 * ReLU is v < 0 ? 0 : v (a NaN stays); the 2x2 max-pool hands a NaN on, as torch's.  3x3 convolutions use pad 1.
 *
 *   x  = cbr7x7(image, 3 -> c0, pad 3);  x0 = cbr3x3(x, c0 -> c0);  x1 = cbr3x3(x0, c0 -> c1, stride 2)
 *   xk = tree(levels[k], x_{k-1}, c_{k-1} -> c_k, stride 2, level_root = (k > 2))         k = 2 .. 5; returned: x2 .. x5
 *   basic(x, s, residual) = relu(cb3x3(relu(cb3x3(x, stride s))) + residual)
 *   tree(1, x, cin -> cout, s, level_root, handed):
 *       bottom = maxpool2x2(x) if s == 2 else x;  residual = cb1x1(bottom) if cin != cout else bottom      ("project")
 *       x1 = basic(x, s, residual);  x2 = basic(x1, 1, x1)
 *       relu(cb1x1(cat(x2, x1, [bottom if level_root], *handed)))                                           ("root")
 *   tree(2, x, ...): bottom as above;  t = tree(1, x, cin -> cout, s, no level_root, nothing handed)
 *       tree(1, t, cout -> cout, 1, no level_root, handed = [bottom if level_root] + [t])
 *       (upstream evaluates the outer tree's project and discards it: it is not computed and not in the packed image)
 *
 *   launches       3 for the stem (7x7, 3x3, 3x3 stride 2; the two c0-channel maps go through the workspace), 6 per
 *                  levels = 1 tree, 11 per levels = 2 tree: 37 for DLA-34.  No cat and no pooled map is materialised.
 *   convolutions   "launch order": base_layer, level0, level1, then per tree(1): project (if cin != cout), tree1.conv1,
 *                  tree1.conv2, tree2.conv1, tree2.conv2, root; a tree(2) is its tree1 then its tree2 (37 for DLA-34;
 *                  smot_dla_pack checks the count).
 *   packed         smot_dla_packed_floats(...) floats, 16-byte aligned, written by smot_dla_pack (one launch per
 *                  convolution on `stream`; pack again when a parameter changes) from HOST arrays [num_convs] of DEVICE
 *                  pointers in launch order: w[i] the filters [Cout, Cin, k, k], scale[i], shift[i] [Cout], all fp32.
 *   image          [num_images, 3, H, W] contiguous NCHW of `in_type` (SMOT_FEAT_F32 / F16 / BF16; a half call returns bit
 *                  for bit what the call returns on the upcast image)
 *   ws             smot_dla_ws_bytes(...) bytes, 16-byte aligned, owned by the caller: the fp32 intermediates (and, for a
 *                  half `out_type`, the fp32 twins of x2 .. x4 that the next level reads)
 *   out            HOST array of four DEVICE pointers: out[k] [num_images, channels[k + 2], H >> (k + 2), W >> (k + 2)],
 *                  contiguous NCHW of `out_type` (fp32, or fp16 / bf16: the fp32 value rounded to nearest even, NaN kept)
 *   contract       an output depends on its own image alone, with a summation order fixed by the channel counts and the
 *                  position: image i of a call equals the one-image call on it bit for bit; deterministic.
 *   capacities     levels[0] == levels[1] == 1, levels[2..5] in {1, 2}; channels[0] in {16, 32}; channels[1..5] % 32 == 0,
 *                  32 <= . <= 1024;
 *                  H % 32 == 0, W % 32 == 0, H, W >= 32 (the stride-2 convolution gives ceil(H / 2) and the pool
 *                  floor(H / 2): upstream itself raises on any other size); every map of one image below 2^31 elements
 *                  (SMOT_ERR_UNSUPPORTED beyond).  1 <= num_images <= SMOT_MAX_IMAGES, non-null pointers at their
 *                  alignment, in_type / out_type as above (SMOT_ERR_BAD_ARG).  smot_dla_packed_floats and
 *                  smot_dla_ws_bytes return -1 for what smot_dla_fwd refuses.  Nothing is launched by a refused call.
 *
 * The operators alone (each packs its filters into caller memory, then runs: two or more launches):
 *   smot_dla_conv3x3_fwd   x [N, Cin, H, W] fp32 -> out [N, Cout, Ho, Wo] fp32, Ho = H (stride 1) or (H - 1) / 2 + 1
 *                  (stride 2), any H, W >= 1 with zeros beyond the map; w [Cout, Cin, 3, 3]; residual [N, Cout, Ho, Wo] or
 *                  null, with residual_h = residual_w = 0; or [N, Cout, residual_h, residual_w] read through a 2x2
 *                  max-pool (residual_h / 2 == Ho, residual_w / 2 == Wo: what a stage that keeps its width adds);
 *                  relu 0 / 1; packed: smot_dla_conv_packed_floats(3, Cin, Cout) floats, 16-byte aligned.
 *   smot_dla_conv3x3_form  which form of the 3x3 kernel that call runs: 10 * WR + NM (WR = 1, 2 or 4 row groups of the
 *                  workgroup's four waves, NM = M-tiles per pair: 41 42 22 12); chosen by Cout, the stride and the
 *                  number of 8 x 16 output tiles of all images; an output's value does not depend on it.  -1: bad argument.
 *                  Cin % 8 == 0, Cout 16 or % 32 == 0, both <= 1024 (SMOT_ERR_UNSUPPORTED beyond).
 *   smot_dla_conv1x1_fwd   a 1x1 convolution over the concatenation of num_sources (1 .. 4) fp32 maps, HOST arrays:
 *                  sources[s] [N, source_channels[s], source_heights[s], source_widths[s]]; source_pooled[s] != 0: read
 *                  through a 2x2 max-pool (heights / 2 == H, widths / 2 == W), else the map is H x W; w [Cout, sum of the
 *                  channels]; out [N, Cout, H, W] of out_type; packed: smot_dla_conv_packed_floats(1, sum, Cout) floats.
 *                  source_channels[s] % 16 == 0, Cout % 32 == 0, all <= 1024 (SMOT_ERR_UNSUPPORTED beyond).
 *   smot_dla_stem_fwd      image -> x1 [N, c1, H / 2, W / 2] fp32; w / scale / shift: HOST arrays of the three layers'
 *                  DEVICE pointers (base_layer, level0, level1); ws: smot_dla_stem_ws_bytes(...) bytes, 16-byte aligned.
 *                  c0 in {16, 32}, c1 % 32 == 0, c1 <= 1024, H and W even (SMOT_ERR_UNSUPPORTED beyond).
 */
long long smot_dla_packed_floats(const int* levels, const int* channels);
int smot_dla_pack(const int* levels, const int* channels, const float* const* w, const float* const* scale,
                  const float* const* shift, int num_convs, float* packed, smot_stream_t stream);
long long smot_dla_ws_bytes(const int* levels, const int* channels, int num_images, int H, int W);
int smot_dla_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                 const float* packed, float* ws, void* const* out, int out_type, smot_stream_t stream);
long long smot_dla_conv_packed_floats(int kernel_size, int Cin, int Cout);
int smot_dla_conv3x3_fwd(const float* x, int num_images, int Cin, int H, int W, const float* w, const float* scale,
                         const float* shift, int Cout, int stride, const float* residual, int residual_h, int residual_w,
                         int relu, float* packed, float* out, smot_stream_t stream);
int smot_dla_conv3x3_form(int num_images, int H, int W, int Cout, int stride);
int smot_dla_conv1x1_fwd(const float* const* sources, const int* source_channels, const int* source_pooled,
                         const int* source_heights, const int* source_widths, int num_sources, int num_images, int H, int W,
                         const float* w, const float* scale, const float* shift, int Cout, int relu, float* packed, void* out,
                         int out_type, smot_stream_t stream);
long long smot_dla_stem_ws_bytes(int num_images, int H, int W, int c0, int c1);
int smot_dla_stem_fwd(const void* image, int in_type, int num_images, int H, int W, int c0, int c1, const float* const* w,
                      const float* const* scale, const float* const* shift, float* ws, float* out, smot_stream_t stream);

/* DLA BACKBONE, SPLIT OPERANDS: the same network with the 3x3 convolutions of the trees (level2 .. level5) on
 * v_mfma_f32_16x16x32_bf16.  Every fp32 input value and filter is split into three bf16 parts (x = x1 + x2 + x3, round to
 * nearest even; exact for normal values), six of the nine part products are accumulated in fp32 (the dropped ones are
 * <= 2^-26 of a term): the result is an fp32-grade evaluation in another summation order, needs no knowledge of the data's
 * range (bf16 has fp32's exponents: no scaling, no maxima), and a non-finite input cell still reaches exactly the outputs
 * whose window covers it (as NaN, also where the fp32 kernel gives inf).  The 7x7, the stem's two 3x3 and every 1x1
 * convolution are the fp32 mode's kernels and packed images.  Each function is the twin of the one named without `split`:
 * same arguments, checks and error codes, with these differences:
 *   smot_dla_split_packed_floats / smot_dla_split_pack   the packed image holds the trees' 3x3 filters as split parts (1.5
 *                  times the fp32 image's size for them); it is NOT interchangeable with smot_dla_pack's.
 *   smot_dla_split_fwd             packed: smot_dla_split_pack's; ws: smot_dla_ws_bytes(...) bytes, as in fp32 mode.
 *   smot_dla_conv3x3_split_fwd     Cin % 32 == 0 (SMOT_ERR_UNSUPPORTED otherwise, nothing launched); packed:
 *                  smot_dla_conv_split_packed_floats(3, Cin, Cout) floats.
 *   smot_dla_conv3x3_split_form    the form that call runs (today the fp32 mode's rule).
 *   smot_dla_conv_split_packed_floats   kernel_size 3: the split image (-1 unless Cin % 32 == 0); 1 and 7: the fp32 mode's.
 */
long long smot_dla_split_packed_floats(const int* levels, const int* channels);
int smot_dla_split_pack(const int* levels, const int* channels, const float* const* w, const float* const* scale,
                        const float* const* shift, int num_convs, float* packed, smot_stream_t stream);
int smot_dla_split_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                       const float* packed, float* ws, void* const* out, int out_type, smot_stream_t stream);
long long smot_dla_conv_split_packed_floats(int kernel_size, int Cin, int Cout);
int smot_dla_conv3x3_split_fwd(const float* x, int num_images, int Cin, int H, int W, const float* w, const float* scale,
                               const float* shift, int Cout, int stride, const float* residual, int residual_h, int residual_w,
                               int relu, float* packed, float* out, smot_stream_t stream);
int smot_dla_conv3x3_split_form(int num_images, int H, int W, int Cout, int stride);

/* DLA BACKBONE, BOTTLENECK BLOCKS AND DEEPER TREES: upstream's DLA(levels, channels, block, residual_root) for block =
 * DlaBasic or DlaBottleneck (cardinality 1, base width 64) and trees of depth 1 .. 5: DLA-34, DLA-46-C, DLA-60, DLA-102,
 * DLA-169.  A second family next to smot_dla_*, with the DLA BACKBONE block's conventions (frozen BN, ReLU, pool, image, out,
 * ws, packed, "launch order", alignment, error codes) and these definitions:
 *
 *   bottleneck(x, s, residual) = relu(cb1x1(relu(cb3x3(relu(cb1x1(x, cin -> mid)), mid -> mid, stride s)), mid -> cout)
 *                                     + residual),  mid = cout / 2; conv1 runs at the block's INPUT resolution, the stride
 *                                is on the 3x3, as upstream
 *   block          SMOT_DLA_BLOCK_BASIC: basic(x, s, residual) of the DLA BACKBONE block; SMOT_DLA_BLOCK_BOTTLENECK: the above
 *   tree(1, x, cin -> cout, s, level_root, handed):  as in the DLA BACKBONE block with `block` for `basic`; with
 *       residual_root != 0 the root is relu(cb1x1(cat(x2, x1, ...)) + x2): every root adds its first source before the ReLU
 *   tree(n, x, cin -> cout, s, level_root, handed), n = 2 .. 5:  bottom as above
 *       t = tree(n - 1, x, cin -> cout, s, no level_root, nothing handed)
 *       tree(n - 1, t, cout -> cout, 1, no level_root, [bottom if level_root] + handed + [t])
 *       so the innermost root reads (x2, x1, [bottom], t of the outermost tree, ..., t of its parent): n + 2 maps for a
 *       level with level_root, n + 1 for level2.  A project is evaluated only in a depth-1 tree with cin != cout; the outer
 *       ones are not computed and not in the packed image.
 *   launches       = evaluated convolutions (smot_dla_net_num_convs; the stem's 3 included): per depth-1 tree project (if cin
 *                  != cout), tree1.conv1 .. conv3 (conv1, conv2 for basic), tree2.conv1 .., root; a deeper tree is its tree1
 *                  then its tree2.  DLA-34 37, DLA-46-C 48, DLA-60 63, DLA-102 105, DLA-169 168.
 *   split          != 0: the trees' 3x3 convolutions on the split-operand kernel and image (SPLIT OPERANDS above); every 1x1,
 *                  the stem and the workspace are the fp32 mode's.
 *   ws             smot_dla_net_ws_bytes(...) bytes.  A block's intermediate maps are released when the block returns and a
 *                  subtree's maps when its root has been written: a depth-n tree holds n - 1 tree1 results, one depth-1
 *                  tree's project, x1 and x2 and one block's intermediates at a time, whatever the number of blocks.
 *   contract       image i of a call equals the one-image call bit for bit; deterministic; no host synchronisation and no
 *                  allocation.  With block = BASIC, residual_root = 0 and levels[2..5] in {1, 2} the packed image has
 *                  smot_dla_packed_floats' (smot_dla_split_packed_floats') size and layout and smot_dla_net_fwd returns bit
 *                  for bit what smot_dla_fwd (smot_dla_split_fwd) returns.
 *   capacities     levels[0] == levels[1] == 1, levels[2..5] in 1 .. 5; channels[0] in {16, 32}; channels[1] % 32 == 0;
 *                  channels[2..5] % 32 == 0 (basic) or % 64 == 0 (bottleneck: mid % 32 == 0), all <= 1024; images as for
 *                  smot_dla_fwd, with a bottleneck's conv1 map (twice a level's own map) below 2^31 elements as well
 *                  (SMOT_ERR_UNSUPPORTED beyond).  block another value, null or misaligned pointers, num_images, in_type,
 *                  out_type: SMOT_ERR_BAD_ARG.  The size functions and smot_dla_net_num_convs return -1 for what
 *                  smot_dla_net_fwd refuses.  Nothing is launched by a refused call.
 *
 *   smot_dla_conv1x1_res_fwd   smot_dla_conv1x1_fwd with num_sources 1 .. 8 and an optional residual:
 *                  out = relu?(conv1x1(cat(sources)) * scale + shift + residual), one fp32 addition after the BN and before
 *                  the ReLU (a NaN or inf residual cell reaches exactly its own output cell).  residual: null, or
 *                  [N, Cout, H, W] fp32 with residual_h = residual_w = 0, or [N, Cout, residual_h, residual_w] read through
 *                  the 2x2 max-pool (residual_h / 2 == H, residual_w / 2 == W; SMOT_ERR_BAD_ARG otherwise), as
 *                  smot_dla_conv3x3_fwd's.  It is only read and may be one of the sources.  The K order is the
 *                  concatenation's order; with <= 4 sources and no residual the call returns the bits of smot_dla_conv1x1_fwd.
 */
#define SMOT_DLA_BLOCK_BASIC 0
#define SMOT_DLA_BLOCK_BOTTLENECK 1
int smot_dla_net_num_convs(const int* levels, const int* channels, int block);
long long smot_dla_net_packed_floats(const int* levels, const int* channels, int block, int residual_root, int split);
int smot_dla_net_pack(const int* levels, const int* channels, int block, int residual_root, int split, const float* const* w,
                      const float* const* scale, const float* const* shift, int num_convs, float* packed, smot_stream_t stream);
long long smot_dla_net_ws_bytes(const int* levels, const int* channels, int block, int residual_root, int num_images, int H,
                                int W);
int smot_dla_net_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                     int block, int residual_root, int split, const float* packed, float* ws, void* const* out, int out_type,
                     smot_stream_t stream);
int smot_dla_conv1x1_res_fwd(const float* const* sources, const int* source_channels, const int* source_pooled,
                             const int* source_heights, const int* source_widths, int num_sources, int num_images, int H, int W,
                             const float* w, const float* scale, const float* shift, int Cout, int relu, const float* residual,
                             int residual_h, int residual_w, float* packed, void* out, int out_type, smot_stream_t stream);

/* DLA BACKBONE, HALF COMPUTE: the same networks with every TREE convolution (level2 .. level5: the 3x3 convolutions and all
 * 1x1 convolutions — a bottleneck's conv1 / conv3, every root, every evaluated project) on v_mfma_f32_16x16x32_f16 /
 * v_mfma_f32_16x16x32_bf16 with ONE 16-bit operand per value.  compute_type: SMOT_FEAT_F16 (1) or SMOT_FEAT_BF16 (2);
 * anything else is SMOT_ERR_BAD_ARG (-1 from the size functions).
 *   operands     the input activation is rounded to compute_type as it is loaded, the filters once, by the pack kernels: round
 *                to nearest even, as torch's tensor.to(dtype).  An fp16 operand beyond 65,504 in magnitude is +-inf (as
 *                .half() makes it); bf16 keeps fp32's range.  Products are exact, accumulation is fp32.
 *   epilogue     the fp32 mode's, in fp32: acc * scale + shift (two roundings), + residual, ReLU in which a NaN stays.
 *   fp32 stays   the stem (base_layer, level0, level1: the fp32 kernels and images), scale / shift, residuals, every map in
 *                the workspace, the walker, the launches (37 / 48 / 63 / 105 / 168) and the workspace: smot_dla_net_ws_bytes.
 *   K padding    a K step is 32 channels and every width is a multiple of 32; a dead position of a tile and an absent
 *                M-tile multiply zeros or nothing, never a loaded value: a non-finite cell reaches exactly the outputs
 *                whose window covers it.
 *   contract     as smot_dla_net_fwd's: image i of a call equals the one-image call bit for bit; an output's sum order is
 *                fixed by the channel counts and its position; no host synchronisation, no allocation.  The result is NOT the
 *                fp32 mode's: it is the fp32 evaluation of the rounded operands in another summation order.
 *   smot_dla_half_packed_floats / smot_dla_half_pack / smot_dla_half_fwd   smot_dla_net_*'s arguments, checks and capacities
 *                with compute_type in place of split (basic and bottleneck blocks, any depth, residual roots).  The packed
 *                image is of one compute_type and serves no other mode.
 *   smot_dla_conv_half_packed_floats(kernel_size, Cin, Cout)   3: the one-part 3x3 image; 1: the half 1x1 image (both -1
 *                unless Cin % 32 == 0); 7: the fp32 mode's.  Each is followed by fp32 scale / shift as in fp32 mode.
 *   smot_dla_conv3x3_half_fwd   smot_dla_conv3x3_split_fwd's arguments with compute_type before packed; Cin % 32 == 0
 *                (SMOT_ERR_UNSUPPORTED otherwise, the message names Cin; nothing launched, out and packed untouched).
 *   smot_dla_conv3x3_half_form  the form that call runs (the fp32 mode's rule).
 *   smot_dla_conv1x1_half_fwd   smot_dla_conv1x1_res_fwd's arguments with compute_type before packed; every source a multiple
 *                of 32 channels (SMOT_ERR_UNSUPPORTED otherwise, the message names the source's width; nothing launched).
 *   smot_dla_conv1x1_half_form  the M-tiles (of 16 output channels) per workgroup that call runs: 4 where that still gives
 *                every CU a workgroup, else 2; -1: bad argument.  The form does not touch an output's sum order.
 */
long long smot_dla_half_packed_floats(const int* levels, const int* channels, int block, int residual_root, int compute_type);
int smot_dla_half_pack(const int* levels, const int* channels, int block, int residual_root, int compute_type,
                       const float* const* w, const float* const* scale, const float* const* shift, int num_convs, float* packed,
                       smot_stream_t stream);
int smot_dla_half_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                      int block, int residual_root, int compute_type, const float* packed, float* ws, void* const* out,
                      int out_type, smot_stream_t stream);
long long smot_dla_conv_half_packed_floats(int kernel_size, int Cin, int Cout);
int smot_dla_conv3x3_half_fwd(const float* x, int num_images, int Cin, int H, int W, const float* w, const float* scale,
                              const float* shift, int Cout, int stride, const float* residual, int residual_h, int residual_w,
                              int relu, int compute_type, float* packed, float* out, smot_stream_t stream);
int smot_dla_conv3x3_half_form(int num_images, int H, int W, int Cout, int stride);
int smot_dla_conv1x1_half_form(int num_images, int H, int W, int Cout);
int smot_dla_conv1x1_half_fwd(const float* const* sources, const int* source_channels, const int* source_pooled,
                              const int* source_heights, const int* source_widths, int num_sources, int num_images, int H, int W,
                              const float* w, const float* scale, const float* shift, int Cout, int relu, const float* residual,
                              int residual_h, int residual_w, int compute_type, float* packed, void* out, int out_type,
                              smot_stream_t stream);

/* DLA BACKBONE, HALF STORAGE: the half compute mode above with every map that a TREE convolution writes STORED in the compute
 * type: block intermediates, block outputs, project outputs, roots and the four returned stage maps.
 *   stored value the fp32 epilogue value (acc * scale + shift, + residual, ReLU) rounded once to compute_type, round to nearest
 *                even as torch's tensor.to(dtype); an fp16 value beyond 65,504 in magnitude is stored as +-inf, a NaN stays.
 *   operands     unchanged: half compute mode rounds an activation to compute_type as it loads it, rounding a stored value
 *                again gives the stored bits, and the 2 x 2 max-pool commutes with a monotone rounding.  What changes: a
 *                residual that is a stored map is added as the rounded value, and the returned maps are the stored maps.
 *   fp32 stays   the stem (base_layer, level0, level1) and its output x1 in the workspace: read as a convolution's input it
 *                changes nothing; as a residual (channels[1] == channels[2] only) its fp32 value is added.  Products,
 *                accumulation, scale / shift and the residual add stay fp32.  The packed image is smot_dla_half_pack's.
 *   contract     an operator here returns, bit for bit, what the half-mode operator (smot_dla_conv3x3_half_fwd /
 *                smot_dla_conv1x1_half_fwd) returns on the inputs and the residual widened to fp32, rounded once to
 *                compute_type: the same forms by the same rules, the same sum order.  Image i of a call equals the one-image
 *                call; no host synchronisation, no allocation; the launches are half mode's (37 / 48 / 63 / 105 / 168).
 *   types        in_type and res_type are each SMOT_FEAT_F32 or compute_type (anything else: SMOT_ERR_BAD_ARG, as a
 *                compute_type that is neither SMOT_FEAT_F16 nor SMOT_FEAT_BF16); a pointer must be aligned for its type (4 / 2
 *                bytes).  All sources of one 1x1 call have in_type.  res_type is not read where residual is null.
 *   smot_dla_half_storage_ws_bytes   the workspace of smot_dla_half_storage_fwd (-1 where smot_dla_net_ws_bytes is -1 or the
 *                compute_type is bad): x1 and the stem's two full-resolution maps in fp32, the tree maps in 2 bytes per
 *                element, no fp32 twin of a returned map.  Never above smot_dla_net_ws_bytes, and below it wherever a tree
 *                is that form's peak (where the stem's two fp32 maps and x1 are the peak of both forms, as for DLA-34, the
 *                two answers are equal); never below the stem's need plus x1.
 *   smot_dla_half_storage_fwd        smot_dla_half_fwd's arguments, checks and refusals without out_type: out[0..3] are
 *                [N, channels[k], H >> k, W >> k], k = 2 .. 5, of compute_type, 2-byte aligned.
 *   smot_dla_conv3x3_half_storage_fwd / smot_dla_conv1x1_half_storage_fwd   smot_dla_conv3x3_half_fwd's /
 *                smot_dla_conv1x1_half_fwd's arguments, checks and refusals with in_type behind x / sources and res_type behind
 *                residual, and without out_type: out is of compute_type.  A refused call launches nothing.
 */
long long smot_dla_half_storage_ws_bytes(const int* levels, const int* channels, int block, int residual_root, int compute_type,
                                         int num_images, int H, int W);
int smot_dla_half_storage_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                              int block, int residual_root, int compute_type, const float* packed, float* ws, void* const* out,
                              smot_stream_t stream);
int smot_dla_conv3x3_half_storage_fwd(const void* x, int in_type, int num_images, int Cin, int H, int W, const float* w,
                                      const float* scale, const float* shift, int Cout, int stride, const void* residual,
                                      int res_type, int residual_h, int residual_w, int relu, int compute_type, float* packed,
                                      void* out, smot_stream_t stream);
int smot_dla_conv1x1_half_storage_fwd(const void* const* sources, int in_type, const int* source_channels, const int* source_pooled,
                                      const int* source_heights, const int* source_widths, int num_sources, int num_images, int H,
                                      int W, const float* w, const float* scale, const float* shift, int Cout, int relu,
                                      const void* residual, int res_type, int residual_h, int residual_w, int compute_type,
                                      float* packed, void* out, smot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SMOT_EMM_H */
