// Internal: the launchers one .hip file of the library calls in another — one prototype each, here, instead of a hand-written
// copy in every caller.
//
// `const ImageRows* I` throughout: the validated row ranges of a batched call (smot_emm_*_batched_fwd: the batched kernels),
// or nullptr for one image (the single-image kernels).
#pragma once
#include "roi_common.h"
#include "logit_src.h"

namespace smot {

// The rows of one image of R rois as a batch of one — what a kernel that exists in a batched form only (the channels-last
// ones) is given for a single image: {1, [0, R, R, ...]}, as fill_image_rows packs it.
inline ImageRows one_image_rows(int R) {
    ImageRows one;
    one.num_images = 1;
    one.row_start[0] = 0;
    for (int b = 1; b <= SMOT_MAX_IMAGES; ++b) one.row_start[b] = R;
    return one;
}

// `f(FT())` with FT = the maps' element type of the call in progress (float, f16_t or bf16_t: feat_type()); returns what f does
template <typename F>
inline auto with_feat_type(F&& f) {
    switch (feat_type()) {
        case SMOT_FEAT_F32: return f(float());
        case SMOT_FEAT_F16: return f(f16_t());
        default: return f(bf16_t());
    }
}

// ---- roi_align.hip: smot_roi_align_levels_fwd's host code (`who` names the entry point in error texts) ----------------------
int roi_align_levels_impl(const float* const* feats, const int* heights, const int* widths, const int* pad_cells,
                          const float* scales, int num_levels, int C, const float* rois, const float* level_boxes, int R,
                          int out_h, int out_w, int sampling_ratio, float* out, int32_t* levels_out, hipStream_t st,
                          const ImageRows* I, const char* who);

// ---- sr_xcorr.hip: the separable pooling kernel (pooled sizes 7 / 15 / 30, 2 x 2 samples) and its fused forms ---------------
int launch_roi_pool_separable(const LevelParams& P, int C, const float* rois, const float* level_boxes, int R,
                              int out_size, float* out, int32_t* levels_out, hipStream_t st, const ImageRows* I);
// EMM.extract_cache in one launch (rz = 15 or 7): n_valid = the device count of a masked call, or nullptr
int launch_extract_cache(const float* const* feats, const int* heights, const int* widths, const float* scales,
                         int num_levels, int C, const float* boxes, int N, int rz, float pad_pixels, float half_e,
                         float two_e, float min_wh, float* templates, float* sr, const int* n_valid, float* order_hint,
                         hipStream_t st, int hint_extra_rows, const ImageRows* I);
int sr_xcorr_fused_impl(const float* const* feats, const int* heights, const int* widths, const int* pad_cells,
                        const float* scales, int num_levels, int C, const float* boxes, const float* sr,
                        const float* templates, int N, float* resp, float* x_debug, const float* order_hint,
                        hipStream_t st, const int** hint_status, float* plane_max, const ImageRows* I);

// ---- sr_xcorr_small.hip: the 35 / 7 gather kernel ----------------------------------------------------------------------------
int sr_xcorr_gather_impl(const float* const* feats, const int* heights, const int* widths, const int* pad_cells,
                         const float* scales, int num_levels, int C, const float* boxes, const float* sr,
                         const float* templates, int N, float* resp, hipStream_t st, float* plane_max, const ImageRows* I);

// ---- tower_wino.hip, predictor.hip, decode.hip: the head behind the response -------------------------------------------------
int launch_plane_absmax(const float* resp, int planes, int hw, float* pm, hipStream_t st);
int predictor_impl(const float* resp, int N, int C, int Ho, const float* cls_tower_w, const float* cls_gn_w,
                   const float* cls_gn_b, const float* reg_tower_w, const float* reg_gn_w, const float* reg_gn_b,
                   const float* cls_w, const float* cls_b, const float* center_w, const float* center_b,
                   const float* reg_w, const float* reg_b, int gn_groups, float gn_eps,
                   const float* tower_packed, float* tower_ws, float* logits, smot_stream_t stream, int* tiles_out,
                   unsigned* zero_words, bool* zeroed, const float* plane_max);
int decode_impl(LogitSrc L, const float* sr, const float* boxes, const float* hann, int N, int Ho, int up, int rx,
                int rz, float pad_pixels, float one_minus_sigma, float sigma, int use_centerness, float clip_w,
                float clip_h, float* cand_ws, float* bb, float* conf, int64_t* idx, bool tickets_zeroed,
                hipStream_t st, const int* poison);
unsigned* decode_tickets(float* cand_ws, int N, int Ho);

// ---- linear_rows.hip: the box head's layers ----------------------------------------------------------------------------------
int launch_linear_rows(const float* x, int M, int K, const float* W, const float* bias, int N, int relu, float* ws,
                       float* y, int ldy, hipStream_t st);
int launch_linear_rows2(const float* x, int M, int K, const float* W, const float* bias, int N1, const float* W2,
                        const float* bias2, int N2, int relu, float* ws, float* y, int ldy, hipStream_t st);
void linear_rows_layout(int M, int K, int N, int* S, int* nblk, int* rows_pad);
// K-slice scratch (floats) of launch_linear_rows / launch_linear_rows2 on M rows — any M: beyond 128 the launchers run row
// blocks of 128 in the same two launches (the C entry smot_linear_rows_fwd keeps its 128)
size_t linear_rows_part_floats(int M, int K, int N);
int launch_linear_rows_chain(const float* x, int M, int K, const float* WA, const float* bA, int NA, int reluA, float* ws_a,
                             const float* WB, int N1, const float* WB2, int N2, float* ws_b, hipStream_t st, int* rc);

}  // namespace smot
