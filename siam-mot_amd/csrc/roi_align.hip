// K1 — FPN-level-routed ROIAlign with virtual zero padding, and the search-region geometry.
//
// Replaces (see include/smot_emm.h): SRPooler.forward (reference EMM/sr_pool.py:53-91) incl.
// LevelMapper and ROIAlign [UPSTREAM maskrcnn_benchmark csrc/cuda/ROIAlign_cuda.cu], the
// TrackUtils.pad_feature pass (track_head/track_utils.py:87-107) and
// update_boxes_in_pad_images + extend_bbox (track_utils.py:62-85,109-135).
//
// Work decomposition: one workgroup per (roi, group of CH_PER_BLOCK channels).  The per-axis
// sample bookkeeping of the legacy ROIAlign (validity, clamp, low/high cell, bilinear weights —
// all channel-independent) is computed once per workgroup into LDS tables; cells that fall in
// the virtual zero border get weight 0 and a safe index, so the inner loop is branch-free.
// The bounding window of the cells a roi really touches (<= ~58x58 cells when the level matches
// the box; found with two LDS atomics per table entry) is staged per channel into LDS with
// coalesced row reads — every feature cell is fetched from HBM/L2 once instead of being gathered
// 16x per output; co-resident workgroups (2-3 per CU) overlap one's staging with another's pooling.
// Lanes walk the flattened (ph,pw) bin index (tables of one bin in registers, channels inner), so
// stores are fully coalesced.  Windows that exceed the LDS budget
// (degenerate aspect ratios) fall back to direct gathers from the map, same arithmetic.
#include "pool_launch.h"
#include "knobs.h"
#include <type_traits>

namespace smot {

constexpr int RA_WIN_FLOATS = 4096;   // LDS window budget per channel (16 KiB)
constexpr int RA_CH = 4;              // channels per workgroup (windows staged together: 64 KiB)

template <int G>
__global__ void __launch_bounds__(256)
roi_align_levels_kernel(LevelParams P, int C, const float* __restrict__ rois,
                        const float* __restrict__ level_boxes, int PH, int PW, int ch_per_block,
                        float* __restrict__ out, int32_t* __restrict__ levels_out, int num_images) {
    constexpr bool BATCHED = false;
    constexpr NoImages I{};
    using FT = float;
    constexpr bool NHWC = false;
#include "roi_align_body.h"
}

// A batch of images: [R,4] rois, the rows of image b are [I.row_start[b], I.row_start[b+1]) (smot_emm_*_batched_fwd)
template <int G>
__global__ void __launch_bounds__(256)
roi_align_levels_batched_kernel(LevelParams P, int C, const float* __restrict__ rois,
                                const float* __restrict__ level_boxes, int PH, int PW, int ch_per_block,
                                float* __restrict__ out, int32_t* __restrict__ levels_out, int num_images, ImageRows I) {
    constexpr bool BATCHED = true;
    using FT = float;
    constexpr bool NHWC = false;
#include "roi_align_body.h"
}

// The same two kernels on fp16 / bf16 maps (FT = f16_t / bf16_t; smot_*_typed_fwd): P.feat[] is read as `const FT*`.
// (The workgroups per CU of the fp32 twins asked for: left alone, the 3x3-sample forms took 188 registers.)
template <typename FT, int G>
__global__ void __launch_bounds__(256, G <= 2 ? 3 : (G == 3 ? 2 : 1))
roi_align_levels_half_kernel(LevelParams P, int C, const float* __restrict__ rois,
                             const float* __restrict__ level_boxes, int PH, int PW, int ch_per_block,
                             float* __restrict__ out, int32_t* __restrict__ levels_out, int num_images) {
    static_assert(sizeof(FT) == 2, "fp16 / bf16 maps");
    constexpr bool BATCHED = false;
    constexpr NoImages I{};
    constexpr bool NHWC = false;
#include "roi_align_body.h"
}
template <typename FT, int G>
__global__ void __launch_bounds__(256, G <= 3 ? 3 : 1)
roi_align_levels_half_batched_kernel(LevelParams P, int C, const float* __restrict__ rois,
                                     const float* __restrict__ level_boxes, int PH, int PW, int ch_per_block,
                                     float* __restrict__ out, int32_t* __restrict__ levels_out, int num_images,
                                     ImageRows I) {
    static_assert(sizeof(FT) == 2, "fp16 / bf16 maps");
    constexpr bool BATCHED = true;
    constexpr bool NHWC = false;
#include "roi_align_body.h"
}

// The same kernel on CHANNELS-LAST maps of every element type (SMOT_FEAT_CHANNELS_LAST; FT = float / f16_t / bf16_t): the
// window is staged from the pixels' channel runs into the same LDS image, the pooling behind it is the NCHW kernels' text —
// bit-identical results.  BATCHED_ = false: I is not read.
template <typename FT, int G, bool BATCHED_>
__global__ void __launch_bounds__(256, (sizeof(FT) == 2 && G <= 3) ? 2 : 1)
roi_align_levels_nhwc_kernel(LevelParams P, int C, const float* __restrict__ rois, const float* __restrict__ level_boxes,
                             int PH, int PW, int ch_per_block, float* __restrict__ out, int32_t* __restrict__ levels_out,
                             int num_images, ImageRows I) {
    constexpr bool BATCHED = BATCHED_;
    constexpr bool NHWC = true;
#include "roi_align_body.h"
}

// The generic kernel's ONE launch site: grid, LDS size and opt-in, and the wrapper by (channels_last(), feat_type(), I,
// samples per bin).  rois = [R,4] with level_boxes (the levels form), or [R,5] with num_images > 0 (smot_roi_align_fwd).
static int launch_roi_align(const LevelParams& P, int C, const float* rois, const float* level_boxes, int R, int PH, int PW,
                            int sampling_ratio, float* out, int32_t* levels_out, int num_images, hipStream_t st,
                            const ImageRows* I, const char* who) {
    const dim3 grid(R, (C + RA_CH - 1) / RA_CH);
    const size_t smem = (size_t)(PH + PW) * sampling_ratio * 16 + (size_t)RA_CH * RA_WIN_FLOATS * sizeof(float);
    SMOT_REQUIRE(smem <= 96 * 1024, "%s: pooled size %dx%d needs too much LDS", who, PH, PW);
    // (the batched wrappers and the channels-last ones take row ranges behind the single-image wrappers' arguments)
    auto launch = [&](auto kernel, const auto&... rows) {
        const int rco = ensure_lds_optin((const void*)kernel, 96 * 1024, "roi_align");
        if (rco) return rco;
        hipLaunchKernelGGL(kernel, grid, dim3(256), smem, st, P, C, rois, level_boxes, PH, PW, RA_CH, out, levels_out,
                           num_images, rows...);
        return check_launch(who);
    };
    auto by_samples = [&](auto g) {
        constexpr int G = decltype(g)::value;
        return with_feat_type([&](auto ft) {
            using FT = decltype(ft);
            if (channels_last()) {
                if (I) return launch(roi_align_levels_nhwc_kernel<FT, G, true>, *I);
                return launch(roi_align_levels_nhwc_kernel<FT, G, false>, one_image_rows(R));      // (not read)
            } else if constexpr (sizeof(FT) == 4) {
                if (I) return launch(roi_align_levels_batched_kernel<G>, *I);
                return launch(roi_align_levels_kernel<G>);
            } else {
                if (I) return launch(roi_align_levels_half_batched_kernel<FT, G>, *I);
                return launch(roi_align_levels_half_kernel<FT, G>);
            }
        });
    };
    switch (sampling_ratio) {
        case 1: return by_samples(std::integral_constant<int, 1>());
        case 2: return by_samples(std::integral_constant<int, 2>());
        case 3: return by_samples(std::integral_constant<int, 3>());
        default: return by_samples(std::integral_constant<int, 4>());
    }
}

__global__ void search_region_kernel(const float* __restrict__ boxes, int N, float pad, float half_e,
                                     float two_e, float min_wh, float* __restrict__ sr) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float x1 = add_rn(boxes[n * 4 + 0], pad), y1 = add_rn(boxes[n * 4 + 1], pad);
    const float x2 = add_rn(boxes[n * 4 + 2], pad), y2 = add_rn(boxes[n * 4 + 3], pad);
    const float w = add_rn(sub_rn(x2, x1), 1.0f);
    const float h = add_rn(sub_rn(y2, y1), 1.0f);
    const float w_ext = max_nan(div_rn(sub_rn(min_wh, w), two_e), mul_rn(w, half_e));
    const float h_ext = max_nan(div_rn(sub_rn(min_wh, h), two_e), mul_rn(h, half_e));
    sr[n * 4 + 0] = sub_rn(x1, w_ext);
    sr[n * 4 + 1] = sub_rn(y1, h_ext);
    sr[n * 4 + 2] = add_rn(x2, w_ext);
    sr[n * 4 + 3] = add_rn(y2, h_ext);
}

// smot_roi_align_levels_fwd's host code for one image (I == nullptr) or the rows of a batch (the generic branches of
// smot_emm_*_batched_fwd: the rows of image b are [I->row_start[b], I->row_start[b+1]) of rois / level_boxes / out).
int roi_align_levels_impl(const float* const* feats, const int* heights, const int* widths, const int* pad_cells,
                          const float* scales, int num_levels, int C, const float* rois, const float* level_boxes, int R,
                          int out_h, int out_w, int sampling_ratio, float* out, int32_t* levels_out, hipStream_t st,
                          const ImageRows* I, const char* who) {
    SMOT_REQUIRE(C > 0 && out_h > 0 && out_w > 0 && R >= 0, "%s: bad sizes C=%d out=%dx%d R=%d", who, C, out_h, out_w, R);
    if (sampling_ratio <= 0 || sampling_ratio > 4) {
        set_error("%s: sampling_ratio=%d unsupported (need 1..4; adaptive grid not implemented)", who, sampling_ratio);
        return SMOT_ERR_UNSUPPORTED;
    }
    if (R == 0) return SMOT_OK;
    SMOT_REQUIRE(rois && out, "%s: null rois/out", who);
    SMOT_REQUIRE(num_levels == 1 || level_boxes, "%s: level_boxes required for num_levels>1", who);
    LevelParams P;
    const int rc = fill_level_params(&P, feats, heights, widths, pad_cells, scales, num_levels, who, C);
    if (rc) return rc;
    // the EMM pooler shapes (15x15 templates, 30x30 search regions) and the box head's 7x7, 2x2 samples, take the separable
    // wave-per-two-planes kernel of sr_xcorr.hip; everything else the generic kernel above
    if (out_h == out_w && (out_h == 7 || out_h == 15 || out_h == 30) && sampling_ratio == 2 && !knobs().roi_generic)
        return launch_roi_pool_separable(P, C, rois, num_levels > 1 ? level_boxes : rois, R, out_h, out, levels_out, st, I);
    return launch_roi_align(P, C, rois, level_boxes, R, out_h, out_w, sampling_ratio, out, levels_out, 0, st, I, who);
}
}  // namespace smot

extern "C" int smot_roi_align_levels_fwd(const float* const* feats, const int* heights,
                                         const int* widths, const int* pad_cells,
                                         const float* scales, int num_levels, int C,
                                         const float* rois, const float* level_boxes, int R,
                                         int out_h, int out_w, int sampling_ratio, float* out,
                                         int32_t* levels_out, smot_stream_t stream) {
    return smot::roi_align_levels_impl(feats, heights, widths, pad_cells, scales, num_levels, C, rois, level_boxes, R, out_h,
                                       out_w, sampling_ratio, out, levels_out, (hipStream_t)stream, nullptr, "roi_align");
}

extern "C" int smot_roi_align_fwd(const float* input, int num_images, int C, int H, int W, int pad_cells,
                                  const float* rois5, int R, float spatial_scale, int pooled_h, int pooled_w,
                                  int sampling_ratio, float* out, smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(num_images > 0 && C > 0 && H > 0 && W > 0 && pooled_h > 0 && pooled_w > 0 && R >= 0 && pad_cells >= 0 &&
                     spatial_scale > 0.f,
                 "roi_align: bad sizes B=%d C=%d H=%d W=%d pooled=%dx%d R=%d pad=%d scale=%g", num_images, C, H, W,
                 pooled_h, pooled_w, R, pad_cells, (double)spatial_scale);
    if (sampling_ratio <= 0 || sampling_ratio > 4) {
        set_error("roi_align: sampling_ratio=%d unsupported (need 1..4; adaptive grid not implemented)",
                  sampling_ratio);
        return SMOT_ERR_UNSUPPORTED;
    }
    if (R == 0) return SMOT_OK;
    SMOT_REQUIRE(input && rois5 && out, "roi_align: null pointer");
    LevelParams P;
    const int rc = fill_level_params(&P, &input, &H, &W, &pad_cells, &spatial_scale, 1, "roi_align", C);
    if (rc) return rc;
    return launch_roi_align(P, C, rois5, nullptr, R, pooled_h, pooled_w, sampling_ratio, out, nullptr, num_images,
                            (hipStream_t)stream, nullptr, "roi_align");
}

extern "C" int smot_search_region_fwd(const float* boxes, int N, float pad_pixels, float search_expansion,
                                      float min_search_wh, float* sr, smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(N >= 0, "search_region: N=%d", N);
    if (N == 0) return SMOT_OK;
    SMOT_REQUIRE(boxes && sr, "search_region: null pointer");
    // the reference forms e/2 and e*2 in Python double before they meet the fp32 tensors
    const float half_e = (float)((double)search_expansion / 2.0);
    const float two_e = (float)((double)search_expansion * 2.0);
    hipLaunchKernelGGL(search_region_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, boxes, N,
                       pad_pixels, half_e, two_e, min_search_wh, sr);
    return check_launch("search_region");
}

// ---- fp16 / bf16 maps (include/smot_emm.h, "fp16 / bf16 FEATURE MAPS"): the element type is checked, set for the call's
// duration (FeatTypeScope: the launch sites above pick the kernels by it) and the fp32 entry point's host code runs ----------
extern "C" int smot_roi_align_levels_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                               const int* pad_cells, const float* scales, int num_levels, int C,
                                               const float* rois, const float* level_boxes, int R, int out_h, int out_w,
                                               int sampling_ratio, float* out, int32_t* levels_out, smot_stream_t stream) {
    const int rc = smot::check_feat_type(feat_type, "roi_align_levels_typed");
    if (rc) return rc;
    smot::FeatTypeScope scope(feat_type);
    return smot_roi_align_levels_fwd(reinterpret_cast<const float* const*>(feats), heights, widths, pad_cells, scales, num_levels,
                                     C, rois, level_boxes, R, out_h, out_w, sampling_ratio, out, levels_out, stream);
}

// several images per call: the maps are [num_images, C, H_l, W_l], the rows of image b are [row_start[b], row_start[b+1])
extern "C" int smot_roi_align_levels_batched_typed_fwd(const void* const* feats, int feat_type, const int* heights,
                                                       const int* widths, const int* pad_cells, const float* scales,
                                                       int num_levels, int C, const float* rois, const float* level_boxes,
                                                       int R, int out_h, int out_w, int sampling_ratio, float* out,
                                                       int32_t* levels_out, smot_stream_t stream, int num_images,
                                                       const int* row_start) {
    using namespace smot;
    const int rc = check_feat_type(feat_type, "roi_align_levels_batched_typed");
    if (rc) return rc;
    FeatTypeScope scope(feat_type);
    ImageRows I;
    const int rci = fill_image_rows(&I, num_images, row_start, R, "roi_align_levels_batched_typed");
    if (rci) return rci;
    return roi_align_levels_impl(reinterpret_cast<const float* const*>(feats), heights, widths, pad_cells, scales, num_levels,
                                 C, rois, level_boxes, R, out_h, out_w, sampling_ratio, out, levels_out, (hipStream_t)stream,
                                 &I, "roi_align_levels_batched_typed");
}

extern "C" int smot_roi_align_typed_fwd(const void* input, int feat_type, int num_images, int C, int H, int W, int pad_cells,
                                        const float* rois5, int R, float spatial_scale, int pooled_h, int pooled_w,
                                        int sampling_ratio, float* out, smot_stream_t stream) {
    const int rc = smot::check_feat_type(feat_type, "roi_align_typed");
    if (rc) return rc;
    smot::FeatTypeScope scope(feat_type);
    return smot_roi_align_fwd(reinterpret_cast<const float*>(input), num_images, C, H, W, pad_cells, rois5, R, spatial_scale,
                              pooled_h, pooled_w, sampling_ratio, out, stream);
}
