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
#include "roi_common.h"
#include "knobs.h"

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

template <typename FT, int G, bool B>
static int launch_roi_align_nhwc_one(dim3 grid, size_t smem, hipStream_t st, const LevelParams& P, int C, const float* rois,
                                     const float* level_boxes, int PH, int PW, float* out, int32_t* levels_out,
                                     int num_images, const ImageRows& I) {
    const int rco = ensure_lds_optin((const void*)roi_align_levels_nhwc_kernel<FT, G, B>, 96 * 1024, "roi_align");
    if (rco) return rco;
    hipLaunchKernelGGL((roi_align_levels_nhwc_kernel<FT, G, B>), grid, dim3(256), smem, st, P, C, rois, level_boxes, PH, PW,
                       RA_CH, out, levels_out, num_images, I);
    return SMOT_OK;
}
// the channels-last launch of a typed call in progress (channels_last()): I = the batch's row ranges, or nullptr
static int launch_roi_align_nhwc(int sampling_ratio, dim3 grid, size_t smem, hipStream_t st, const LevelParams& P, int C,
                                 const float* rois, const float* level_boxes, int PH, int PW, float* out,
                                 int32_t* levels_out, int num_images, const ImageRows* I) {
    ImageRows none;
    none.num_images = 1;
    for (int b = 0; b <= SMOT_MAX_IMAGES; ++b) none.row_start[b] = 0;
#define SMOT_RA_NHWC(FT_, G_)                                                                                          \
    (I != nullptr ? launch_roi_align_nhwc_one<FT_, G_, true>(grid, smem, st, P, C, rois, level_boxes, PH, PW, out,      \
                                                             levels_out, num_images, *I)                              \
                  : launch_roi_align_nhwc_one<FT_, G_, false>(grid, smem, st, P, C, rois, level_boxes, PH, PW, out,     \
                                                              levels_out, num_images, none))
#define SMOT_RA_NHWC_G(G_)                                                                                             \
    (feat_type() == SMOT_FEAT_F32 ? SMOT_RA_NHWC(float, G_)                                                            \
                                  : (feat_type() == SMOT_FEAT_F16 ? SMOT_RA_NHWC(f16_t, G_) : SMOT_RA_NHWC(bf16_t, G_)))
    switch (sampling_ratio) {
        case 1: return SMOT_RA_NHWC_G(1);
        case 2: return SMOT_RA_NHWC_G(2);
        case 3: return SMOT_RA_NHWC_G(3);
        default: return SMOT_RA_NHWC_G(4);
    }
#undef SMOT_RA_NHWC_G
#undef SMOT_RA_NHWC
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

}  // namespace smot

namespace smot {
int launch_roi_pool_separable(const LevelParams& P, int C, const float* rois, const float* level_boxes, int R,
                              int out_size, float* out, int32_t* levels_out, hipStream_t st);   // sr_xcorr.hip
}

namespace smot {
int launch_roi_pool_separable_batched(const LevelParams& P, int C, const float* rois, const float* level_boxes, int R,
                                      int out_size, float* out, hipStream_t st, const ImageRows& I);   // sr_xcorr.hip

// smot_roi_align_levels_fwd over a batch (the generic branches of smot_emm_*_batched_fwd): same routing, same kernels'
// batched forms; the rows of image b are [I.row_start[b], I.row_start[b+1]) of rois / level_boxes / out
int roi_align_levels_batched(const float* const* feats, const int* heights, const int* widths, const int* pad_cells,
                             const float* scales, int num_levels, int C, const float* rois, const float* level_boxes, int R,
                             int out_hw, int sampling_ratio, float* out, hipStream_t st, const ImageRows& I) {
    SMOT_REQUIRE(C > 0 && out_hw > 0 && R >= 0, "roi_align_batched: bad sizes C=%d out=%d R=%d", C, out_hw, R);
    if (sampling_ratio <= 0 || sampling_ratio > 4) {
        set_error("roi_align_batched: sampling_ratio=%d unsupported (need 1..4)", sampling_ratio);
        return SMOT_ERR_UNSUPPORTED;
    }
    if (R == 0) return SMOT_OK;
    LevelParams P;
    const int rc = fill_level_params(&P, feats, heights, widths, pad_cells, scales, num_levels, "roi_align_batched", C);
    if (rc) return rc;
    if ((out_hw == 7 || out_hw == 15 || out_hw == 30) && sampling_ratio == 2 && !knobs().roi_generic)
        return launch_roi_pool_separable_batched(P, C, rois, num_levels > 1 ? level_boxes : rois, R, out_hw, out, st, I);
    dim3 grid(R, (C + RA_CH - 1) / RA_CH);
    const size_t smem = (size_t)(2 * out_hw) * sampling_ratio * 16 + (size_t)RA_CH * RA_WIN_FLOATS * sizeof(float);
    SMOT_REQUIRE(smem <= 96 * 1024, "roi_align_batched: pooled size %d needs too much LDS", out_hw);
#define LAUNCH(G)                                                                                                  \
    if (feat_type() != SMOT_FEAT_F32) {                                                                            \
        SMOT_HALF_TYPES(                                                                                           \
            const int rco = ensure_lds_optin((const void*)roi_align_levels_half_batched_kernel<FT, G>, 96 * 1024,  \
                                             "roi_align");                                                         \
            if (rco) return rco;                                                                                   \
            hipLaunchKernelGGL((roi_align_levels_half_batched_kernel<FT, G>), grid, dim3(256), smem, st, P, C,      \
                               rois, level_boxes, out_hw, out_hw, RA_CH, out, (int32_t*)nullptr, 0, I))            \
    } else {                                                                                                       \
        const int rco = ensure_lds_optin((const void*)roi_align_levels_batched_kernel<G>, 96 * 1024, "roi_align");  \
        if (rco) return rco;                                                                                       \
        hipLaunchKernelGGL(roi_align_levels_batched_kernel<G>, grid, dim3(256), smem, st, P, C, rois, level_boxes,  \
                           out_hw, out_hw, RA_CH, out, (int32_t*)nullptr, 0, I);                                  \
    }
    if (channels_last()) {
        const int rcn = launch_roi_align_nhwc(sampling_ratio, grid, smem, st, P, C, rois, level_boxes, out_hw, out_hw, out,
                                              nullptr, 0, &I);
        return rcn ? rcn : check_launch("roi_align_batched");
    }
    switch (sampling_ratio) {
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        case 3: LAUNCH(3); break;
        default: LAUNCH(4); break;
    }
#undef LAUNCH
    return check_launch("roi_align_batched");
}
}  // namespace smot

extern "C" int smot_roi_align_levels_fwd(const float* const* feats, const int* heights,
                                         const int* widths, const int* pad_cells,
                                         const float* scales, int num_levels, int C,
                                         const float* rois, const float* level_boxes, int R,
                                         int out_h, int out_w, int sampling_ratio, float* out,
                                         int32_t* levels_out, smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(C > 0 && out_h > 0 && out_w > 0 && R >= 0, "roi_align: bad sizes C=%d out=%dx%d R=%d", C,
                 out_h, out_w, R);
    if (sampling_ratio <= 0 || sampling_ratio > 4) {
        set_error("roi_align: sampling_ratio=%d unsupported (need 1..4; adaptive grid not implemented)",
                  sampling_ratio);
        return SMOT_ERR_UNSUPPORTED;
    }
    if (R == 0) return SMOT_OK;
    SMOT_REQUIRE(rois && out, "roi_align: null rois/out");
    SMOT_REQUIRE(num_levels == 1 || level_boxes, "roi_align: level_boxes required for num_levels>1");
    LevelParams P;
    {
        const int rc = fill_level_params(&P, feats, heights, widths, pad_cells, scales, num_levels, "roi_align", C);
        if (rc) return rc;
    }

    // the EMM pooler shapes (15x15 templates, 30x30 search regions) and the box head's 7x7, 2x2 samples, take the separable
    // wave-per-two-planes kernel of sr_xcorr.hip; everything else the generic kernel below
    if (out_h == out_w && (out_h == 7 || out_h == 15 || out_h == 30) && sampling_ratio == 2 && !knobs().roi_generic)
        return launch_roi_pool_separable(P, C, rois, num_levels > 1 ? level_boxes : rois, R, out_h, out, levels_out,
                                         (hipStream_t)stream);
    const int ch_per_block = RA_CH;
    dim3 grid(R, (C + ch_per_block - 1) / ch_per_block);
    const size_t smem = (size_t)(out_h + out_w) * sampling_ratio * 16 + (size_t)RA_CH * RA_WIN_FLOATS * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(G)                                                                                        \
    if (feat_type() != SMOT_FEAT_F32) {                                                                  \
        SMOT_HALF_TYPES(                                                                                 \
            const int rco = ensure_lds_optin((const void*)roi_align_levels_half_kernel<FT, G>, 96 * 1024, "roi_align"); \
            if (rco) return rco;                                                                         \
            hipLaunchKernelGGL((roi_align_levels_half_kernel<FT, G>), grid, dim3(256), smem, st, P, C, rois, \
                               level_boxes, out_h, out_w, ch_per_block, out, levels_out, 0))             \
    } else {                                                                                             \
        const int rco = ensure_lds_optin((const void*)roi_align_levels_kernel<G>, 96 * 1024, "roi_align");   \
        if (rco) return rco;                                                                             \
        hipLaunchKernelGGL(roi_align_levels_kernel<G>, grid, dim3(256), smem, st, P, C, rois, level_boxes, \
                           out_h, out_w, ch_per_block, out, levels_out, 0);                              \
    }
    SMOT_REQUIRE(smem <= 96 * 1024, "roi_align: pooled size %dx%d needs too much LDS", out_h, out_w);
    if (channels_last()) {
        const int rcn = launch_roi_align_nhwc(sampling_ratio, grid, smem, st, P, C, rois, level_boxes, out_h, out_w, out,
                                              levels_out, 0, nullptr);
        return rcn ? rcn : check_launch("roi_align");
    }
    switch (sampling_ratio) {
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        case 3: LAUNCH(3); break;
        default: LAUNCH(4); break;
    }
#undef LAUNCH
    return check_launch("roi_align");
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
    {
        const int rc = fill_level_params(&P, &input, &H, &W, &pad_cells, &spatial_scale, 1, "roi_align", C);
        if (rc) return rc;
    }
    dim3 grid(R, (C + RA_CH - 1) / RA_CH);
    const size_t smem = (size_t)(pooled_h + pooled_w) * sampling_ratio * 16 + (size_t)RA_CH * RA_WIN_FLOATS * sizeof(float);
    SMOT_REQUIRE(smem <= 96 * 1024, "roi_align: pooled size %dx%d needs too much LDS", pooled_h, pooled_w);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(G)                                                                                        \
    if (feat_type() != SMOT_FEAT_F32) {                                                                  \
        SMOT_HALF_TYPES(                                                                                 \
            const int rco = ensure_lds_optin((const void*)roi_align_levels_half_kernel<FT, G>, 96 * 1024, "roi_align"); \
            if (rco) return rco;                                                                         \
            hipLaunchKernelGGL((roi_align_levels_half_kernel<FT, G>), grid, dim3(256), smem, st, P, C, rois5, \
                               (const float*)nullptr, pooled_h, pooled_w, RA_CH, out, (int32_t*)nullptr, num_images)) \
    } else {                                                                                             \
        const int rco = ensure_lds_optin((const void*)roi_align_levels_kernel<G>, 96 * 1024, "roi_align");   \
        if (rco) return rco;                                                                             \
        hipLaunchKernelGGL(roi_align_levels_kernel<G>, grid, dim3(256), smem, st, P, C, rois5,           \
                           (const float*)nullptr, pooled_h, pooled_w, RA_CH, out, (int32_t*)nullptr, num_images); \
    }
    if (channels_last()) {
        const int rcn = launch_roi_align_nhwc(sampling_ratio, grid, smem, st, P, C, rois5, nullptr, pooled_h, pooled_w, out,
                                              nullptr, num_images, nullptr);
        return rcn ? rcn : check_launch("roi_align");
    }
    switch (sampling_ratio) {
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        case 3: LAUNCH(3); break;
        default: LAUNCH(4); break;
    }
#undef LAUNCH
    return check_launch("roi_align");
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

extern "C" int smot_roi_align_typed_fwd(const void* input, int feat_type, int num_images, int C, int H, int W, int pad_cells,
                                        const float* rois5, int R, float spatial_scale, int pooled_h, int pooled_w,
                                        int sampling_ratio, float* out, smot_stream_t stream) {
    const int rc = smot::check_feat_type(feat_type, "roi_align_typed");
    if (rc) return rc;
    smot::FeatTypeScope scope(feat_type);
    return smot_roi_align_fwd(reinterpret_cast<const float*>(input), num_images, C, H, W, pad_cells, rois5, R, spatial_scale,
                              pooled_h, pooled_w, sampling_ratio, out, stream);
}
