// K1+K2 for the reference's SECOND yaml family (configs/dla/DLA_34_FPN_EMM_AOT.yaml:52-63: 7x7 templates, search regions
// x5 -> 35x35 bins, 29x29 responses): search-region pooling feeding the depthwise correlation inside one kernel.
//
// Replaces, for this shape, the pair roi_align_levels_kernel<2> (SRPooler.forward, reference EMM/sr_pool.py:53-91 ->
// ROIAlign, with the virtual zero padding of track_utils.py:87-107) + xcorr_dw_rowpatch_kernel<35, 7> (xcorr_depthwise,
// EMM/xcorr.py:37-46): the [N, C, 35, 35] search-region tensor (18.8 MB at 30 tracks, written and read back) never
// reaches HBM and one launch disappears.
//
// The arithmetic is the two kernels' own, operation for operation, so the responses are bit-identical to the pair's
// (tests/test_hip_parity.py): a bin is the sum of its 2 x 2 samples' four weighted corners in the generic kernel's order
// (w1 v1 + w2 v2 + w3 v3 + w4 v4 per sample, accumulated sample by sample, / 4), a response is one fmaf chain over the 49
// taps, u-major / v-minor.  The search windows of this family are 50 x 100 .. 80 x 160 cells — beyond what a workgroup
// can stage — so the corners are gathered straight from the map, as the generic kernel does for such windows (a separable
// / staged form was measured slower there: measure/r03_generic_roi_separable.patch).
//
//   workgroup = (roi, 4 channels), 256 threads:
//     tables   the per-axis sample bookkeeping (70 + 70 samples: cell pair, weight pair), once for the four channels;
//     pooling  thread = bins t, t + 256, ...: the bin's tables in registers, channels inner; the pooled planes go to LDS
//              rows padded to 40 floats (the correlation's row segments are read as float4);
//     xcorr    thread = (response row, group of four response columns): the template's 49 taps in registers, per window row
//              one 10-float segment feeds 28 FMAs; plane after plane.
#include "pool_launch.h"
#include "knobs.h"
#include "tower_common.h"      // plane_max_wave

namespace smot {

constexpr int SX_CH = 4;             // channels per workgroup

// one cell of a plane by the maps' element type (the gathers of lanes whose cells do not lie in one piece)
template <typename FT>
__device__ __forceinline__ float sx_load1(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
    if constexpr (sizeof(FT) == 4) {
        return __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, 0, 0));
    } else {
        return feat_cvt<FT>((unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rsrc, voff, 0, 0));
    }
}

template <int RX, int RZ, int G>
__global__ void __launch_bounds__(256)
sr_xcorr_gather_kernel(LevelParams P, int C, const float* __restrict__ rois, const float* __restrict__ level_boxes,
                       const float* __restrict__ z, float* __restrict__ resp, float* __restrict__ plane_max) {
    constexpr bool BATCHED = false;
    constexpr NoImages I{};
    using FT = float;
#include "sr_xcorr_gather_body.h"
}

// A batch of images (smot_emm_track_batched_fwd): the rows of image b are [I.row_start[b], I.row_start[b+1])
template <int RX, int RZ, int G>
__global__ void __launch_bounds__(256)
sr_xcorr_gather_batched_kernel(LevelParams P, int C, const float* __restrict__ rois, const float* __restrict__ level_boxes,
                               const float* __restrict__ z, float* __restrict__ resp, float* __restrict__ plane_max,
                               ImageRows I) {
    constexpr bool BATCHED = true;
    using FT = float;
#include "sr_xcorr_gather_body.h"
}

// The same two kernels on fp16 / bf16 maps (FT = f16_t / bf16_t; smot_*_typed_fwd): P.feat[] is read as `const FT*`
template <typename FT, int RX, int RZ, int G>
__global__ void __launch_bounds__(256)
sr_xcorr_gather_half_kernel(LevelParams P, int C, const float* __restrict__ rois, const float* __restrict__ level_boxes,
                            const float* __restrict__ z, float* __restrict__ resp, float* __restrict__ plane_max) {
    static_assert(sizeof(FT) == 2, "fp16 / bf16 maps");
    constexpr bool BATCHED = false;
    constexpr NoImages I{};
#include "sr_xcorr_gather_body.h"
}
template <typename FT, int RX, int RZ, int G>
__global__ void __launch_bounds__(256)
sr_xcorr_gather_half_batched_kernel(LevelParams P, int C, const float* __restrict__ rois,
                                    const float* __restrict__ level_boxes, const float* __restrict__ z,
                                    float* __restrict__ resp, float* __restrict__ plane_max, ImageRows I) {
    static_assert(sizeof(FT) == 2, "fp16 / bf16 maps");
    constexpr bool BATCHED = true;
#include "sr_xcorr_gather_body.h"
}

// The (35, 7, sampling ratio 2) head's pooling + correlation — the only shape the kernel has; its callers check it.  One image
// (I == nullptr) or the rows of a batch: the wrapper by I and the maps' element type, everything else once.
int sr_xcorr_gather_impl(const float* const* feats, const int* heights, const int* widths, const int* pad_cells,
                         const float* scales, int num_levels, int C, const float* boxes, const float* sr,
                         const float* templates, int N, float* resp, hipStream_t st, float* plane_max, const ImageRows* I) {
    const char* who = I ? "sr_xcorr_gather_batched" : "sr_xcorr_gather";
    LevelParams P;
    const int rc = fill_level_params(&P, feats, heights, widths, pad_cells, scales, num_levels, who);
    if (rc) return rc;
    if (N == 0) return SMOT_OK;
    const dim3 grid(N, (C + SX_CH - 1) / SX_CH);
    // (the batched wrappers take the row ranges behind the single-image wrappers' arguments)
    auto launch = [&](auto kernel, auto... rows) {
        SMOT_LAUNCH(kernel, grid, dim3(256), 0, st, P, C, sr, boxes, templates, resp, plane_max, rows...);
    };
    timer_mark(0, 0, st);
    if (feat_type() == SMOT_FEAT_F32) {
        if (I) launch(sr_xcorr_gather_batched_kernel<35, 7, 2>, *I);
        else launch(sr_xcorr_gather_kernel<35, 7, 2>);
    } else {
        SMOT_HALF_TYPES(if (I) launch(sr_xcorr_gather_half_batched_kernel<FT, 35, 7, 2>, *I);
                        else launch(sr_xcorr_gather_half_kernel<FT, 35, 7, 2>))
    }
    timer_mark(0, 1, st);
    return check_launch(who);
}

}  // namespace smot

// The C entry of the 35 / 7 shape (smot_sr_xcorr_fused_fwd covers 30 / 15): arguments as there, no pooled-plane output.
extern "C" int smot_sr_xcorr_gather_fwd(const float* const* feats, const int* heights, const int* widths,
                                        const int* pad_cells, const float* scales, int num_levels, int C,
                                        const float* boxes, const float* sr, const float* templates, int N, int rx, int rz,
                                        int sampling_ratio, float* resp, smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(N >= 0 && C > 0, "sr_xcorr_gather: bad sizes N=%d C=%d", N, C);
    if (!(rx == 35 && rz == 7 && sampling_ratio == 2)) {
        set_error("sr_xcorr_gather: only Rx=35, Rz=7, sampling_ratio=2 (got %d, %d, %d); use smot_sr_xcorr_fused_fwd (30 / 15) or "
                  "smot_roi_align_levels_fwd + smot_xcorr_dw_fwd", rx, rz, sampling_ratio);
        return SMOT_ERR_UNSUPPORTED;
    }
    if (N == 0) return SMOT_OK;
    SMOT_REQUIRE(boxes && sr && templates && resp, "sr_xcorr_gather: null pointer");
    return sr_xcorr_gather_impl(feats, heights, widths, pad_cells, scales, num_levels, C, boxes, sr, templates, N, resp,
                                (hipStream_t)stream, nullptr, nullptr);
}

// fp16 / bf16 maps (include/smot_emm.h, "fp16 / bf16 FEATURE MAPS")
extern "C" int smot_sr_xcorr_gather_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                              const int* pad_cells, const float* scales, int num_levels, int C,
                                              const float* boxes, const float* sr, const float* templates, int N, int rx,
                                              int rz, int sampling_ratio, float* resp, smot_stream_t stream) {
    const int rc = smot::check_feat_type(feat_type, "sr_xcorr_gather_typed");
    if (rc) return rc;
    smot::FeatTypeScope scope(feat_type);
    return smot_sr_xcorr_gather_fwd(reinterpret_cast<const float* const*>(feats), heights, widths, pad_cells, scales, num_levels,
                                    C, boxes, sr, templates, N, rx, rz, sampling_ratio, resp, stream);
}
