// Shared by roi_align.hip and sr_xcorr.hip: level parameters, [UPSTREAM] LevelMapper and the per-axis
// sample bookkeeping of the legacy ROIAlign with virtual zero padding.
#pragma once
#include "smot_common.h"

namespace smot {

struct LevelParams {
    const float* feat[SMOT_MAX_LEVELS];
    int H[SMOT_MAX_LEVELS];
    int W[SMOT_MAX_LEVELS];
    int pad[SMOT_MAX_LEVELS];
    float scale[SMOT_MAX_LEVELS];
    int num_levels;
    float k_min, k_max;
};

// Element types of the feature maps (SMOT_FEAT_*).  Only the maps have a type: the kernels that read them convert right
// behind the load — fp16 with the exact hardware conversion (subnormals kept: the code objects run with fp16 denormals
// on), bf16 by a 16-bit shift — and every later instruction is the fp32 kernel's, so a call on maps of type T returns
// bit for bit what the fp32 call returns on the upcast maps.  LevelParams keeps its `const float*` slots for every type
// (the fp32 kernels' argument layout is untouched); a typed kernel reads them as `const FT*`.
struct f16_t {
    unsigned short bits;
};
struct bf16_t {
    unsigned short bits;
};
// one element from its 16 bits (the low half of `b`; the high half is ignored)
template <typename FT>
__device__ __forceinline__ float feat_cvt(unsigned b) {
    if constexpr (sizeof(FT) == 4) {
        return __uint_as_float(b);
    } else if constexpr (__is_same(FT, f16_t)) {
        return (float)__builtin_bit_cast(_Float16, (unsigned short)b);
    } else {
        return __uint_as_float(b << 16);
    }
}
// element k (0 / 1) of a dword that holds two 2-byte elements
template <typename FT, int K>
__device__ __forceinline__ float feat_of_pair(unsigned d) {
    if constexpr (__is_same(FT, f16_t)) {
        return (float)__builtin_bit_cast(_Float16, (unsigned short)(K == 0 ? d : d >> 16));
    } else {
        return __uint_as_float(K == 0 ? d << 16 : d & 0xffff0000u);
    }
}
template <typename FT>
__device__ __forceinline__ float feat_ld(const FT* p) {
    if constexpr (sizeof(FT) == 4) {
        return *p;
    } else {
        return feat_cvt<FT>(p->bits);
    }
}

// Channels-last maps (SMOT_FEAT_CHANNELS_LAST): N consecutive channels of one pixel, N * sizeof(FT) = 8, 16 or 32 bytes at
// that alignment (C % 8 == 0, a channel group's first channel a multiple of N), as 8- or 16-byte loads; converted like feat_ld.
template <typename FT, int N>
__device__ __forceinline__ void feat_ld_run(const FT* p, float* out) {
    constexpr int DW = N * (int)sizeof(FT) / 4;
    static_assert(DW == 2 || DW == 4 || DW == 8, "a run of 8, 16 or 32 bytes");
    unsigned d[DW];
    if constexpr (DW == 2) {
        const uint2 a = *reinterpret_cast<const uint2*>(p);
        d[0] = a.x;
        d[1] = a.y;
    } else {
#pragma unroll
        for (int q = 0; q < DW / 4; ++q) {
            const uint4 a = reinterpret_cast<const uint4*>(p)[q];
            d[4 * q + 0] = a.x;
            d[4 * q + 1] = a.y;
            d[4 * q + 2] = a.z;
            d[4 * q + 3] = a.w;
        }
    }
#pragma unroll
    for (int q = 0; q < DW; ++q) {
        if constexpr (sizeof(FT) == 4) {
            out[q] = __uint_as_float(d[q]);
        } else {
            out[2 * q] = feat_of_pair<FT, 0>(d[q]);
            out[2 * q + 1] = feat_of_pair<FT, 1>(d[q]);
        }
    }
}
template <typename FT>
__device__ __forceinline__ void feat_ld8(const FT* p, float* out) {
    feat_ld_run<FT, 8>(p, out);
}

// Rows of a batched call (smot_emm_*_batched_fwd): the rois of image b are [row_start[b], row_start[b+1]) and the maps are
// [num_images, C, H_l, W_l].  A kernel argument of the batched instantiations only; the single-image kernels take NoImages
// (nothing) and are unchanged.
struct ImageRows {
    static constexpr bool batched = true;
    int num_images;
    int row_start[SMOT_MAX_IMAGES + 1];
};
struct NoImages {                  // (members only so that code behind `if constexpr (BATCHED)` is well-formed; never read)
    static constexpr bool batched = false;
    static constexpr int num_images = 1;
    static constexpr int row_start[SMOT_MAX_IMAGES + 1] = {};
};

// The image of (wave-uniform) row n: the largest b < num_images with row_start[b] <= n (images without rows are skipped),
// by a binary search of scalar loads from the kernel-argument segment — at most 6 for 64 images.
__device__ __forceinline__ int image_of_row(const ImageRows& I, int n) {
    int lo = 0, hi = I.num_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (I.row_start[mid] <= n) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}
__device__ __forceinline__ int image_of_row(const NoImages&, int) { return 0; }

// Host side: check a batched call's row ranges (before any launch) and pack them.
inline int fill_image_rows(ImageRows* I, int num_images, const int* row_start, int N, const char* who) {
    if (num_images < 1 || num_images > SMOT_MAX_IMAGES) {
        set_error("%s: num_images=%d not in [1,%d]", who, num_images, SMOT_MAX_IMAGES);
        return SMOT_ERR_BAD_ARG;
    }
    if (row_start == nullptr) {
        set_error("%s: null row_start", who);
        return SMOT_ERR_BAD_ARG;
    }
    if (row_start[0] != 0) {
        set_error("%s: row_start[0]=%d, expected 0", who, row_start[0]);
        return SMOT_ERR_BAD_ARG;
    }
    for (int b = 0; b < num_images; ++b) {
        if (row_start[b + 1] < row_start[b]) {
            set_error("%s: row_start decreases at image %d (%d -> %d)", who, b, row_start[b], row_start[b + 1]);
            return SMOT_ERR_BAD_ARG;
        }
    }
    if (row_start[num_images] != N) {
        set_error("%s: row_start[%d]=%d, expected N=%d", who, num_images, row_start[num_images], N);
        return SMOT_ERR_BAD_ARG;
    }
    I->num_images = num_images;
    for (int b = 0; b <= SMOT_MAX_IMAGES; ++b) I->row_start[b] = b <= num_images ? row_start[b] : N;
    return SMOT_OK;
}

// [UPSTREAM] LevelMapper: floor(4 + log2(sqrt(area)/224 + 1e-6)), clamped, 0-based.
__device__ __forceinline__ int map_level(const float* b, float k_min, float k_max) {
    const float w = add_rn(sub_rn(b[2], b[0]), 1.0f);
    const float h = add_rn(sub_rn(b[3], b[1]), 1.0f);
    const float s = sqrtf(mul_rn(w, h));
    float lvl = floorf(add_rn(4.0f, log2f(add_rn(div_rn(s, 224.0f), 1e-6f))));
    lvl = fminf(fmaxf(lvl, k_min), k_max);
    return (int)lvl - (int)k_min;
}

// One axis sample of the legacy ROIAlign, evaluated against the PADDED extent `size_p`
// (= real + 2*pad) and re-expressed as indices into the REAL map.
__device__ __forceinline__ void axis_sample(float start, float bin, int G, int s, int size_real,
                                            int pad, int* lo, int* hi, float* w_lo, float* w_hi) {
    const int p = s / G;
    const int i = s - p * G;
    const int size_p = size_real + 2 * pad;
    // roi_start + p*bin + (i+.5f)*bin/G, each op rounded separately as in the reference
    float c = add_rn(add_rn(start, mul_rn((float)p, bin)),
                     div_rn(mul_rn((float)i + 0.5f, bin), (float)G));
    const bool valid = !(c < -1.0f || c > (float)size_p);
    if (c <= 0.0f) c = 0.0f;
    int l = (int)c;
    int h;
    if (l >= size_p - 1) {
        h = l = size_p - 1;
        c = (float)l;
    } else {
        h = l + 1;
    }
    const float fl = sub_rn(c, (float)l);   // weight of the high cell
    const float fh = sub_rn(1.0f, fl);      // weight of the low cell
    const int lr = l - pad, hr = h - pad;
    const bool lo_in = valid && lr >= 0 && lr < size_real;
    const bool hi_in = valid && hr >= 0 && hr < size_real;
    *lo = lo_in ? lr : 0;
    *hi = hi_in ? hr : 0;
    *w_lo = lo_in ? fh : 0.0f;
    *w_hi = hi_in ? fl : 0.0f;
}

// Host side: validate the per-level HOST arrays of the C ABI and pack them into kernel parameters.
// `nhwc_C`: the channel count when the caller has kernels for channels-last maps, 0 when it has none — a typed call with
// SMOT_FEAT_CHANNELS_LAST is then refused here (SMOT_ERR_UNSUPPORTED), as are C % 8 != 0 and maps that are not 16-byte aligned.
inline int fill_level_params(LevelParams* P, const float* const* feats, const int* heights, const int* widths,
                             const int* pad_cells, const float* scales, int num_levels, const char* who, int nhwc_C = 0) {
    if (channels_last() && (nhwc_C <= 0 || nhwc_C % 8 != 0)) {
        if (nhwc_C <= 0) set_error("%s: no channels-last (SMOT_FEAT_CHANNELS_LAST) form; pass NCHW maps", who);
        else set_error("%s: channels-last maps need C %% 8 == 0 (got C=%d); pass NCHW maps", who, nhwc_C);
        return SMOT_ERR_UNSUPPORTED;
    }
    if (!(feats && heights && widths && scales)) {
        set_error("%s: null level array", who);
        return SMOT_ERR_BAD_ARG;
    }
    if (num_levels < 1 || num_levels > SMOT_MAX_LEVELS) {
        set_error("%s: num_levels=%d not in [1,%d]", who, num_levels, SMOT_MAX_LEVELS);
        return SMOT_ERR_BAD_ARG;
    }
    for (int l = 0; l < num_levels; ++l) {
        const int pad = pad_cells ? pad_cells[l] : 0;
        if (!(feats[l] && heights[l] > 0 && widths[l] > 0 && pad >= 0 && scales[l] > 0.f)) {
            set_error("%s: bad level %d", who, l);
            return SMOT_ERR_BAD_ARG;
        }
        if (channels_last() && (reinterpret_cast<uintptr_t>(feats[l]) & 15) != 0) {
            set_error("%s: channels-last level %d is not 16-byte aligned", who, l);
            return SMOT_ERR_BAD_ARG;
        }
        P->feat[l] = feats[l];
        P->H[l] = heights[l];
        P->W[l] = widths[l];
        P->pad[l] = pad;
        P->scale[l] = scales[l];
    }
    P->num_levels = num_levels;
    P->k_min = -log2f(scales[0]);
    P->k_max = -log2f(scales[num_levels - 1]);
    return SMOT_OK;
}

}  // namespace smot
