// 3x3 convolution (pad 1, stride 1) as an implicit GEMM on v_mfma_f32_16x16x4_f32: the staging / matrix stage that
// fpn.hip's fpn_layer_kernel is built on (the scheme of rpn_head_kernel's first stage, see csrc/rpn_head.hip:8-21).
//
//   workgroup = 256 threads (4 waves) x one 8 x 16 tile of output positions x a BLOCK of up to 128 output channels: wave w
//               owns the block's channels [32 w, 32 w + 32) (two M-tiles) x the tile's eight rows (eight N-tiles of 16
//               positions): 16 accumulator tiles.  K order: input-channel chunk (8) > 4 channels per MFMA (2 k-steps) > tap (9).
//   A operand = packed filters (cv_pack_index): a wave's 36 values per lane and chunk are nine contiguous 16-byte loads,
//               straight into registers; the next chunk's nine loads are in flight while the current chunk multiplies.
//   B operand = one ds_read_b32 per MFMA from the chunk's eight zero-haloed 10 x 18 input planes in LDS (plane stride 208
//               dwords = 16 (mod 32): the four channels of a k-step fall on alternate halves of the 32 banks); cells outside
//               the map are ZEROS WRITTEN TO LDS (masked loads); the next chunk's cells are fetched into registers while the
//               current one is multiplied (two buffers: 2 x 8 x 208 x 4 = 13,312 B of LDS).
//
// A column of the product depends on that column of B alone: a non-finite input cell reaches exactly the outputs whose 3x3
// window covers it.  An output's sum order is fixed by the channel count and the position in its tile.
//
// The same stage with a stride of 1 or 2, Cin != Cout and a wave split between channels and rows (cvg_*, for csrc/dla.hip)
// follows at the end of the file.
#pragma once
#include "roi_common.h"

namespace smot {

typedef float cv_f32x4 __attribute__((ext_vector_type(4)));

constexpr int CV_TH = 8, CV_TW = 16;                 // output tile
constexpr int CV_PW = CV_TW + 2, CV_PH = CV_TH + 2;    // haloed input tile
constexpr int CV_CELLS = CV_PW * CV_PH;              // 180
constexpr int CV_PLANE = 208;                        // plane stride in LDS: = 16 (mod 32)
constexpr int CV_IC = 8;                             // input channels per chunk
constexpr int CV_BUF = CV_IC * CV_PLANE;             // floats per stage buffer
constexpr int CV_NLD = (CV_IC * CV_CELLS + 255) / 256;
constexpr int CV_MID = 128;                          // output channels per block
constexpr int CV_SMEM_FLOATS = 2 * CV_BUF;
static_assert(CV_CELLS <= CV_PLANE, "the stride holds a plane");

// Element i of the packed image of filters W [C, C, 3, 3] (9 C^2 floats) -> its index in W.  The image is
// [pair of M-tiles p][chunk c][q 0..8][lane][e 0..3]: value j = 4q + e of the lane's 36: M-tile m = j / 18, k-step
// ks = (j % 18) / 9, tap = j % 9 -> W[32p + 16m + lane % 16][8c + 4ks + lane / 16][tap].
__host__ __device__ inline long long cv_pack_index(long long i, int C) {
    const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
    long long r = i >> 8;
    const int q = (int)(r % 9);
    r /= 9;
    const int nch = C / CV_IC;
    const int c = (int)(r % nch), p = (int)(r / nch);
    const int j = 4 * q + e, m = j / 18, ks = (j % 18) / 9, tap = j % 9;
    const int oc = 32 * p + 16 * m + (lane & 15), ic = CV_IC * c + 4 * ks + (lane >> 4);
    return ((long long)oc * C + ic) * 9 + tap;
}

// fp32 -> OT at p: fp32 as it is; fp16 / bf16 by round-to-nearest-even (what torch's .to() does), NaN kept
template <typename OT>
__device__ __forceinline__ void cv_store(OT* p, float f) {
    if constexpr (sizeof(OT) == 4) {
        *p = f;
    } else if constexpr (__is_same(OT, f16_t)) {
        p->bits = __builtin_bit_cast(unsigned short, (_Float16)f);
    } else {
        const unsigned u = __float_as_uint(f);
        p->bits = (unsigned short)((f != f) ? 0x7fc0u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
}

// The tile's staging plan of one thread: element e = tid + 256 j of a chunk -> (offset in the chunk's eight planes or -1: a
// zero, LDS offset or -1: none).
struct CvPlan {
    int src[CV_NLD], dst[CV_NLD];
};
__device__ __forceinline__ void cv_plan(CvPlan& pl, int tid, int y0, int x0, int H, int W) {
    const int HW = H * W;
#pragma unroll
    for (int j = 0; j < CV_NLD; ++j) {
        const int e = tid + 256 * j;
        const int ic = e / CV_CELLS, cell = e - ic * CV_CELLS;
        const int r = cell / CV_PW, col = cell - r * CV_PW;
        const int gy = y0 - 1 + r, gx = x0 - 1 + col;
        const bool live = e < CV_IC * CV_CELLS;
        pl.dst[j] = live ? ic * CV_PLANE + r * CV_PW + col : -1;
        pl.src[j] = (live && gy >= 0 && gy < H && gx >= 0 && gx < W) ? ic * HW + gy * W + gx : -1;
    }
}

// acc[m][nt][r] (zeroed here) = sum over the C input channels and nine taps for output channel 32 pair + 16 m + 4 (lane / 16)
// + r of the packed filters at tile row nt, column lane % 16.  `in`: the image's [C, H, W] planes; `sm`: CV_SMEM_FLOATS
// floats of LDS that no wave reads any more (the caller's barrier); `active`: wave-uniform, false for a wave without
// channels in this block (it stages and meets the barriers, and multiplies nothing).  Ends behind a barrier.
template <typename FT>
__device__ __forceinline__ void cv_block(float* sm, const FT* __restrict__ in, int HW, int C, const CvPlan& pl,
                                         const float* __restrict__ packed, int pair, bool active, int tid,
                                         cv_f32x4 (&acc)[2][CV_TH]) {
    const int lane = tid & 63, kq = lane >> 4, xl = lane & 15;
    const int nch = C / CV_IC;
    const int boff = kq * CV_PLANE + xl;                   // B operand of lane (kq, xl): channel kq of the k-step, column xl
    float pre[CV_NLD];
    auto fetch = [&](int chunk) {
        const FT* __restrict__ base = in + (size_t)chunk * CV_IC * HW;
#pragma unroll
        for (int j = 0; j < CV_NLD; ++j) pre[j] = pl.src[j] >= 0 ? feat_ld<FT>(base + pl.src[j]) : 0.0f;
    };
    auto stash = [&](float* buf) {
#pragma unroll
        for (int j = 0; j < CV_NLD; ++j)
            if (pl.dst[j] >= 0) buf[pl.dst[j]] = pre[j];
    };
    const cv_f32x4* __restrict__ ap = reinterpret_cast<const cv_f32x4*>(packed) + (size_t)(active ? pair : 0) * nch * 9 * 64 + lane;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nt = 0; nt < CV_TH; ++nt) acc[m][nt] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cv_f32x4 an[9], ac[9];
    fetch(0);
#pragma unroll
    for (int q = 0; q < 9; ++q) an[q] = ap[q * 64];
    stash(sm);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const float* buf = sm + (c & 1) * CV_BUF;
#pragma unroll
        for (int q = 0; q < 9; ++q) ac[q] = an[q];
        if (c + 1 < nch) {
            fetch(c + 1);
#pragma unroll
            for (int q = 0; q < 9; ++q) an[q] = ap[((size_t)(c + 1) * 9 + q) * 64];
        }
        if (active) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int j0 = ks * 9 + tap, j1 = 18 + ks * 9 + tap;
                    const float a0 = ac[j0 >> 2][j0 & 3], a1 = ac[j1 >> 2][j1 & 3];
#pragma unroll
                    for (int nt = 0; nt < CV_TH; ++nt) {
                        const float b = buf[boff + ks * 4 * CV_PLANE + (nt + tap / 3) * CV_PW + (tap % 3)];
                        acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][nt], 0, 0, 0);
                        acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][nt], 0, 0, 0);
                    }
                }
        }
        if (c + 1 < nch) stash(sm + ((c + 1) & 1) * CV_BUF);     // the other buffer: its readers passed a barrier
        __syncthreads();
    }
}

// ---- the stage generalised (csrc/dla.hip): stride 1 or 2, Cin != Cout, the waves split between channel pairs and tile rows --
// Nothing above is touched: fpn_layer_kernel instantiates cv_plan / cv_block as they were.
//
//   STRIDE 2: the haloed input tile of an 8 x 16 output tile is 17 x 33 cells and a row's B reads are two dwords apart: the
//   16 lanes of one channel fall on 16 banks of ONE parity (ds_read_b32: 32 banks, conflicts within a 32-lane half).  The plane
//   stride is the cell count itself, 561, which is ODD: the second channel of the half lands on the banks of the other
//   parity, so a k-step's read is conflict-free with no padding at all (2 x 8 x 561 x 4 = 35,904 B of LDS).
//   WR: the four waves are WP = 4 / WR channel pairs x WR groups of 8 / WR tile rows, so that a layer of 32 (64) output
//   channels keeps four (two x two) waves busy instead of one (two); NM = 1: the pair's second M-tile does not exist
//   (Cout = 16) and is not multiplied.
template <int STRIDE>
struct CvGeom {
    static_assert(STRIDE == 1 || STRIDE == 2, "stride 1 or 2");
    static constexpr int PW = CV_TW * STRIDE + 3 - STRIDE;       // 18 | 33
    static constexpr int PH = CV_TH * STRIDE + 3 - STRIDE;       // 10 | 17
    static constexpr int CELLS = PW * PH;                        // 180 | 561
    static constexpr int PLANE = STRIDE == 1 ? CV_PLANE : CELLS;  // 208 = 16 (mod 32) | 561 = 1 (mod 2)
    static constexpr int BUF = CV_IC * PLANE;
    static constexpr int NLD = (CV_IC * CELLS + 255) / 256;      // 6 | 18
    static constexpr int SMEM_FLOATS = 2 * BUF;
};

// cv_pack_index for filters W [Cout, Cin, 3, 3], Cin % 8 == 0, the pairs padded to 32 output channels: -1 is a zero
__host__ __device__ inline long long cvg_pack_index(long long i, int Cin, int Cout) {
    const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
    long long r = i >> 8;
    const int q = (int)(r % 9);
    r /= 9;
    const int nch = Cin / CV_IC;
    const int c = (int)(r % nch), p = (int)(r / nch);
    const int j = 4 * q + e, m = j / 18, ks = (j % 18) / 9, tap = j % 9;
    const int oc = 32 * p + 16 * m + (lane & 15), ic = CV_IC * c + 4 * ks + (lane >> 4);
    return oc < Cout ? ((long long)oc * Cin + ic) * 9 + tap : -1;
}
__host__ __device__ inline long long cvg_packed_floats(int Cin, int Cout) {
    return (long long)((Cout + 31) / 32) * (Cin / CV_IC) * 9 * 256;
}

template <int STRIDE>
struct CvgPlan {
    int src[CvGeom<STRIDE>::NLD];                                // (the LDS offset follows from e: cvg_block's stash)
};
// (y0, x0): the OUTPUT tile's first position; H, W: the INPUT map
template <int STRIDE>
__device__ __forceinline__ void cvg_plan(CvgPlan<STRIDE>& pl, int tid, int y0, int x0, int H, int W) {
    using G = CvGeom<STRIDE>;
    const int HW = H * W;
#pragma unroll
    for (int j = 0; j < G::NLD; ++j) {
        const int e = tid + 256 * j;
        const int ic = e / G::CELLS, cell = e - ic * G::CELLS;
        const int r = cell / G::PW, col = cell - r * G::PW;
        const int gy = y0 * STRIDE - 1 + r, gx = x0 * STRIDE - 1 + col;
        const bool live = e < CV_IC * G::CELLS;
        pl.src[j] = (live && gy >= 0 && gy < H && gx >= 0 && gx < W) ? ic * HW + gy * W + gx : -1;
    }
}

// cv_block over Cin input channels for the wave's tile rows [row0, row0 + 8 / WR): acc[m][nt] is tile row row0 + nt.
template <typename FT, int STRIDE, int WR, int NM>
__device__ __forceinline__ void cvg_block(float* sm, const FT* __restrict__ in, int HW, int Cin, const CvgPlan<STRIDE>& pl,
                                          const float* __restrict__ packed, int pair, bool active, int tid, int row0,
                                          cv_f32x4 (&acc)[NM][CV_TH / WR]) {
    using G = CvGeom<STRIDE>;
    constexpr int ROWS = CV_TH / WR;
    const int lane = tid & 63, kq = lane >> 4, xl = lane & 15;
    const int nch = Cin / CV_IC;
    const int boff = kq * G::PLANE + row0 * STRIDE * G::PW + xl * STRIDE;
    float pre[G::NLD];
    auto fetch = [&](int chunk) {
        const FT* __restrict__ base = in + (size_t)chunk * CV_IC * HW;
#pragma unroll
        for (int j = 0; j < G::NLD; ++j) pre[j] = pl.src[j] >= 0 ? feat_ld<FT>(base + pl.src[j]) : 0.0f;
    };
    auto stash = [&](float* buf) {
#pragma unroll
        for (int j = 0; j < G::NLD; ++j) {
            if constexpr (G::PLANE == G::CELLS) {                // element e of the chunk lies at e: no table
                if (tid + 256 * j < CV_IC * G::CELLS) buf[tid + 256 * j] = pre[j];
            } else {
                const int e = tid + 256 * j, ic = e / G::CELLS;  // (recomputed per chunk: the table would cost registers)
                if (e < CV_IC * G::CELLS) buf[ic * G::PLANE + (e - ic * G::CELLS)] = pre[j];
            }
        }
    };
    const cv_f32x4* __restrict__ ap = reinterpret_cast<const cv_f32x4*>(packed) + (size_t)(active ? pair : 0) * nch * 9 * 64 + lane;
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int nt = 0; nt < ROWS; ++nt) acc[m][nt] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cv_f32x4 an[9], ac[9];
    fetch(0);
#pragma unroll
    for (int q = 0; q < 9; ++q) an[q] = ap[q * 64];
    stash(sm);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const float* buf = sm + (c & 1) * G::BUF;
#pragma unroll
        for (int q = 0; q < 9; ++q) ac[q] = an[q];
        if (c + 1 < nch) {
            fetch(c + 1);
#pragma unroll
            for (int q = 0; q < 9; ++q) an[q] = ap[((size_t)(c + 1) * 9 + q) * 64];
        }
        if (active) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int j0 = ks * 9 + tap, j1 = 18 + ks * 9 + tap;
                    const float a0 = ac[j0 >> 2][j0 & 3], a1 = ac[j1 >> 2][j1 & 3];
#pragma unroll
                    for (int nt = 0; nt < ROWS; ++nt) {
                        const float b = buf[boff + ks * 4 * G::PLANE + (nt * STRIDE + tap / 3) * G::PW + (tap % 3)];
                        acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][nt], 0, 0, 0);
                        if constexpr (NM == 2) acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][nt], 0, 0, 0);
                    }
                }
        }
        if (c + 1 < nch) stash(sm + ((c + 1) & 1) * G::BUF);     // the other buffer: its readers passed a barrier
        __syncthreads();
    }
}

}  // namespace smot
