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

// ---- the generalised stage with THREE-PART bf16 OPERANDS on v_mfma_f32_16x16x32_bf16 (cvs_*, for csrc/dla.hip) ---------------
// Nothing above is touched.  Same tiling (8 x 16 output tile, WR / NM as cvg_block), chunks of 32 input channels.
//
//   x = x1 + x2 + x3, x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2) (round to nearest even; the differences are
//   exact in fp32): |x2| <= 2^-9 |x|, |x3| <= 2^-18 |x|, and x is met to 2^-27 |x| or exactly.  Filters are split the same
//   way, once, by the pack kernel.  Of the nine part products the six with part indices i + j <= 4 are kept, (w3 x1), (w1 x3),
//   (w2 x2), (w2 x1), (w1 x2), (w1 x1) in this order, into ONE fp32 accumulator per tile: what is dropped is <= 2^-26 of a
//   term.  bf16 has fp32's exponent range: no scaling, no per-map maximum, and a column of the product still depends on that
//   column of B alone — an inf cell has x1 = inf, x2 = NaN (inf - inf), a NaN cell x1 = NaN: the outputs whose window covers
//   it are NaN, the others are untouched.  (A finite value that bf16() would round to inf — within 2^-9 of the largest —
//   keeps its first part truncated instead; the other two parts hold the rest.)
//   A operand = packed parts (cvs_pack_index): per tap 3 parts x NM M-tiles of 16 bytes per lane, straight into registers,
//               the next tap's in flight while the current tap multiplies (a chunk's 216 registers cannot be held).
//   B operand = the chunk's haloed cells in LDS as [part][group of 8 channels kq][cell] 16-byte slots: a lane's fragment
//               (channels 8 kq .. 8 kq + 7 of one position) is ONE aligned ds_read_b128 per part.  ds_read_b128 is served in
//               four groups of 16 lanes, each 8 lanes of one kq and 8 of the next, over 16 slots of a 256-byte bank row:
//               stride 1: a kq's lanes read consecutive slots and the group pitch GP = 192 = 0 (mod 16) puts the other
//               kq's eight on the eight slots left; stride 2: they read every other slot and GP = 561 is odd.  Conflict-free.
//   Staging   = a thread takes (kq, cell) units: eight coalesced-over-cells global loads (masked: cells outside the map are
//               ZEROS WRITTEN TO LDS), the split in registers, one ds_write_b128 per part.
//   LDS       = stride 1: two buffers of 3 x 4 x 192 x 16 = 36,864 B (73,728 B: two workgroups per CU); stride 2: 3 x 4 x
//               561 x 16 = 107,712 B, which fits once: ONE buffer, the next chunk's cells wait in registers across the
//               multiply (one workgroup per CU, hence 512 registers) and are stored between two barriers.
// An output's sum order is fixed by the channel counts and the position in its tile, as above.
constexpr int CVS_IC = 32;                                       // input channels per chunk
typedef unsigned cvs_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 cvs_bf16x8 __attribute__((ext_vector_type(8)));

template <int STRIDE>
struct CvsGeom {
    using G = CvGeom<STRIDE>;
    static constexpr int GP = STRIDE == 1 ? 192 : G::CELLS;      // slots between channel groups: = 0 (mod 16) | odd
    static constexpr int UNITS = 4 * G::CELLS;                   // (kq, cell): 720 | 2244
    static constexpr int NLD = (UNITS + 255) / 256;              // 3 | 9
    static constexpr int BUF = 3 * 4 * GP;                       // slots per stage buffer
    static constexpr int NBUF = STRIDE == 1 ? 2 : 1;
    static constexpr int SMEM_SLOTS = NBUF * BUF;
    static_assert(G::CELLS <= GP && (STRIDE == 1 ? GP % 16 == 0 : GP % 2 == 1), "the group pitch");
};

// bf16(v) by round-to-nearest-even in the low 16 bits; a NaN stays a NaN
__device__ __forceinline__ unsigned cvs_bf16(float v) {
    const unsigned u = __float_as_uint(v);
    return (v != v) ? 0x7fc0u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// v -> its three bf16 parts (header comment)
__device__ __forceinline__ void cvs_split(float v, unsigned (&p)[3]) {
    const unsigned u = __float_as_uint(v);
    unsigned p1 = cvs_bf16(v);
    if ((p1 & 0x7f80u) == 0x7f80u && (u & 0x7f800000u) != 0x7f800000u) p1 = u >> 16;
    const float r1 = v - __uint_as_float(p1 << 16);
    const unsigned p2 = cvs_bf16(r1);
    const float r2 = r1 - __uint_as_float(p2 << 16);
    p[0] = p1;
    p[1] = p2;
    p[2] = cvs_bf16(r2);
}

// Dword i of the packed image of the split filters W [Cout, Cin, 3, 3], Cin % 32 == 0, the pairs padded to 32 output
// channels -> the index in W of its LOW bf16 (the high one is the next input channel, 9 floats on), or -1: zeros; *part: 0..2.
// The image is [pair p][chunk c][tap][part][M-tile m][lane][e 0..3]: the lane's A fragment of v_mfma_f32_16x16x32_bf16,
// A[row lane % 16][k = 8 (lane / 16) + j], j = 2e, 2e + 1 -> W[32p + 16m + lane % 16][32c + 8 (lane / 16) + j][tap].
__host__ __device__ inline long long cvs_pack_index(long long i, int Cin, int Cout, int* part) {
    const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
    long long r = i >> 8;
    const int m = (int)(r & 1);
    r >>= 1;
    *part = (int)(r % 3);
    r /= 3;
    const int tap = (int)(r % 9);
    r /= 9;
    const int nch = Cin / CVS_IC;
    const int c = (int)(r % nch), p = (int)(r / nch);
    const int oc = 32 * p + 16 * m + (lane & 15), ic = CVS_IC * c + 8 * (lane >> 4) + 2 * e;
    return oc < Cout ? ((long long)oc * Cin + ic) * 9 + tap : -1;
}
__host__ __device__ inline long long cvs_packed_floats(int Cin, int Cout) {
    return (long long)((Cout + 31) / 32) * (Cin / CVS_IC) * 9 * 3 * 2 * 256;
}

template <int STRIDE>
struct CvsPlan {
    int src[CvsGeom<STRIDE>::NLD];                               // unit u = tid + 256 j: offset of its first channel, or -1
};
// (y0, x0): the OUTPUT tile's first position; H, W: the INPUT map
template <int STRIDE>
__device__ __forceinline__ void cvs_plan(CvsPlan<STRIDE>& pl, int tid, int y0, int x0, int H, int W) {
    using S = CvsGeom<STRIDE>;
    using G = CvGeom<STRIDE>;
    const int HW = H * W;
#pragma unroll
    for (int j = 0; j < S::NLD; ++j) {
        const int u = tid + 256 * j;
        const int kq = u / G::CELLS, cell = u - kq * G::CELLS;
        const int r = cell / G::PW, col = cell - r * G::PW;
        const int gy = y0 * STRIDE - 1 + r, gx = x0 * STRIDE - 1 + col;
        pl.src[j] = (u < S::UNITS && gy >= 0 && gy < H && gx >= 0 && gx < W) ? 8 * kq * HW + gy * W + gx : -1;
    }
}

// cvg_block with split operands: sm: CvsGeom<STRIDE>::SMEM_SLOTS 16-byte slots; packed: the cvs_pack_index image
template <typename FT, int STRIDE, int WR, int NM>
__device__ __forceinline__ void cvs_block(cvs_u32x4* sm, const FT* __restrict__ in, int HW, int Cin, const CvsPlan<STRIDE>& pl,
                                          const float* __restrict__ packed, int pair, bool active, int tid, int row0,
                                          cv_f32x4 (&acc)[NM][CV_TH / WR]) {
    using S = CvsGeom<STRIDE>;
    using G = CvGeom<STRIDE>;
    constexpr int ROWS = CV_TH / WR;
    static_assert(ROWS % 2 == 0, "rows are multiplied two at a time");
    const int lane = tid & 63, kq = lane >> 4, xl = lane & 15;
    const int nch = Cin / CVS_IC;
    const int boff = kq * S::GP + row0 * STRIDE * G::PW + xl * STRIDE;
    float pre[S::NLD][8];
    auto fetch = [&](int chunk) {
        const FT* __restrict__ base = in + (size_t)chunk * CVS_IC * HW;
#pragma unroll
        for (int j = 0; j < S::NLD; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) pre[j][k] = pl.src[j] >= 0 ? feat_ld<FT>(base + pl.src[j] + k * HW) : 0.0f;
    };
    auto stash = [&](cvs_u32x4* buf) {
#pragma unroll
        for (int j = 0; j < S::NLD; ++j) {
            const int u = tid + 256 * j, g = u / G::CELLS;
            if (u < S::UNITS) {
                unsigned lo[3], hi[3];
                cvs_u32x4 v[3];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cvs_split(pre[j][2 * e], lo);
                    cvs_split(pre[j][2 * e + 1], hi);
#pragma unroll
                    for (int p = 0; p < 3; ++p) v[p][e] = lo[p] | (hi[p] << 16);
                }
#pragma unroll
                for (int p = 0; p < 3; ++p) buf[(4 * p + g) * S::GP + (u - g * G::CELLS)] = v[p];
            }
        }
    };
    constexpr int AT = 3 * 2 * 64;                               // 16-byte values per (pair, chunk, tap)
    const cvs_u32x4* __restrict__ ap = reinterpret_cast<const cvs_u32x4*>(packed) + (size_t)(active ? pair : 0) * nch * 9 * AT + lane;
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int nt = 0; nt < ROWS; ++nt) acc[m][nt] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cvs_u32x4 an[3][NM], ac[3][NM];
    auto fetch_a = [&](int t) {                                  // t = 9 chunk + tap
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int m = 0; m < NM; ++m) an[p][m] = ap[(size_t)t * AT + (2 * p + m) * 64];
    };
    fetch(0);
    fetch_a(0);
    stash(sm);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const cvs_u32x4* buf = sm + (S::NBUF == 2 ? (c & 1) * S::BUF : 0);
        if (c + 1 < nch) fetch(c + 1);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int m = 0; m < NM; ++m) ac[p][m] = an[p][m];
            if (9 * c + tap + 1 < 9 * nch) fetch_a(9 * c + tap + 1);
            if (active) {
#pragma unroll
                for (int nt = 0; nt < ROWS; nt += 2) {
                    cvs_u32x4 b[2][3];
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int p = 0; p < 3; ++p)
                            b[r][p] = buf[4 * p * S::GP + boff + ((nt + r) * STRIDE + tap / 3) * G::PW + (tap % 3)];
                    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};      // (filter part, input part)
#pragma unroll
                    for (int q = 0; q < 6; ++q)
#pragma unroll
                        for (int r = 0; r < 2; ++r)
#pragma unroll
                            for (int m = 0; m < NM; ++m)
                                acc[m][nt + r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                    __builtin_bit_cast(cvs_bf16x8, ac[PA[q]][m]), __builtin_bit_cast(cvs_bf16x8, b[r][PB[q]]),
                                    acc[m][nt + r], 0, 0, 0);
                }
            }
        }
        if constexpr (S::NBUF == 1) __syncthreads();             // the one buffer: every wave is done reading it
        if (c + 1 < nch) stash(sm + (S::NBUF == 2 ? ((c + 1) & 1) * S::BUF : 0));
        __syncthreads();
    }
}

// ---- the generalised stage with ONE 16-bit OPERAND per value on v_mfma_f32_16x16x32_f16 / _bf16 (cvh_*, for csrc/dla.hip) -----
// Nothing above is touched.  The half compute mode: x and w are rounded to CT (SMOT_FEAT_F16 or SMOT_FEAT_BF16; round to
// nearest even, torch's .to(): an fp16 value beyond 65,504 becomes +-inf), the products are exact and the accumulation is
// fp32.  cvs_block's tiling, forms (WR, NM), staging units (cvs_plan), zero-written halo and slot layout with one part
// instead of three: one matrix instruction per tap, M-tile and row instead of six, a third of the LDS and of the A traffic.
//   LDS       = [group of 8 channels kq][cell] 16-byte slots, group pitch as cvs_block's (192 | 561: the same conflict-free
//               ds_read_b128 pattern within the one part): a buffer is 4 x 192 x 16 = 12,288 B (stride 1) / 4 x 561 x 16 =
//               35,904 B (stride 2).  BOTH strides take two buffers (24,576 B / 71,808 B) and two workgroups per CU (143,616 B
//               of the CU's 160 KB at stride 2): the next chunk is stored while the current one multiplies, one barrier per
//               chunk, and the stride-2 stage needs neither the single buffer nor the 512 registers of cvs_block.
//   Staging   = cvs_block's (kq, cell) units in GROUPS OF THREE: a group is loaded, waits in registers across three taps
//               (stride 2: 9 units, three groups; stride 1: 3 units, one group across all nine taps) and is rounded and
//               stored into the other buffer, which no wave reads during this chunk: 24 staging registers at either
//               stride instead of 72 at stride 2, which is what lets that stage fit the 256 registers of two workgroups per CU.
//   A operand = per tap NM M-tiles of 16 bytes per lane (cvh_pack_index), the next tap's in flight while this one multiplies.
// An output's sum order is fixed by the channel counts and the position in its tile, as above.
typedef _Float16 cvh_f16x8 __attribute__((ext_vector_type(8)));

// the 16 bits of v rounded to CT
template <int CT>
__device__ __forceinline__ unsigned cvh_bits(float v) {
    if constexpr (CT == SMOT_FEAT_F16) return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)v);
    else return cvs_bf16(v);
}
template <int CT>
__device__ __forceinline__ unsigned cvh_pack2(float lo, float hi) { return cvh_bits<CT>(lo) | (cvh_bits<CT>(hi) << 16); }
template <int CT>
__device__ __forceinline__ cv_f32x4 cvh_mfma(const cvs_u32x4& a, const cvs_u32x4& b, const cv_f32x4& c) {
    if constexpr (CT == SMOT_FEAT_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(cvh_f16x8, a), __builtin_bit_cast(cvh_f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cvs_bf16x8, a), __builtin_bit_cast(cvs_bf16x8, b), c, 0, 0, 0);
}

template <int STRIDE>
struct CvhGeom {
    using G = CvGeom<STRIDE>;
    static constexpr int GP = CvsGeom<STRIDE>::GP;               // slots between channel groups
    static constexpr int BUF = 4 * GP;                           // slots per stage buffer
    static constexpr int SMEM_SLOTS = 2 * BUF;
};

// Dword i of the packed image of the rounded filters W [Cout, Cin, 3, 3], Cin % 32 == 0, the pairs padded to 32 output
// channels -> the index in W of its LOW half (the high one is the next input channel, 9 floats on), or -1: zeros.
// The image is [pair p][chunk c][tap][M-tile m][lane][e 0..3]: the lane's A fragment, A[row lane % 16][k = 8 (lane / 16) + j],
// j = 2e, 2e + 1 -> W[32p + 16m + lane % 16][32c + 8 (lane / 16) + j][tap].
__host__ __device__ inline long long cvh_pack_index(long long i, int Cin, int Cout) {
    const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
    long long r = i >> 8;
    const int m = (int)(r & 1);
    r >>= 1;
    const int tap = (int)(r % 9);
    r /= 9;
    const int nch = Cin / CVS_IC;
    const int c = (int)(r % nch), p = (int)(r / nch);
    const int oc = 32 * p + 16 * m + (lane & 15), ic = CVS_IC * c + 8 * (lane >> 4) + 2 * e;
    return oc < Cout ? ((long long)oc * Cin + ic) * 9 + tap : -1;
}
__host__ __device__ inline long long cvh_packed_floats(int Cin, int Cout) {
    return (long long)((Cout + 31) / 32) * (Cin / CVS_IC) * 9 * 2 * 256;
}

// cvs_block with one part: sm: CvhGeom<STRIDE>::SMEM_SLOTS 16-byte slots; pl: cvs_plan's; packed: the cvh_pack_index image.
// FT: the input's element type (fp32, or f16_t / bf16_t: a stored value widens exactly and rounds to CT back to its own bits).
// USER: names the calling kernel family and is not read: the staging lambdas below are functions of their own per
// instantiation, and a second kernel that shared one would change how the compiler inlines them into the first (measured: the
// stride-1 half kernels took 3 - 6 more registers and one lost a wave of occupancy), so each family takes its own copy.
template <int CT, typename FT, int STRIDE, int WR, int NM, int USER = 0>
__device__ __forceinline__ void cvh_block(cvs_u32x4* sm, const FT* __restrict__ in, int HW, int Cin, const CvsPlan<STRIDE>& pl,
                                          const float* __restrict__ packed, int pair, bool active, int tid, int row0,
                                          cv_f32x4 (&acc)[NM][CV_TH / WR]) {
    using S = CvsGeom<STRIDE>;
    using Hh = CvhGeom<STRIDE>;
    using G = CvGeom<STRIDE>;
    constexpr int ROWS = CV_TH / WR;
    const int lane = tid & 63, kq = lane >> 4, xl = lane & 15;
    const int nch = Cin / CVS_IC;
    const int boff = kq * Hh::GP + row0 * STRIDE * G::PW + xl * STRIDE;
    // staging in groups of GRP units: a group is fetched, waits in registers across a third of the taps (stride 2: three
    // groups; stride 1: its three units are one group and wait across all nine) and is stored into the OTHER buffer, which
    // nobody reads during this chunk: 24 staging registers at either stride
    constexpr int GRP = 3, NG = S::NLD / GRP, TPG = 9 / NG;
    static_assert(S::NLD % GRP == 0 && 9 % NG == 0, "whole groups, whole taps per group");
    float pre[GRP][8];
    auto fetch = [&](int chunk, int gi) {
        const FT* __restrict__ base = in + (size_t)chunk * CVS_IC * HW;
        int hw = HW;
        asm volatile("" : "+s"(hw));                             // (opaque per chunk: the 72 addresses src + k HW of a
                                                                 // stride-2 tile are recomputed, not kept in registers)
#pragma unroll
        for (int j = 0; j < GRP; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) pre[j][k] = pl.src[GRP * gi + j] >= 0 ? feat_ld<FT>(base + pl.src[GRP * gi + j] + k * hw) : 0.0f;
    };
    auto stash = [&](cvs_u32x4* buf, int gi) {
#pragma unroll
        for (int j = 0; j < GRP; ++j) {
            const int u = tid + 256 * (GRP * gi + j), g = u / G::CELLS;
            if (u < S::UNITS) {
                cvs_u32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = cvh_pack2<CT>(pre[j][2 * e], pre[j][2 * e + 1]);
                buf[g * Hh::GP + (u - g * G::CELLS)] = v;
            }
        }
    };
    constexpr int AT = 2 * 64;                                   // 16-byte values per (pair, chunk, tap)
    const cvs_u32x4* __restrict__ ap = reinterpret_cast<const cvs_u32x4*>(packed) + (size_t)(active ? pair : 0) * nch * 9 * AT + lane;
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int nt = 0; nt < ROWS; ++nt) acc[m][nt] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cvs_u32x4 an[NM], ac[NM];
    auto fetch_a = [&](int t) {                                  // t = 9 chunk + tap
#pragma unroll
        for (int m = 0; m < NM; ++m) an[m] = ap[(size_t)t * AT + m * 64];
    };
    fetch_a(0);
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
        fetch(0, gi);
        stash(sm, gi);
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const cvs_u32x4* buf = sm + (c & 1) * Hh::BUF;
        cvs_u32x4* nxt = sm + ((c + 1) & 1) * Hh::BUF;           // its readers passed the barrier that ended chunk c - 1
        const bool more = c + 1 < nch;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap % TPG == 0 && more) {
                if (tap > 0) stash(nxt, tap / TPG - 1);
                fetch(c + 1, tap / TPG);
            }
#pragma unroll
            for (int m = 0; m < NM; ++m) ac[m] = an[m];
            if (9 * c + tap + 1 < 9 * nch) fetch_a(9 * c + tap + 1);
            if (active) {
#pragma unroll
                for (int nt = 0; nt < ROWS; ++nt) {
                    const cvs_u32x4 b = buf[boff + (nt * STRIDE + tap / 3) * G::PW + (tap % 3)];
#pragma unroll
                    for (int m = 0; m < NM; ++m) acc[m][nt] = cvh_mfma<CT>(ac[m], b, acc[m][nt]);
                }
            }
        }
        if (more) stash(nxt, NG - 1);
        __syncthreads();
    }
}

}  // namespace smot
