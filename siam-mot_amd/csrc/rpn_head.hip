// RPN head and anchor grid — [UPSTREAM] maskrcnn_benchmark RPNHead.forward and AnchorGenerator.grid_anchors, for every
// image and every FPN level of a call in ONE launch each.
//
//   t   = relu(conv3x3(x_l, Wc, pad 1) + bc)     C -> C      (never leaves the chip)
//   obj = conv1x1(t, Wo) + bo                    C -> A      -> objectness[l]  [N, A,  H_l, W_l]
//   reg = conv1x1(t, Wr) + br                    C -> 4A     -> regression[l]  [N, 4A, H_l, W_l]   (channel 4a + c)
//
// rpn_head_kernel: both stages are GEMMs on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).
//
//   workgroup = (image, level, 8 x 16 tile of output positions) x ALL C mid channels, 4 waves.  The flat workgroup index
//               is mapped to (image, level, tile) through a per-level prefix table in the kernel arguments.
//   3x3 stage = implicit GEMM, in blocks of 128 mid channels: wave w owns the block's mid channels [32 w, 32 w + 32) (two
//               M-tiles) x the tile's eight rows (eight N-tiles of 16 positions): 16 accumulator tiles.
//               K order: input-channel chunk (8) > 4 channels per MFMA (2 k-steps) > tap (9).
//   A operand = the packed filters (smot_rpn_head_pack): a wave's 36 values per lane and chunk are nine contiguous
//               16-byte loads, straight from L2 into registers — no wave shares another's, so LDS would add nothing.  The next
//               chunk's nine loads are in flight while the current chunk feeds the matrix cores.
//   B operand = one ds_read_b32 per MFMA from the chunk's eight zero-haloed 10 x 18 input planes in LDS (plane stride 208
//               dwords: the four channels of a k-step fall on alternate halves of the 32 banks); every (k-step, tap, row)
//               offset is an immediate.  Cells outside the map are ZEROS WRITTEN TO LDS (virtual padding, masked loads);
//               the next chunk's cells are fetched into registers while the current one is multiplied (two buffers).
//   epilogue  = + bias, ReLU (NaN kept) -> LDS t[128][144] laid over the stage buffers; then the two 1x1 heads as one more
//               MFMA pass with M = 5A padded to 16-row tiles (rows [0, A) objectness, [A, 5A) regression, zero rows
//               behind), accumulated over the mid-channel blocks in registers: wave w takes tile rows 2w, 2w + 1.
//   stores    = masked by the map's edge and by row < 5A, fp32 NCHW — what smot_rpn_proposals_fwd reads in place.
//
// A column of either product depends on that column of its B operand alone: a non-finite input cell reaches exactly the
// outputs whose 3x3 window covers it.  An output's sum order is fixed by (C, A) — it does not depend on the image's
// index, the number of images or the other levels of the call.
// LDS: 128 x 144 x 4 = 73,728 B -> two workgroups per CU; launch bound 256 VGPRs.
//
// HALF COMPUTE MODE (the smot_rpn_head_half_* entry points; CT = SMOT_FEAT_F16 or SMOT_FEAT_BF16): rpn_head_half_kernel<CT, FT>
// is the kernel above with the 3x3 stage on v_mfma_f32_16x16x32_f16 / _bf16 (conv3x3_mfma.h's cvh_block<CT, FT, 1, 1, 2>:
// chunks of 32 input channels, x rounded to CT as it is staged, Wc rounded once by the pack kernel, exact products, fp32
// accumulation; its two 12,288 B stage buffers lie under t as the fp32 buffers do).  t = relu(conv + bc) stays fp32 in LDS
// and the two 1x1 heads run on it as above, on the fp32 matrix instruction with unrounded weights: the mode is the 3x3's,
// and the result is "rounded operands, fp32 sum order" with no second, data-dependent rounding.  Same workgroups, barriers,
// LDS and launch bound.
#include "conv3x3_mfma.h"

namespace smot {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RH_TH = 8, RH_TW = 16;                 // output tile
constexpr int RH_PW = RH_TW + 2, RH_PH = RH_TH + 2;    // haloed input tile
constexpr int RH_CELLS = RH_PW * RH_PH;              // 180
constexpr int RH_PLANE = 208;                        // plane stride in LDS: = 16 (mod 32)
constexpr int RH_IC = 8;                             // input channels per chunk
constexpr int RH_BUF = RH_IC * RH_PLANE;             // floats per stage buffer
constexpr int RH_NLD = (RH_IC * RH_CELLS + 255) / 256;
constexpr int RH_MID = 128;                          // mid channels per block
constexpr int RH_TS = 144;                           // row stride of t in LDS: = 16 (mod 32)
constexpr int RH_SMEM_FLOATS = RH_MID * RH_TS;
constexpr int RH_MAX_HEAD_TILES = 4;
static_assert(2 * RH_BUF <= RH_SMEM_FLOATS, "t lies over the two stage buffers");
static_assert(RH_CELLS <= RH_PLANE && RH_TH * RH_TW <= RH_TS, "strides hold a plane / a row of t");

struct RpnHeadLevel {
    const void* in;      // [N, C, H, W] of the call's element type
    float* obj;          // [N, A, H, W]
    float* reg;          // [N, 4A, H, W]
    int H, W;
    int tiles_x;
    int tile0;           // tiles of the levels before this one (per image)
};
struct RpnHeadArgs {
    RpnHeadLevel lv[SMOT_MAX_LEVELS];
    const float* packed;
    int L, C, A, tiles_per_image;
};

__host__ __device__ inline int rh_head_rows(int A) { return (5 * A + 15) & ~15; }
__host__ __device__ inline long long rh_off_bias(int C) { return 9LL * C * C; }
__host__ __device__ inline long long rh_off_head(int C) { return 9LL * C * C + C; }
__host__ __device__ inline long long rh_off_head_bias(int C, int A) { return rh_off_head(C) + (long long)rh_head_rows(A) * C; }
__host__ __device__ inline long long rh_packed_floats(int C, int A) { return rh_off_head_bias(C, A) + rh_head_rows(A); }

// packed[0, 9 C^2): conv filters as the kernel's A operand — [pair of M-tiles p][chunk c][q 0..8][lane][e 0..3]: value
//   j = 4q + e of the lane's 36: M-tile m = j / 18, k-step ks = (j % 18) / 9, tap = j % 9 -> Wc[32p + 16m + lane % 16][8c + 4ks
//   + lane / 16][tap]
// then the C conv biases, then the heads' A operand [row tile][k-step][lane] -> W[16 tile + lane % 16][4 ks + lane / 16]
// (rows [0, A): cls_logits, [A, 5A): bbox_pred, zero behind), then the padded rows' biases.
__global__ void __launch_bounds__(256)
rpn_head_pack_kernel(const float* __restrict__ conv_w, const float* __restrict__ conv_b, const float* __restrict__ cls_w,
                     const float* __restrict__ cls_b, const float* __restrict__ bbox_w, const float* __restrict__ bbox_b,
                     int C, int A, float* __restrict__ packed, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long ob = rh_off_bias(C), oh = rh_off_head(C), ohb = rh_off_head_bias(C, A);
    float v;
    if (i < ob) {
        const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
        long long r = i >> 8;
        const int q = (int)(r % 9);
        r /= 9;
        const int nch = C / RH_IC;
        const int c = (int)(r % nch), p = (int)(r / nch);
        const int j = 4 * q + e, m = j / 18, ks = (j % 18) / 9, tap = j % 9;
        const int oc = 32 * p + 16 * m + (lane & 15), ic = RH_IC * c + 4 * ks + (lane >> 4);
        v = conv_w[((size_t)oc * C + ic) * 9 + tap];
    } else if (i < oh) {
        v = conv_b[i - ob];
    } else if (i < ohb) {
        const long long r = i - oh;
        const int lane = (int)(r & 63);
        const int ks = (int)((r >> 6) % (C / 4)), mh = (int)((r >> 6) / (C / 4));
        const int row = 16 * mh + (lane & 15), k = 4 * ks + (lane >> 4);
        v = row < A ? cls_w[(size_t)row * C + k] : (row < 5 * A ? bbox_w[(size_t)(row - A) * C + k] : 0.0f);
    } else {
        const int row = (int)(i - ohb);
        v = row < A ? cls_b[row] : (row < 5 * A ? bbox_b[row - A] : 0.0f);
    }
    packed[i] = v;
}

template <typename FT>
__global__ void __launch_bounds__(256, 2)
rpn_head_kernel(RpnHeadArgs P) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int C = P.C, A = P.A;

    // flat workgroup index -> (image, level, tile)
    const int n = blockIdx.x / P.tiles_per_image;
    const int rem = blockIdx.x - n * P.tiles_per_image;
    RpnHeadLevel lv = P.lv[0];
#pragma unroll
    for (int k = 1; k < SMOT_MAX_LEVELS; ++k)
        if (k < P.L && rem >= P.lv[k].tile0) lv = P.lv[k];
    const int t = rem - lv.tile0;
    const int ty = t / lv.tiles_x, tx = t - ty * lv.tiles_x;
    const int y0 = ty * RH_TH, x0 = tx * RH_TW;
    const int H = lv.H, W = lv.W, HW = H * W;
    const FT* __restrict__ in = reinterpret_cast<const FT*>(lv.in) + (size_t)n * C * HW;

    // staged element e = tid + 256 j of a chunk -> (offset in the chunk's eight planes or -1: a zero, LDS offset or -1: none)
    int ld_src[RH_NLD], ld_dst[RH_NLD];
#pragma unroll
    for (int j = 0; j < RH_NLD; ++j) {
        const int e = tid + 256 * j;
        const int ic = e / RH_CELLS, cell = e - ic * RH_CELLS;
        const int r = cell / RH_PW, col = cell - r * RH_PW;
        const int gy = y0 - 1 + r, gx = x0 - 1 + col;
        const bool live = e < RH_IC * RH_CELLS;
        ld_dst[j] = live ? ic * RH_PLANE + r * RH_PW + col : -1;
        ld_src[j] = (live && gy >= 0 && gy < H && gx >= 0 && gx < W) ? ic * HW + gy * W + gx : -1;
    }
    float pre[RH_NLD];
    auto fetch = [&](int chunk) {
        const FT* __restrict__ base = in + (size_t)chunk * RH_IC * HW;
#pragma unroll
        for (int j = 0; j < RH_NLD; ++j) pre[j] = ld_src[j] >= 0 ? feat_ld<FT>(base + ld_src[j]) : 0.0f;
    };
    auto stash = [&](float* buf) {
#pragma unroll
        for (int j = 0; j < RH_NLD; ++j)
            if (ld_dst[j] >= 0) buf[ld_dst[j]] = pre[j];
    };

    const int nch = C / RH_IC, npairs = C >> 5, nmb = (npairs + 3) >> 2;
    const int mht = rh_head_rows(A) >> 4;
    const float* __restrict__ cbias = P.packed + rh_off_bias(C);
    const float* __restrict__ hw = P.packed + rh_off_head(C);
    const float* __restrict__ hbias = P.packed + rh_off_head_bias(C, A);
    const int boff = kq * RH_PLANE + xl;                   // B operand of lane (kq, xl): channel kq of the k-step, column xl

    f32x4 hacc[RH_MAX_HEAD_TILES][2];
#pragma unroll
    for (int mh = 0; mh < RH_MAX_HEAD_TILES; ++mh)
        hacc[mh][0] = hacc[mh][1] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int mb = 0; mb < nmb; ++mb) {
        const int pair = mb * 4 + wave;
        const bool active = pair < npairs;                 // wave-uniform: C % 128 != 0 leaves waves of the last block idle
        const f32x4* __restrict__ ap = reinterpret_cast<const f32x4*>(P.packed) + (size_t)(active ? pair : 0) * nch * 9 * 64 + lane;
        f32x4 acc[2][RH_TH];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nt = 0; nt < RH_TH; ++nt) acc[m][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 an[9], ac[9];
        fetch(0);
#pragma unroll
        for (int q = 0; q < 9; ++q) an[q] = ap[q * 64];
        stash(sm);                                         // (every wave is past its last read of t: the barrier below the heads)
        __syncthreads();
        for (int c = 0; c < nch; ++c) {
            const float* buf = sm + (c & 1) * RH_BUF;
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
                        for (int nt = 0; nt < RH_TH; ++nt) {
                            const float b = buf[boff + ks * 4 * RH_PLANE + (nt + tap / 3) * RH_PW + (tap % 3)];
                            acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][nt], 0, 0, 0);
                            acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][nt], 0, 0, 0);
                        }
                    }
            }
            if (c + 1 < nch) stash(sm + ((c + 1) & 1) * RH_BUF);     // the other buffer: its readers passed a barrier
            __syncthreads();
        }
        // ---- + bias, ReLU -> t[mid channel of the block][position] over the stage buffers ---------------------------
        if (active) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int chl = (wave * 2 + m) * 16 + 4 * kq + r;
                    const float bv = cbias[mb * RH_MID + chl];
#pragma unroll
                    for (int nt = 0; nt < RH_TH; ++nt) sm[chl * RH_TS + nt * RH_TW + xl] = relu_nan(acc[m][nt][r] + bv);
                }
        }
        __syncthreads();
        // ---- the two 1x1 heads over this block's mid channels -------------------------------------------------------
        const int ksteps = min(RH_MID, C - mb * RH_MID) >> 2;
        const float* tb = sm + kq * RH_TS + (2 * wave) * RH_TW + xl;
        const float* hwp = hw + (size_t)(mb * (RH_MID / 4)) * 64 + lane;
        for (int ks = 0; ks < ksteps; ++ks) {
            const float b0 = tb[ks * 4 * RH_TS], b1 = tb[ks * 4 * RH_TS + RH_TW];
#pragma unroll
            for (int mh = 0; mh < RH_MAX_HEAD_TILES; ++mh)
                if (mh < mht) {
                    const float a = hwp[((size_t)mh * (C >> 2) + ks) * 64];
                    hacc[mh][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, hacc[mh][0], 0, 0, 0);
                    hacc[mh][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, hacc[mh][1], 0, 0, 0);
                }
        }
        __syncthreads();                                   // t is read: the next block stages over it
    }

    // ---- + bias, masked stores: hacc[mh][j][r] = row 16 mh + 4 kq + r at tile row 2 wave + j, column xl --------------
    const int x = x0 + xl;
#pragma unroll
    for (int mh = 0; mh < RH_MAX_HEAD_TILES; ++mh)
        if (mh < mht) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int y = y0 + 2 * wave + j;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * mh + 4 * kq + r;
                    if (y < H && x < W && row < 5 * A) {
                        const float v = hacc[mh][j][r] + hbias[row];
                        float* dst = row < A ? lv.obj + ((size_t)n * A + row) * HW : lv.reg + ((size_t)n * 4 * A + (row - A)) * HW;
                        dst[y * W + x] = v;
                    }
                }
            }
        }
}

// ---- half compute mode ----------------------------------------------------------------------------------------------------------
// the half packed image: [cvh_pack_index image of conv.weight rounded to CT: 9 C^2 / 2 dwords][C conv biases][the heads' A
// operand][the padded rows' biases]: everything behind the filters is fp32 and laid out as rpn_head_pack_kernel writes it
__host__ __device__ inline long long rhh_off_bias(int C) { return cvh_packed_floats(C, C); }
__host__ __device__ inline long long rhh_off_head(int C) { return rhh_off_bias(C) + C; }
__host__ __device__ inline long long rhh_off_head_bias(int C, int A) { return rhh_off_head(C) + (long long)rh_head_rows(A) * C; }
__host__ __device__ inline long long rhh_packed_floats(int C, int A) { return rhh_off_head_bias(C, A) + rh_head_rows(A); }

template <int CT>
__global__ void __launch_bounds__(256)
rpn_head_half_pack_kernel(const float* __restrict__ conv_w, const float* __restrict__ conv_b, const float* __restrict__ cls_w,
                          const float* __restrict__ cls_b, const float* __restrict__ bbox_w, const float* __restrict__ bbox_b,
                          int C, int A, float* __restrict__ packed, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long ob = rhh_off_bias(C), oh = rhh_off_head(C), ohb = rhh_off_head_bias(C, A);
    float v;
    if (i < ob) {
        const long long s = cvh_pack_index(i, C, C);           // (C % 32 == 0: no padded pair, s >= 0)
        v = __uint_as_float(cvh_pack2<CT>(conv_w[s], conv_w[s + 9]));
    } else if (i < oh) {
        v = conv_b[i - ob];
    } else if (i < ohb) {
        const long long r = i - oh;
        const int lane = (int)(r & 63);
        const int ks = (int)((r >> 6) % (C / 4)), mh = (int)((r >> 6) / (C / 4));
        const int row = 16 * mh + (lane & 15), k = 4 * ks + (lane >> 4);
        v = row < A ? cls_w[(size_t)row * C + k] : (row < 5 * A ? bbox_w[(size_t)(row - A) * C + k] : 0.0f);
    } else {
        const int row = (int)(i - ohb);
        v = row < A ? cls_b[row] : (row < 5 * A ? bbox_b[row - A] : 0.0f);
    }
    packed[i] = v;
}

static_assert(CvhGeom<1>::SMEM_SLOTS * 16 <= RH_SMEM_FLOATS * 4, "t lies over the two half stage buffers");

template <int CT, typename FT>
__global__ void __launch_bounds__(256, 2)
rpn_head_half_kernel(RpnHeadArgs P) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int C = P.C, A = P.A;

    // flat workgroup index -> (image, level, tile)
    const int n = blockIdx.x / P.tiles_per_image;
    const int rem = blockIdx.x - n * P.tiles_per_image;
    RpnHeadLevel lv = P.lv[0];
#pragma unroll
    for (int k = 1; k < SMOT_MAX_LEVELS; ++k)
        if (k < P.L && rem >= P.lv[k].tile0) lv = P.lv[k];
    const int t = rem - lv.tile0;
    const int ty = t / lv.tiles_x, tx = t - ty * lv.tiles_x;
    const int y0 = ty * RH_TH, x0 = tx * RH_TW;
    const int H = lv.H, W = lv.W, HW = H * W;
    const FT* __restrict__ in = reinterpret_cast<const FT*>(lv.in) + (size_t)n * C * HW;

    CvsPlan<1> pl;
    cvs_plan<1>(pl, tid, y0, x0, H, W);
    cvs_u32x4* stage = reinterpret_cast<cvs_u32x4*>(sm);   // the two stage buffers, under t

    const int npairs = C >> 5, nmb = (npairs + 3) >> 2;
    const int mht = rh_head_rows(A) >> 4;
    const float* __restrict__ cbias = P.packed + rhh_off_bias(C);
    const float* __restrict__ hw = P.packed + rhh_off_head(C);
    const float* __restrict__ hbias = P.packed + rhh_off_head_bias(C, A);

    f32x4 hacc[RH_MAX_HEAD_TILES][2];
#pragma unroll
    for (int mh = 0; mh < RH_MAX_HEAD_TILES; ++mh)
        hacc[mh][0] = hacc[mh][1] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int mb = 0; mb < nmb; ++mb) {
        const int pair = mb * 4 + wave;
        const bool active = pair < npairs;                 // wave-uniform: C % 128 != 0 leaves waves of the last block idle
        cv_f32x4 acc[2][RH_TH];
        // (cvh_block stores its first chunk BEFORE its first barrier: every wave is past its last read of t — the barrier
        // below the heads — and it ends behind a barrier: no wave reads a stage buffer when t is written over them)
        cvh_block<CT, FT, 1, 1, 2>(stage, in, HW, C, pl, P.packed, pair, active, tid, 0, acc);
        // ---- + bias, ReLU -> t[mid channel of the block][position] over the stage buffers ---------------------------
        if (active) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int chl = (wave * 2 + m) * 16 + 4 * kq + r;
                    const float bv = cbias[mb * RH_MID + chl];
#pragma unroll
                    for (int nt = 0; nt < RH_TH; ++nt) sm[chl * RH_TS + nt * RH_TW + xl] = relu_nan(acc[m][nt][r] + bv);
                }
        }
        __syncthreads();
        // ---- the two 1x1 heads over this block's mid channels: fp32, as rpn_head_kernel's -----------------------------
        const int ksteps = min(RH_MID, C - mb * RH_MID) >> 2;
        const float* tb = sm + kq * RH_TS + (2 * wave) * RH_TW + xl;
        const float* hwp = hw + (size_t)(mb * (RH_MID / 4)) * 64 + lane;
        for (int ks = 0; ks < ksteps; ++ks) {
            const float b0 = tb[ks * 4 * RH_TS], b1 = tb[ks * 4 * RH_TS + RH_TW];
#pragma unroll
            for (int mh = 0; mh < RH_MAX_HEAD_TILES; ++mh)
                if (mh < mht) {
                    const float a = hwp[((size_t)mh * (C >> 2) + ks) * 64];
                    hacc[mh][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, hacc[mh][0], 0, 0, 0);
                    hacc[mh][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, hacc[mh][1], 0, 0, 0);
                }
        }
        __syncthreads();                                   // t is read: the next block stages over it
    }

    // ---- + bias, masked stores: hacc[mh][j][r] = row 16 mh + 4 kq + r at tile row 2 wave + j, column xl --------------
    const int x = x0 + xl;
#pragma unroll
    for (int mh = 0; mh < RH_MAX_HEAD_TILES; ++mh)
        if (mh < mht) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int y = y0 + 2 * wave + j;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * mh + 4 * kq + r;
                    if (y < H && x < W && row < 5 * A) {
                        const float v = hacc[mh][j][r] + hbias[row];
                        float* dst = row < A ? lv.obj + ((size_t)n * A + row) * HW : lv.reg + ((size_t)n * 4 * A + (row - A)) * HW;
                        dst[y * W + x] = v;
                    }
                }
            }
        }
}

// ---- anchors: out_l[(h W + w) A + a] = cell_l[a] + (w s, h s, w s, h s), all levels in one launch ---------------------
struct AnchorLevel {
    const float* cell;   // [A, 4]
    float* out;          // [H W A, 4]
    int A, W, stride;
    int row0;            // rows of the levels before this one
};
struct AnchorArgs {
    AnchorLevel lv[SMOT_MAX_LEVELS];
    int L, rows;
};

__global__ void __launch_bounds__(256)
rpn_anchors_kernel(AnchorArgs P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.rows) return;
    AnchorLevel lv = P.lv[0];
#pragma unroll
    for (int k = 1; k < SMOT_MAX_LEVELS; ++k)
        if (k < P.L && i >= P.lv[k].row0) lv = P.lv[k];
    const int k = i - lv.row0;
    const int cellidx = k / lv.A, a = k - cellidx * lv.A;
    const int h = cellidx / lv.W, w = cellidx - h * lv.W;
    const float sx = (float)(w * lv.stride), sy = (float)(h * lv.stride);
    const f32x4 c = *reinterpret_cast<const f32x4*>(lv.cell + 4 * a);
    *reinterpret_cast<f32x4*>(lv.out + 4 * (size_t)k) = (f32x4){add_rn(c[0], sx), add_rn(c[1], sy), add_rn(c[2], sx), add_rn(c[3], sy)};
}

static int rpn_head_shape(int C, int A, const char* who) {
    if (C < 32 || C % 32 != 0 || C > 512) {
        set_error("%s: C = %d (supported: multiples of 32 up to 512)", who, C);
        return SMOT_ERR_UNSUPPORTED;
    }
    if (A < 1 || 5 * A > 16 * RH_MAX_HEAD_TILES) {
        set_error("%s: A = %d anchors per cell (supported: 1 <= A, 5 A <= %d)", who, A, 16 * RH_MAX_HEAD_TILES);
        return SMOT_ERR_UNSUPPORTED;
    }
    return SMOT_OK;
}

template <typename FT>
static int rpn_head_launch(const RpnHeadArgs& P, int grid, hipStream_t st) {
    const size_t smem = (size_t)RH_SMEM_FLOATS * sizeof(float);
    const int rco = ensure_lds_optin(reinterpret_cast<const void*>(&rpn_head_kernel<FT>), smem, "rpn_head");
    if (rco) return rco;
    SMOT_LAUNCH(rpn_head_kernel<FT>, dim3(grid), dim3(256), smem, st, P);
    return check_launch("rpn_head");
}

template <int CT, typename FT>
static int rpn_head_half_launch(const RpnHeadArgs& P, int grid, hipStream_t st) {
    const size_t smem = (size_t)RH_SMEM_FLOATS * sizeof(float);
    const int rco = ensure_lds_optin(reinterpret_cast<const void*>(&rpn_head_half_kernel<CT, FT>), smem, "rpn_head_half");
    if (rco) return rco;
    SMOT_LAUNCH((rpn_head_half_kernel<CT, FT>), dim3(grid), dim3(256), smem, st, P);
    return check_launch("rpn_head_half");
}

template <int CT>
static int rpn_head_half_pick(const RpnHeadArgs& P, int grid, int feat_type, hipStream_t st) {
    if (feat_type == SMOT_FEAT_F32) return rpn_head_half_launch<CT, float>(P, grid, st);
    if (feat_type == SMOT_FEAT_F16) return rpn_head_half_launch<CT, f16_t>(P, grid, st);
    return rpn_head_half_launch<CT, bf16_t>(P, grid, st);
}

static bool rpn_head_ctype_ok(int ctype) { return ctype == SMOT_FEAT_F16 || ctype == SMOT_FEAT_BF16; }

}  // namespace smot

using namespace smot;

extern "C" long long smot_rpn_head_packed_floats(int C, int A) {
    if (rpn_head_shape(C, A, "rpn_head_packed_floats")) return -1;
    return rh_packed_floats(C, A);
}

extern "C" int smot_rpn_head_pack(const float* conv_w, const float* conv_b, const float* cls_w, const float* cls_b,
                                  const float* bbox_w, const float* bbox_b, int C, int A, float* packed,
                                  smot_stream_t stream) {
    const int rs = rpn_head_shape(C, A, "rpn_head_pack");
    if (rs) return rs;
    SMOT_REQUIRE(conv_w && conv_b && cls_w && cls_b && bbox_w && bbox_b && packed, "rpn_head_pack: null pointer");
    SMOT_REQUIRE(((uintptr_t)packed & 15) == 0, "rpn_head_pack: packed must be 16-byte aligned");
    const long long total = rh_packed_floats(C, A);
    hipLaunchKernelGGL(rpn_head_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, conv_w,
                       conv_b, cls_w, cls_b, bbox_w, bbox_b, C, A, packed, total);
    return check_launch("rpn_head_pack");
}

// smot_rpn_head_fwd (ctype 0) and smot_rpn_head_half_fwd (ctype SMOT_FEAT_F16 / _BF16): the same checks, geometry and launch;
// the mode selects the packed image's layout and the kernel
static int rpn_head_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths, int num_levels,
                        int num_images, int C, int A, const float* packed, float* const* objectness_out,
                        float* const* regression_out, smot_stream_t stream, int ctype, const char* who) {
    const int rf = check_feat_type(feat_type, who);
    if (rf) return rf;
    if (feat_type & SMOT_FEAT_CHANNELS_LAST) {
        set_error("%s: channels-last maps are not read in place (pass contiguous NCHW maps)", who);
        return SMOT_ERR_UNSUPPORTED;
    }
    SMOT_REQUIRE(num_levels >= 1 && num_levels <= SMOT_MAX_LEVELS, "%s: num_levels = %d (1 .. %d)", who, num_levels,
                 SMOT_MAX_LEVELS);
    SMOT_REQUIRE(num_images >= 1 && num_images <= SMOT_MAX_IMAGES, "%s: num_images = %d (1 .. %d)", who, num_images,
                 SMOT_MAX_IMAGES);
    const int rs = rpn_head_shape(C, A, who);
    if (rs) return rs;
    SMOT_REQUIRE(feats && heights && widths && packed && objectness_out && regression_out, "%s: null pointer", who);
    SMOT_REQUIRE(((uintptr_t)packed & 15) == 0, "%s: packed must be 16-byte aligned", who);
    RpnHeadArgs P = {};
    long long tiles = 0;
    for (int l = 0; l < num_levels; ++l) {
        SMOT_REQUIRE(feats[l] && objectness_out[l] && regression_out[l], "%s: null tensor at level %d", who, l);
        SMOT_REQUIRE(heights[l] >= 1 && widths[l] >= 1, "%s: level %d is %d x %d", who, l, heights[l], widths[l]);
        if ((long long)heights[l] * widths[l] * (ctype ? CVS_IC : RH_IC) >= (1LL << 31)) {
            set_error("%s: level %d (%d x %d) is beyond the kernel's 32-bit plane offsets", who, l, heights[l], widths[l]);
            return SMOT_ERR_UNSUPPORTED;
        }
        RpnHeadLevel& v = P.lv[l];
        v.in = feats[l];
        v.obj = objectness_out[l];
        v.reg = regression_out[l];
        v.H = heights[l];
        v.W = widths[l];
        v.tiles_x = (v.W + RH_TW - 1) / RH_TW;
        v.tile0 = (int)tiles;
        tiles += (long long)v.tiles_x * ((v.H + RH_TH - 1) / RH_TH);
        if (tiles * num_images >= (1LL << 31)) {
            set_error("%s: %d images of these maps are more than 2^31 tiles", who, num_images);
            return SMOT_ERR_UNSUPPORTED;
        }
    }
    P.packed = packed;
    P.L = num_levels;
    P.C = C;
    P.A = A;
    P.tiles_per_image = (int)tiles;
    const int grid = (int)(tiles * num_images);
    hipStream_t st = (hipStream_t)stream;
    if (ctype == SMOT_FEAT_F16) return rpn_head_half_pick<SMOT_FEAT_F16>(P, grid, feat_type, st);
    if (ctype == SMOT_FEAT_BF16) return rpn_head_half_pick<SMOT_FEAT_BF16>(P, grid, feat_type, st);
    if (feat_type == SMOT_FEAT_F32) return rpn_head_launch<float>(P, grid, st);
    if (feat_type == SMOT_FEAT_F16) return rpn_head_launch<f16_t>(P, grid, st);
    return rpn_head_launch<bf16_t>(P, grid, st);
}

extern "C" int smot_rpn_head_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                 int num_levels, int num_images, int C, int A, const float* packed,
                                 float* const* objectness_out, float* const* regression_out, smot_stream_t stream) {
    return rpn_head_fwd(feats, feat_type, heights, widths, num_levels, num_images, C, A, packed, objectness_out, regression_out,
                        stream, 0, "rpn_head");
}

// ---- half compute mode (include/smot_emm.h, RPN HEAD, HALF COMPUTE) ---------------------------------------------------------------
extern "C" long long smot_rpn_head_half_packed_floats(int C, int A, int compute_type) {
    if (!rpn_head_ctype_ok(compute_type)) {
        set_error("rpn_head_half_packed_floats: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
        return -1;
    }
    if (rpn_head_shape(C, A, "rpn_head_half_packed_floats")) return -1;
    return rhh_packed_floats(C, A);
}

extern "C" int smot_rpn_head_half_pack(const float* conv_w, const float* conv_b, const float* cls_w, const float* cls_b,
                                       const float* bbox_w, const float* bbox_b, int C, int A, int compute_type, float* packed,
                                       smot_stream_t stream) {
    SMOT_REQUIRE(rpn_head_ctype_ok(compute_type), "rpn_head_half_pack: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)",
                 compute_type);
    const int rs = rpn_head_shape(C, A, "rpn_head_half_pack");
    if (rs) return rs;
    SMOT_REQUIRE(conv_w && conv_b && cls_w && cls_b && bbox_w && bbox_b && packed, "rpn_head_half_pack: null pointer");
    SMOT_REQUIRE(((uintptr_t)packed & 15) == 0, "rpn_head_half_pack: packed must be 16-byte aligned");
    const long long total = rhh_packed_floats(C, A);
    const dim3 g((unsigned)((total + 255) / 256));
    if (compute_type == SMOT_FEAT_F16)
        hipLaunchKernelGGL(rpn_head_half_pack_kernel<SMOT_FEAT_F16>, g, dim3(256), 0, (hipStream_t)stream, conv_w, conv_b, cls_w,
                           cls_b, bbox_w, bbox_b, C, A, packed, total);
    else
        hipLaunchKernelGGL(rpn_head_half_pack_kernel<SMOT_FEAT_BF16>, g, dim3(256), 0, (hipStream_t)stream, conv_w, conv_b, cls_w,
                           cls_b, bbox_w, bbox_b, C, A, packed, total);
    return check_launch("rpn_head_half_pack");
}

extern "C" int smot_rpn_head_half_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                      int num_levels, int num_images, int C, int A, int compute_type, const float* packed,
                                      float* const* objectness_out, float* const* regression_out, smot_stream_t stream) {
    SMOT_REQUIRE(rpn_head_ctype_ok(compute_type), "rpn_head_half: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)",
                 compute_type);
    return rpn_head_fwd(feats, feat_type, heights, widths, num_levels, num_images, C, A, packed, objectness_out, regression_out,
                        stream, compute_type, "rpn_head_half");
}

extern "C" int smot_rpn_anchors_fwd(const float* const* cell_anchors, const int* num_anchors, const int* strides,
                                    const int* heights, const int* widths, int num_levels, float* const* out,
                                    smot_stream_t stream) {
    SMOT_REQUIRE(num_levels >= 1 && num_levels <= SMOT_MAX_LEVELS, "rpn_anchors: num_levels = %d (1 .. %d)", num_levels,
                 SMOT_MAX_LEVELS);
    SMOT_REQUIRE(cell_anchors && num_anchors && strides && heights && widths && out, "rpn_anchors: null pointer");
    AnchorArgs P = {};
    long long rows = 0;
    for (int l = 0; l < num_levels; ++l) {
        SMOT_REQUIRE(cell_anchors[l] && out[l], "rpn_anchors: null tensor at level %d", l);
        SMOT_REQUIRE(num_anchors[l] >= 1 && strides[l] >= 1 && heights[l] >= 1 && widths[l] >= 1,
                     "rpn_anchors: level %d has %d anchors, stride %d, %d x %d cells", l, num_anchors[l], strides[l], heights[l],
                     widths[l]);
        SMOT_REQUIRE((((uintptr_t)cell_anchors[l] | (uintptr_t)out[l]) & 15) == 0, "rpn_anchors: level %d is not 16-byte aligned", l);
        // shifts are exact in fp32 (and the row index fits an int)
        if ((long long)heights[l] * strides[l] > (1 << 24) || (long long)widths[l] * strides[l] > (1 << 24)) {
            set_error("rpn_anchors: level %d spans more than 2^24 pixels", l);
            return SMOT_ERR_UNSUPPORTED;
        }
        AnchorLevel& v = P.lv[l];
        v.cell = cell_anchors[l];
        v.out = out[l];
        v.A = num_anchors[l];
        v.W = widths[l];
        v.stride = strides[l];
        v.row0 = (int)rows;
        rows += (long long)heights[l] * widths[l] * num_anchors[l];
        if (rows >= (1LL << 31) - 256) {
            set_error("rpn_anchors: more than 2^31 anchors in one call");
            return SMOT_ERR_UNSUPPORTED;
        }
    }
    P.L = num_levels;
    P.rows = (int)rows;
    hipLaunchKernelGGL(rpn_anchors_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P);
    return check_launch("rpn_anchors");
}
