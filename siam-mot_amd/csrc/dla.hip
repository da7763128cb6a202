// DLA backbone body — [UPSTREAM] siammot/modelling/backbone/dla.py with DlaBasic blocks (DLA-34 and its family) or
// DlaBottleneck blocks at cardinality 1 (DLA-46-C, DLA-60, DLA-102, DLA-169) and maskrcnn_benchmark's FrozenBatchNorm2d,
// inference: an image batch -> the four stage maps x2 .. x5.
//
//   x  = cbr7x7(image, 3 -> c0)              base_layer          cbr = conv (no bias) -> y * scale + shift -> ReLU
//   x0 = cbr3x3(x, c0 -> c0)                 level0              cb  = the same without the ReLU
//   x1 = cbr3x3(x0, c0 -> c1, stride 2)      level1
//   xk = tree_k(x_{k-1}), stride 2           level2 .. level5    (include/smot_emm.h, DLA BACKBONE, states the trees)
//
// Every convolution runs on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation); the weights are packed once
// into the A operand's lane order with the frozen BN's scale and shift behind them; the epilogue is acc * scale + shift
// (two roundings, as torch's x * scale + shift), + residual, ReLU (v < 0 ? 0 : v: a NaN stays), store.
//
// dla_conv3x3_kernel<FT, STRIDE, WR, NM>: conv3x3_mfma.h's generalised stage (cvg_block): workgroup = (image, 8 x 16 output
//   tile, block of 32 * 4 / WR output channels), chunks of 8 input channels through two LDS buffers.  The four waves are
//   4 / WR channel pairs x WR row groups: Cout <= 32 -> WR = 4 (all waves share the pair and split the rows); wider layers
//   take the widest block that still gives every CU a workgroup (dl_conv3_pick): the coarse levels have few tiles.
//   LDS 13,312 B (stride 1) / 35,904 B (stride 2: 17 x 33 cells per plane, plane stride 561, odd).
// dla_conv3x3_split_kernel<FT, STRIDE, WR, NM>: the same workgroup for the trees' 3x3 convolutions in SPLIT MODE (the
//   smot_dla_split_* entry points): three-part bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulation, chunks of 32
//   input channels (conv3x3_mfma.h, cvs_block); fp32-grade results in another summation order.  The other kernels are shared.
// dla_conv1x1_kernel<OT>: fpn_lateral_kernel's scheme (64 positions x 32 output channels per workgroup, B operand read in
//   place) over a VIRTUAL concatenation of up to four source maps, each read as it is or through a 2 x 2 max-pool of a map
//   twice as fine (torch's max_pool2d: a NaN in the window is the result).  Serves every root and every project.  No LDS.
// dla_conv1x1_res_kernel<OT>: the same over up to eight sources with a plain or 2 x 2 max-pooled residual in the epilogue: the
//   last third of a DlaBottleneck block, the residual roots and the roots of trees more than two levels deep (the
//   smot_dla_net_* entry points: DLA-46-C, DLA-60, DLA-102, DLA-169; dn_tree walks trees of any depth).
// dla_conv7x7_kernel<FT>: base_layer.  K = 3 * 49 = 147 padded to 148 (37 k-steps; the pad reads a zero cell of LDS, so a
//   non-finite image cell meets no 0 * inf); the 14 x 22 x 3 window of an 8 x 16 tile is staged once; wave w owns rows 2w, 2w + 1.
//
// The stem (base_layer, level0, level1) is three launches here (7x7, 3x3 WR = 4 NM = 1 | 2, 3x3 stride 2 WR = 4): the
// c0-channel full-resolution maps go through the workspace.  DESIGN.md §7 states what that costs.
//
// HALF COMPUTE MODE (the smot_dla_half_* entry points): every tree convolution with one fp16 / bf16 operand per value on
//   v_mfma_f32_16x16x32_f16 / _bf16, fp32 accumulation and the fp32 epilogue; the stem stays on the kernels above.
// dla_conv3x3_half_kernel<CT, FT, STRIDE, WR, NM>: dla_conv3x3_split_kernel's workgroup and forms over conv3x3_mfma.h's
//   cvh_block (one part; two LDS buffers and two workgroups per CU at both strides: 24,576 B / 71,808 B).
// dla_conv1x1_half_kernel<CT, OT, MT>: what dla_conv1x1_res_kernel covers (eight sources, plain or pooled, residual, ReLU,
//   OT + fp32 copy), 64 positions x 16 MT output channels per workgroup, K steps of 32 channels, the B operand read in
//   place (eight channels of one position per lane) and rounded in registers.  No LDS.
//
// An output's sum order is fixed by the channel counts and the position in its tile: it does not depend on the image's index
// or the number of images.
#include "conv3x3_mfma.h"

namespace smot {

constexpr int DL_POS = 64, DL_MT = 2;                // 1x1: positions and M-tiles per workgroup
constexpr int DL_MAX_SRC = 4;
constexpr int DL_MAX_CONVS = 512;              // (four depth-5 bottleneck trees and the stem: 455)
constexpr int S7_PW = CV_TW + 6, S7_PH = CV_TH + 6, S7_PLANE = S7_PW * S7_PH;   // 22 x 14 = 308
constexpr int S7_ZERO = 3 * S7_PLANE;                // a run of zeros behind the planes: the K pad's B operand
constexpr int S7_SMEM = S7_ZERO + 160;
constexpr int S7_KS = 37, S7_Q = 10;                 // k-steps; 16-byte A loads per lane and M-tile

// ---- packed image of one convolution --------------------------------------------------------------------------------
//   kind 3: cvg_pack_index image (pairs padded to 32 channels), scale [32 pairs], shift [32 pairs]
//   kind 4: a 3x3 convolution's filters split into three bf16 parts: cvs_pack_index image (dwords of two bf16 each; Cin % 32
//           == 0), scale [32 pairs], shift [32 pairs] in fp32 as for kind 3
//   kind 1: [M-tile][group of four k-steps][lane][e] -> W[16 m + lane % 16][16 g + 4 e + lane / 16], scale [Cout], shift [Cout]
//   kind 7: [M-tile][q 0..9][lane][e] -> W[16 m + lane % 16][k = 4 (4 q + e) + lane / 16] (k < 147, else 0), scale, shift
//   kind 5: a 3x3 convolution's filters rounded to fp16 / bf16: cvh_pack_index image (dwords of two halves; Cin % 32 == 0),
//           scale [32 pairs], shift [32 pairs] in fp32 as for kind 3
//   kind 6: a 1x1 convolution's filters rounded to fp16 / bf16 (Cin % 32 == 0): [M-tile][K step of 32][lane][e] dwords of two
//           halves -> W[16 m + lane % 16][32 g + 8 (lane / 16) + 2 e, + 1], scale [Cout], shift [Cout] in fp32
__host__ __device__ inline long long dl_conv_floats(int kind, int Cin, int Cout) {
    if (kind == 3) return cvg_packed_floats(Cin, Cout) + 2LL * 32 * ((Cout + 31) / 32);
    if (kind == 4) return cvs_packed_floats(Cin, Cout) + 2LL * 32 * ((Cout + 31) / 32);
    if (kind == 1) return (long long)Cout * Cin + 2LL * Cout;
    if (kind == 5) return cvh_packed_floats(Cin, Cout) + 2LL * 32 * ((Cout + 31) / 32);
    if (kind == 6) return (long long)Cout * Cin / 2 + 2LL * Cout;
    return (long long)(Cout / 16) * S7_Q * 256 + 2LL * Cout;
}

__global__ void __launch_bounds__(256)
dla_pack_kernel(int kind, const float* __restrict__ w, const float* __restrict__ scale, const float* __restrict__ shift,
                int Cin, int Cout, long long total, float* __restrict__ packed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long nw = total - (kind == 3 || kind == 4 ? 2LL * 32 * ((Cout + 31) / 32) : 2LL * Cout);
    float v = 0.0f;
    if (i < nw) {
        if (kind == 3) {
            const long long s = cvg_pack_index(i, Cin, Cout);
            v = s >= 0 ? w[s] : 0.0f;
        } else if (kind == 4) {                                  // (a dword of two bf16: stored through the float as bits)
            int part;
            const long long s = cvs_pack_index(i, Cin, Cout, &part);
            if (s >= 0) {
                unsigned lo[3], hi[3];
                cvs_split(w[s], lo);
                cvs_split(w[s + 9], hi);
                v = __uint_as_float(lo[part] | (hi[part] << 16));
            }
        } else if (kind == 1) {
            const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
            const long long t = i >> 8;
            const int ng = Cin / 16;
            const int g = (int)(t % ng), m = (int)(t / ng);
            v = w[(size_t)(16 * m + (lane & 15)) * Cin + 16 * g + 4 * e + (lane >> 4)];
        } else {
            const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
            const long long t = i >> 8;
            const int q = (int)(t % S7_Q), m = (int)(t / S7_Q);
            const int k = 4 * (4 * q + e) + (lane >> 4);
            v = k < 147 ? w[(size_t)(16 * m + (lane & 15)) * 147 + k] : 0.0f;
        }
    } else {
        const long long r = i - nw;
        const int half = (int)((total - nw) / 2);
        const int ch = (int)(r % half);
        v = ch < Cout ? (r < half ? scale[ch] : shift[ch]) : 0.0f;
    }
    packed[i] = v;
}

// kinds 5 and 6: the filters rounded to CT (round to nearest even, as torch's .to(); fp16: beyond 65,504 -> +-inf), two to a
// dword stored through the float as bits; scale and shift behind them as dla_pack_kernel writes them
template <int CT>
__global__ void __launch_bounds__(256)
dla_pack_half_kernel(int kind, const float* __restrict__ w, const float* __restrict__ scale, const float* __restrict__ shift,
                     int Cin, int Cout, long long total, float* __restrict__ packed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long nw = total - (kind == 5 ? 2LL * 32 * ((Cout + 31) / 32) : 2LL * Cout);
    float v = 0.0f;
    if (i < nw) {
        if (kind == 5) {
            const long long s = cvh_pack_index(i, Cin, Cout);
            if (s >= 0) v = __uint_as_float(cvh_pack2<CT>(w[s], w[s + 9]));
        } else {
            const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
            const long long t = i >> 8;
            const int ng = Cin / 32;
            const int g = (int)(t % ng), m = (int)(t / ng);
            const float* __restrict__ q = w + (size_t)(16 * m + (lane & 15)) * Cin + 32 * g + 8 * (lane >> 4) + 2 * e;
            v = __uint_as_float(cvh_pack2<CT>(q[0], q[1]));
        }
    } else {
        const long long r = i - nw;
        const int half = (int)((total - nw) / 2);
        const int ch = (int)(r % half);
        v = ch < Cout ? (r < half ? scale[ch] : shift[ch]) : 0.0f;
    }
    packed[i] = v;
}

// ---- 3x3 ----------------------------------------------------------------------------------------------------------------
struct DlaConv3Args {
    const void* in;          // [N, Cin, H, W]
    const float* w;          // the convolution's packed image
    const float* res;        // [N, Cout, Ho, Wo], or nullptr; res_w != 0: [N, Cout, res_h, res_w] read through a 2 x 2 max-pool
    float* out;              // [N, Cout, Ho, Wo]
    int Cin, Cout, H, W, Ho, Wo;
    int tiles_x, tiles_per_image, relu, res_h, res_w;
};

// torch's max_pool2d: `if (v > m || isnan(v)) m = v` over the window in row-major order
__device__ __forceinline__ float dl_pool_step(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float dl_pool(const float* __restrict__ q, int Ws) {
    return dl_pool_step(dl_pool_step(dl_pool_step(q[0], q[1]), q[Ws]), q[Ws + 1]);
}

// dla_conv3x3_kernel's epilogue as a function, for the split kernel below: acc[m][nt] of channel pair `pair`, tile rows
// row0 + nt at (y0, x) of image planes res / out -> acc * scale + shift (+ the plain or 2 x 2 max-pooled residual), ReLU,
// store.  (dla_conv3x3_kernel itself keeps the loop in its body, which follows: calling this function from it gives the
// same values and another register allocation, and the fp32 mode's code is to stay what it was.)
template <int NM, int ROWS>
__device__ __forceinline__ void dl_conv3_store(const cv_f32x4 (&acc)[NM][ROWS], int pair, int kq, int x, int y0, int row0, int Cout,
                                               int Ho, int Wo, int HWo, int res_w, int HWr, int relu,
                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                               const float* __restrict__ res, float* __restrict__ out) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ch = 32 * pair + 16 * m + 4 * kq + r;
            if (ch >= Cout) continue;
            const float sc = scale[ch], sh = shift[ch];
#pragma unroll
            for (int nt = 0; nt < ROWS; ++nt) {
                const int y = y0 + row0 + nt;
                if (y < Ho) {
                    const int o = ch * HWo + y * Wo + x;
                    float v = add_rn(mul_rn(acc[m][nt][r], sc), sh);
                    if (res) v = add_rn(v, res_w ? dl_pool(res + ch * HWr + 2 * y * res_w + 2 * x, res_w) : res[o]);
                    out[o] = relu ? relu_nan(v) : v;
                }
            }
        }
}

template <typename FT, int STRIDE, int WR, int NM>
__global__ void __launch_bounds__(256, 2)
dla_conv3x3_kernel(DlaConv3Args P) {
    using G = CvGeom<STRIDE>;
    constexpr int WP = 4 / WR, ROWS = CV_TH / WR;
    __shared__ __attribute__((aligned(16))) float sm[G::SMEM_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int n = blockIdx.x / P.tiles_per_image;
    const int t = blockIdx.x - n * P.tiles_per_image;
    const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
    const int y0 = ty * CV_TH, x0 = tx * CV_TW;
    const int HW = P.H * P.W, HWo = P.Ho * P.Wo, Cout = P.Cout;
    const FT* __restrict__ in = reinterpret_cast<const FT*>(P.in) + (size_t)n * P.Cin * HW;
    const int npairs = (Cout + 31) >> 5;
    const float* __restrict__ scale = P.w + cvg_packed_floats(P.Cin, Cout);
    const float* __restrict__ shift = scale + 32 * npairs;
    const int HWr = P.res_w ? P.res_h * P.res_w : HWo;
    const float* __restrict__ res = P.res ? P.res + (size_t)n * Cout * HWr : nullptr;
    float* __restrict__ out = P.out + (size_t)n * Cout * HWo;
    const int wp = WR == 1 ? wave : wave % WP, row0 = WR == 1 ? 0 : (wave / WP) * ROWS;

    CvgPlan<STRIDE> pl;
    cvg_plan<STRIDE>(pl, tid, y0, x0, P.H, P.W);
    const int x = x0 + xl;
    {
        const int pair = blockIdx.y * WP + wp;                  // grid.y: the blocks of 32 WP output channels
        const bool active = pair < npairs;
        cv_f32x4 acc[NM][ROWS];
        cvg_block<FT, STRIDE, WR, NM>(sm, in, HW, P.Cin, pl, P.w, pair, active, tid, row0, acc);
        if (active && x < P.Wo) {
#pragma unroll
            for (int m = 0; m < NM; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ch = 32 * pair + 16 * m + 4 * kq + r;
                    if (ch >= Cout) continue;
                    const float sc = scale[ch], sh = shift[ch];
#pragma unroll
                    for (int nt = 0; nt < ROWS; ++nt) {
                        const int y = y0 + row0 + nt;
                        if (y < P.Ho) {
                            const int o = ch * HWo + y * P.Wo + x;
                            float v = add_rn(mul_rn(acc[m][nt][r], sc), sh);
                            if (res) v = add_rn(v, P.res_w ? dl_pool(res + ch * HWr + 2 * y * P.res_w + 2 * x, P.res_w) : res[o]);
                            out[o] = P.relu ? relu_nan(v) : v;
                        }
                    }
                }
        }
    }
}

// dla_conv3x3_split_kernel<FT, STRIDE, WR, NM>: the same workgroup on v_mfma_f32_16x16x32_bf16 with three-part bf16 operands
//   (conv3x3_mfma.h, cvs_block): chunks of 32 input channels, P.w the kind-4 packed image, the same epilogue.  LDS 73,728 B
//   (stride 1: two workgroups per CU) / 107,712 B (stride 2: one, with 512 registers).
template <typename FT, int STRIDE, int WR, int NM>
__global__ void __launch_bounds__(256, STRIDE == 1 ? 2 : 1)
dla_conv3x3_split_kernel(DlaConv3Args P) {
    using S = CvsGeom<STRIDE>;
    constexpr int WP = 4 / WR, ROWS = CV_TH / WR;
    __shared__ __attribute__((aligned(16))) cvs_u32x4 sm[S::SMEM_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int n = blockIdx.x / P.tiles_per_image;
    const int t = blockIdx.x - n * P.tiles_per_image;
    const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
    const int y0 = ty * CV_TH, x0 = tx * CV_TW;
    const int HW = P.H * P.W, HWo = P.Ho * P.Wo, Cout = P.Cout;
    const FT* __restrict__ in = reinterpret_cast<const FT*>(P.in) + (size_t)n * P.Cin * HW;
    const int npairs = (Cout + 31) >> 5;
    const float* __restrict__ scale = P.w + cvs_packed_floats(P.Cin, Cout);
    const float* __restrict__ shift = scale + 32 * npairs;
    const int HWr = P.res_w ? P.res_h * P.res_w : HWo;
    const float* __restrict__ res = P.res ? P.res + (size_t)n * Cout * HWr : nullptr;
    float* __restrict__ out = P.out + (size_t)n * Cout * HWo;
    const int wp = WR == 1 ? wave : wave % WP, row0 = WR == 1 ? 0 : (wave / WP) * ROWS;

    CvsPlan<STRIDE> pl;
    cvs_plan<STRIDE>(pl, tid, y0, x0, P.H, P.W);
    const int x = x0 + xl;
    const int pair = blockIdx.y * WP + wp;                      // grid.y: the blocks of 32 WP output channels
    const bool active = pair < npairs;
    cv_f32x4 acc[NM][ROWS];
    cvs_block<FT, STRIDE, WR, NM>(sm, in, HW, P.Cin, pl, P.w, pair, active, tid, row0, acc);
    if (active && x < P.Wo) dl_conv3_store<NM, ROWS>(acc, pair, kq, x, y0, row0, Cout, P.Ho, P.Wo, HWo, P.res_w, HWr, P.relu, scale, shift, res, out);
}

// dla_conv3x3_half_kernel<CT, FT, STRIDE, WR, NM>: the same workgroup in HALF COMPUTE MODE (conv3x3_mfma.h, cvh_block): one
//   fp16 / bf16 operand per value, chunks of 32 input channels, P.w the kind-5 packed image, the same epilogue.  LDS 24,576 B
//   (stride 1) / 71,808 B (stride 2), two workgroups per CU at both.
template <int CT, typename FT, int STRIDE, int WR, int NM>
__global__ void __launch_bounds__(256, 2)
dla_conv3x3_half_kernel(DlaConv3Args P) {
    using Hh = CvhGeom<STRIDE>;
    constexpr int WP = 4 / WR, ROWS = CV_TH / WR;
    __shared__ __attribute__((aligned(16))) cvs_u32x4 sm[Hh::SMEM_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int n = blockIdx.x / P.tiles_per_image;
    const int t = blockIdx.x - n * P.tiles_per_image;
    const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
    const int y0 = ty * CV_TH, x0 = tx * CV_TW;
    const int HW = P.H * P.W, HWo = P.Ho * P.Wo, Cout = P.Cout;
    const FT* __restrict__ in = reinterpret_cast<const FT*>(P.in) + (size_t)n * P.Cin * HW;
    const int npairs = (Cout + 31) >> 5;
    const float* __restrict__ scale = P.w + cvh_packed_floats(P.Cin, Cout);
    const float* __restrict__ shift = scale + 32 * npairs;
    const int HWr = P.res_w ? P.res_h * P.res_w : HWo;
    const float* __restrict__ res = P.res ? P.res + (size_t)n * Cout * HWr : nullptr;
    float* __restrict__ out = P.out + (size_t)n * Cout * HWo;
    const int wp = WR == 1 ? wave : wave % WP, row0 = WR == 1 ? 0 : (wave / WP) * ROWS;

    CvsPlan<STRIDE> pl;
    cvs_plan<STRIDE>(pl, tid, y0, x0, P.H, P.W);
    const int x = x0 + xl;
    const int pair = blockIdx.y * WP + wp;                      // grid.y: the blocks of 32 WP output channels
    const bool active = pair < npairs;
    cv_f32x4 acc[NM][ROWS];
    cvh_block<CT, FT, STRIDE, WR, NM>(sm, in, HW, P.Cin, pl, P.w, pair, active, tid, row0, acc);
    if (active && x < P.Wo) dl_conv3_store<NM, ROWS>(acc, pair, kq, x, y0, row0, Cout, P.Ho, P.Wo, HWo, P.res_w, HWr, P.relu, scale, shift, res, out);
}

// ---- HALF STORAGE: the half compute mode with the maps between layers stored in the compute type -----------------------------
// (the smot_dla_half_storage_* entry points).  A map type is the element type of the compute type: f16_t or bf16_t.  Widening
// a stored value is exact and monotone, so rounding it again on load gives the stored bits and the max-pool of widened values
// is the widened max-pool: an operator here returns what the half-mode operator returns on the widened maps, rounded once.
template <int CT>
struct DlMapOf {
    using type = f16_t;
};
template <>
struct DlMapOf<SMOT_FEAT_BF16> {
    using type = bf16_t;
};
// dl_pool over a map of any type
template <typename RT>
__device__ __forceinline__ float dl_pool_of(const RT* __restrict__ q, int Ws) {
    return dl_pool_step(dl_pool_step(dl_pool_step(feat_ld<RT>(q), feat_ld<RT>(q + 1)), feat_ld<RT>(q + Ws)), feat_ld<RT>(q + Ws + 1));
}
// the residual at element `o` (plain) or through the 2 x 2 pool at `op` of a row of Ws; f32: (wave-uniform) it is an fp32 map
template <typename MT_>
__device__ __forceinline__ float dl_res_of(const void* __restrict__ res, int f32, int Ws, size_t o, size_t op) {
    if (f32) {
        const float* __restrict__ r = reinterpret_cast<const float*>(res);
        return Ws ? dl_pool(r + op, Ws) : r[o];
    }
    const MT_* __restrict__ r = reinterpret_cast<const MT_*>(res);
    return Ws ? dl_pool_of<MT_>(r + op, Ws) : feat_ld<MT_>(r + o);
}

struct DlaConv3HsArgs {
    const void* in;          // [N, Cin, H, W] of the kernel's FT
    const float* w;          // the convolution's kind-5 packed image
    const void* res;         // as DlaConv3Args', of fp32 (res_f32) or the map type
    void* out;               // [N, Cout, Ho, Wo] of the map type
    int Cin, Cout, H, W, Ho, Wo;
    int tiles_x, tiles_per_image, relu, res_h, res_w, res_f32;
};

// dla_conv3x3_hs_kernel<CT, FT, STRIDE, WR, NM>: dla_conv3x3_half_kernel's workgroup, stage (cvh_block) and sum order with the
//   input of type FT (fp32 or CT's map type), the residual of either type (a wave-uniform switch in the epilogue) and the
//   output stored rounded once to CT.  LDS as dla_conv3x3_half_kernel's.
template <int CT, typename FT, int STRIDE, int WR, int NM>
__global__ void __launch_bounds__(256, 2)
dla_conv3x3_hs_kernel(DlaConv3HsArgs P) {
    using Hh = CvhGeom<STRIDE>;
    using MapT = typename DlMapOf<CT>::type;
    constexpr int WP = 4 / WR, ROWS = CV_TH / WR;
    __shared__ __attribute__((aligned(16))) cvs_u32x4 sm[Hh::SMEM_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int n = blockIdx.x / P.tiles_per_image;
    const int t = blockIdx.x - n * P.tiles_per_image;
    const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
    const int y0 = ty * CV_TH, x0 = tx * CV_TW;
    const int HW = P.H * P.W, HWo = P.Ho * P.Wo, Cout = P.Cout;
    const FT* __restrict__ in = reinterpret_cast<const FT*>(P.in) + (size_t)n * P.Cin * HW;
    const int npairs = (Cout + 31) >> 5;
    const float* __restrict__ scale = P.w + cvh_packed_floats(P.Cin, Cout);
    const float* __restrict__ shift = scale + 32 * npairs;
    const int HWr = P.res_w ? P.res_h * P.res_w : HWo;
    const size_t rimg = (size_t)n * Cout * HWr;                 // the image's first residual element
    MapT* __restrict__ out = reinterpret_cast<MapT*>(P.out) + (size_t)n * Cout * HWo;
    const int wp = WR == 1 ? wave : wave % WP, row0 = WR == 1 ? 0 : (wave / WP) * ROWS;

    CvsPlan<STRIDE> pl;
    cvs_plan<STRIDE>(pl, tid, y0, x0, P.H, P.W);
    const int x = x0 + xl;
    const int pair = blockIdx.y * WP + wp;                      // grid.y: the blocks of 32 WP output channels
    const bool active = pair < npairs;
    cv_f32x4 acc[NM][ROWS];
    cvh_block<CT, FT, STRIDE, WR, NM, 1>(sm, in, HW, P.Cin, pl, P.w, pair, active, tid, row0, acc);
    if (active && x < P.Wo) {
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 32 * pair + 16 * m + 4 * kq + r;
                if (ch >= Cout) continue;
                const float sc = scale[ch], sh = shift[ch];
#pragma unroll
                for (int nt = 0; nt < ROWS; ++nt) {
                    const int y = y0 + row0 + nt;
                    if (y < P.Ho) {
                        const int o = ch * HWo + y * P.Wo + x;
                        float v = add_rn(mul_rn(acc[m][nt][r], sc), sh);
                        if (P.res)
                            v = add_rn(v, dl_res_of<MapT>(P.res, P.res_f32, P.res_w, rimg + o,
                                                          rimg + (size_t)ch * HWr + 2 * y * P.res_w + 2 * x));
                        cv_store<MapT>(out + o, P.relu ? relu_nan(v) : v);
                    }
                }
            }
    }
}

// ---- 1x1 over a virtual concatenation ---------------------------------------------------------------------------------------
struct DlaSrc {
    const float* p;          // [N, C, Hs, Ws]
    int C;                   // % 16 == 0
    int pooled;              // 1: position (y, x) is the max of (2y .. 2y + 1, 2x .. 2x + 1) of a map with Hs / 2 == H, Ws / 2 == W
    int Hs, Ws;
};
struct DlaConv1Args {
    DlaSrc src[DL_MAX_SRC];
    const float* a;          // the convolution's packed image
    void* out;               // [N, Cout, H, W] of OT
    float* out32;            // the same in fp32 as well, or nullptr
    int nsrc, K, Cout, H, W, tiles_per_image, relu;
};

template <typename OT>
__global__ void __launch_bounds__(256, 4)
dla_conv1x1_kernel(DlaConv1Args P) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int Cout = P.Cout, HW = P.H * P.W;
    const int n = blockIdx.x / P.tiles_per_image;
    const int tile = blockIdx.x - n * P.tiles_per_image;
    const int p = tile * DL_POS + wave * 16 + xl;
    const bool live = p < HW;
    const int y = live ? p / P.W : 0, x = live ? p - y * P.W : 0;
    const int ng = P.K >> 4;
    const float* __restrict__ scale = P.a + (size_t)Cout * P.K;
    const float* __restrict__ shift = scale + Cout;
    const int m0 = blockIdx.y * DL_MT;
    const cv_f32x4* __restrict__ ap = reinterpret_cast<const cv_f32x4*>(P.a) + (size_t)m0 * ng * 64 + lane;
    cv_f32x4 acc[DL_MT];
#pragma unroll
    for (int m = 0; m < DL_MT; ++m) acc[m] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cv_f32x4 an[DL_MT], ac[DL_MT];
    float bn[4], bc[4];
    // one source after the other (the K order of the concatenation); within a source the next 16 channels' operands are in
    // flight while the current ones multiply
    int g0 = 0;
    auto source = [&](const float* __restrict__ sp, int sC, int spool, int sHs, int sWs) {
        const int sg = sC >> 4;
        const int HWs = spool ? sHs * sWs : HW;
        const float* __restrict__ bp = sp + ((size_t)n * sC + kq) * HWs + (spool ? (2 * y) * sWs + 2 * x : p);
        auto fetch = [&](int gl) {
#pragma unroll
            for (int m = 0; m < DL_MT; ++m) an[m] = ap[((size_t)m * ng + g0 + gl) * 64];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = 0.0f;
                if (live) {
                    const float* __restrict__ q = bp + (size_t)(16 * gl + 4 * e) * HWs;
                    v = spool ? dl_pool(q, sWs) : q[0];
                }
                bn[e] = v;
            }
        };
        fetch(0);
#pragma unroll 1
        for (int gl = 0; gl < sg; ++gl) {
#pragma unroll
            for (int m = 0; m < DL_MT; ++m) ac[m] = an[m];
#pragma unroll
            for (int e = 0; e < 4; ++e) bc[e] = bn[e];
            if (gl + 1 < sg) fetch(gl + 1);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int m = 0; m < DL_MT; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[m][e], bc[e], acc[m], 0, 0, 0);
        }
        g0 += sg;
    };
    source(P.src[0].p, P.src[0].C, P.src[0].pooled, P.src[0].Hs, P.src[0].Ws);
    if (P.nsrc > 1) source(P.src[1].p, P.src[1].C, P.src[1].pooled, P.src[1].Hs, P.src[1].Ws);
    if (P.nsrc > 2) source(P.src[2].p, P.src[2].C, P.src[2].pooled, P.src[2].Hs, P.src[2].Ws);
    if (P.nsrc > 3) source(P.src[3].p, P.src[3].C, P.src[3].pooled, P.src[3].Hs, P.src[3].Ws);
    if (live) {
        OT* __restrict__ oimg = reinterpret_cast<OT*>(P.out) + (size_t)n * Cout * HW;
        float* __restrict__ o32 = P.out32 ? P.out32 + (size_t)n * Cout * HW : nullptr;
#pragma unroll
        for (int m = 0; m < DL_MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 16 * (m0 + m) + 4 * kq + r;
                float v = add_rn(mul_rn(acc[m][r], scale[ch]), shift[ch]);
                if (P.relu) v = relu_nan(v);
                cv_store<OT>(oimg + (size_t)ch * HW + p, v);
                if (o32) o32[(size_t)ch * HW + p] = v;
            }
    }
}

// dla_conv1x1_res_kernel<OT>: the same workgroup, operand order and k-loop over up to EIGHT sources, with an optional
//   residual in the epilogue: out = relu?(acc * scale + shift + residual), one fp32 add_rn after the BN and before the ReLU,
//   as in the 3x3 kernel.  The residual is [N, Cout, H, W], or (res_w != 0) [N, Cout, res_h, res_w] read through the 2 x 2
//   max-pool; it is only read, so it may be one of the sources (a residual root adds its first source).  Serves a bottleneck
//   block's conv3, the residual roots and every root over more than four maps.  (dla_conv1x1_kernel keeps its body, which
//   precedes: one template over both argument structs gives the same values and another register allocation, and the code
//   that DLA-34 runs is to stay what it was.  With <= 4 sources and no residual the two give the same bits: the sequence
//   of matrix instructions is the same.)
constexpr int DL_MAX_SRC_RES = 8;
struct DlaConv1ResArgs {
    DlaSrc src[DL_MAX_SRC_RES];
    const float* a;          // the convolution's packed image
    void* out;               // [N, Cout, H, W] of OT
    float* out32;            // the same in fp32 as well, or nullptr
    const float* res;        // [N, Cout, H, W], or nullptr; res_w != 0: [N, Cout, res_h, res_w] read through a 2 x 2 max-pool
    int nsrc, K, Cout, H, W, tiles_per_image, relu, res_h, res_w;
};

template <typename OT>
__global__ void __launch_bounds__(256, 4)
dla_conv1x1_res_kernel(DlaConv1ResArgs P) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int Cout = P.Cout, HW = P.H * P.W;
    const int n = blockIdx.x / P.tiles_per_image;
    const int tile = blockIdx.x - n * P.tiles_per_image;
    const int p = tile * DL_POS + wave * 16 + xl;
    const bool live = p < HW;
    const int y = live ? p / P.W : 0, x = live ? p - y * P.W : 0;
    const int ng = P.K >> 4;
    const float* __restrict__ scale = P.a + (size_t)Cout * P.K;
    const float* __restrict__ shift = scale + Cout;
    const int m0 = blockIdx.y * DL_MT;
    const cv_f32x4* __restrict__ ap = reinterpret_cast<const cv_f32x4*>(P.a) + (size_t)m0 * ng * 64 + lane;
    cv_f32x4 acc[DL_MT];
#pragma unroll
    for (int m = 0; m < DL_MT; ++m) acc[m] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cv_f32x4 an[DL_MT], ac[DL_MT];
    float bn[4], bc[4];
    int g0 = 0;
    auto source = [&](const float* sp, int sC, int spool, int sHs, int sWs) {
        const int sg = sC >> 4;
        const int HWs = spool ? sHs * sWs : HW;
        const float* bp = sp + ((size_t)n * sC + kq) * HWs + (spool ? (2 * y) * sWs + 2 * x : p);
        auto fetch = [&](int gl) {
#pragma unroll
            for (int m = 0; m < DL_MT; ++m) an[m] = ap[((size_t)m * ng + g0 + gl) * 64];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = 0.0f;
                if (live) {
                    const float* q = bp + (size_t)(16 * gl + 4 * e) * HWs;
                    v = spool ? dl_pool(q, sWs) : q[0];
                }
                bn[e] = v;
            }
        };
        fetch(0);
#pragma unroll 1
        for (int gl = 0; gl < sg; ++gl) {
#pragma unroll
            for (int m = 0; m < DL_MT; ++m) ac[m] = an[m];
#pragma unroll
            for (int e = 0; e < 4; ++e) bc[e] = bn[e];
            if (gl + 1 < sg) fetch(gl + 1);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int m = 0; m < DL_MT; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[m][e], bc[e], acc[m], 0, 0, 0);
        }
        g0 += sg;
    };
#pragma unroll
    for (int s = 0; s < DL_MAX_SRC_RES; ++s)
        if (s < P.nsrc) source(P.src[s].p, P.src[s].C, P.src[s].pooled, P.src[s].Hs, P.src[s].Ws);
    if (live) {
        OT* __restrict__ oimg = reinterpret_cast<OT*>(P.out) + (size_t)n * Cout * HW;
        float* __restrict__ o32 = P.out32 ? P.out32 + (size_t)n * Cout * HW : nullptr;
        const int HWr = P.res_w ? P.res_h * P.res_w : HW;
        const float* res = P.res ? P.res + (size_t)n * Cout * HWr + (P.res_w ? 2 * y * P.res_w + 2 * x : p) : nullptr;
#pragma unroll
        for (int m = 0; m < DL_MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 16 * (m0 + m) + 4 * kq + r;
                float v = add_rn(mul_rn(acc[m][r], scale[ch]), shift[ch]);
                if (res) v = add_rn(v, P.res_w ? dl_pool(res + (size_t)ch * HWr, P.res_w) : res[(size_t)ch * HWr]);
                if (P.relu) v = relu_nan(v);
                cv_store<OT>(oimg + (size_t)ch * HW + p, v);
                if (o32) o32[(size_t)ch * HW + p] = v;
            }
    }
}

// dla_conv1x1_half_kernel<CT, OT, MT>: dla_conv1x1_res_kernel's job in HALF COMPUTE MODE on v_mfma_f32_16x16x32_f16 / _bf16.
//   workgroup = 64 positions (wave w: positions 16 w .. 16 w + 15 of the tile) x MT M-tiles (16 MT output channels; M-tiles
//   beyond Cout / 16 — the tail of the last block — are neither loaded nor multiplied).  One K step is 32 channels of ONE
//   source (every source is a multiple of 32 wide).
//   A operand: the kind-6 image, 16 bytes per lane and M-tile, straight into registers.
//   B operand: lane (kq, xl) loads channels 8 kq .. 8 kq + 7 of its position in place (plain, or the 2 x 2 max-pool of the
//   window) as fp32 and rounds them to CT in registers; a dead position of the last tile supplies zeros, never a loaded value.
//   The next K step's A and B are in flight while the current one multiplies.  No LDS: a B value is used by one lane
//   only, so staging it would add a write and a read per value for nothing but the coalescing, which a lane group's sixteen
//   consecutive positions (64 bytes per channel) already have; what is re-read is B once per block of 16 MT output
//   channels, and MT = 4 halves that against dla_conv1x1_res_kernel wherever the launch still fills the CUs (dl_conv1_half_mt).
//   An output's sum order is the K order of the concatenation: fixed by the channel counts alone.
template <int CT, typename OT, int MT>
__global__ void __launch_bounds__(256, 2)
dla_conv1x1_half_kernel(DlaConv1ResArgs P) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int Cout = P.Cout, HW = P.H * P.W;
    const int n = blockIdx.x / P.tiles_per_image;
    const int tile = blockIdx.x - n * P.tiles_per_image;
    const int p = tile * DL_POS + wave * 16 + xl;
    const bool live = p < HW;
    const int y = live ? p / P.W : 0, x = live ? p - y * P.W : 0;
    const int ng = P.K >> 5;
    const float* __restrict__ scale = P.a + (size_t)Cout * P.K / 2;
    const float* __restrict__ shift = scale + Cout;
    const int m0 = blockIdx.y * MT;
    const int nm = min(MT, (Cout >> 4) - m0);                   // (block-uniform) the M-tiles this block has
    const cvs_u32x4* __restrict__ ap = reinterpret_cast<const cvs_u32x4*>(P.a) + (size_t)m0 * ng * 64 + lane;
    cv_f32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cvs_u32x4 an[MT], ac[MT], bc;
    float bn[8];
    int g0 = 0;
    auto source = [&](const float* sp, int sC, int spool, int sHs, int sWs) {
        const int sg = sC >> 5;
        const int HWs = spool ? sHs * sWs : HW;
        const float* bp = sp + ((size_t)n * sC + 8 * kq) * HWs + (spool ? (2 * y) * sWs + 2 * x : p);
        auto fetch = [&](int gl) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (m < nm) an[m] = ap[((size_t)m * ng + g0 + gl) * 64];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = 0.0f;
                if (live) {
                    const float* q = bp + (size_t)(32 * gl + j) * HWs;
                    v = spool ? dl_pool(q, sWs) : q[0];
                }
                bn[j] = v;
            }
        };
        fetch(0);
#pragma unroll 1
        for (int gl = 0; gl < sg; ++gl) {
#pragma unroll
            for (int m = 0; m < MT; ++m) ac[m] = an[m];
#pragma unroll
            for (int e = 0; e < 4; ++e) bc[e] = cvh_pack2<CT>(bn[2 * e], bn[2 * e + 1]);
            if (gl + 1 < sg) fetch(gl + 1);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (m < nm) acc[m] = cvh_mfma<CT>(ac[m], bc, acc[m]);
        }
        g0 += sg;
    };
#pragma unroll
    for (int s = 0; s < DL_MAX_SRC_RES; ++s)
        if (s < P.nsrc) source(P.src[s].p, P.src[s].C, P.src[s].pooled, P.src[s].Hs, P.src[s].Ws);
    if (live) {
        OT* __restrict__ oimg = reinterpret_cast<OT*>(P.out) + (size_t)n * Cout * HW;
        float* __restrict__ o32 = P.out32 ? P.out32 + (size_t)n * Cout * HW : nullptr;
        const int HWr = P.res_w ? P.res_h * P.res_w : HW;
        const float* res = P.res ? P.res + (size_t)n * Cout * HWr + (P.res_w ? 2 * y * P.res_w + 2 * x : p) : nullptr;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m >= nm) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 16 * (m0 + m) + 4 * kq + r;
                float v = add_rn(mul_rn(acc[m][r], scale[ch]), shift[ch]);
                if (res) v = add_rn(v, P.res_w ? dl_pool(res + (size_t)ch * HWr, P.res_w) : res[(size_t)ch * HWr]);
                if (P.relu) v = relu_nan(v);
                cv_store<OT>(oimg + (size_t)ch * HW + p, v);
                if (o32) o32[(size_t)ch * HW + p] = v;
            }
        }
    }
}

// dla_conv1x1_hs_kernel<CT, ST, MT>: dla_conv1x1_half_kernel's workgroup, K order and k-loop in HALF STORAGE: every source of
//   this launch is of type ST (fp32, or CT's map type: a lane then loads its eight channels as eight 2-byte values, sixteen
//   consecutive positions of a lane group are 32 bytes per channel), widened in registers — exact — and rounded to CT as the
//   half kernel rounds, which gives the stored bits back; the residual is fp32 or of the map type (a wave-uniform switch in
//   the epilogue); the output is stored rounded once to CT and no fp32 copy exists.  No LDS.
struct DlaConv1HsArgs {
    DlaSrc src[DL_MAX_SRC_RES];   // (p: of the launch's source type ST)
    const float* a;          // the convolution's kind-6 packed image
    void* out;               // [N, Cout, H, W] of the map type
    const void* res;         // as DlaConv1ResArgs', of fp32 (res_f32) or the map type
    int nsrc, K, Cout, H, W, tiles_per_image, relu, res_h, res_w, res_f32;
};

template <int CT, typename ST, int MT>
__global__ void __launch_bounds__(256, 2)
dla_conv1x1_hs_kernel(DlaConv1HsArgs P) {
    using MapT = typename DlMapOf<CT>::type;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int Cout = P.Cout, HW = P.H * P.W;
    const int n = blockIdx.x / P.tiles_per_image;
    const int tile = blockIdx.x - n * P.tiles_per_image;
    const int p = tile * DL_POS + wave * 16 + xl;
    const bool live = p < HW;
    const int y = live ? p / P.W : 0, x = live ? p - y * P.W : 0;
    const int ng = P.K >> 5;
    const float* __restrict__ scale = P.a + (size_t)Cout * P.K / 2;
    const float* __restrict__ shift = scale + Cout;
    const int m0 = blockIdx.y * MT;
    const int nm = min(MT, (Cout >> 4) - m0);                   // (block-uniform) the M-tiles this block has
    const cvs_u32x4* __restrict__ ap = reinterpret_cast<const cvs_u32x4*>(P.a) + (size_t)m0 * ng * 64 + lane;
    cv_f32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cvs_u32x4 an[MT], ac[MT], bc;
    float bn[8];
    int g0 = 0;
    auto source = [&](const float* sp, int sC, int spool, int sHs, int sWs) {
        const int sg = sC >> 5;
        const int HWs = spool ? sHs * sWs : HW;
        const ST* bp = reinterpret_cast<const ST*>(sp) + ((size_t)n * sC + 8 * kq) * HWs + (spool ? (2 * y) * sWs + 2 * x : p);
        auto fetch = [&](int gl) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (m < nm) an[m] = ap[((size_t)m * ng + g0 + gl) * 64];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = 0.0f;
                if (live) {
                    const ST* q = bp + (size_t)(32 * gl + j) * HWs;
                    v = spool ? dl_pool_of<ST>(q, sWs) : feat_ld<ST>(q);
                }
                bn[j] = v;
            }
        };
        fetch(0);
#pragma unroll 1
        for (int gl = 0; gl < sg; ++gl) {
#pragma unroll
            for (int m = 0; m < MT; ++m) ac[m] = an[m];
#pragma unroll
            for (int e = 0; e < 4; ++e) bc[e] = cvh_pack2<CT>(bn[2 * e], bn[2 * e + 1]);
            if (gl + 1 < sg) fetch(gl + 1);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (m < nm) acc[m] = cvh_mfma<CT>(ac[m], bc, acc[m]);
        }
        g0 += sg;
    };
#pragma unroll
    for (int s = 0; s < DL_MAX_SRC_RES; ++s)
        if (s < P.nsrc) source(P.src[s].p, P.src[s].C, P.src[s].pooled, P.src[s].Hs, P.src[s].Ws);
    if (live) {
        MapT* __restrict__ oimg = reinterpret_cast<MapT*>(P.out) + (size_t)n * Cout * HW;
        const int HWr = P.res_w ? P.res_h * P.res_w : HW;
        const size_t r0 = (size_t)n * Cout * HWr;               // the image's first residual element
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m >= nm) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 16 * (m0 + m) + 4 * kq + r;
                float v = add_rn(mul_rn(acc[m][r], scale[ch]), shift[ch]);
                if (P.res)
                    v = add_rn(v, dl_res_of<MapT>(P.res, P.res_f32, P.res_w, r0 + (size_t)ch * HWr + p,
                                                  r0 + (size_t)ch * HWr + 2 * y * P.res_w + 2 * x));
                if (P.relu) v = relu_nan(v);
                cv_store<MapT>(oimg + (size_t)ch * HW + p, v);
            }
        }
    }
}

// ---- 7x7 (base_layer) -------------------------------------------------------------------------------------------------------
struct DlaConv7Args {
    const void* in;          // [N, 3, H, W] of FT
    const float* a;          // the convolution's packed image
    float* out;              // [N, C0, H, W]
    int C0, H, W, tiles_x, tiles_per_image;
};

template <typename FT>
__global__ void __launch_bounds__(256, 2)
dla_conv7x7_kernel(DlaConv7Args P) {
    __shared__ __attribute__((aligned(16))) float sm[S7_SMEM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int n = blockIdx.x / P.tiles_per_image;
    const int t = blockIdx.x - n * P.tiles_per_image;
    const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
    const int y0 = ty * CV_TH, x0 = tx * CV_TW;
    const int H = P.H, W = P.W, HW = H * W, C0 = P.C0;
    const FT* __restrict__ in = reinterpret_cast<const FT*>(P.in) + (size_t)n * 3 * HW;
    for (int e = tid; e < S7_SMEM; e += 256) {
        float v = 0.0f;
        if (e < S7_ZERO) {
            const int ic = e / S7_PLANE, cell = e - ic * S7_PLANE;
            const int r = cell / S7_PW, col = cell - r * S7_PW;
            const int gy = y0 - 3 + r, gx = x0 - 3 + col;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = feat_ld<FT>(in + ic * HW + gy * W + gx);
        }
        sm[e] = v;
    }
    __syncthreads();
    const int mt = C0 >> 4;
    const float* __restrict__ scale = P.a + (size_t)mt * S7_Q * 256;
    const float* __restrict__ shift = scale + C0;
    float* __restrict__ out = P.out + (size_t)n * C0 * HW;
    const int x = x0 + xl;
    // B operand of lane (kq, xl) at k-step ks: cell (ic, ky, kx) of k = 4 ks + kq, or the zero run for the K pad; it depends on
    // the lane alone, so it is worked out once, in front of the M-tiles
    int off[S7_KS];
#pragma unroll
    for (int ks = 0; ks < S7_KS; ++ks) {
        const int k = 4 * ks + kq;
        const int ic = k / 49, tap = k - ic * 49, ky = tap / 7, kx = tap - ky * 7;
        off[ks] = (k < 147 ? ic * S7_PLANE + ky * S7_PW + kx + xl : S7_ZERO) + 2 * wave * S7_PW;
    }
    for (int m = 0; m < mt; ++m) {
        const cv_f32x4* __restrict__ ap = reinterpret_cast<const cv_f32x4*>(P.a) + (size_t)m * S7_Q * 64 + lane;
        cv_f32x4 a[S7_Q];
#pragma unroll
        for (int q = 0; q < S7_Q; ++q) a[q] = ap[q * 64];
        cv_f32x4 acc[2] = {(cv_f32x4){0.f, 0.f, 0.f, 0.f}, (cv_f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < S7_KS; ++ks) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const float b = sm[off[ks] + nt * S7_PW];
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks >> 2][ks & 3], b, acc[nt], 0, 0, 0);
            }
        }
        if (x < W) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 16 * m + 4 * kq + r;
                const float sc = scale[ch], sh = shift[ch];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int y = y0 + 2 * wave + nt;
                    if (y < H) out[ch * HW + y * W + x] = relu_nan(add_rn(mul_rn(acc[nt][r], sc), sh));
                }
            }
        }
    }
}

// ---- host: one launch each -------------------------------------------------------------------------------------------------
// ctype: the compute type of kinds 5 and 6 (SMOT_FEAT_F16 or SMOT_FEAT_BF16); the other kinds do not read it
static int dl_pack_launch(int kind, const float* w, const float* scale, const float* shift, int Cin, int Cout, float* packed,
                          hipStream_t st, int ctype = 0) {
    const long long total = dl_conv_floats(kind, Cin, Cout);
    if (kind == 5 || kind == 6) {
        const dim3 g((unsigned)((total + 255) / 256));
        if (ctype == SMOT_FEAT_F16) {
            SMOT_LAUNCH(dla_pack_half_kernel<SMOT_FEAT_F16>, g, dim3(256), 0, st, kind, w, scale, shift, Cin, Cout, total, packed);
        } else {
            SMOT_LAUNCH(dla_pack_half_kernel<SMOT_FEAT_BF16>, g, dim3(256), 0, st, kind, w, scale, shift, Cin, Cout, total, packed);
        }
        return check_launch("dla_pack_half");
    }
    SMOT_LAUNCH(dla_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, kind, w, scale, shift, Cin, Cout, total,
                packed);
    return check_launch("dla_pack");
}

// The wave split of a launch: the fewest row groups (the widest channel block: the input is staged once per block) that
// still give every CU a workgroup; a coarse level has few tiles and gets them from its channels instead.  The split does not
// touch an output's sum order.  (Stride 2 with four pairs x eight rows does not fit 256 registers beside its 18 staged cells
// per thread — hipcc spills two —: its widest block is 64 channels.)
// DL_MIN_WORKGROUPS is the CU count of the part this library is built for (MI355X, gfx950: 256 CUs): below one workgroup
// per CU a launch leaves CUs idle whatever the workgroups do.  It decides WHICH FORM a shape and image count run, so a
// retune moves shapes between forms: tests/test_dla.py::test_conv3x3_forms pins, through smot_dla_conv3x3_form, that its
// cases reach every form, and checks each against the oracle.
constexpr int DL_MIN_WORKGROUPS = 256;
// -> WR (1, 2 or 4) of a launch of `tiles` (8 x 16 output tiles of all images) with Cout output channels
static int dl_conv3_wr(int stride, int Cout, long long tiles) {
    const int npairs = (Cout + 31) >> 5;
    int wr = stride == 2 ? 2 : 1;
    while (wr < 4 && (4 / wr > npairs || tiles * ((npairs + 4 / wr - 1) / (4 / wr)) < DL_MIN_WORKGROUPS)) wr *= 2;
    return wr;
}
template <typename FT, int STRIDE>
static int dl_conv3_pick(const DlaConv3Args& P, int grid, hipStream_t st) {
    const int npairs = (P.Cout + 31) >> 5;
    const int wr = dl_conv3_wr(STRIDE, P.Cout, grid);
    const dim3 g(grid, (npairs + 4 / wr - 1) / (4 / wr));
    if (P.Cout <= 16) {
        SMOT_LAUNCH((dla_conv3x3_kernel<FT, STRIDE, 4, 1>), g, dim3(256), 0, st, P);
    } else if (wr == 4) {
        SMOT_LAUNCH((dla_conv3x3_kernel<FT, STRIDE, 4, 2>), g, dim3(256), 0, st, P);
    } else if (wr == 2) {
        SMOT_LAUNCH((dla_conv3x3_kernel<FT, STRIDE, 2, 2>), g, dim3(256), 0, st, P);
    } else {
        if constexpr (STRIDE == 1) SMOT_LAUNCH((dla_conv3x3_kernel<FT, 1, 1, 2>), g, dim3(256), 0, st, P);
    }
    return check_launch("dla_conv3x3");
}

// The split kernel's launch: the same wave split by the same rule (dl_conv3_wr), so a shape runs the same (WR, NM) in both
// modes; stride 2 has no WR = 1 form here either.
template <typename FT, int STRIDE>
static int dl_conv3_pick_split(const DlaConv3Args& P, int grid, hipStream_t st) {
    const int npairs = (P.Cout + 31) >> 5;
    const int wr = dl_conv3_wr(STRIDE, P.Cout, grid);
    const dim3 g(grid, (npairs + 4 / wr - 1) / (4 / wr));
    if (P.Cout <= 16) {
        SMOT_LAUNCH((dla_conv3x3_split_kernel<FT, STRIDE, 4, 1>), g, dim3(256), 0, st, P);
    } else if (wr == 4) {
        SMOT_LAUNCH((dla_conv3x3_split_kernel<FT, STRIDE, 4, 2>), g, dim3(256), 0, st, P);
    } else if (wr == 2) {
        SMOT_LAUNCH((dla_conv3x3_split_kernel<FT, STRIDE, 2, 2>), g, dim3(256), 0, st, P);
    } else {
        if constexpr (STRIDE == 1) SMOT_LAUNCH((dla_conv3x3_split_kernel<FT, 1, 1, 2>), g, dim3(256), 0, st, P);
    }
    return check_launch("dla_conv3x3_split");
}

// The half compute mode's launch: the same wave split by the same rule (dl_conv3_wr), so a shape runs the same (WR, NM) in
// every mode; stride 2 has no WR = 1 form here either.
template <int CT, typename FT, int STRIDE>
static int dl_conv3_pick_half(const DlaConv3Args& P, int grid, hipStream_t st) {
    const int npairs = (P.Cout + 31) >> 5;
    const int wr = dl_conv3_wr(STRIDE, P.Cout, grid);
    const dim3 g(grid, (npairs + 4 / wr - 1) / (4 / wr));
    if (P.Cout <= 16) {
        SMOT_LAUNCH((dla_conv3x3_half_kernel<CT, FT, STRIDE, 4, 1>), g, dim3(256), 0, st, P);
    } else if (wr == 4) {
        SMOT_LAUNCH((dla_conv3x3_half_kernel<CT, FT, STRIDE, 4, 2>), g, dim3(256), 0, st, P);
    } else if (wr == 2) {
        SMOT_LAUNCH((dla_conv3x3_half_kernel<CT, FT, STRIDE, 2, 2>), g, dim3(256), 0, st, P);
    } else {
        if constexpr (STRIDE == 1) SMOT_LAUNCH((dla_conv3x3_half_kernel<CT, FT, 1, 1, 2>), g, dim3(256), 0, st, P);
    }
    return check_launch("dla_conv3x3_half");
}

// in [N, Cin, H, W] fp32 -> out [N, Cout, Ho, Wo]; the shapes were checked by the caller (dl_conv3_ok); split: w is a kind-4
// image and Cin % 32 == 0; ctype != 0 (SMOT_FEAT_F16 or SMOT_FEAT_BF16): w is a kind-5 image of that type and Cin % 32 == 0
static int dl_conv3(const float* in, int N, int Cin, int H, int W, const float* w, int Cout, int stride, const float* res,
                    int relu, float* out, hipStream_t st, int res_h = 0, int res_w = 0, bool split = false, int ctype = 0) {
    DlaConv3Args P = {};
    P.in = in;
    P.w = w;
    P.res = res;
    P.out = out;
    P.Cin = Cin;
    P.Cout = Cout;
    P.H = H;
    P.W = W;
    P.Ho = stride == 2 ? (H - 1) / 2 + 1 : H;
    P.Wo = stride == 2 ? (W - 1) / 2 + 1 : W;
    P.tiles_x = (P.Wo + CV_TW - 1) / CV_TW;
    P.tiles_per_image = P.tiles_x * ((P.Ho + CV_TH - 1) / CV_TH);
    P.relu = relu;
    P.res_h = res_h;
    P.res_w = res_w;
    const int grid = P.tiles_per_image * N;
    if (ctype == SMOT_FEAT_F16)
        return stride == 2 ? dl_conv3_pick_half<SMOT_FEAT_F16, float, 2>(P, grid, st) : dl_conv3_pick_half<SMOT_FEAT_F16, float, 1>(P, grid, st);
    if (ctype == SMOT_FEAT_BF16)
        return stride == 2 ? dl_conv3_pick_half<SMOT_FEAT_BF16, float, 2>(P, grid, st) : dl_conv3_pick_half<SMOT_FEAT_BF16, float, 1>(P, grid, st);
    if (split) return stride == 2 ? dl_conv3_pick_split<float, 2>(P, grid, st) : dl_conv3_pick_split<float, 1>(P, grid, st);
    return stride == 2 ? dl_conv3_pick<float, 2>(P, grid, st) : dl_conv3_pick<float, 1>(P, grid, st);
}

// Half storage: the half mode's wave split by the same rule, so a shape runs the same (WR, NM) and sum order
template <int CT, typename FT, int STRIDE>
static int dl_conv3_pick_hs(const DlaConv3HsArgs& P, int grid, hipStream_t st) {
    const int npairs = (P.Cout + 31) >> 5;
    const int wr = dl_conv3_wr(STRIDE, P.Cout, grid);
    const dim3 g(grid, (npairs + 4 / wr - 1) / (4 / wr));
    if (P.Cout <= 16) {
        SMOT_LAUNCH((dla_conv3x3_hs_kernel<CT, FT, STRIDE, 4, 1>), g, dim3(256), 0, st, P);
    } else if (wr == 4) {
        SMOT_LAUNCH((dla_conv3x3_hs_kernel<CT, FT, STRIDE, 4, 2>), g, dim3(256), 0, st, P);
    } else if (wr == 2) {
        SMOT_LAUNCH((dla_conv3x3_hs_kernel<CT, FT, STRIDE, 2, 2>), g, dim3(256), 0, st, P);
    } else {
        if constexpr (STRIDE == 1) SMOT_LAUNCH((dla_conv3x3_hs_kernel<CT, FT, 1, 1, 2>), g, dim3(256), 0, st, P);
    }
    return check_launch("dla_conv3x3_hs");
}
template <int CT>
static int dl_conv3_hs_of(const DlaConv3HsArgs& P, int in_type, int stride, int grid, hipStream_t st) {
    using MapT = typename DlMapOf<CT>::type;
    if (in_type == SMOT_FEAT_F32)
        return stride == 2 ? dl_conv3_pick_hs<CT, float, 2>(P, grid, st) : dl_conv3_pick_hs<CT, float, 1>(P, grid, st);
    return stride == 2 ? dl_conv3_pick_hs<CT, MapT, 2>(P, grid, st) : dl_conv3_pick_hs<CT, MapT, 1>(P, grid, st);
}
// dl_conv3 in half storage: in of in_type, res of res_type (each fp32 or ctype), out of ctype; w a kind-5 image of ctype
static int dl_conv3_hs(const void* in, int in_type, int N, int Cin, int H, int W, const float* w, int Cout, int stride,
                       const void* res, int res_type, int relu, void* out, hipStream_t st, int res_h, int res_w, int ctype) {
    DlaConv3HsArgs P = {};
    P.in = in;
    P.w = w;
    P.res = res;
    P.out = out;
    P.Cin = Cin;
    P.Cout = Cout;
    P.H = H;
    P.W = W;
    P.Ho = stride == 2 ? (H - 1) / 2 + 1 : H;
    P.Wo = stride == 2 ? (W - 1) / 2 + 1 : W;
    P.tiles_x = (P.Wo + CV_TW - 1) / CV_TW;
    P.tiles_per_image = P.tiles_x * ((P.Ho + CV_TH - 1) / CV_TH);
    P.relu = relu;
    P.res_h = res ? res_h : 0;
    P.res_w = res ? res_w : 0;
    P.res_f32 = res_type == SMOT_FEAT_F32 ? 1 : 0;
    const int grid = P.tiles_per_image * N;
    if (ctype == SMOT_FEAT_F16) return dl_conv3_hs_of<SMOT_FEAT_F16>(P, in_type, stride, grid, st);
    return dl_conv3_hs_of<SMOT_FEAT_BF16>(P, in_type, stride, grid, st);
}

template <typename OT>
static int dl_conv1_launch(const DlaConv1Args& P, int grid, hipStream_t st) {
    SMOT_LAUNCH(dla_conv1x1_kernel<OT>, dim3(grid, (P.Cout >> 4) / DL_MT), dim3(256), 0, st, P);
    return check_launch("dla_conv1x1");
}

template <typename OT>
static int dl_conv1_res_launch(const DlaConv1ResArgs& P, int grid, hipStream_t st) {
    SMOT_LAUNCH(dla_conv1x1_res_kernel<OT>, dim3(grid, (P.Cout >> 4) / DL_MT), dim3(256), 0, st, P);
    return check_launch("dla_conv1x1_res");
}

// more than four sources, or a residual (res_w != 0: read through the 2 x 2 max-pool of a res_h x res_w map)
static int dl_conv1_res(const DlaSrc* src, int nsrc, int N, int H, int W, const float* a, int Cout, int relu, void* out,
                        int out_type, float* out32, hipStream_t st, const float* res, int res_h, int res_w) {
    DlaConv1ResArgs P = {};
    int K = 0;
    for (int s = 0; s < nsrc; ++s) {
        P.src[s] = src[s];
        K += src[s].C;
    }
    P.a = a;
    P.out = out;
    P.out32 = out32;
    P.res = res;
    P.nsrc = nsrc;
    P.K = K;
    P.Cout = Cout;
    P.H = H;
    P.W = W;
    P.tiles_per_image = (int)(((long long)H * W + DL_POS - 1) / DL_POS);
    P.relu = relu;
    P.res_h = res ? res_h : 0;
    P.res_w = res ? res_w : 0;
    const int grid = P.tiles_per_image * N;
    if (out_type == SMOT_FEAT_F32) return dl_conv1_res_launch<float>(P, grid, st);
    if (out_type == SMOT_FEAT_F16) return dl_conv1_res_launch<f16_t>(P, grid, st);
    return dl_conv1_res_launch<bf16_t>(P, grid, st);
}

// up to four sources and no residual: dla_conv1x1_kernel; anything else: dla_conv1x1_res_kernel
static int dl_conv1(const DlaSrc* src, int nsrc, int N, int H, int W, const float* a, int Cout, int relu, void* out,
                    int out_type, float* out32, hipStream_t st, const float* res = nullptr, int res_h = 0, int res_w = 0) {
    if (nsrc > DL_MAX_SRC || res) return dl_conv1_res(src, nsrc, N, H, W, a, Cout, relu, out, out_type, out32, st, res, res_h, res_w);
    DlaConv1Args P = {};
    int K = 0;
    for (int s = 0; s < nsrc; ++s) {
        P.src[s] = src[s];
        K += src[s].C;
    }
    P.a = a;
    P.out = out;
    P.out32 = out32;
    P.nsrc = nsrc;
    P.K = K;
    P.Cout = Cout;
    P.H = H;
    P.W = W;
    P.tiles_per_image = (int)(((long long)H * W + DL_POS - 1) / DL_POS);
    P.relu = relu;
    const int grid = P.tiles_per_image * N;
    if (out_type == SMOT_FEAT_F32) return dl_conv1_launch<float>(P, grid, st);
    if (out_type == SMOT_FEAT_F16) return dl_conv1_launch<f16_t>(P, grid, st);
    return dl_conv1_launch<bf16_t>(P, grid, st);
}

// The half 1x1 kernel's M-tiles per workgroup: 4 (64 output channels: the B operand is read half as often) wherever that still
// gives every CU a workgroup, else 2 (dla_conv1x1_res_kernel's block).  It does not touch an output's sum order.
static int dl_conv1_half_mt(int Cout, long long tiles) {
    return tiles * ((Cout / 16 + 3) / 4) >= DL_MIN_WORKGROUPS ? 4 : 2;
}
template <int CT, typename OT>
static int dl_conv1_half_launch(const DlaConv1ResArgs& P, int grid, hipStream_t st) {
    const int mt = P.Cout >> 4;
    if (dl_conv1_half_mt(P.Cout, grid) == 4) {
        SMOT_LAUNCH((dla_conv1x1_half_kernel<CT, OT, 4>), dim3(grid, (mt + 3) / 4), dim3(256), 0, st, P);
    } else {
        SMOT_LAUNCH((dla_conv1x1_half_kernel<CT, OT, 2>), dim3(grid, (mt + 1) / 2), dim3(256), 0, st, P);
    }
    return check_launch("dla_conv1x1_half");
}
// dl_conv1 in half compute mode: a: a kind-6 image of ctype; every source a multiple of 32 channels (the caller checked)
static int dl_conv1_half(const DlaSrc* src, int nsrc, int N, int H, int W, const float* a, int Cout, int relu, void* out,
                         int out_type, float* out32, hipStream_t st, const float* res, int res_h, int res_w, int ctype) {
    DlaConv1ResArgs P = {};
    int K = 0;
    for (int s = 0; s < nsrc; ++s) {
        P.src[s] = src[s];
        K += src[s].C;
    }
    P.a = a;
    P.out = out;
    P.out32 = out32;
    P.res = res;
    P.nsrc = nsrc;
    P.K = K;
    P.Cout = Cout;
    P.H = H;
    P.W = W;
    P.tiles_per_image = (int)(((long long)H * W + DL_POS - 1) / DL_POS);
    P.relu = relu;
    P.res_h = res ? res_h : 0;
    P.res_w = res ? res_w : 0;
    const int grid = P.tiles_per_image * N;
    if (ctype == SMOT_FEAT_F16) {
        if (out_type == SMOT_FEAT_F32) return dl_conv1_half_launch<SMOT_FEAT_F16, float>(P, grid, st);
        if (out_type == SMOT_FEAT_F16) return dl_conv1_half_launch<SMOT_FEAT_F16, f16_t>(P, grid, st);
        return dl_conv1_half_launch<SMOT_FEAT_F16, bf16_t>(P, grid, st);
    }
    if (out_type == SMOT_FEAT_F32) return dl_conv1_half_launch<SMOT_FEAT_BF16, float>(P, grid, st);
    if (out_type == SMOT_FEAT_F16) return dl_conv1_half_launch<SMOT_FEAT_BF16, f16_t>(P, grid, st);
    return dl_conv1_half_launch<SMOT_FEAT_BF16, bf16_t>(P, grid, st);
}

// Half storage: the half mode's M-tiles per workgroup by the same rule (dl_conv1_half_mt)
template <int CT, typename ST>
static int dl_conv1_hs_launch(const DlaConv1HsArgs& P, int grid, hipStream_t st) {
    const int mt = P.Cout >> 4;
    if (dl_conv1_half_mt(P.Cout, grid) == 4) {
        SMOT_LAUNCH((dla_conv1x1_hs_kernel<CT, ST, 4>), dim3(grid, (mt + 3) / 4), dim3(256), 0, st, P);
    } else {
        SMOT_LAUNCH((dla_conv1x1_hs_kernel<CT, ST, 2>), dim3(grid, (mt + 1) / 2), dim3(256), 0, st, P);
    }
    return check_launch("dla_conv1x1_hs");
}
// dl_conv1_half in half storage: every source of src_type, res of res_type (each fp32 or ctype), out of ctype
static int dl_conv1_hs(const DlaSrc* src, int nsrc, int src_type, int N, int H, int W, const float* a, int Cout, int relu,
                       void* out, hipStream_t st, const void* res, int res_type, int res_h, int res_w, int ctype) {
    DlaConv1HsArgs P = {};
    int K = 0;
    for (int s = 0; s < nsrc; ++s) {
        P.src[s] = src[s];
        K += src[s].C;
    }
    P.a = a;
    P.out = out;
    P.res = res;
    P.nsrc = nsrc;
    P.K = K;
    P.Cout = Cout;
    P.H = H;
    P.W = W;
    P.tiles_per_image = (int)(((long long)H * W + DL_POS - 1) / DL_POS);
    P.relu = relu;
    P.res_h = res ? res_h : 0;
    P.res_w = res ? res_w : 0;
    P.res_f32 = res_type == SMOT_FEAT_F32 ? 1 : 0;
    const int grid = P.tiles_per_image * N;
    if (ctype == SMOT_FEAT_F16) {
        if (src_type == SMOT_FEAT_F32) return dl_conv1_hs_launch<SMOT_FEAT_F16, float>(P, grid, st);
        return dl_conv1_hs_launch<SMOT_FEAT_F16, f16_t>(P, grid, st);
    }
    if (src_type == SMOT_FEAT_F32) return dl_conv1_hs_launch<SMOT_FEAT_BF16, float>(P, grid, st);
    return dl_conv1_hs_launch<SMOT_FEAT_BF16, bf16_t>(P, grid, st);
}

static int dl_conv7(const void* image, int in_type, int N, int H, int W, const float* a, int C0, float* out, hipStream_t st) {
    DlaConv7Args P = {};
    P.in = image;
    P.a = a;
    P.out = out;
    P.C0 = C0;
    P.H = H;
    P.W = W;
    P.tiles_x = (W + CV_TW - 1) / CV_TW;
    P.tiles_per_image = P.tiles_x * ((H + CV_TH - 1) / CV_TH);
    const dim3 grid(P.tiles_per_image * N);
    if (in_type == SMOT_FEAT_F32) {
        SMOT_LAUNCH(dla_conv7x7_kernel<float>, grid, dim3(256), 0, st, P);
    } else if (in_type == SMOT_FEAT_F16) {
        SMOT_LAUNCH(dla_conv7x7_kernel<f16_t>, grid, dim3(256), 0, st, P);
    } else {
        SMOT_LAUNCH(dla_conv7x7_kernel<bf16_t>, grid, dim3(256), 0, st, P);
    }
    return check_launch("dla_conv7x7");
}

// ---- host: the network ----------------------------------------------------------------------------------------------------
struct DlaConv {
    int kind, cin, cout;
    long long off;           // first float in the packed image
};
struct DlaNet {
    int n, k3;               // k3: the kind of the trees' 3x3 images (3; 4: split operands; 5: half compute mode)
    int k1, ctype;           // k1: the kind of the trees' 1x1 images (1; 6: half compute mode, of compute type ctype)
    DlaConv conv[DL_MAX_CONVS];
    long long total;
};

static void dl_add(DlaNet& net, int kind, int cin, int cout) {
    DlaConv& c = net.conv[net.n++];
    c.kind = kind;
    c.cin = cin;
    c.cout = cout;
    c.off = net.total;
    net.total += dl_conv_floats(kind, cin, cout);
}
// a levels = 1 tree, in the order its launches run: project, tree1.conv1, tree1.conv2, tree2.conv1, tree2.conv2, root
// (k3: the kind of the tree's 3x3 images: 3, or 4 in split mode)
static void dl_add_tree1(DlaNet& net, int cin, int cout, int root_extra, int k3) {
    if (cin != cout) dl_add(net, 1, cin, cout);
    dl_add(net, k3, cin, cout);
    dl_add(net, k3, cout, cout);
    dl_add(net, k3, cout, cout);
    dl_add(net, k3, cout, cout);
    dl_add(net, 1, 2 * cout + root_extra, cout);
}

// The convolutions of the network in launch order.  SMOT_ERR_BAD_ARG for null arrays, SMOT_ERR_UNSUPPORTED beyond the capacities.
// split: the trees' 3x3 convolutions are kind 4 (every one has Cin = a channels[k >= 1], a multiple of 32); the stem's stay kind 3.
static int dla_net(const int* levels, const int* ch, DlaNet& net, const char* who, bool split = false) {
    if (!levels || !ch) {
        set_error("%s: null pointer", who);
        return SMOT_ERR_BAD_ARG;
    }
    bool ok = levels[0] == 1 && levels[1] == 1 && (ch[0] == 16 || ch[0] == 32) && ch[1] >= 32 && ch[1] % 32 == 0 && ch[1] <= 1024;
    for (int k = 2; k < 6; ++k)
        ok = ok && (levels[k] == 1 || levels[k] == 2) && ch[k] >= 32 && ch[k] % 32 == 0 && ch[k] <= 1024;
    if (!ok) {
        set_error("%s: levels (%d,%d,%d,%d,%d,%d), channels (%d,%d,%d,%d,%d,%d) (supported: levels[0] = levels[1] = 1, levels[2..5] "
                  "in {1, 2}; channels[0] in {16, 32}, the others multiples of 32 up to 1024)",
                  who, levels[0], levels[1], levels[2], levels[3], levels[4], levels[5], ch[0], ch[1], ch[2], ch[3], ch[4], ch[5]);
        return SMOT_ERR_UNSUPPORTED;
    }
    net.n = 0;
    net.total = 0;
    net.k3 = split ? 4 : 3;
    net.k1 = 1;
    net.ctype = 0;
    dl_add(net, 7, 3, ch[0]);
    dl_add(net, 3, ch[0], ch[0]);
    dl_add(net, 3, ch[0], ch[1]);
    for (int k = 2; k < 6; ++k) {
        const int cin = ch[k - 1], cout = ch[k], root = k > 2 ? cin : 0;      // level_root: level3 .. level5
        if (levels[k] == 1) {
            dl_add_tree1(net, cin, cout, root, net.k3);
        } else {
            dl_add_tree1(net, cin, cout, 0, net.k3);
            dl_add_tree1(net, cout, cout, root + cout, net.k3);
        }
    }
    return SMOT_OK;
}

static int dla_size_ok(int N, int H, int W, const char* who) {
    if (N < 1 || N > SMOT_MAX_IMAGES) {
        set_error("%s: num_images = %d (1 .. %d)", who, N, SMOT_MAX_IMAGES);
        return SMOT_ERR_BAD_ARG;
    }
    if (H < 32 || W < 32 || H % 32 != 0 || W % 32 != 0) {
        set_error("%s: image %d x %d (supported: both sides positive multiples of 32, as upstream)", who, H, W);
        return SMOT_ERR_UNSUPPORTED;
    }
    return SMOT_OK;
}

// The walk over the network: `dry` counts the workspace and launches nothing.
struct DlaCtx {
    const DlaNet* net;
    int ci;                  // the next convolution
    const float* packed;
    float* ws;
    long long bump, peak;    // floats
    bool dry;
    int N, rc;
    hipStream_t st;
    int block, rroot;        // dn_walk's: the block type (SMOT_DLA_BLOCK_*) and "every root adds its first source"
    int mt;                  // dn_walk's: the element type of the TREE maps: SMOT_FEAT_F32 (= 0), or the compute type in half storage
};
static float* dl_alloc(DlaCtx& c, long long floats) {
    float* p = c.dry ? nullptr : c.ws + c.bump;
    c.bump += (floats + 3) & ~3LL;
    if (c.bump > c.peak) c.peak = c.bump;
    return p;
}
static int dl_type_bytes(int type) { return type == SMOT_FEAT_F32 ? 4 : 2; }
// a tree map of `elems` elements of c.mt: carved in bytes of that type, in units of 16 bytes (fp32 maps: dl_alloc's answer)
static void* dl_alloc_map(DlaCtx& c, long long elems) {
    return dl_alloc(c, (elems * dl_type_bytes(c.mt) + 3) / 4);
}
static const float* dl_next(DlaCtx& c, int kind, int cin, int cout) {
    const DlaConv& v = c.net->conv[c.ci++];
    if (v.kind != kind || v.cin != cin || v.cout != cout) c.rc = SMOT_ERR_BAD_ARG;      // (the two walks disagree: a bug)
    return c.dry ? nullptr : c.packed + v.off;
}
// in_type, res_type: read in half storage (c.mt != SMOT_FEAT_F32) only, where a tree convolution's input and residual are
// of fp32 (x1) or of c.mt and its output is of c.mt; everywhere else every map is fp32
static void dl_run3(DlaCtx& c, int kind, const void* in, int Cin, int H, int W, int Cout, int stride, const void* res,
                    void* out, int res_h = 0, int res_w = 0, int in_type = SMOT_FEAT_F32, int res_type = SMOT_FEAT_F32) {
    const float* w = dl_next(c, kind, Cin, Cout);
    if (c.dry || c.rc) return;
    if (kind == 5 && c.mt != SMOT_FEAT_F32)
        c.rc = dl_conv3_hs(in, in_type, c.N, Cin, H, W, w, Cout, stride, res, res_type, 1, out, c.st, res_h, res_w, c.net->ctype);
    else
        c.rc = dl_conv3((const float*)in, c.N, Cin, H, W, w, Cout, stride, (const float*)res, 1, (float*)out, c.st, res_h, res_w,
                        kind == 4, kind == 5 ? c.net->ctype : 0);
}
// (half storage: out_type and out32 are not read: the output is of c.mt; src_type: the type of every source)
static void dl_run1(DlaCtx& c, const DlaSrc* src, int nsrc, int H, int W, int Cout, int relu, void* out, int out_type, float* out32,
                    const void* res = nullptr, int res_h = 0, int res_w = 0, int src_type = SMOT_FEAT_F32,
                    int res_type = SMOT_FEAT_F32) {
    int K = 0;
    for (int s = 0; s < nsrc; ++s) K += src[s].C;
    const int k1 = c.net->k1;
    const float* a = dl_next(c, k1, K, Cout);
    if (c.dry || c.rc) return;
    if (k1 == 6 && c.mt != SMOT_FEAT_F32)
        c.rc = dl_conv1_hs(src, nsrc, src_type, c.N, H, W, a, Cout, relu, out, c.st, res, res_type, res_h, res_w, c.net->ctype);
    else if (k1 == 6) c.rc = dl_conv1_half(src, nsrc, c.N, H, W, a, Cout, relu, out, out_type, out32, c.st, (const float*)res, res_h, res_w, c.net->ctype);
    else c.rc = dl_conv1(src, nsrc, c.N, H, W, a, Cout, relu, out, out_type, out32, c.st, (const float*)res, res_h, res_w);
}

// A levels = 1 tree on x [N, cin, H, W] -> [N, cout, Ho, Wo] at `out` (of out_type; fp32 at out32 as well if non-null), or in
// the workspace if `out` is null.  extra: what the parent handed down, concatenated behind (x2, x1, [bottom]).  -> the fp32 map.
static const float* dl_tree1(DlaCtx& c, const float* x, int cin, int H, int W, int cout, int stride, bool level_root,
                             const DlaSrc* extra, int nextra, void* out, int out_type, float* out32) {
    const int Ho = H / stride, Wo = W / stride;
    const long long on = (long long)c.N * cout * Ho * Wo;
    const DlaSrc bottom = {x, cin, stride == 2 ? 1 : 0, H, W};
    const float* residual = x;
    if (cin != cout) {
        float* r = dl_alloc(c, on);
        dl_run1(c, &bottom, 1, Ho, Wo, cout, 0, r, SMOT_FEAT_F32, nullptr);
        residual = r;
    }
    float* t1 = dl_alloc(c, on);
    float* x1 = dl_alloc(c, on);
    float* t2 = dl_alloc(c, on);
    float* x2 = dl_alloc(c, on);
    const int k3 = c.net->k3;
    dl_run3(c, k3, x, cin, H, W, cout, stride, nullptr, t1);
    // (cin == cout at stride 2: the residual is the pooled input itself, read through the pool)
    const bool rpool = cin == cout && stride == 2;
    dl_run3(c, k3, t1, cout, Ho, Wo, cout, 1, residual, x1, rpool ? H : 0, rpool ? W : 0);
    dl_run3(c, k3, x1, cout, Ho, Wo, cout, 1, nullptr, t2);
    dl_run3(c, k3, t2, cout, Ho, Wo, cout, 1, x1, x2);
    DlaSrc src[DL_MAX_SRC] = {{x2, cout, 0, Ho, Wo}, {x1, cout, 0, Ho, Wo}};
    int ns = 2;
    if (level_root) src[ns++] = bottom;
    for (int e = 0; e < nextra; ++e) src[ns++] = extra[e];
    const float* result;
    if (out) {
        dl_run1(c, src, ns, Ho, Wo, cout, 1, out, out_type, out32);
        result = out_type == SMOT_FEAT_F32 ? (const float*)out : out32;
    } else {
        float* o = dl_alloc(c, on);
        dl_run1(c, src, ns, Ho, Wo, cout, 1, o, SMOT_FEAT_F32, nullptr);
        result = o;
    }
    return result;
}

// image -> x1 [N, c1, H / 2, W / 2] at `x1` (fp32); the two c0-channel maps in the workspace
static void dl_stem(DlaCtx& c, const void* image, int in_type, int H, int W, int c0, int c1, float* x1) {
    const long long n0 = (long long)c.N * c0 * H * W;
    float* x = dl_alloc(c, n0);
    float* x0 = dl_alloc(c, n0);
    const float* a = dl_next(c, 7, 3, c0);
    if (!c.dry && !c.rc) c.rc = dl_conv7(image, in_type, c.N, H, W, a, c0, x, c.st);
    dl_run3(c, 3, x, c0, H, W, c0, 1, nullptr, x0);
    dl_run3(c, 3, x0, c0, H, W, c1, 2, nullptr, x1);
}

static void dl_walk(DlaCtx& c, const void* image, int in_type, int H, int W, const int* levels, const int* ch, void* const* out,
                    int out_type) {
    float* x1 = dl_alloc(c, (long long)c.N * ch[1] * (H / 2) * (W / 2));
    long long mark = c.bump;
    dl_stem(c, image, in_type, H, W, ch[0], ch[1], x1);
    const float* x = x1;
    int h = H / 2, w = W / 2;
    for (int k = 2; k < 6; ++k) {
        c.bump = mark;
        const int cin = ch[k - 1], cout = ch[k], ho = h / 2, wo = w / 2;
        const bool root = k > 2;
        // a half output map that the next level reads: its fp32 twin lives below the mark until that level is done
        float* out32 = (out_type != SMOT_FEAT_F32 && k < 5) ? dl_alloc(c, (long long)c.N * cout * ho * wo) : nullptr;
        const long long next_mark = c.bump;
        void* o = c.dry ? (void*)&c : out[k - 2];              // (dry: only "is there an output" is read)
        if (levels[k] == 1) {
            x = dl_tree1(c, x, cin, h, w, cout, 2, root, nullptr, 0, o, out_type, out32);
        } else {
            DlaSrc children[2];
            int nc = 0;
            if (root) children[nc++] = DlaSrc{x, cin, 1, h, w};
            const float* t = dl_tree1(c, x, cin, h, w, cout, 2, false, nullptr, 0, nullptr, 0, nullptr);
            children[nc++] = DlaSrc{t, cout, 0, ho, wo};
            x = dl_tree1(c, t, cout, ho, wo, cout, 1, false, children, nc, o, out_type, out32);
        }
        mark = next_mark;
        h = ho;
        w = wo;
    }
}

// ---- host: networks of either block type and any depth (smot_dla_net_*) -----------------------------------------------------
// The convolutions in launch order: per depth-1 tree project (if cin != cout), tree1's convolutions, tree2's, root; a deeper
// tree is its tree1 (nothing handed down) then its tree2 (cout -> cout, its root wider by what is handed: root_extra + cout).
static void dn_add_block(DlaNet& net, int block, int cin, int cout, int k3) {
    if (block == SMOT_DLA_BLOCK_BOTTLENECK) {
        const int mid = cout / 2;
        dl_add(net, net.k1, cin, mid);
        dl_add(net, k3, mid, mid);
        dl_add(net, net.k1, mid, cout);
    } else {
        dl_add(net, k3, cin, cout);
        dl_add(net, k3, cout, cout);
    }
}
static void dn_add_tree(DlaNet& net, int depth, int block, int cin, int cout, int root_extra, int k3) {
    if (depth > 1) {
        dn_add_tree(net, depth - 1, block, cin, cout, 0, k3);
        dn_add_tree(net, depth - 1, block, cout, cout, root_extra + cout, k3);
        return;
    }
    if (cin != cout) dl_add(net, net.k1, cin, cout);
    dn_add_block(net, block, cin, cout, k3);
    dn_add_block(net, block, cout, cout, k3);
    dl_add(net, net.k1, 2 * cout + root_extra, cout);
}

constexpr int DN_MAX_DEPTH = 5;                      // a root reads x2, x1, bottom and depth - 1 handed maps: 7 <= DL_MAX_SRC_RES

// ctype != 0 (SMOT_FEAT_F16 or SMOT_FEAT_BF16, checked by the caller): half compute mode: the trees' images are kinds 5 and 6
// (every tree convolution's Cin is a multiple of 32: channels[1..5], mid, and sums of them)
static int dn_net(const int* levels, const int* ch, int block, DlaNet& net, const char* who, bool split = false, int ctype = 0) {
    if (!levels || !ch) {
        set_error("%s: null pointer", who);
        return SMOT_ERR_BAD_ARG;
    }
    if (block != SMOT_DLA_BLOCK_BASIC && block != SMOT_DLA_BLOCK_BOTTLENECK) {
        set_error("%s: block = %d (SMOT_DLA_BLOCK_BASIC or SMOT_DLA_BLOCK_BOTTLENECK)", who, block);
        return SMOT_ERR_BAD_ARG;
    }
    const int step = block == SMOT_DLA_BLOCK_BOTTLENECK ? 64 : 32;     // (bottleneck: mid = cout / 2 is a multiple of 32)
    bool ok = levels[0] == 1 && levels[1] == 1 && (ch[0] == 16 || ch[0] == 32) && ch[1] >= 32 && ch[1] % 32 == 0 && ch[1] <= 1024;
    for (int k = 2; k < 6; ++k)
        ok = ok && levels[k] >= 1 && levels[k] <= DN_MAX_DEPTH && ch[k] >= step && ch[k] % step == 0 && ch[k] <= 1024;
    if (!ok) {
        set_error("%s: levels (%d,%d,%d,%d,%d,%d), channels (%d,%d,%d,%d,%d,%d) (supported: levels[0] = levels[1] = 1, levels[2..5] "
                  "in 1 .. %d; channels[0] in {16, 32}, channels[1] a multiple of 32, channels[2..5] multiples of %d, up to 1024)",
                  who, levels[0], levels[1], levels[2], levels[3], levels[4], levels[5], ch[0], ch[1], ch[2], ch[3], ch[4], ch[5],
                  DN_MAX_DEPTH, step);
        return SMOT_ERR_UNSUPPORTED;
    }
    net.n = 0;
    net.total = 0;
    net.k3 = ctype ? 5 : split ? 4 : 3;
    net.k1 = ctype ? 6 : 1;
    net.ctype = ctype;
    dl_add(net, 7, 3, ch[0]);
    dl_add(net, 3, ch[0], ch[0]);
    dl_add(net, 3, ch[0], ch[1]);
    for (int k = 2; k < 6; ++k) dn_add_tree(net, levels[k], block, ch[k - 1], ch[k], k > 2 ? ch[k - 1] : 0, net.k3);
    return SMOT_OK;
}

// One block on x [N, cin, H, W] -> out [N, cout, H / stride, W / stride] fp32, + res (res_w != 0: through the pool) before the
// last ReLU.  Its intermediate maps are released when it returns (every launch is on one stream: a later launch that reuses
// the memory runs after the ones that read it).
// The maps are of c.mt (fp32 outside half storage); x and res are of x_type and res_type: c.mt, or fp32 where they are the
// stem's x1.  (A DlaSrc carries its map as `const float*` whatever the type: the launch knows the type of its sources.)
static void dn_block(DlaCtx& c, const void* x, int x_type, int cin, int H, int W, int cout, int stride, const void* res, int res_type,
                     int res_h, int res_w, void* out) {
    const int Ho = H / stride, Wo = W / stride, k3 = c.net->k3;
    const long long mark = c.bump;
    if (c.block == SMOT_DLA_BLOCK_BOTTLENECK) {      // conv1 at the input's resolution, the stride on the 3x3, as upstream
        const int mid = cout / 2;
        void* m1 = dl_alloc_map(c, (long long)c.N * mid * H * W);
        void* m2 = dl_alloc_map(c, (long long)c.N * mid * Ho * Wo);
        const DlaSrc s1 = {(const float*)x, cin, 0, H, W}, s3 = {(const float*)m2, mid, 0, Ho, Wo};
        dl_run1(c, &s1, 1, H, W, mid, 1, m1, SMOT_FEAT_F32, nullptr, nullptr, 0, 0, x_type);
        dl_run3(c, k3, m1, mid, H, W, mid, stride, nullptr, m2, 0, 0, c.mt);
        dl_run1(c, &s3, 1, Ho, Wo, cout, 1, out, SMOT_FEAT_F32, nullptr, res, res_h, res_w, c.mt, res_type);
    } else {
        void* t = dl_alloc_map(c, (long long)c.N * cout * Ho * Wo);
        dl_run3(c, k3, x, cin, H, W, cout, stride, nullptr, t, 0, 0, x_type);
        dl_run3(c, k3, t, cout, Ho, Wo, cout, 1, res, out, res_h, res_w, c.mt, res_type);
    }
    c.bump = mark;
}

struct DlaDst {
    void* out;               // [N, cout, Ho, Wo] of out_type
    int out_type;
    float* out32;            // the same in fp32 as well, or nullptr
};

// tree(depth) on x [N, cin, H, W] -> dst, which the caller owns.  handed: what the parent handed down.  Everything the
// subtree allocates is released when its root has been written: a depth-n tree holds n - 1 tree1 results, one depth-1
// tree's maps (project, x1, x2) and one block's intermediates at a time, whatever the number of blocks.
// x is of x_type: c.mt, or fp32 for the stem's x1 under level 2 (which has no level_root: x1 joins no root, so every source of
// a root is of c.mt; x1 is read alone by a project and by tree1's first convolution, and added as a residual where cin == cout).
static void dn_tree(DlaCtx& c, int depth, const void* x, int x_type, int cin, int H, int W, int cout, int stride, bool level_root,
                    const DlaSrc* handed, int nhanded, const DlaDst& dst) {
    const int Ho = H / stride, Wo = W / stride;
    const long long on = (long long)c.N * cout * Ho * Wo, mark = c.bump;
    const DlaSrc bottom = {(const float*)x, cin, stride == 2 ? 1 : 0, H, W};
    DlaSrc src[DL_MAX_SRC_RES];
    int ns = 0;
    if (depth > 1) {
        void* t = dl_alloc_map(c, on);
        dn_tree(c, depth - 1, x, x_type, cin, H, W, cout, stride, false, nullptr, 0, DlaDst{t, SMOT_FEAT_F32, nullptr});
        if (level_root) src[ns++] = bottom;
        for (int e = 0; e < nhanded; ++e) src[ns++] = handed[e];
        src[ns++] = DlaSrc{(const float*)t, cout, 0, Ho, Wo};
        dn_tree(c, depth - 1, t, c.mt, cout, Ho, Wo, cout, 1, false, src, ns, dst);
        c.bump = mark;
        return;
    }
    const void* residual = x;
    int res_type = x_type;
    if (cin != cout) {
        void* r = dl_alloc_map(c, on);
        dl_run1(c, &bottom, 1, Ho, Wo, cout, 0, r, SMOT_FEAT_F32, nullptr, nullptr, 0, 0, x_type);
        residual = r;
        res_type = c.mt;
    }
    // (cin == cout at stride 2: the residual is the pooled input itself, read through the pool)
    const bool rpool = cin == cout && stride == 2;
    void* x1 = dl_alloc_map(c, on);
    void* x2 = dl_alloc_map(c, on);
    dn_block(c, x, x_type, cin, H, W, cout, stride, residual, res_type, rpool ? H : 0, rpool ? W : 0, x1);
    dn_block(c, x1, c.mt, cout, Ho, Wo, cout, 1, x1, c.mt, 0, 0, x2);
    src[ns++] = DlaSrc{(const float*)x2, cout, 0, Ho, Wo};
    src[ns++] = DlaSrc{(const float*)x1, cout, 0, Ho, Wo};
    if (level_root) src[ns++] = bottom;
    for (int e = 0; e < nhanded; ++e) src[ns++] = handed[e];
    dl_run1(c, src, ns, Ho, Wo, cout, 1, dst.out, dst.out_type, dst.out32, c.rroot ? x2 : nullptr, 0, 0, c.mt, c.mt);
    c.bump = mark;
}

// dl_walk for these networks.  Below the levels' mark live x1 and, for half outputs, the fp32 twins the next level reads.
static void dn_walk(DlaCtx& c, const void* image, int in_type, int H, int W, const int* levels, const int* ch, void* const* out,
                    int out_type) {
    float* x1 = dl_alloc(c, (long long)c.N * ch[1] * (H / 2) * (W / 2));
    long long mark = c.bump;
    dl_stem(c, image, in_type, H, W, ch[0], ch[1], x1);
    const void* x = x1;
    int x_type = SMOT_FEAT_F32;
    const bool hs = c.mt != SMOT_FEAT_F32;                       // half storage: out_type is c.mt and the next level reads the
                                                                 // returned map itself: no fp32 twin exists
    int h = H / 2, w = W / 2;
    for (int k = 2; k < 6; ++k) {
        c.bump = mark;
        const int cout = ch[k], ho = h / 2, wo = w / 2;
        float* out32 = (!hs && out_type != SMOT_FEAT_F32 && k < 5) ? dl_alloc(c, (long long)c.N * cout * ho * wo) : nullptr;
        mark = c.bump;
        void* o = c.dry ? nullptr : out[k - 2];
        dn_tree(c, levels[k], x, x_type, ch[k - 1], h, w, cout, 2, k > 2, nullptr, 0, DlaDst{o, out_type, out32});
        x = hs || out_type == SMOT_FEAT_F32 ? (const void*)o : out32;
        x_type = c.mt;
        h = ho;
        w = wo;
    }
}

static int dl_f32_ptr(const void* p) { return p && ((uintptr_t)p & 3) == 0; }
// non-null and aligned for elements of `type` (SMOT_FEAT_*)
static int dl_map_ptr(const void* p, int type) { return p && ((uintptr_t)p & (type == SMOT_FEAT_F32 ? 3 : 1)) == 0; }

}  // namespace smot

using namespace smot;

// Every entry point below exists for both operand modes (include/smot_emm.h): `split` selects the trees' 3x3 kernel and
// packed image, and nothing else.
static long long dla_packed_floats_impl(const int* levels, const int* channels, bool split) {
    DlaNet net;
    if (dla_net(levels, channels, net, "dla_packed_floats", split)) return -1;
    return net.total;
}
extern "C" long long smot_dla_packed_floats(const int* levels, const int* channels) {
    return dla_packed_floats_impl(levels, channels, false);
}
extern "C" long long smot_dla_split_packed_floats(const int* levels, const int* channels) {
    return dla_packed_floats_impl(levels, channels, true);
}

static int dla_pack_net(const DlaNet& net, const float* const* w, const float* const* scale, const float* const* shift,
                        int num_convs, float* packed, smot_stream_t stream);
static int dla_pack_impl(const int* levels, const int* channels, const float* const* w, const float* const* scale,
                         const float* const* shift, int num_convs, float* packed, smot_stream_t stream, bool split) {
    DlaNet net;
    const int rn = dla_net(levels, channels, net, "dla_pack", split);
    if (rn) return rn;
    return dla_pack_net(net, w, scale, shift, num_convs, packed, stream);
}
static int dla_pack_net(const DlaNet& net, const float* const* w, const float* const* scale, const float* const* shift,
                        int num_convs, float* packed, smot_stream_t stream) {
    SMOT_REQUIRE(w && scale && shift && packed, "dla_pack: null pointer");
    SMOT_REQUIRE(num_convs == net.n, "dla_pack: %d convolutions passed, the network has %d in launch order", num_convs, net.n);
    SMOT_REQUIRE(((uintptr_t)packed & 15) == 0, "dla_pack: packed must be 16-byte aligned");
    for (int i = 0; i < net.n; ++i)
        SMOT_REQUIRE(dl_f32_ptr(w[i]) && dl_f32_ptr(scale[i]) && dl_f32_ptr(shift[i]),
                     "dla_pack: a tensor of convolution %d is null or not 4-byte aligned", i);
    for (int i = 0; i < net.n; ++i) {
        const DlaConv& c = net.conv[i];
        const int rc = dl_pack_launch(c.kind, w[i], scale[i], shift[i], c.cin, c.cout, packed + c.off, (hipStream_t)stream, net.ctype);
        if (rc) return rc;
    }
    return SMOT_OK;
}
extern "C" int smot_dla_pack(const int* levels, const int* channels, const float* const* w, const float* const* scale,
                             const float* const* shift, int num_convs, float* packed, smot_stream_t stream) {
    return dla_pack_impl(levels, channels, w, scale, shift, num_convs, packed, stream, false);
}
extern "C" int smot_dla_split_pack(const int* levels, const int* channels, const float* const* w, const float* const* scale,
                                   const float* const* shift, int num_convs, float* packed, smot_stream_t stream) {
    return dla_pack_impl(levels, channels, w, scale, shift, num_convs, packed, stream, true);
}

extern "C" long long smot_dla_ws_bytes(const int* levels, const int* channels, int num_images, int H, int W) {
    DlaNet net;
    if (dla_net(levels, channels, net, "dla_ws_bytes") || dla_size_ok(num_images, H, W, "dla_ws_bytes")) return -1;
    DlaCtx c = {};
    c.net = &net;
    c.dry = true;
    c.N = num_images;
    // (the half form: it holds the fp32 twins of the returned maps as well, an upper bound of the fp32 form)
    dl_walk(c, nullptr, SMOT_FEAT_F32, H, W, levels, channels, nullptr, SMOT_FEAT_F16);
    return c.rc ? -1 : c.peak * (long long)sizeof(float);
}

// the checks and the walk of a network that dla_net (block < 0: DlaBasic, depth <= 2, dl_walk) or dn_net (block >= 0: dn_walk)
// described with the code rn
static int dla_fwd_net(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                       const float* packed, float* ws, void* const* out, int out_type, smot_stream_t stream, const DlaNet& net,
                       int rn, int block, int residual_root, int map_type = SMOT_FEAT_F32);
static int dla_fwd_impl(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                        const float* packed, float* ws, void* const* out, int out_type, smot_stream_t stream, bool split) {
    DlaNet net;
    const int rn = dla_net(levels, channels, net, "dla", split);
    return dla_fwd_net(image, in_type, num_images, H, W, levels, channels, packed, ws, out, out_type, stream, net, rn, -1, 0);
}
static int dla_fwd_net(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                       const float* packed, float* ws, void* const* out, int out_type, smot_stream_t stream, const DlaNet& net,
                       int rn, int block, int residual_root, int map_type) {
    SMOT_REQUIRE(in_type == SMOT_FEAT_F32 || in_type == SMOT_FEAT_F16 || in_type == SMOT_FEAT_BF16,
                 "dla: in_type = %d (SMOT_FEAT_F32, _F16 or _BF16, NCHW)", in_type);
    SMOT_REQUIRE(out_type == SMOT_FEAT_F32 || out_type == SMOT_FEAT_F16 || out_type == SMOT_FEAT_BF16,
                 "dla: out_type = %d (SMOT_FEAT_F32, _F16 or _BF16)", out_type);
    if (rn == SMOT_ERR_BAD_ARG) return rn;
    SMOT_REQUIRE(num_images >= 1 && num_images <= SMOT_MAX_IMAGES, "dla: num_images = %d (1 .. %d)", num_images, SMOT_MAX_IMAGES);
    SMOT_REQUIRE(image && packed && ws && out, "dla: null pointer");
    SMOT_REQUIRE(((uintptr_t)image & (in_type == SMOT_FEAT_F32 ? 3 : 1)) == 0, "dla: the image is misaligned");
    SMOT_REQUIRE((((uintptr_t)packed | (uintptr_t)ws) & 15) == 0, "dla: packed and ws must be 16-byte aligned");
    for (int k = 0; k < 4; ++k)
        SMOT_REQUIRE(out[k] && ((uintptr_t)out[k] & (out_type == SMOT_FEAT_F32 ? 3 : 1)) == 0, "dla: output %d is null or misaligned", k);
    if (rn) return rn;
    const int rs = dla_size_ok(num_images, H, W, "dla");
    if (rs) return rs;
    long long widest = (long long)H * W * channels[0];         // the largest map of one image, in elements
    for (int k = 1; k < 6; ++k) {
        // (a bottleneck's conv1 gives channels[k] / 2 maps at its input's resolution: twice the level's own map)
        const long long m = (long long)(H >> k) * (W >> k) * channels[k] * (block == SMOT_DLA_BLOCK_BOTTLENECK && k >= 2 ? 2 : 1);
        if (m > widest) widest = m;
    }
    if (widest >= (1LL << 31) || (long long)H * W / 128 * num_images >= (1LL << 31)) {
        set_error("dla: %d images of %d x %d are beyond the kernels' 32-bit offsets", num_images, H, W);
        return SMOT_ERR_UNSUPPORTED;
    }
    DlaCtx c = {};
    c.net = &net;
    c.packed = packed;
    c.ws = ws;
    c.N = num_images;
    c.st = (hipStream_t)stream;
    c.block = block;
    c.rroot = residual_root ? 1 : 0;
    c.mt = map_type;                                 // (half storage: dn_walk alone, and out_type == map_type)
    if (block < 0) dl_walk(c, image, in_type, H, W, levels, channels, out, out_type);
    else dn_walk(c, image, in_type, H, W, levels, channels, out, out_type);
    return c.rc;
}
extern "C" int smot_dla_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                            const float* packed, float* ws, void* const* out, int out_type, smot_stream_t stream) {
    return dla_fwd_impl(image, in_type, num_images, H, W, levels, channels, packed, ws, out, out_type, stream, false);
}
// (the workspace is the fp32 mode's: smot_dla_ws_bytes)
extern "C" int smot_dla_split_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels,
                                  const int* channels, const float* packed, float* ws, void* const* out, int out_type,
                                  smot_stream_t stream) {
    return dla_fwd_impl(image, in_type, num_images, H, W, levels, channels, packed, ws, out, out_type, stream, true);
}

// ---- networks of either block type and any depth (include/smot_emm.h, DLA BACKBONE, BOTTLENECK BLOCKS AND DEEPER TREES) ----
extern "C" int smot_dla_net_num_convs(const int* levels, const int* channels, int block) {
    DlaNet net;
    if (dn_net(levels, channels, block, net, "dla_net_num_convs")) return -1;
    return net.n;
}

extern "C" long long smot_dla_net_packed_floats(const int* levels, const int* channels, int block, int residual_root, int split) {
    (void)residual_root;                             // (a residual root has no parameters of its own)
    DlaNet net;
    if (dn_net(levels, channels, block, net, "dla_net_packed_floats", split != 0)) return -1;
    return net.total;
}

extern "C" int smot_dla_net_pack(const int* levels, const int* channels, int block, int residual_root, int split,
                                 const float* const* w, const float* const* scale, const float* const* shift, int num_convs,
                                 float* packed, smot_stream_t stream) {
    (void)residual_root;
    DlaNet net;
    const int rn = dn_net(levels, channels, block, net, "dla_net_pack", split != 0);
    if (rn) return rn;
    return dla_pack_net(net, w, scale, shift, num_convs, packed, stream);
}

extern "C" long long smot_dla_net_ws_bytes(const int* levels, const int* channels, int block, int residual_root, int num_images,
                                           int H, int W) {
    DlaNet net;
    if (dn_net(levels, channels, block, net, "dla_net_ws_bytes") || dla_size_ok(num_images, H, W, "dla_net_ws_bytes")) return -1;
    DlaCtx c = {};
    c.net = &net;
    c.dry = true;
    c.N = num_images;
    c.block = block;
    c.rroot = residual_root ? 1 : 0;
    // (the half form, as smot_dla_ws_bytes: an upper bound of the fp32 form)
    dn_walk(c, nullptr, SMOT_FEAT_F32, H, W, levels, channels, nullptr, SMOT_FEAT_F16);
    return c.rc ? -1 : c.peak * (long long)sizeof(float);
}

extern "C" int smot_dla_net_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels, const int* channels,
                                int block, int residual_root, int split, const float* packed, float* ws, void* const* out,
                                int out_type, smot_stream_t stream) {
    DlaNet net;
    const int rn = dn_net(levels, channels, block, net, "dla_net", split != 0);
    return dla_fwd_net(image, in_type, num_images, H, W, levels, channels, packed, ws, out, out_type, stream, net, rn,
                       rn == SMOT_ERR_BAD_ARG ? 0 : block, residual_root);
}

// ---- the three operators alone -------------------------------------------------------------------------------------------------
// hs: half storage (ctype != 0): x of in_type, residual of res_type, out of ctype; otherwise all three are fp32
static int dla_conv3x3_impl(const void* x, int num_images, int Cin, int H, int W, const float* w, const float* scale,
                            const float* shift, int Cout, int stride, const void* residual, int residual_h, int residual_w,
                            int relu, float* packed, void* out, smot_stream_t stream, bool split, int ctype = 0, bool hs = false,
                            int in_type = SMOT_FEAT_F32, int res_type = SMOT_FEAT_F32) {
    SMOT_REQUIRE(dl_map_ptr(x, in_type) && dl_f32_ptr(w) && dl_f32_ptr(scale) && dl_f32_ptr(shift) &&
                     dl_map_ptr(out, hs ? ctype : SMOT_FEAT_F32) && (!residual || dl_map_ptr(residual, res_type)),
                 "dla_conv3x3: a null or misaligned pointer");
    SMOT_REQUIRE(packed && ((uintptr_t)packed & 15) == 0, "dla_conv3x3: packed must be 16-byte aligned");
    SMOT_REQUIRE(num_images >= 1 && num_images <= SMOT_MAX_IMAGES && H >= 1 && W >= 1 && (stride == 1 || stride == 2),
                 "dla_conv3x3: %d images of %d x %d, stride %d", num_images, H, W, stride);
    const int Ho = stride == 2 ? (H - 1) / 2 + 1 : H, Wo = stride == 2 ? (W - 1) / 2 + 1 : W;
    const bool rpool = residual && (residual_h != 0 || residual_w != 0);
    SMOT_REQUIRE(!rpool || (residual_h / 2 == Ho && residual_w / 2 == Wo),
                 "dla_conv3x3: a pooled residual of %d x %d for an output of %d x %d", residual_h, residual_w, Ho, Wo);
    const int cstep = split || ctype ? CVS_IC : CV_IC;
    if (Cin < cstep || Cin % cstep != 0 || Cin > 1024 || Cout < 16 || Cout % 16 != 0 || (Cout > 16 && Cout % 32 != 0) || Cout > 1024) {
        set_error("dla_conv3x3: Cin = %d, Cout = %d (supported: Cin a multiple of %d, Cout 16 or a multiple of 32, up to 1024)", Cin,
                  Cout, cstep);
        return SMOT_ERR_UNSUPPORTED;
    }
    if ((long long)H * W * (Cin > Cout ? Cin : Cout) >= (1LL << 31) || (long long)H * W / 128 * num_images >= (1LL << 31) ||
        (rpool && (long long)residual_h * residual_w * Cout >= (1LL << 31))) {
        set_error("dla_conv3x3: %d images of %d x %d are beyond the kernel's 32-bit offsets", num_images, H, W);
        return SMOT_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const int rp = dl_pack_launch(ctype ? 5 : split ? 4 : 3, w, scale, shift, Cin, Cout, packed, st, ctype);
    if (rp) return rp;
    if (hs)
        return dl_conv3_hs(x, in_type, num_images, Cin, H, W, packed, Cout, stride, residual, res_type, relu ? 1 : 0, out, st,
                           rpool ? residual_h : 0, rpool ? residual_w : 0, ctype);
    return dl_conv3((const float*)x, num_images, Cin, H, W, packed, Cout, stride, (const float*)residual, relu ? 1 : 0, (float*)out,
                    st, rpool ? residual_h : 0, rpool ? residual_w : 0, split, ctype);
}
extern "C" int smot_dla_conv3x3_fwd(const float* x, int num_images, int Cin, int H, int W, const float* w, const float* scale,
                                    const float* shift, int Cout, int stride, const float* residual, int residual_h,
                                    int residual_w, int relu, float* packed, float* out, smot_stream_t stream) {
    return dla_conv3x3_impl(x, num_images, Cin, H, W, w, scale, shift, Cout, stride, residual, residual_h, residual_w, relu, packed,
                            out, stream, false);
}
extern "C" int smot_dla_conv3x3_split_fwd(const float* x, int num_images, int Cin, int H, int W, const float* w,
                                          const float* scale, const float* shift, int Cout, int stride, const float* residual,
                                          int residual_h, int residual_w, int relu, float* packed, float* out,
                                          smot_stream_t stream) {
    return dla_conv3x3_impl(x, num_images, Cin, H, W, w, scale, shift, Cout, stride, residual, residual_h, residual_w, relu, packed,
                            out, stream, true);
}

// (both modes pick the wave split by dl_conv3_wr: the split twin answers for its own launch site)
extern "C" int smot_dla_conv3x3_split_form(int num_images, int H, int W, int Cout, int stride) {
    return smot_dla_conv3x3_form(num_images, H, W, Cout, stride);
}

extern "C" int smot_dla_conv3x3_form(int num_images, int H, int W, int Cout, int stride) {
    if (num_images < 1 || H < 1 || W < 1 || Cout < 16 || (stride != 1 && stride != 2)) return -1;
    const int Ho = stride == 2 ? (H - 1) / 2 + 1 : H, Wo = stride == 2 ? (W - 1) / 2 + 1 : W;
    const long long tiles = (long long)((Wo + CV_TW - 1) / CV_TW) * ((Ho + CV_TH - 1) / CV_TH) * num_images;
    return 10 * dl_conv3_wr(stride, Cout, tiles) + (Cout <= 16 ? 1 : 2);
}

extern "C" long long smot_dla_conv_packed_floats(int kernel_size, int Cin, int Cout) {
    if ((kernel_size != 1 && kernel_size != 3 && kernel_size != 7) || Cin < 1 || Cout < 16 || Cout % 16 != 0) return -1;
    if (kernel_size == 3 && Cin % 8 != 0) return -1;
    if (kernel_size == 1 && Cin % 16 != 0) return -1;
    return dl_conv_floats(kernel_size, Cin, Cout);
}

// the same in split mode: the 3x3 image is kind 4 (Cin % 32 == 0); the 1x1 and 7x7 images are the fp32 mode's
extern "C" long long smot_dla_conv_split_packed_floats(int kernel_size, int Cin, int Cout) {
    if (kernel_size != 3) return smot_dla_conv_packed_floats(kernel_size, Cin, Cout);
    if (Cin < 1 || Cin % CVS_IC != 0 || Cout < 16 || Cout % 16 != 0) return -1;
    return dl_conv_floats(4, Cin, Cout);
}

// max_sources: 4 for smot_dla_conv1x1_fwd (no residual), 8 for smot_dla_conv1x1_res_fwd; ctype != 0: half compute mode (every
// source a multiple of 32 channels, the kind-6 image, dla_conv1x1_half_kernel)
// hs: half storage (ctype != 0): every source of in_type, residual of res_type, out_type == ctype
static int dla_conv1x1_impl(const void* const* sources, const int* source_channels, const int* source_pooled,
                            const int* source_heights, const int* source_widths, int num_sources, int max_sources, int num_images,
                            int H, int W, const float* w, const float* scale, const float* shift, int Cout, int relu,
                            const void* residual, int residual_h, int residual_w, float* packed, void* out, int out_type,
                            smot_stream_t stream, int ctype = 0, bool hs = false, int in_type = SMOT_FEAT_F32,
                            int res_type = SMOT_FEAT_F32) {
    SMOT_REQUIRE(out_type == SMOT_FEAT_F32 || out_type == SMOT_FEAT_F16 || out_type == SMOT_FEAT_BF16,
                 "dla_conv1x1: out_type = %d (SMOT_FEAT_F32, _F16 or _BF16)", out_type);
    SMOT_REQUIRE(num_sources >= 1 && num_sources <= max_sources, "dla_conv1x1: %d sources (1 .. %d)", num_sources, max_sources);
    SMOT_REQUIRE(!residual || dl_map_ptr(residual, res_type), "dla_conv1x1: the residual is misaligned");
    const bool rpool = residual && (residual_h != 0 || residual_w != 0);
    SMOT_REQUIRE(!rpool || (residual_h / 2 == H && residual_w / 2 == W),
                 "dla_conv1x1: a pooled residual of %d x %d for an output of %d x %d", residual_h, residual_w, H, W);
    SMOT_REQUIRE(sources && source_channels && source_pooled && source_heights && source_widths, "dla_conv1x1: null pointer");
    SMOT_REQUIRE(dl_f32_ptr(w) && dl_f32_ptr(scale) && dl_f32_ptr(shift), "dla_conv1x1: a null or misaligned pointer");
    SMOT_REQUIRE(out && ((uintptr_t)out & (out_type == SMOT_FEAT_F32 ? 3 : 1)) == 0, "dla_conv1x1: the output is null or misaligned");
    SMOT_REQUIRE(packed && ((uintptr_t)packed & 15) == 0, "dla_conv1x1: packed must be 16-byte aligned");
    SMOT_REQUIRE(num_images >= 1 && num_images <= SMOT_MAX_IMAGES && H >= 1 && W >= 1, "dla_conv1x1: %d images of %d x %d",
                 num_images, H, W);
    DlaSrc src[DL_MAX_SRC_RES];
    long long K = 0;
    bool ok = Cout >= 32 && Cout % 32 == 0 && Cout <= 1024 && !(rpool && (long long)residual_h * residual_w * Cout >= (1LL << 31));
    for (int s = 0; s < num_sources; ++s) {
        SMOT_REQUIRE(dl_map_ptr(sources[s], in_type), "dla_conv1x1: source %d is null or misaligned", s);
        const int pooled = source_pooled[s] ? 1 : 0, hsrc = source_heights[s], wsrc = source_widths[s];
        SMOT_REQUIRE(pooled ? (hsrc / 2 == H && wsrc / 2 == W) : (hsrc == H && wsrc == W),
                     "dla_conv1x1: source %d is %d x %d for an output of %d x %d (pooled: %d)", s, hsrc, wsrc, H, W, pooled);
        src[s] = DlaSrc{(const float*)sources[s], source_channels[s], pooled, hsrc, wsrc};
        ok = ok && source_channels[s] >= 16 && source_channels[s] % 16 == 0 && source_channels[s] <= 1024;
        K += source_channels[s] > 0 ? source_channels[s] : 0;
        if (ctype && source_channels[s] % 32 != 0) {
            set_error("dla_conv1x1_half: source %d has %d channels (supported: every source a multiple of 32 channels: a K step "
                      "of the 16-bit matrix instruction is 32 channels of one source)", s, source_channels[s]);
            return SMOT_ERR_UNSUPPORTED;
        }
        if ((long long)hsrc * wsrc * (source_channels[s] > 0 ? source_channels[s] : 1) >= (1LL << 31)) ok = false;
    }
    if (!ok || (long long)H * W * Cout >= (1LL << 31) || (long long)H * W / 64 * num_images >= (1LL << 31)) {
        set_error("dla_conv1x1: Cout = %d over %lld concatenated channels (supported: Cout a multiple of 32 up to 1024, every source a "
                  "multiple of 16 channels up to 1024, maps within 32-bit offsets)", Cout, K);
        return SMOT_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const int rp = dl_pack_launch(ctype ? 6 : 1, w, scale, shift, (int)K, Cout, packed, st, ctype);
    if (rp) return rp;
    if (hs)
        return dl_conv1_hs(src, num_sources, in_type, num_images, H, W, packed, Cout, relu ? 1 : 0, out, st, residual, res_type,
                           rpool ? residual_h : 0, rpool ? residual_w : 0, ctype);
    if (ctype)
        return dl_conv1_half(src, num_sources, num_images, H, W, packed, Cout, relu ? 1 : 0, out, out_type, nullptr, st,
                             (const float*)residual, rpool ? residual_h : 0, rpool ? residual_w : 0, ctype);
    return dl_conv1(src, num_sources, num_images, H, W, packed, Cout, relu ? 1 : 0, out, out_type, nullptr, st,
                    (const float*)residual, rpool ? residual_h : 0, rpool ? residual_w : 0);
}
extern "C" int smot_dla_conv1x1_fwd(const float* const* sources, const int* source_channels, const int* source_pooled,
                                    const int* source_heights, const int* source_widths, int num_sources, int num_images, int H,
                                    int W, const float* w, const float* scale, const float* shift, int Cout, int relu,
                                    float* packed, void* out, int out_type, smot_stream_t stream) {
    return dla_conv1x1_impl((const void* const*)sources, source_channels, source_pooled, source_heights, source_widths, num_sources, DL_MAX_SRC,
                            num_images, H, W, w, scale, shift, Cout, relu, nullptr, 0, 0, packed, out, out_type, stream);
}
extern "C" int smot_dla_conv1x1_res_fwd(const float* const* sources, const int* source_channels, const int* source_pooled,
                                        const int* source_heights, const int* source_widths, int num_sources, int num_images,
                                        int H, int W, const float* w, const float* scale, const float* shift, int Cout, int relu,
                                        const float* residual, int residual_h, int residual_w, float* packed, void* out,
                                        int out_type, smot_stream_t stream) {
    return dla_conv1x1_impl((const void* const*)sources, source_channels, source_pooled, source_heights, source_widths, num_sources, DL_MAX_SRC_RES,
                            num_images, H, W, w, scale, shift, Cout, relu, residual, residual_h, residual_w, packed, out, out_type,
                            stream);
}

// ---- half compute mode (include/smot_emm.h, DLA BACKBONE, HALF COMPUTE) ---------------------------------------------------------
static bool dl_ctype_ok(int t) { return t == SMOT_FEAT_F16 || t == SMOT_FEAT_BF16; }

extern "C" long long smot_dla_half_packed_floats(const int* levels, const int* channels, int block, int residual_root,
                                                 int compute_type) {
    (void)residual_root;
    DlaNet net;
    if (!dl_ctype_ok(compute_type)) {
        set_error("dla_half_packed_floats: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
        return -1;
    }
    if (dn_net(levels, channels, block, net, "dla_half_packed_floats", false, compute_type)) return -1;
    return net.total;
}

extern "C" int smot_dla_half_pack(const int* levels, const int* channels, int block, int residual_root, int compute_type,
                                  const float* const* w, const float* const* scale, const float* const* shift, int num_convs,
                                  float* packed, smot_stream_t stream) {
    (void)residual_root;
    SMOT_REQUIRE(dl_ctype_ok(compute_type), "dla_half_pack: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
    DlaNet net;
    const int rn = dn_net(levels, channels, block, net, "dla_half_pack", false, compute_type);
    if (rn) return rn;
    return dla_pack_net(net, w, scale, shift, num_convs, packed, stream);
}

// (the workspace is the fp32 mode's: smot_dla_net_ws_bytes)
extern "C" int smot_dla_half_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels,
                                 const int* channels, int block, int residual_root, int compute_type, const float* packed,
                                 float* ws, void* const* out, int out_type, smot_stream_t stream) {
    SMOT_REQUIRE(dl_ctype_ok(compute_type), "dla_half: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
    DlaNet net;
    const int rn = dn_net(levels, channels, block, net, "dla_half", false, compute_type);
    return dla_fwd_net(image, in_type, num_images, H, W, levels, channels, packed, ws, out, out_type, stream, net, rn,
                       rn == SMOT_ERR_BAD_ARG ? 0 : block, residual_root);
}

extern "C" long long smot_dla_conv_half_packed_floats(int kernel_size, int Cin, int Cout) {
    if (kernel_size == 7) return smot_dla_conv_packed_floats(kernel_size, Cin, Cout);
    if ((kernel_size != 1 && kernel_size != 3) || Cin < 1 || Cin % 32 != 0 || Cout < 16 || Cout % 16 != 0) return -1;
    return dl_conv_floats(kernel_size == 3 ? 5 : 6, Cin, Cout);
}

extern "C" int smot_dla_conv3x3_half_form(int num_images, int H, int W, int Cout, int stride) {
    return smot_dla_conv3x3_form(num_images, H, W, Cout, stride);
}

// -> the M-tiles per workgroup (2 or 4) that smot_dla_conv1x1_half_fwd runs for this output
extern "C" int smot_dla_conv1x1_half_form(int num_images, int H, int W, int Cout) {
    if (num_images < 1 || H < 1 || W < 1 || Cout < 32 || Cout % 32 != 0) return -1;
    return dl_conv1_half_mt(Cout, (((long long)H * W + DL_POS - 1) / DL_POS) * num_images);
}

extern "C" int smot_dla_conv3x3_half_fwd(const float* x, int num_images, int Cin, int H, int W, const float* w, const float* scale,
                                         const float* shift, int Cout, int stride, const float* residual, int residual_h,
                                         int residual_w, int relu, int compute_type, float* packed, float* out,
                                         smot_stream_t stream) {
    SMOT_REQUIRE(dl_ctype_ok(compute_type), "dla_conv3x3_half: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
    return dla_conv3x3_impl(x, num_images, Cin, H, W, w, scale, shift, Cout, stride, residual, residual_h, residual_w, relu, packed,
                            out, stream, false, compute_type);
}

extern "C" int smot_dla_conv1x1_half_fwd(const float* const* sources, const int* source_channels, const int* source_pooled,
                                         const int* source_heights, const int* source_widths, int num_sources, int num_images,
                                         int H, int W, const float* w, const float* scale, const float* shift, int Cout, int relu,
                                         const float* residual, int residual_h, int residual_w, int compute_type, float* packed,
                                         void* out, int out_type, smot_stream_t stream) {
    SMOT_REQUIRE(dl_ctype_ok(compute_type), "dla_conv1x1_half: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
    return dla_conv1x1_impl((const void* const*)sources, source_channels, source_pooled, source_heights, source_widths, num_sources, DL_MAX_SRC_RES,
                            num_images, H, W, w, scale, shift, Cout, relu, residual, residual_h, residual_w, packed, out, out_type,
                            stream, compute_type);
}

// ---- half storage (include/smot_emm.h, DLA BACKBONE, HALF STORAGE) ---------------------------------------------------------------
// fp32 or the compute type
static bool dl_hs_type_ok(int t, int ctype) { return t == SMOT_FEAT_F32 || t == ctype; }

extern "C" long long smot_dla_half_storage_ws_bytes(const int* levels, const int* channels, int block, int residual_root,
                                                    int compute_type, int num_images, int H, int W) {
    if (!dl_ctype_ok(compute_type)) {
        set_error("dla_half_storage_ws_bytes: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
        return -1;
    }
    DlaNet net;
    if (dn_net(levels, channels, block, net, "dla_half_storage_ws_bytes", false, compute_type) ||
        dla_size_ok(num_images, H, W, "dla_half_storage_ws_bytes"))
        return -1;
    DlaCtx c = {};
    c.net = &net;
    c.dry = true;
    c.N = num_images;
    c.block = block;
    c.rroot = residual_root ? 1 : 0;
    c.mt = compute_type;
    dn_walk(c, nullptr, SMOT_FEAT_F32, H, W, levels, channels, nullptr, compute_type);
    return c.rc ? -1 : c.peak * (long long)sizeof(float);
}

extern "C" int smot_dla_half_storage_fwd(const void* image, int in_type, int num_images, int H, int W, const int* levels,
                                         const int* channels, int block, int residual_root, int compute_type, const float* packed,
                                         float* ws, void* const* out, smot_stream_t stream) {
    SMOT_REQUIRE(dl_ctype_ok(compute_type), "dla_half_storage: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
    DlaNet net;
    const int rn = dn_net(levels, channels, block, net, "dla_half_storage", false, compute_type);
    return dla_fwd_net(image, in_type, num_images, H, W, levels, channels, packed, ws, out, compute_type, stream, net, rn,
                       rn == SMOT_ERR_BAD_ARG ? 0 : block, residual_root, compute_type);
}

extern "C" int smot_dla_conv3x3_half_storage_fwd(const void* x, int in_type, int num_images, int Cin, int H, int W, const float* w,
                                                 const float* scale, const float* shift, int Cout, int stride,
                                                 const void* residual, int res_type, int residual_h, int residual_w, int relu,
                                                 int compute_type, float* packed, void* out, smot_stream_t stream) {
    SMOT_REQUIRE(dl_ctype_ok(compute_type), "dla_conv3x3_half_storage: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)",
                 compute_type);
    SMOT_REQUIRE(dl_hs_type_ok(in_type, compute_type) && (!residual || dl_hs_type_ok(res_type, compute_type)),
                 "dla_conv3x3_half_storage: in_type = %d, res_type = %d (each SMOT_FEAT_F32 or the compute type %d)", in_type,
                 res_type, compute_type);
    return dla_conv3x3_impl(x, num_images, Cin, H, W, w, scale, shift, Cout, stride, residual, residual_h, residual_w, relu, packed,
                            out, stream, false, compute_type, true, in_type, residual ? res_type : SMOT_FEAT_F32);
}

extern "C" int smot_dla_conv1x1_half_storage_fwd(const void* const* sources, int in_type, const int* source_channels,
                                                 const int* source_pooled, const int* source_heights, const int* source_widths,
                                                 int num_sources, int num_images, int H, int W, const float* w, const float* scale,
                                                 const float* shift, int Cout, int relu, const void* residual, int res_type,
                                                 int residual_h, int residual_w, int compute_type, float* packed, void* out,
                                                 smot_stream_t stream) {
    SMOT_REQUIRE(dl_ctype_ok(compute_type), "dla_conv1x1_half_storage: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)",
                 compute_type);
    SMOT_REQUIRE(dl_hs_type_ok(in_type, compute_type) && (!residual || dl_hs_type_ok(res_type, compute_type)),
                 "dla_conv1x1_half_storage: in_type = %d, res_type = %d (each SMOT_FEAT_F32 or the compute type %d)", in_type,
                 res_type, compute_type);
    return dla_conv1x1_impl(sources, source_channels, source_pooled, source_heights, source_widths, num_sources, DL_MAX_SRC_RES,
                            num_images, H, W, w, scale, shift, Cout, relu, residual, residual_h, residual_w, packed, out,
                            compute_type, stream, compute_type, true, in_type, residual ? res_type : SMOT_FEAT_F32);
}

extern "C" long long smot_dla_stem_ws_bytes(int num_images, int H, int W, int c0, int c1) {
    if (num_images < 1 || num_images > SMOT_MAX_IMAGES || H < 1 || W < 1 || c0 < 1 || c1 < 1) return -1;
    const long long n0 = ((long long)num_images * c0 * H * W + 3) & ~3LL;
    const long long packed = dl_conv_floats(7, 3, c0) + dl_conv_floats(3, c0, c0) + dl_conv_floats(3, c0, c1);
    return (2 * n0 + packed) * (long long)sizeof(float);
}

extern "C" int smot_dla_stem_fwd(const void* image, int in_type, int num_images, int H, int W, int c0, int c1,
                                 const float* const* w, const float* const* scale, const float* const* shift, float* ws,
                                 float* out, smot_stream_t stream) {
    SMOT_REQUIRE(in_type == SMOT_FEAT_F32 || in_type == SMOT_FEAT_F16 || in_type == SMOT_FEAT_BF16,
                 "dla_stem: in_type = %d (SMOT_FEAT_F32, _F16 or _BF16, NCHW)", in_type);
    SMOT_REQUIRE(image && ((uintptr_t)image & (in_type == SMOT_FEAT_F32 ? 3 : 1)) == 0, "dla_stem: the image is null or misaligned");
    SMOT_REQUIRE(w && scale && shift && dl_f32_ptr(out), "dla_stem: a null or misaligned pointer");
    SMOT_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, "dla_stem: ws must be 16-byte aligned");
    for (int i = 0; i < 3; ++i)
        SMOT_REQUIRE(dl_f32_ptr(w[i]) && dl_f32_ptr(scale[i]) && dl_f32_ptr(shift[i]),
                     "dla_stem: a tensor of layer %d is null or not 4-byte aligned", i);
    SMOT_REQUIRE(num_images >= 1 && num_images <= SMOT_MAX_IMAGES, "dla_stem: num_images = %d (1 .. %d)", num_images, SMOT_MAX_IMAGES);
    if (!(c0 == 16 || c0 == 32) || c1 < 32 || c1 % 32 != 0 || c1 > 1024 || H < 2 || W < 2 || H % 2 != 0 || W % 2 != 0 ||
        (long long)H * W * (c0 > c1 / 4 ? c0 : c1 / 4) >= (1LL << 31) || (long long)H * W / 128 * num_images >= (1LL << 31)) {
        set_error("dla_stem: c0 = %d, c1 = %d, image %d x %d (supported: c0 in {16, 32}, c1 a multiple of 32 up to 1024, even sides "
                  "within 32-bit offsets)", c0, c1, H, W);
        return SMOT_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const int kinds[3] = {7, 3, 3}, cins[3] = {3, c0, c0}, couts[3] = {c0, c0, c1};
    DlaNet net = {};
    for (int i = 0; i < 3; ++i) dl_add(net, kinds[i], cins[i], couts[i]);
    const long long n0 = ((long long)num_images * c0 * H * W + 3) & ~3LL;
    float* packed = ws + 2 * n0;
    for (int i = 0; i < 3; ++i) {
        const int rc = dl_pack_launch(kinds[i], w[i], scale[i], shift[i], cins[i], couts[i], packed + net.conv[i].off, st);
        if (rc) return rc;
    }
    DlaCtx c = {};
    c.net = &net;
    c.packed = packed;
    c.ws = ws;
    c.N = num_images;
    c.st = st;
    dl_stem(c, image, in_type, H, W, c0, c1, out);
    return c.rc;
}
