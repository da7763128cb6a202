// Feature pyramid — [UPSTREAM] maskrcnn_benchmark FPN.forward with the top-down path resized bilinearly to the lateral's size
// (so that the stage maps need not halve exactly), for every image of a call, in num_levels + 1 launches:
//
//   last[L-1] = conv1x1(x[L-1], Wi) + bi
//   last[l]   = conv1x1(x[l], Wi) + bi + resize(last[l+1] -> (H_l, W_l))        l = L-2 .. 0     (fp32, in the workspace)
//   P[l]      = conv3x3(last[l], Wl, pad 1) + bl                                every l
//   P[L]      = P[L-1][:, :, ::2, ::2]                                          LastLevelMaxPool (max_pool2d(1, 2, 0))
//
// fpn_lateral_kernel<FT>: one launch per level, coarsest first.  A GEMM with M = C, K = Cin_l, N = the positions of all images
//   on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).  workgroup = (image, 64 consecutive positions of its
//   plane, block of 32 output channels), 4 waves; a wave owns 16 positions x the block's two M-tiles.  A operand = the
//   packed filters, one 16-byte load per M-tile and four k-steps, straight into registers; B operand = the stage map read in
//   place (one element per lane and k-step: 16 consecutive positions of four channels), widened exactly; the next 16 input
//   channels' operands are in flight while the current ones multiply.  Epilogue: + bias, + the four-tap bilinear sample of
//   last[l+1] as torch's F.interpolate(mode="bilinear", align_corners=False) evaluates it in fp32 (all four products, also
//   where a weight is 0: a non-finite coarse cell spreads as it does there), fp32 store.
// fpn_layer_kernel<OT>: the 3x3 convolutions of all levels and images in one launch on conv3x3_mfma.h's stage: workgroup =
//   (image, level, 8 x 16 tile) through a per-level prefix table in the kernel arguments, the level selects its filters in
//   the packed image.  Epilogue: + bias, store as OT (fp32, or fp16 / bf16 by round-to-nearest-even); at the last level
//   the positions with even y and x are stored a second time into P[L].
//
// An output's sum order is fixed by (Cin_l, C) and the position: it does not depend on the image's index, the number of
// images or the other levels.  LDS: 13,312 B (layer kernel), none (lateral kernel).
//
// HALF COMPUTE MODE (the smot_fpn_half_* entry points; CT = SMOT_FEAT_F16 or SMOT_FEAT_BF16): the same L + 1 launches, grids,
// workspace and epilogues with both convolutions on v_mfma_f32_16x16x32_f16 / _bf16.  Operands are rounded to CT (round to
// nearest even, torch's .to(): an fp16 value beyond 65,504 is +-inf) — activations as they are loaded and widened, filters
// once by the pack kernel — products are exact and the accumulation is fp32:
//   last[l] = conv1x1(rnd(x[l]), rnd(Wi)) + bi + resize(last[l+1])      fp32 in the workspace, fp32 mode's epilogue
//   P[l]    = conv3x3(rnd(last[l]), rnd(Wl)) + bl                       (last is rounded AGAIN as the 3x3 stage loads it)
// fpn_lateral_half_kernel<CT, FT>: fpn_lateral_kernel's grid and epilogue; K steps of 32 channels (Cin_l % 32 == 0): lane
//   (kq, xl) reads channels 8 kq .. 8 kq + 7 of its position in place and rounds them in registers, the A operand is one
//   16-byte load per M-tile from the 16-bit packed image; the next step's operands are in flight.  No LDS.
// fpn_layer_half_kernel<CT, OT>: fpn_layer_kernel's workgroup mapping, epilogue and max-pool store around conv3x3_mfma.h's
//   cvh_block<CT, float, 1, 1, 2> (chunks of 32 channels, 24,576 B of LDS).  One form: sums do not depend on the image count.
#include "conv3x3_mfma.h"

namespace smot {

constexpr int FL_POS = 64;                           // positions per workgroup: one N-tile per wave
constexpr int FL_MT = 2;                             // M-tiles (of 16 output channels) per workgroup: C % 32 == 0
constexpr int FLH_WGS = 3;                           // workgroups per CU the half layer kernel is compiled for: 146 VGPRs
                                                     // of the 168 that three waves per SIMD leave, 3 x 24,576 B of LDS

// ---- the packed image: per level [lateral A operand C Cin_l][lateral bias C][layer A operand 9 C^2][layer bias C] ----------
__host__ __device__ inline long long fp_level_floats(int Cin, int C) { return (long long)C * Cin + C + 9LL * C * C + C; }

struct FpnPackArgs {
    const float* inner_w[SMOT_MAX_LEVELS];
    const float* inner_b[SMOT_MAX_LEVELS];
    const float* layer_w[SMOT_MAX_LEVELS];
    const float* layer_b[SMOT_MAX_LEVELS];
    long long off[SMOT_MAX_LEVELS];                  // first float of the level
    int cin[SMOT_MAX_LEVELS];
    int L, C;
    long long total;
};

// lateral A operand: [M-tile m][group of four k-steps g][lane][e] -> Wi[16 m + lane % 16][16 g + 4 e + lane / 16]
__global__ void __launch_bounds__(256)
fpn_pack_kernel(FpnPackArgs P, float* __restrict__ packed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.total) return;
    int l = 0;
#pragma unroll
    for (int k = 1; k < SMOT_MAX_LEVELS; ++k)
        if (k < P.L && i >= P.off[k]) l = k;
    const int C = P.C, Cin = P.cin[l];
    long long r = i - P.off[l];
    float v;
    if (r < (long long)C * Cin) {
        const int e = (int)(r & 3), lane = (int)((r >> 2) & 63);
        const long long t = r >> 8;
        const int ng = Cin / 16;
        const int g = (int)(t % ng), m = (int)(t / ng);
        v = P.inner_w[l][(size_t)(16 * m + (lane & 15)) * Cin + 16 * g + 4 * e + (lane >> 4)];
    } else if ((r -= (long long)C * Cin) < C) {
        v = P.inner_b[l][r];
    } else if ((r -= C) < 9LL * C * C) {
        v = P.layer_w[l][cv_pack_index(r, C)];
    } else {
        v = P.layer_b[l][r - 9LL * C * C];
    }
    packed[i] = v;
}

// ---- lateral: 1x1 convolution + bias + bilinear sample of the coarser level ---------------------------------------------
struct FpnLateralArgs {
    const void* in;          // [N, Cin, H, W] of the call's element type
    const float* a;          // the level's packed A operand, then its C biases
    const float* coarse;     // last[l+1] [N, C, Hc, Wc], or nullptr at the coarsest level
    float* out;              // last[l] [N, C, H, W]
    int Cin, C, H, W, Hc, Wc;
    float scale_h, scale_w;  // float(Hc) / float(H), float(Wc) / float(W)
    int tiles_per_image;
};

// torch's source index and weights of one axis (area_pixel_compute_source_index, align_corners = false)
__device__ __forceinline__ void fp_axis(int dst, float scale, int in_size, int& i0, int& i1, float& w0, float& w1) {
    float src = sub_rn(mul_rn(scale, add_rn((float)dst, 0.5f)), 0.5f);
    if (src < 0.0f) src = 0.0f;
    i0 = min((int)src, in_size - 1);
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    w1 = fminf(fmaxf(sub_rn(src, (float)i0), 0.0f), 1.0f);
    w0 = sub_rn(1.0f, w1);
}

template <typename FT>
__global__ void __launch_bounds__(256, 4)
fpn_lateral_kernel(FpnLateralArgs P) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int C = P.C, Cin = P.Cin, HW = P.H * P.W;
    const int n = blockIdx.x / P.tiles_per_image;
    const int tile = blockIdx.x - n * P.tiles_per_image;
    const int p = tile * FL_POS + wave * 16 + xl;
    const bool live = p < HW;
    // B operand of lane (kq, xl): channel kq of the k-step at position p (a column behind the plane's end reads zeros)
    const FT* __restrict__ bp = reinterpret_cast<const FT*>(P.in) + (size_t)n * Cin * HW + (size_t)kq * HW + (live ? p : 0);
    const int ng = Cin >> 4;
    const float* __restrict__ bias = P.a + (size_t)C * Cin;

    int y0i = 0, y1i = 0, x0i = 0, x1i = 0;
    float h0 = 0.f, h1 = 0.f, w0 = 0.f, w1 = 0.f;
    const int y = live ? p / P.W : 0, x = live ? p - y * P.W : 0;
    const bool top = P.coarse != nullptr;
    if (top) {
        fp_axis(y, P.scale_h, P.Hc, y0i, y1i, h0, h1);
        fp_axis(x, P.scale_w, P.Wc, x0i, x1i, w0, w1);
    }
    const int HWc = P.Hc * P.Wc;
    const int o00 = y0i * P.Wc + x0i, o01 = y0i * P.Wc + x1i, o10 = y1i * P.Wc + x0i, o11 = y1i * P.Wc + x1i;

    const int m0 = blockIdx.y * FL_MT;                         // the workgroup's block of output channels
    const cv_f32x4* __restrict__ ap = reinterpret_cast<const cv_f32x4*>(P.a) + (size_t)m0 * ng * 64 + lane;
    cv_f32x4 acc[FL_MT];
#pragma unroll
    for (int m = 0; m < FL_MT; ++m) acc[m] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cv_f32x4 an[FL_MT], ac[FL_MT];
    float bn[4], bc[4];
    auto fetch = [&](int g) {
#pragma unroll
        for (int m = 0; m < FL_MT; ++m)
            an[m] = ap[((size_t)m * ng + g) * 64];
#pragma unroll
        for (int e = 0; e < 4; ++e) bn[e] = live ? feat_ld<FT>(bp + (size_t)(16 * g + 4 * e) * HW) : 0.0f;
    };
    fetch(0);
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
#pragma unroll
        for (int m = 0; m < FL_MT; ++m) ac[m] = an[m];
#pragma unroll
        for (int e = 0; e < 4; ++e) bc[e] = bn[e];
        if (g + 1 < ng) fetch(g + 1);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int m = 0; m < FL_MT; ++m)
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[m][e], bc[e], acc[m], 0, 0, 0);
    }
    // ---- acc[m][r] = output channel 16 (m0 + m) + 4 kq + r at position p --------------------------------------------
    // (32-bit offsets from the image's planes)
    if (live) {
        const float* __restrict__ cimg = top ? P.coarse + (size_t)n * C * HWc : nullptr;
        float* __restrict__ oimg = P.out + (size_t)n * C * HW;
#pragma unroll
        for (int m = 0; m < FL_MT; ++m) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 16 * (m0 + m) + 4 * kq + r;
                float v = add_rn(acc[m][r], bias[ch]);
                if (top) {
                    const int cb = ch * HWc;
                    const float v00 = cimg[cb + o00], v01 = cimg[cb + o01], v10 = cimg[cb + o10], v11 = cimg[cb + o11];
                    const float up = add_rn(mul_rn(h0, add_rn(mul_rn(w0, v00), mul_rn(w1, v01))),
                                            mul_rn(h1, add_rn(mul_rn(w0, v10), mul_rn(w1, v11))));
                    v = add_rn(v, up);
                }
                oimg[ch * HW + p] = v;
            }
        }
    }
}

// ---- layer: the 3x3 convolutions of all levels -----------------------------------------------------------------------------
struct FpnLayerLevel {
    const float* in;         // last[l] [N, C, H, W]
    void* out;               // P[l] [N, C, H, W] of the call's output type
    const float* w;          // the level's packed filters (cv_pack_index), then its C biases
    int H, W;
    int tiles_x;
    int tile0;               // tiles of the levels before this one (per image)
};
struct FpnLayerArgs {
    FpnLayerLevel lv[SMOT_MAX_LEVELS];
    void* top;               // P[L] [N, C, (H + 1) / 2, (W + 1) / 2] of the last level, or nullptr
    int L, C, tiles_per_image;
};

template <typename OT>
__global__ void __launch_bounds__(256, 2)
fpn_layer_kernel(FpnLayerArgs P) {
    __shared__ __attribute__((aligned(16))) float sm[CV_SMEM_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int C = P.C;

    // flat workgroup index -> (image, level, tile)
    const int n = blockIdx.x / P.tiles_per_image;
    const int rem = blockIdx.x - n * P.tiles_per_image;
    FpnLayerLevel lv = P.lv[0];
    bool last = P.L == 1;
#pragma unroll
    for (int k = 1; k < SMOT_MAX_LEVELS; ++k)
        if (k < P.L && rem >= P.lv[k].tile0) {
            lv = P.lv[k];
            last = k == P.L - 1;
        }
    const int t = rem - lv.tile0;
    const int ty = t / lv.tiles_x, tx = t - ty * lv.tiles_x;
    const int y0 = ty * CV_TH, x0 = tx * CV_TW;
    const int H = lv.H, W = lv.W, HW = H * W;
    const float* __restrict__ in = lv.in + (size_t)n * C * HW;
    const float* __restrict__ bias = lv.w + 9 * (size_t)C * C;
    OT* __restrict__ out = reinterpret_cast<OT*>(lv.out) + (size_t)n * C * HW;
    const bool pool = last && P.top != nullptr;
    const int Wt = (W + 1) >> 1, HWt = ((H + 1) >> 1) * Wt;
    OT* __restrict__ topo = reinterpret_cast<OT*>(P.top) + (size_t)n * C * HWt;

    CvPlan pl;
    cv_plan(pl, tid, y0, x0, H, W);
    const int npairs = C >> 5, nmb = (npairs + 3) >> 2;
    const int x = x0 + xl;
    for (int mb = 0; mb < nmb; ++mb) {
        const int pair = mb * 4 + wave;
        const bool active = pair < npairs;                 // wave-uniform: C % 128 != 0 leaves waves of the last block idle
        cv_f32x4 acc[2][CV_TH];
        cv_block<float>(sm, in, HW, C, pl, lv.w, pair, active, tid, acc);
        if (active && x < W) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ch = 32 * pair + 16 * m + 4 * kq + r;
                    const float bv = bias[ch];
#pragma unroll
                    for (int nt = 0; nt < CV_TH; ++nt) {
                        const int y = y0 + nt;
                        if (y < H) {
                            const float v = add_rn(acc[m][nt][r], bv);
                            cv_store<OT>(out + (size_t)ch * HW + y * W + x, v);
                            if (pool && !((y | x) & 1)) cv_store<OT>(topo + (size_t)ch * HWt + (y >> 1) * Wt + (x >> 1), v);
                        }
                    }
                }
        }
    }
}

// ---- half compute mode ----------------------------------------------------------------------------------------------------------
// the half packed image: per level [lateral A operand C Cin_l / 2 dwords][lateral bias C][cvh_pack_index image of the layer's
// filters][layer bias C]: 16-bit operands two to a dword stored through the float as bits, biases fp32
__host__ __device__ inline long long fph_level_floats(int Cin, int C) {
    return (long long)C * Cin / 2 + C + cvh_packed_floats(C, C) + C;
}

// lateral A operand: [M-tile m][K step g][lane][e] -> the halves Wi[16 m + lane % 16][32 g + 8 (lane / 16) + 2 e, + 1]: the
// lane's A fragment of v_mfma_f32_16x16x32_f16 / _bf16
template <int CT>
__global__ void __launch_bounds__(256)
fpn_half_pack_kernel(FpnPackArgs P, float* __restrict__ packed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.total) return;
    int l = 0;
#pragma unroll
    for (int k = 1; k < SMOT_MAX_LEVELS; ++k)
        if (k < P.L && i >= P.off[k]) l = k;
    const int C = P.C, Cin = P.cin[l];
    long long r = i - P.off[l];
    const long long na = (long long)C * Cin / 2, nl = cvh_packed_floats(C, C);
    float v;
    if (r < na) {
        const int e = (int)(r & 3), lane = (int)((r >> 2) & 63);
        const long long t = r >> 8;
        const int ng = Cin / 32;
        const int g = (int)(t % ng), m = (int)(t / ng);
        const float* __restrict__ q = P.inner_w[l] + (size_t)(16 * m + (lane & 15)) * Cin + 32 * g + 8 * (lane >> 4) + 2 * e;
        v = __uint_as_float(cvh_pack2<CT>(q[0], q[1]));
    } else if ((r -= na) < C) {
        v = P.inner_b[l][r];
    } else if ((r -= C) < nl) {
        const long long s = cvh_pack_index(r, C, C);         // (C % 32 == 0: no padded pair, s >= 0)
        v = __uint_as_float(cvh_pack2<CT>(P.layer_w[l][s], P.layer_w[l][s + 9]));
    } else {
        v = P.layer_b[l][r - nl];
    }
    packed[i] = v;
}

// P.a: the level's half A operand, then its C biases (fp32)
template <int CT, typename FT>
__global__ void __launch_bounds__(256, 4)
fpn_lateral_half_kernel(FpnLateralArgs P) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int C = P.C, Cin = P.Cin, HW = P.H * P.W;
    const int n = blockIdx.x / P.tiles_per_image;
    const int tile = blockIdx.x - n * P.tiles_per_image;
    const int p = tile * FL_POS + wave * 16 + xl;
    const bool live = p < HW;
    // B operand of lane (kq, xl): channels 8 kq .. 8 kq + 7 of the K step at position p (a column behind the plane's end: zeros)
    const FT* __restrict__ bp = reinterpret_cast<const FT*>(P.in) + (size_t)n * Cin * HW + (size_t)(8 * kq) * HW + (live ? p : 0);
    const int ng = Cin >> 5;
    const float* __restrict__ bias = P.a + (size_t)C * Cin / 2;

    int y0i = 0, y1i = 0, x0i = 0, x1i = 0;
    float h0 = 0.f, h1 = 0.f, w0 = 0.f, w1 = 0.f;
    const int y = live ? p / P.W : 0, x = live ? p - y * P.W : 0;
    const bool top = P.coarse != nullptr;
    if (top) {
        fp_axis(y, P.scale_h, P.Hc, y0i, y1i, h0, h1);
        fp_axis(x, P.scale_w, P.Wc, x0i, x1i, w0, w1);
    }
    const int HWc = P.Hc * P.Wc;
    const int o00 = y0i * P.Wc + x0i, o01 = y0i * P.Wc + x1i, o10 = y1i * P.Wc + x0i, o11 = y1i * P.Wc + x1i;

    const int m0 = blockIdx.y * FL_MT;                         // the workgroup's block of output channels
    const cvs_u32x4* __restrict__ ap = reinterpret_cast<const cvs_u32x4*>(P.a) + (size_t)m0 * ng * 64 + lane;
    cv_f32x4 acc[FL_MT];
#pragma unroll
    for (int m = 0; m < FL_MT; ++m) acc[m] = (cv_f32x4){0.f, 0.f, 0.f, 0.f};
    cvs_u32x4 an[FL_MT], ac[FL_MT], bc;
    float bn[8];
    auto fetch = [&](int g) {
#pragma unroll
        for (int m = 0; m < FL_MT; ++m)
            an[m] = ap[((size_t)m * ng + g) * 64];
#pragma unroll
        for (int j = 0; j < 8; ++j) bn[j] = live ? feat_ld<FT>(bp + (size_t)(32 * g + j) * HW) : 0.0f;
    };
    fetch(0);
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
#pragma unroll
        for (int m = 0; m < FL_MT; ++m) ac[m] = an[m];
#pragma unroll
        for (int e = 0; e < 4; ++e) bc[e] = cvh_pack2<CT>(bn[2 * e], bn[2 * e + 1]);
        if (g + 1 < ng) fetch(g + 1);
#pragma unroll
        for (int m = 0; m < FL_MT; ++m) acc[m] = cvh_mfma<CT>(ac[m], bc, acc[m]);
    }
    // ---- acc[m][r] = output channel 16 (m0 + m) + 4 kq + r at position p: fpn_lateral_kernel's epilogue ---------------
    if (live) {
        const float* __restrict__ cimg = top ? P.coarse + (size_t)n * C * HWc : nullptr;
        float* __restrict__ oimg = P.out + (size_t)n * C * HW;
#pragma unroll
        for (int m = 0; m < FL_MT; ++m) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 16 * (m0 + m) + 4 * kq + r;
                float v = add_rn(acc[m][r], bias[ch]);
                if (top) {
                    const int cb = ch * HWc;
                    const float v00 = cimg[cb + o00], v01 = cimg[cb + o01], v10 = cimg[cb + o10], v11 = cimg[cb + o11];
                    const float up = add_rn(mul_rn(h0, add_rn(mul_rn(w0, v00), mul_rn(w1, v01))),
                                            mul_rn(h1, add_rn(mul_rn(w0, v10), mul_rn(w1, v11))));
                    v = add_rn(v, up);
                }
                oimg[ch * HW + p] = v;
            }
        }
    }
}

// lv.w: the level's cvh_pack_index image, then its C biases (fp32)
template <int CT, typename OT>
__global__ void __launch_bounds__(256, FLH_WGS)
fpn_layer_half_kernel(FpnLayerArgs P) {
    __shared__ __attribute__((aligned(16))) cvs_u32x4 sm[CvhGeom<1>::SMEM_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, xl = lane & 15;
    const int C = P.C;

    // flat workgroup index -> (image, level, tile)
    const int n = blockIdx.x / P.tiles_per_image;
    const int rem = blockIdx.x - n * P.tiles_per_image;
    FpnLayerLevel lv = P.lv[0];
    bool last = P.L == 1;
#pragma unroll
    for (int k = 1; k < SMOT_MAX_LEVELS; ++k)
        if (k < P.L && rem >= P.lv[k].tile0) {
            lv = P.lv[k];
            last = k == P.L - 1;
        }
    const int t = rem - lv.tile0;
    const int ty = t / lv.tiles_x, tx = t - ty * lv.tiles_x;
    const int y0 = ty * CV_TH, x0 = tx * CV_TW;
    const int H = lv.H, W = lv.W, HW = H * W;
    const float* __restrict__ in = lv.in + (size_t)n * C * HW;
    const float* __restrict__ bias = lv.w + cvh_packed_floats(C, C);
    OT* __restrict__ out = reinterpret_cast<OT*>(lv.out) + (size_t)n * C * HW;
    const bool pool = last && P.top != nullptr;
    const int Wt = (W + 1) >> 1, HWt = ((H + 1) >> 1) * Wt;
    OT* __restrict__ topo = reinterpret_cast<OT*>(P.top) + (size_t)n * C * HWt;

    CvsPlan<1> pl;
    cvs_plan<1>(pl, tid, y0, x0, H, W);
    const int npairs = C >> 5, nmb = (npairs + 3) >> 2;
    const int x = x0 + xl;
    for (int mb = 0; mb < nmb; ++mb) {
        const int pair = mb * 4 + wave;
        const bool active = pair < npairs;                 // wave-uniform: C % 128 != 0 leaves waves of the last block idle
        cv_f32x4 acc[2][CV_TH];
        cvh_block<CT, float, 1, 1, 2>(sm, in, HW, C, pl, lv.w, pair, active, tid, 0, acc);
        if (active && x < W) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ch = 32 * pair + 16 * m + 4 * kq + r;
                    const float bv = bias[ch];
#pragma unroll
                    for (int nt = 0; nt < CV_TH; ++nt) {
                        const int y = y0 + nt;
                        if (y < H) {
                            const float v = add_rn(acc[m][nt][r], bv);
                            cv_store<OT>(out + (size_t)ch * HW + y * W + x, v);
                            if (pool && !((y | x) & 1)) cv_store<OT>(topo + (size_t)ch * HWt + (y >> 1) * Wt + (x >> 1), v);
                        }
                    }
                }
        }
    }
}

static int fpn_shape(int num_levels, const int* in_channels, int C, const char* who) {
    if (num_levels < 1 || num_levels > SMOT_MAX_LEVELS - 1) {
        set_error("%s: num_levels = %d (1 .. %d)", who, num_levels, SMOT_MAX_LEVELS - 1);
        return SMOT_ERR_BAD_ARG;
    }
    if (!in_channels) {
        set_error("%s: null pointer", who);
        return SMOT_ERR_BAD_ARG;
    }
    if (C < 32 || C % 32 != 0 || C > 512) {
        set_error("%s: C = %d (supported: multiples of 32 up to 512)", who, C);
        return SMOT_ERR_UNSUPPORTED;
    }
    for (int l = 0; l < num_levels; ++l)
        if (in_channels[l] < 16 || in_channels[l] % 16 != 0 || in_channels[l] > 2048) {
            set_error("%s: Cin = %d at level %d (supported: multiples of 16 up to 2048)", who, in_channels[l], l);
            return SMOT_ERR_UNSUPPORTED;
        }
    return SMOT_OK;
}

static bool fpn_ctype_ok(int ctype) { return ctype == SMOT_FEAT_F16 || ctype == SMOT_FEAT_BF16; }

// fpn_shape + the half compute mode's K step: Cin_l % 32 == 0
static int fpn_half_shape(int num_levels, const int* in_channels, int C, const char* who) {
    const int rs = fpn_shape(num_levels, in_channels, C, who);
    if (rs) return rs;
    for (int l = 0; l < num_levels; ++l)
        if (in_channels[l] % 32 != 0) {
            set_error("%s: Cin = %d at level %d (supported in half compute mode: multiples of 32: a K step is 32 channels)", who,
                      in_channels[l], l);
            return SMOT_ERR_UNSUPPORTED;
        }
    return SMOT_OK;
}

static long long fpn_ws_offset(int l, const int* heights, const int* widths, int num_images, int C) {
    long long off = 0;
    for (int k = 0; k < l; ++k) off += ((long long)num_images * C * heights[k] * widths[k] + 3) & ~3LL;
    return off;
}

// grid = (position tiles x images, blocks of FL_MT M-tiles): the short chain per wave is what a coarse level, with few
// positions to hide latency behind, needs; an output's sum does not depend on the grid (K runs in one order).
template <typename FT>
static int fpn_lateral_launch(const FpnLateralArgs& P, int grid, hipStream_t st) {
    SMOT_LAUNCH(fpn_lateral_kernel<FT>, dim3(grid, (P.C >> 4) / FL_MT), dim3(256), 0, st, P);
    return check_launch("fpn_lateral");
}

template <typename OT>
static int fpn_layer_launch(const FpnLayerArgs& P, int grid, hipStream_t st) {
    SMOT_LAUNCH(fpn_layer_kernel<OT>, dim3(grid), dim3(256), 0, st, P);
    return check_launch("fpn_layer");
}

template <int CT, typename FT>
static int fpn_lateral_half_launch(const FpnLateralArgs& P, int grid, hipStream_t st) {
    SMOT_LAUNCH((fpn_lateral_half_kernel<CT, FT>), dim3(grid, (P.C >> 4) / FL_MT), dim3(256), 0, st, P);
    return check_launch("fpn_lateral_half");
}

template <int CT, typename OT>
static int fpn_layer_half_launch(const FpnLayerArgs& P, int grid, hipStream_t st) {
    SMOT_LAUNCH((fpn_layer_half_kernel<CT, OT>), dim3(grid), dim3(256), 0, st, P);
    return check_launch("fpn_layer_half");
}

template <int CT>
static int fpn_lateral_half_pick(const FpnLateralArgs& P, int grid, int ft, hipStream_t st) {
    return ft == SMOT_FEAT_F32   ? fpn_lateral_half_launch<CT, float>(P, grid, st)
           : ft == SMOT_FEAT_F16 ? fpn_lateral_half_launch<CT, f16_t>(P, grid, st)
                                 : fpn_lateral_half_launch<CT, bf16_t>(P, grid, st);
}

template <int CT>
static int fpn_layer_half_pick(const FpnLayerArgs& P, int grid, int out_type, hipStream_t st) {
    if (out_type == SMOT_FEAT_F32) return fpn_layer_half_launch<CT, float>(P, grid, st);
    if (out_type == SMOT_FEAT_F16) return fpn_layer_half_launch<CT, f16_t>(P, grid, st);
    return fpn_layer_half_launch<CT, bf16_t>(P, grid, st);
}

}  // namespace smot

using namespace smot;

extern "C" long long smot_fpn_packed_floats(int num_levels, const int* in_channels, int C) {
    if (fpn_shape(num_levels, in_channels, C, "fpn_packed_floats")) return -1;
    long long total = 0;
    for (int l = 0; l < num_levels; ++l) total += fp_level_floats(in_channels[l], C);
    return total;
}

extern "C" int smot_fpn_pack(const float* const* inner_w, const float* const* inner_b, const float* const* layer_w,
                             const float* const* layer_b, int num_levels, const int* in_channels, int C, float* packed,
                             smot_stream_t stream) {
    const int rs = fpn_shape(num_levels, in_channels, C, "fpn_pack");
    if (rs) return rs;
    SMOT_REQUIRE(inner_w && inner_b && layer_w && layer_b && packed, "fpn_pack: null pointer");
    SMOT_REQUIRE(((uintptr_t)packed & 15) == 0, "fpn_pack: packed must be 16-byte aligned");
    FpnPackArgs P = {};
    long long total = 0;
    for (int l = 0; l < num_levels; ++l) {
        SMOT_REQUIRE(inner_w[l] && inner_b[l] && layer_w[l] && layer_b[l], "fpn_pack: null tensor at level %d", l);
        SMOT_REQUIRE((((uintptr_t)inner_w[l] | (uintptr_t)inner_b[l] | (uintptr_t)layer_w[l] | (uintptr_t)layer_b[l]) & 3) == 0,
                     "fpn_pack: a tensor at level %d is not 4-byte aligned", l);
        P.inner_w[l] = inner_w[l];
        P.inner_b[l] = inner_b[l];
        P.layer_w[l] = layer_w[l];
        P.layer_b[l] = layer_b[l];
        P.off[l] = total;
        P.cin[l] = in_channels[l];
        total += fp_level_floats(in_channels[l], C);
    }
    P.L = num_levels;
    P.C = C;
    P.total = total;
    SMOT_LAUNCH(fpn_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, packed);
    return check_launch("fpn_pack");
}

extern "C" long long smot_fpn_ws_bytes(int num_levels, const int* heights, const int* widths, int num_images, int C) {
    if (num_levels < 1 || num_levels > SMOT_MAX_LEVELS - 1 || !heights || !widths || num_images < 1 ||
        num_images > SMOT_MAX_IMAGES || C < 1)
        return -1;
    for (int l = 0; l < num_levels; ++l)
        if (heights[l] < 1 || widths[l] < 1) return -1;
    return fpn_ws_offset(num_levels, heights, widths, num_images, C) * (long long)sizeof(float);
}

// smot_fpn_fwd (ctype 0) and smot_fpn_half_fwd (ctype SMOT_FEAT_F16 / _BF16): the same checks, geometry and launches; the
// mode selects the packed image's layout and the kernels
static int fpn_fwd(const void* const* stages, int stage_type, const int* in_channels, const int* heights, const int* widths,
                   int num_levels, int num_images, int C, const float* packed, float* ws, void* const* out, int out_type,
                   int top_block, smot_stream_t stream, int ctype, const char* who) {
    const int rf = check_feat_type(stage_type, who);
    if (rf) return rf;
    SMOT_REQUIRE(out_type == SMOT_FEAT_F32 || out_type == SMOT_FEAT_F16 || out_type == SMOT_FEAT_BF16,
                 "%s: out_type = %d (SMOT_FEAT_F32, _F16 or _BF16)", who, out_type);
    SMOT_REQUIRE(top_block == 0 || top_block == 1, "%s: top_block = %d (0: none, 1: max-pool)", who, top_block);
    SMOT_REQUIRE(num_images >= 1 && num_images <= SMOT_MAX_IMAGES, "%s: num_images = %d (1 .. %d)", who, num_images, SMOT_MAX_IMAGES);
    const int rs = ctype ? fpn_half_shape(num_levels, in_channels, C, who) : fpn_shape(num_levels, in_channels, C, who);
    if (rs == SMOT_ERR_BAD_ARG) return rs;
    SMOT_REQUIRE(stages && heights && widths && packed && ws && out, "%s: null pointer", who);
    SMOT_REQUIRE((((uintptr_t)packed | (uintptr_t)ws) & 15) == 0, "%s: packed and ws must be 16-byte aligned", who);
    const int esz = out_type == SMOT_FEAT_F32 ? 4 : 2;
    const int ssz = (stage_type & ~SMOT_FEAT_CHANNELS_LAST) == SMOT_FEAT_F32 ? 4 : 2;
    for (int l = 0; l < num_levels + top_block; ++l) {
        SMOT_REQUIRE(out[l] && ((uintptr_t)out[l] & (esz - 1)) == 0, "%s: output %d is null or misaligned", who, l);
        if (l < num_levels) {
            SMOT_REQUIRE(stages[l] && ((uintptr_t)stages[l] & (ssz - 1)) == 0, "%s: stage map %d is null or misaligned", who, l);
            SMOT_REQUIRE(heights[l] >= 1 && widths[l] >= 1, "%s: level %d is %d x %d", who, l, heights[l], widths[l]);
        }
    }
    if (rs) return rs;
    if (stage_type & SMOT_FEAT_CHANNELS_LAST) {
        set_error("%s: channels-last stage maps are not read in place (pass contiguous NCHW maps)", who);
        return SMOT_ERR_UNSUPPORTED;
    }
    FpnLayerArgs A = {};
    long long tiles = 0, poff = 0;
    for (int l = 0; l < num_levels; ++l) {
        const long long hw = (long long)heights[l] * widths[l];
        if (hw * (in_channels[l] > C ? in_channels[l] : C) >= (1LL << 31)) {
            set_error("%s: level %d (%d x %d) is beyond the kernels' 32-bit plane offsets", who, l, heights[l], widths[l]);
            return SMOT_ERR_UNSUPPORTED;
        }
        FpnLayerLevel& v = A.lv[l];
        v.in = ws + fpn_ws_offset(l, heights, widths, num_images, C);
        v.out = out[l];
        v.w = packed + poff + (ctype ? (long long)C * in_channels[l] / 2 : (long long)C * in_channels[l]) + C;
        v.H = heights[l];
        v.W = widths[l];
        v.tiles_x = (v.W + CV_TW - 1) / CV_TW;
        v.tile0 = (int)tiles;
        tiles += (long long)v.tiles_x * ((v.H + CV_TH - 1) / CV_TH);
        poff += ctype ? fph_level_floats(in_channels[l], C) : fp_level_floats(in_channels[l], C);
        if (tiles * num_images >= (1LL << 31) || ((hw + FL_POS - 1) / FL_POS) * num_images >= (1LL << 31)) {
            set_error("%s: %d images of these maps are more than 2^31 tiles", who, num_images);
            return SMOT_ERR_UNSUPPORTED;
        }
    }
    A.top = top_block ? out[num_levels] : nullptr;
    A.L = num_levels;
    A.C = C;
    A.tiles_per_image = (int)tiles;
    hipStream_t st = (hipStream_t)stream;
    const int ft = stage_type;
    for (int l = num_levels - 1; l >= 0; --l) {
        FpnLateralArgs P = {};
        P.in = stages[l];
        P.a = A.lv[l].w - ((ctype ? (long long)C * in_channels[l] / 2 : (long long)C * in_channels[l]) + C);
        P.coarse = l + 1 < num_levels ? A.lv[l + 1].in : nullptr;
        P.out = const_cast<float*>(A.lv[l].in);
        P.Cin = in_channels[l];
        P.C = C;
        P.H = heights[l];
        P.W = widths[l];
        P.Hc = l + 1 < num_levels ? heights[l + 1] : 1;
        P.Wc = l + 1 < num_levels ? widths[l + 1] : 1;
        P.scale_h = (float)P.Hc / (float)P.H;
        P.scale_w = (float)P.Wc / (float)P.W;
        P.tiles_per_image = (int)(((long long)P.H * P.W + FL_POS - 1) / FL_POS);
        const int grid = P.tiles_per_image * num_images;
        const int rc = ctype == SMOT_FEAT_F16    ? fpn_lateral_half_pick<SMOT_FEAT_F16>(P, grid, ft, st)
                       : ctype == SMOT_FEAT_BF16 ? fpn_lateral_half_pick<SMOT_FEAT_BF16>(P, grid, ft, st)
                       : ft == SMOT_FEAT_F32     ? fpn_lateral_launch<float>(P, grid, st)
                       : ft == SMOT_FEAT_F16     ? fpn_lateral_launch<f16_t>(P, grid, st)
                                                 : fpn_lateral_launch<bf16_t>(P, grid, st);
        if (rc) return rc;
    }
    const int grid = (int)(tiles * num_images);
    if (ctype == SMOT_FEAT_F16) return fpn_layer_half_pick<SMOT_FEAT_F16>(A, grid, out_type, st);
    if (ctype == SMOT_FEAT_BF16) return fpn_layer_half_pick<SMOT_FEAT_BF16>(A, grid, out_type, st);
    if (out_type == SMOT_FEAT_F32) return fpn_layer_launch<float>(A, grid, st);
    if (out_type == SMOT_FEAT_F16) return fpn_layer_launch<f16_t>(A, grid, st);
    return fpn_layer_launch<bf16_t>(A, grid, st);
}

extern "C" int smot_fpn_fwd(const void* const* stages, int stage_type, const int* in_channels, const int* heights,
                            const int* widths, int num_levels, int num_images, int C, const float* packed, float* ws,
                            void* const* out, int out_type, int top_block, smot_stream_t stream) {
    return fpn_fwd(stages, stage_type, in_channels, heights, widths, num_levels, num_images, C, packed, ws, out, out_type,
                   top_block, stream, 0, "fpn");
}

// ---- half compute mode (include/smot_emm.h, FEATURE PYRAMID, HALF COMPUTE) --------------------------------------------------------
extern "C" long long smot_fpn_half_packed_floats(int num_levels, const int* in_channels, int C, int compute_type) {
    if (!fpn_ctype_ok(compute_type)) {
        set_error("fpn_half_packed_floats: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
        return -1;
    }
    if (fpn_half_shape(num_levels, in_channels, C, "fpn_half_packed_floats")) return -1;
    long long total = 0;
    for (int l = 0; l < num_levels; ++l) total += fph_level_floats(in_channels[l], C);
    return total;
}

extern "C" int smot_fpn_half_pack(const float* const* inner_w, const float* const* inner_b, const float* const* layer_w,
                                  const float* const* layer_b, int num_levels, const int* in_channels, int C, int compute_type,
                                  float* packed, smot_stream_t stream) {
    SMOT_REQUIRE(fpn_ctype_ok(compute_type), "fpn_half_pack: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
    const int rs = fpn_half_shape(num_levels, in_channels, C, "fpn_half_pack");
    if (rs) return rs;
    SMOT_REQUIRE(inner_w && inner_b && layer_w && layer_b && packed, "fpn_half_pack: null pointer");
    SMOT_REQUIRE(((uintptr_t)packed & 15) == 0, "fpn_half_pack: packed must be 16-byte aligned");
    FpnPackArgs P = {};
    long long total = 0;
    for (int l = 0; l < num_levels; ++l) {
        SMOT_REQUIRE(inner_w[l] && inner_b[l] && layer_w[l] && layer_b[l], "fpn_half_pack: null tensor at level %d", l);
        SMOT_REQUIRE((((uintptr_t)inner_w[l] | (uintptr_t)inner_b[l] | (uintptr_t)layer_w[l] | (uintptr_t)layer_b[l]) & 3) == 0,
                     "fpn_half_pack: a tensor at level %d is not 4-byte aligned", l);
        P.inner_w[l] = inner_w[l];
        P.inner_b[l] = inner_b[l];
        P.layer_w[l] = layer_w[l];
        P.layer_b[l] = layer_b[l];
        P.off[l] = total;
        P.cin[l] = in_channels[l];
        total += fph_level_floats(in_channels[l], C);
    }
    P.L = num_levels;
    P.C = C;
    P.total = total;
    const dim3 g((unsigned)((total + 255) / 256));
    if (compute_type == SMOT_FEAT_F16)
        SMOT_LAUNCH(fpn_half_pack_kernel<SMOT_FEAT_F16>, g, dim3(256), 0, (hipStream_t)stream, P, packed);
    else
        SMOT_LAUNCH(fpn_half_pack_kernel<SMOT_FEAT_BF16>, g, dim3(256), 0, (hipStream_t)stream, P, packed);
    return check_launch("fpn_half_pack");
}

extern "C" int smot_fpn_half_fwd(const void* const* stages, int stage_type, const int* in_channels, const int* heights,
                                 const int* widths, int num_levels, int num_images, int C, int compute_type,
                                 const float* packed, float* ws, void* const* out, int out_type, int top_block,
                                 smot_stream_t stream) {
    SMOT_REQUIRE(fpn_ctype_ok(compute_type), "fpn_half: compute_type = %d (SMOT_FEAT_F16 or SMOT_FEAT_BF16)", compute_type);
    return fpn_fwd(stages, stage_type, in_channels, heights, widths, num_levels, num_images, C, packed, ws, out, out_type,
                   top_block, stream, compute_type, "fpn_half");
}
