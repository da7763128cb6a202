// Frame pre-processing on the GPU — SURVEY.md §8(f) rank 3.
//
// Replaces the per-frame CPU chain of the reference's inference entry points (demos/demo_inference.py:74-82;
// siammot/data/adapters/augmentation/build_augmentation.py:52-66, image_augmentation.py:21-50):
//   PIL.Image.resize((ow, oh), BILINEAR)  ->  ToTensor (uint8 HWC -> float CHW / 255)
//   ->  Normalize ([BGR, * 255], - mean, / std)  [UPSTREAM maskrcnn_benchmark data/transforms/transforms.py]
// in one launch that reads the uint8 RGB frame (2.8 MB at 720p instead of a 10.8 MB fp32 host-to-device copy)
// and writes the fp32 CHW network input.
//
// Bit-exact with Pillow's 8-bit resampler [THIRD PARTY: src/libImaging/Resample.c]: separable, horizontal pass
// first, triangle filter widened by the down-scaling factor, coefficients quantised to 22 fractional bits
// (the host layer computes them in double precision exactly as Pillow does and passes the integer tables),
// integer accumulation started at one half, clip to [0,255], uint8 intermediate between the passes.  An axis
// that keeps its size gets identity tables (one tap of weight 2^22), which reproduces "pass skipped".
// The float tail follows torch op by op (separately rounded / 255, * 255, - mean, / std).
//
// HBM-bound byte work (720p: 2.76 MB in, 10.8 MB out).  Workgroup = 8 output rows x 128 output columns x 3
// channels; the horizontally resampled rows the tile's vertical taps need are built once in LDS (uint8), then
// every thread resolves 4 output pixels; output stores are coalesced along x.
//
// Two kernels: preprocess_kernel (one frame, fp32 CHW out: smot_preprocess_fwd) and, below it, preprocess_batch_kernel (the
// frames of up to 16 cameras per launch, fp32 / fp16 / bf16 out, NCHW or channels-last: smot_preprocess_batch_fwd).
#include "roi_common.h"          // f16_t / bf16_t (the batched kernel's output element types)

namespace smot {

constexpr int PP_BITS = 22;
constexpr int PP_TH = 8, PP_TW = 128;

struct PreNorm {
    float mean[3], std[3];
    int to_bgr255;
};

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> PP_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ void __launch_bounds__(256)
preprocess_kernel(const unsigned char* __restrict__ frame, int H, int W, const int* __restrict__ xb,
                  const int* __restrict__ xk, int kx, const int* __restrict__ yb, const int* __restrict__ yk, int ky,
                  int OH, int OW, int max_rows, PreNorm Nn, float* __restrict__ out) {
    extern __shared__ unsigned char inter[];          // [rows][PP_TW * 3]
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * PP_TW, y0 = blockIdx.y * PP_TH;
    const int ylast = min(y0 + PP_TH, OH) - 1;
    const int r0 = yb[2 * y0];
    const int r1 = yb[2 * ylast] + yb[2 * ylast + 1];  // bounds are monotonic in y
    const int rows = min(r1 - r0, max_rows);
    const int tw = min(PP_TW, OW - x0);
    // pass 1: horizontal resampling of input rows r0..r1 for the tile's columns
    for (int e = tid; e < rows * tw * 3; e += 256) {
        const int r = e / (tw * 3);
        const int xc = e - r * (tw * 3);
        const int xl = xc / 3, c = xc - xl * 3;
        const int x = x0 + xl;
        const int first = xb[2 * x], cnt = xb[2 * x + 1];
        const unsigned char* __restrict__ src = frame + ((size_t)(r0 + r) * W + first) * 3 + c;
        const int* __restrict__ k = xk + (size_t)x * kx;
        int acc = 1 << (PP_BITS - 1);
        for (int t = 0; t < cnt; ++t) acc += (int)src[t * 3] * k[t];
        inter[r * (PP_TW * 3) + xc] = (unsigned char)clip8(acc);
    }
    __syncthreads();
    // pass 2: vertical resampling + ToTensor + Normalize
#pragma unroll
    for (int j = 0; j < PP_TH * PP_TW / 256; ++j) {
        const int o = tid + 256 * j;
        const int yl = o / PP_TW, xl = o - yl * PP_TW;
        const int y = y0 + yl, x = x0 + xl;
        if (y >= OH || x >= OW) continue;
        const int first = yb[2 * y] - r0, cnt = yb[2 * y + 1];
        const int* __restrict__ k = yk + (size_t)y * ky;
        int acc[3] = {1 << (PP_BITS - 1), 1 << (PP_BITS - 1), 1 << (PP_BITS - 1)};
        for (int t = 0; t < cnt; ++t) {
            const unsigned char* p = inter + (first + t) * (PP_TW * 3) + xl * 3;
            const int w = k[t];
            acc[0] += (int)p[0] * w;
            acc[1] += (int)p[1] * w;
            acc[2] += (int)p[2] * w;
        }
#pragma unroll
        for (int oc = 0; oc < 3; ++oc) {
            const int c = Nn.to_bgr255 ? 2 - oc : oc;
            float f = div_rn((float)clip8(acc[c]), 255.0f);
            if (Nn.to_bgr255) f = mul_rn(f, 255.0f);
            f = div_rn(sub_rn(f, Nn.mean[oc]), Nn.std[oc]);
            out[((size_t)oc * OH + y) * OW + x] = f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The frames of several cameras in one launch (smot_preprocess_batch_fwd).  Image = blockIdx.z; what differs per image
// (frame, input size, Pillow tables, LDS rows) sits in a by-value table in the kernel-argument block (16 x 64 B), what is
// one per call (output size, normalisation, output tensor) beside it.  The tile, pass 1 and the integer arithmetic of pass
// 2 are preprocess_kernel's; the fp32 tail is followed by ONE round-to-nearest-even conversion for a half output, which
// is bit for bit `fp32_result.to(dtype)`.  No atomics, no cross-workgroup state.
//
// Stores:  NCHW  out[((b*3+oc)*OH+y)*OW+x]       a thread resolves 1 (fp32) or 2 adjacent (half) pixels of a row
//          NHWC  out[((b*OH+y)*OW+x)*3+oc]       a thread resolves 1 (fp32) or 2 adjacent (half) ELEMENTS of the row's
//                                                3*tw contiguous ones (the bytes of [B,3,OH,OW] in torch.channels_last)
// so a wave always writes 256 contiguous bytes.  A half pair is stored as one dword only where its address is 4-byte
// aligned and its second element exists (odd OW / odd tile widths / odd rows of an odd-width tensor: two scalar stores).
constexpr int PP_CHUNK = 16;              // images per launch

struct PreImage {
    const unsigned char* frame;
    const int *xb, *xk, *yb, *yk;
    int H, W, kx, ky, max_rows;
};
struct PreBatch {
    PreImage img[PP_CHUNK];
};
static_assert(sizeof(PreBatch) == PP_CHUNK * 64, "16 descriptors of 64 bytes: far below the 4 KB argument block");

// fp32 -> the 16 bits of OutT, round to nearest even (what torch's .to(float16) / .to(bfloat16) do)
template <typename OutT>
__device__ __forceinline__ unsigned pp_half_bits(float f) {
    if constexpr (__is_same(OutT, f16_t)) {
        return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)f);
    } else {
        const unsigned u = __float_as_uint(f);
        if (f != f) return 0x7fc0u;
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    }
}

template <typename OutT>
__device__ __forceinline__ void pp_store1(OutT* p, float f) {
    if constexpr (sizeof(OutT) == 4) {
        *p = f;
    } else {
        p->bits = (unsigned short)pp_half_bits<OutT>(f);
    }
}

// N = 1 or 2 adjacent elements at p; `second`: element 1 exists (N == 2)
template <typename OutT, int N>
__device__ __forceinline__ void pp_store(OutT* p, const float* f, bool second) {
    if constexpr (N == 1) {
        pp_store1(p, f[0]);
    } else {
        if (second && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            *reinterpret_cast<unsigned*>(p) = pp_half_bits<OutT>(f[0]) | (pp_half_bits<OutT>(f[1]) << 16);
        } else {
            pp_store1(p, f[0]);
            if (second) pp_store1(p + 1, f[1]);
        }
    }
}

// ToTensor + Normalize of one resampled byte, every operation rounded separately as torch does
__device__ __forceinline__ float pp_tail(int acc, float mean, float std, int to_bgr255) {
    float f = div_rn((float)clip8(acc), 255.0f);
    if (to_bgr255) f = mul_rn(f, 255.0f);
    return div_rn(sub_rn(f, mean), std);
}

template <typename OutT, bool NHWC>
__global__ void __launch_bounds__(256)
preprocess_batch_kernel(OutT* __restrict__ out, int OH, int OW, int b0, PreNorm Nn, PreBatch T) {
    extern __shared__ unsigned char inter[];          // [rows][PP_TW * 3]
    const PreImage& I = T.img[blockIdx.z];
    const unsigned char* __restrict__ frame = I.frame;
    const int* __restrict__ xb = I.xb;
    const int* __restrict__ xk = I.xk;
    const int* __restrict__ yb = I.yb;
    const int* __restrict__ yk = I.yk;
    const int W = I.W, kx = I.kx, ky = I.ky;
    const size_t b = (size_t)(b0 + (int)blockIdx.z);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * PP_TW, y0 = blockIdx.y * PP_TH;
    const int ylast = min(y0 + PP_TH, OH) - 1;
    const int r0 = yb[2 * y0];
    const int r1 = yb[2 * ylast] + yb[2 * ylast + 1];  // bounds are monotonic in y
    const int rows = min(r1 - r0, I.max_rows);
    const int tw = min(PP_TW, OW - x0);
    // pass 1: horizontal resampling of input rows r0..r1 for the tile's columns
    for (int e = tid; e < rows * tw * 3; e += 256) {
        const int r = e / (tw * 3);
        const int xc = e - r * (tw * 3);
        const int xl = xc / 3, c = xc - xl * 3;
        const int x = x0 + xl;
        const int first = xb[2 * x], cnt = xb[2 * x + 1];
        const unsigned char* __restrict__ src = frame + ((size_t)(r0 + r) * W + first) * 3 + c;
        const int* __restrict__ k = xk + (size_t)x * kx;
        int acc = 1 << (PP_BITS - 1);
        for (int t = 0; t < cnt; ++t) acc += (int)src[t * 3] * k[t];
        inter[r * (PP_TW * 3) + xc] = (unsigned char)clip8(acc);
    }
    __syncthreads();
    // pass 2: vertical resampling + ToTensor + Normalize (+ one conversion)
    constexpr int N = sizeof(OutT) == 4 ? 1 : 2;      // adjacent pixels (NCHW) / elements (NHWC) per thread and step
    if constexpr (!NHWC) {
        constexpr int COLS = PP_TW / N;
#pragma unroll
        for (int j = 0; j < PP_TH * COLS / 256; ++j) {
            const int o = tid + 256 * j;
            const int yl = o / COLS, xl = (o - yl * COLS) * N;
            const int y = y0 + yl, x = x0 + xl;
            if (y >= OH || x >= OW) continue;
            const int first = yb[2 * y] - r0, cnt = yb[2 * y + 1];
            const int* __restrict__ k = yk + (size_t)y * ky;
            int acc[N * 3];
#pragma unroll
            for (int q = 0; q < N * 3; ++q) acc[q] = 1 << (PP_BITS - 1);
            for (int t = 0; t < cnt; ++t) {
                // (N == 2 at the tile's last column reads the next 3 bytes of the LDS row: inside the row, unused)
                const unsigned char* p = inter + (first + t) * (PP_TW * 3) + xl * 3;
                const int w = k[t];
#pragma unroll
                for (int q = 0; q < N * 3; ++q) acc[q] += (int)p[q] * w;
            }
#pragma unroll
            for (int oc = 0; oc < 3; ++oc) {
                const int c = Nn.to_bgr255 ? 2 - oc : oc;
                float f[N];
#pragma unroll
                for (int q = 0; q < N; ++q) f[q] = pp_tail(acc[q * 3 + c], Nn.mean[oc], Nn.std[oc], Nn.to_bgr255);
                pp_store<OutT, N>(out + (((b * 3 + oc) * OH + y) * OW + x), f, x + 1 < OW);
            }
        }
    } else {
        constexpr int COLS = PP_TW * 3 / N;
        const int te = tw * 3;                        // the tile row's contiguous output elements
#pragma unroll 2
        for (int j = 0; j < PP_TH * COLS / 256; ++j) {
            const int o = tid + 256 * j;
            const int yl = o / COLS, col = (o - yl * COLS) * N;
            const int y = y0 + yl;
            if (y >= OH || col >= te) continue;
            const int first = yb[2 * y] - r0, cnt = yb[2 * y + 1];
            const int* __restrict__ k = yk + (size_t)y * ky;
            int src[N], acc[N];
            float mean[N], std[N];
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const int xl = (col + q) / 3, oc = (col + q) - xl * 3;
                src[q] = Nn.to_bgr255 ? xl * 3 + 2 - oc : col + q;       // (col + 1 == te: inside the LDS row, unused)
                mean[q] = oc == 0 ? Nn.mean[0] : (oc == 1 ? Nn.mean[1] : Nn.mean[2]);
                std[q] = oc == 0 ? Nn.std[0] : (oc == 1 ? Nn.std[1] : Nn.std[2]);
                acc[q] = 1 << (PP_BITS - 1);
            }
            for (int t = 0; t < cnt; ++t) {
                const unsigned char* p = inter + (first + t) * (PP_TW * 3);
                const int w = k[t];
#pragma unroll
                for (int q = 0; q < N; ++q) acc[q] += (int)p[src[q]] * w;
            }
            float f[N];
#pragma unroll
            for (int q = 0; q < N; ++q) f[q] = pp_tail(acc[q], mean[q], std[q], Nn.to_bgr255);
            pp_store<OutT, N>(out + (((b * OH + y) * OW + x0) * 3 + col), f, col + 1 < te);
        }
    }
}

template <typename OutT, bool NHWC>
static void preprocess_batch_launch(dim3 grid, size_t smem, hipStream_t st, void* out, int OH, int OW, int b0,
                                    const PreNorm& Nn, const PreBatch& T) {
    hipLaunchKernelGGL((preprocess_batch_kernel<OutT, NHWC>), grid, dim3(256), smem, st, reinterpret_cast<OutT*>(out), OH, OW,
                       b0, Nn, T);
}

}  // namespace smot

extern "C" int smot_preprocess_fwd(const unsigned char* frame, int H, int W, const int* xbounds, const int* xcoeffs,
                                   int kx, const int* ybounds, const int* ycoeffs, int ky, int OH, int OW,
                                   int max_tile_rows, const float* mean3, const float* std3, int to_bgr255, float* out,
                                   smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(H > 0 && W > 0 && OH > 0 && OW > 0 && kx > 0 && ky > 0, "preprocess: bad sizes %dx%d -> %dx%d", H, W, OH,
                 OW);
    SMOT_REQUIRE(frame && xbounds && xcoeffs && ybounds && ycoeffs && mean3 && std3 && out, "preprocess: null pointer");
    SMOT_REQUIRE(max_tile_rows > 0, "preprocess: max_tile_rows=%d", max_tile_rows);
    const size_t smem = (size_t)max_tile_rows * PP_TW * 3;
    if (smem > 64 * 1024) {
        set_error("preprocess: %d input rows per 8-row tile need %zu bytes of LDS (down-scaling factor too large)",
                  max_tile_rows, smem);
        return SMOT_ERR_UNSUPPORTED;
    }
    PreNorm Nn;
    for (int i = 0; i < 3; ++i) {
        Nn.mean[i] = mean3[i];       // HOST arrays
        Nn.std[i] = std3[i];
    }
    Nn.to_bgr255 = to_bgr255;
    dim3 grid((OW + PP_TW - 1) / PP_TW, (OH + PP_TH - 1) / PP_TH);
    hipLaunchKernelGGL(preprocess_kernel, grid, dim3(256), smem, (hipStream_t)stream, frame, H, W, xbounds, xcoeffs, kx,
                       ybounds, ycoeffs, ky, OH, OW, max_tile_rows, Nn, out);
    return check_launch("preprocess");
}

extern "C" int smot_preprocess_batch_fwd(int num_images, const unsigned char* const* frames, const int* H, const int* W,
                                         const int* const* xbounds, const int* const* xcoeffs, const int* kx,
                                         const int* const* ybounds, const int* const* ycoeffs, const int* ky,
                                         const int* max_tile_rows, int OH, int OW, const float* mean3, const float* std3,
                                         int to_bgr255, void* out, int out_type, smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(num_images >= 1 && num_images <= SMOT_MAX_IMAGES, "preprocess_batch: num_images=%d, need 1..%d", num_images,
                 SMOT_MAX_IMAGES);
    const int et = out_type & ~SMOT_FEAT_CHANNELS_LAST;
    SMOT_REQUIRE(out_type >= 0 && (et == SMOT_FEAT_F32 || et == SMOT_FEAT_F16 || et == SMOT_FEAT_BF16),
                 "preprocess_batch: out_type=%d is not SMOT_FEAT_F32 (0), SMOT_FEAT_F16 (1) or SMOT_FEAT_BF16 (2), alone or with "
                 "SMOT_FEAT_CHANNELS_LAST (16)", out_type);
    SMOT_REQUIRE(frames && H && W && xbounds && xcoeffs && kx && ybounds && ycoeffs && ky && max_tile_rows && mean3 && std3 &&
                 out, "preprocess_batch: null pointer");
    SMOT_REQUIRE(OH > 0 && OW > 0, "preprocess_batch: bad output size %dx%d", OH, OW);
    SMOT_REQUIRE((reinterpret_cast<uintptr_t>(out) & (et == SMOT_FEAT_F32 ? 3 : 1)) == 0,
                 "preprocess_batch: out is not aligned to its element size");
    for (int b = 0; b < num_images; ++b) {
        SMOT_REQUIRE(frames[b] && xbounds[b] && xcoeffs[b] && ybounds[b] && ycoeffs[b], "preprocess_batch: image %d: null pointer",
                     b);
        SMOT_REQUIRE(H[b] > 0 && W[b] > 0 && kx[b] > 0 && ky[b] > 0, "preprocess_batch: image %d: bad sizes %dx%d -> %dx%d (kx=%d, "
                     "ky=%d)", b, H[b], W[b], OH, OW, kx[b], ky[b]);
        SMOT_REQUIRE(max_tile_rows[b] > 0, "preprocess_batch: image %d: max_tile_rows=%d", b, max_tile_rows[b]);
    }
    for (int b = 0; b < num_images; ++b) {
        const size_t smem = (size_t)max_tile_rows[b] * PP_TW * 3;
        if (smem > 64 * 1024) {
            set_error("preprocess_batch: image %d: %d input rows per 8-row tile need %zu bytes of LDS (down-scaling factor too "
                      "large)", b, max_tile_rows[b], smem);
            return SMOT_ERR_UNSUPPORTED;
        }
    }
    PreNorm Nn;
    for (int i = 0; i < 3; ++i) {
        Nn.mean[i] = mean3[i];       // HOST arrays
        Nn.std[i] = std3[i];
    }
    Nn.to_bgr255 = to_bgr255;
    const bool nhwc = (out_type & SMOT_FEAT_CHANNELS_LAST) != 0;
    for (int b0 = 0; b0 < num_images; b0 += PP_CHUNK) {
        const int n = num_images - b0 < PP_CHUNK ? num_images - b0 : PP_CHUNK;
        PreBatch T;
        size_t smem = 0;
        for (int i = 0; i < PP_CHUNK; ++i) {
            const int b = b0 + (i < n ? i : 0);      // (slots past the launch's images repeat its first: never indexed)
            T.img[i] = PreImage{frames[b], xbounds[b], xcoeffs[b], ybounds[b], ycoeffs[b], H[b], W[b], kx[b], ky[b],
                                max_tile_rows[b]};
            const size_t s = (size_t)max_tile_rows[b] * PP_TW * 3;
            smem = s > smem ? s : smem;
        }
        const dim3 grid((OW + PP_TW - 1) / PP_TW, (OH + PP_TH - 1) / PP_TH, n);
        const hipStream_t st = (hipStream_t)stream;
        if (et == SMOT_FEAT_F32) {
            nhwc ? preprocess_batch_launch<float, true>(grid, smem, st, out, OH, OW, b0, Nn, T)
                 : preprocess_batch_launch<float, false>(grid, smem, st, out, OH, OW, b0, Nn, T);
        } else if (et == SMOT_FEAT_F16) {
            nhwc ? preprocess_batch_launch<f16_t, true>(grid, smem, st, out, OH, OW, b0, Nn, T)
                 : preprocess_batch_launch<f16_t, false>(grid, smem, st, out, OH, OW, b0, Nn, T);
        } else {
            nhwc ? preprocess_batch_launch<bf16_t, true>(grid, smem, st, out, OH, OW, b0, Nn, T)
                 : preprocess_batch_launch<bf16_t, false>(grid, smem, st, out, OH, OW, b0, Nn, T);
        }
        const int rc = check_launch("preprocess_batch");
        if (rc) return rc;
    }
    return SMOT_OK;
}
