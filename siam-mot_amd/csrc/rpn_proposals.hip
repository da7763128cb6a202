// RPN proposal selection — SURVEY.md §8(f) rank 2, the third caller of the NMS (reference operator_patch/rpn_patch.py:15-60
// on top of [UPSTREAM] RPNPostProcessor.forward / select_over_all_levels, modeling/rpn/inference.py).
//
// Replaces, for every FPN level and image: sigmoid + permute_and_flatten + topk(pre_nms_top_n) + two gathers, BoxCoder.decode,
// clip_to_image(remove_empty=False), remove_small_boxes (a nonzero), boxlist_nms (a second nonzero), and across the levels
// the concatenation + topk(fpn_post_nms_top_n) — ~150 launches and ~10 host synchronisations per image as stock torch.
//
// Here: one memset and nine launches, whatever the number of images N and levels L; every (image, level) pair is a grid
// slice of the same launch, found through the level table in the kernel arguments.  No host synchronisation.
//
//   memset   the histograms and the selection counters
//   1-3      rpn_hist_kernel<0|1|2>: radix select on the order-preserving uint32 image of the LOGIT (sigmoid is monotone;
//            it is evaluated for the output rows only): 2048-bin histograms of key bits 31..21, 20..10, 9..0, each over the
//            elements that match the prefix the passes before found.  A level is cut into chunks of 4096 flat indices, one
//            workgroup each (level 0 of the 704 x 1280 input: 42 workgroups per image); a workgroup re-derives the prefix
//            from the finished histograms (a 2048-bin suffix scan) rather than waiting for another launch to publish it.
//   4        rpn_select_kernel: T = the k-th largest key.  Elements with key > T go to the selection buffer in any order
//            (a reserved range per workgroup); every workgroup counts its elements with key == T.
//   5        rpn_ties_kernel: of the elements with key == T the (k - #greater) with the LOWEST flat index follow, in index
//            order (a workgroup's offset is the sum of the counts of the chunks before it): deterministic where torch.topk's
//            tie order is unspecified.
//   6        rpn_decode_kernel, one workgroup per (image, level): bitonic sort of the <= 2048 survivors in LDS on
//            (key descending, flat index ascending), gather of the four deltas from [N, 4A, H, W] and of the anchor row in
//            place, BoxCoder.decode in the reference's op order (un-contracted: only expf can differ from torch), candidate
//            buffers written, clip, min_size filter, ordered compaction.
//   7-8      rpn_nms_mask_kernel / rpn_nms_scan_kernel: the 64 x 64 bitmask and the one-wave greedy scan of nms.hip, batched
//            over (image, level); the scan stops at post_nms_top_n kept boxes and writes the level's list.
//   9        rpn_merge_kernel, one workgroup per image: the level lists are sorted, so a row's rank in the concatenation is
//            its position + binary searches in the other levels' keys (ties: lower concatenated position first); rows with
//            rank < fpn_post_nms_top_n are written with their sigmoid, the rest of the fixed-capacity output is zeroed.
//            One level: upstream skips the selection, the level's list is copied.
//
// Flat index = the reference's permute_and_flatten order (h * W + w) * A + a, read from the [N, A, H, W] tensor in place.
// -0 is ranked as +0 (a stable descending argsort of the logits, which compares them as numbers); NaN keys rank by their
// bits (positive NaN above +inf) — no parity is claimed there, only that every index stays in range.
// fp16 / bf16 objectness and regression: converted right behind the load, every later instruction is the fp32 kernel's.
#include "nms_common.h"
#include "roi_common.h"

namespace smot {

constexpr int RPN_MAX_K = 2048;          // pre_nms_top_n and fpn_post_nms_top_n
constexpr int RPN_BINS = 2048;           // 11 key bits per pass
constexpr int RPN_T = 256;               // threads of the streaming workgroups
constexpr int RPN_PER_THREAD = 16;
constexpr int RPN_CHUNK = RPN_T * RPN_PER_THREAD;
constexpr int RPN_SORT_T = 1024;
constexpr int RPN_MAX_ANCHOR_PTRS = 128; // distinct anchor tensors per call (upstream's generator shares one per level)

struct RpnLevel {
    const void* obj;     // [N, A, H, W]
    const void* reg;     // [N, 4A, H, W]
    int A, HW, n, k;     // n = A * H * W, k = min(pre_nms_top_n, n)
    int chunk0;          // first chunk of the level inside an image's chunk list
};

struct RpnArgs {
    RpnLevel lv[SMOT_MAX_LEVELS];
    int L, N, chunks, pre, post, fpn_post, nblk, amodal;
    float thresh, min_size, wx, wy, ww, wh, xform_clip;
    int* hist;                     // [N*L][3][2048]
    int* sel_count;                // [N*L]
    int* chunk_ties;               // [N][chunks]
    unsigned long long* sel;       // [N*L][2048]: key << 32 | ~flat index
    int* cand_count;               // [N*L]             -- the candidate buffers (include/smot_emm.h)
    int* cand_idx;                 // [N*L][pre]
    float* cand_logit;             // [N*L][pre]
    float* cand_box;               // [N*L][pre][4]
    int* surv_count;               // [N*L]             -- after clip + min_size, score order
    float* surv_box;               // [N*L][pre][4]
    float* surv_logit;             // [N*L][pre]
    unsigned long long* mask;      // [N*L][pre][nblk]
    int* lvl_count;                // [N*L]             -- after the NMS, first `post`
    float* lvl_box;                // [N*L][post][4]
    float* lvl_logit;              // [N*L][post]
    float* out_boxes;              // [N][fpn_post][4]
    float* out_obj;                // [N][fpn_post]
    int* out_count;                // [N]
};

struct RpnImages {
    const float* anchor[RPN_MAX_ANCHOR_PTRS];
    unsigned char slot[SMOT_MAX_IMAGES * SMOT_MAX_LEVELS];     // (image, level) -> anchor[]
    float w[SMOT_MAX_IMAGES], h[SMOT_MAX_IMAGES];               // image sizes (the BoxLists' size)
};

// order-preserving image of a float: a > b  <=>  key(a) > key(b); -0 as +0
__device__ __forceinline__ unsigned rpn_key(float x) {
    const unsigned u = (x == 0.0f) ? 0u : __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int rpn_level_of(const RpnArgs& A, int chunk) {
    int l = 0;
    while (l + 1 < A.L && chunk >= A.lv[l + 1].chunk0) ++l;
    return l;
}

template <typename FT>
__device__ __forceinline__ float rpn_logit(const RpnLevel& lv, int img, int f) {
    const int hw = f / lv.A, a = f - hw * lv.A;
    return feat_ld<FT>(reinterpret_cast<const FT*>(lv.obj) + (size_t)img * lv.n + (size_t)a * lv.HW + hw);
}

// The bin of a 2048-bin histogram that holds its kneed-th largest element (bins in descending order) and the number of
// elements in the bins above it.  All RPN_T threads call it; 1 <= kneed <= the histogram's total.
__device__ int2 rpn_find_bin(const int* __restrict__ hist, int kneed, int* s_scan, int* s_out) {
    const int t = threadIdx.x;
    constexpr int PER = RPN_BINS / RPN_T;
    int c[PER], sum = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        c[q] = hist[RPN_BINS - 1 - (t * PER + q)];
        sum += c[q];
    }
    if (t == 0) s_out[0] = s_out[1] = 0;
    s_scan[t] = sum;
    __syncthreads();
    for (int off = 1; off < RPN_T; off <<= 1) {
        const int v = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    const int incl = s_scan[t];
    int run = incl - sum;
    if (run < kneed && kneed <= incl) {                       // exactly one thread
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            if (run < kneed && kneed <= run + c[q]) {
                s_out[0] = RPN_BINS - 1 - (t * PER + q);
                s_out[1] = run;
            }
            run += c[q];
        }
    }
    __syncthreads();
    const int2 r = make_int2(s_out[0], s_out[1]);
    __syncthreads();
    return r;
}

// histogram pass PASS of the radix select: key bits 31..21, 20..10, 9..0
template <typename FT, int PASS>
__global__ void __launch_bounds__(RPN_T) rpn_hist_kernel(RpnArgs A) {
    __shared__ int s_hist[RPN_BINS];
    __shared__ int s_scan[RPN_T];
    __shared__ int s_out[2];
    const int img = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    const int l = rpn_level_of(A, chunk);
    const RpnLevel lv = A.lv[l];
    int* hist = A.hist + (size_t)(img * A.L + l) * 3 * RPN_BINS;
    unsigned prefix = 0;
    int kneed = lv.k;
    if constexpr (PASS >= 1) {
        const int2 r = rpn_find_bin(hist, kneed, s_scan, s_out);
        prefix = (unsigned)r.x;
        kneed -= r.y;
    }
    if constexpr (PASS >= 2) {
        const int2 r = rpn_find_bin(hist + RPN_BINS, kneed, s_scan, s_out);
        prefix = (prefix << 11) | (unsigned)r.x;
    }
    for (int b = t; b < RPN_BINS; b += RPN_T) s_hist[b] = 0;
    __syncthreads();
    const int f0 = (chunk - lv.chunk0) * RPN_CHUNK;
#pragma unroll 4
    for (int i = 0; i < RPN_PER_THREAD; ++i) {
        const int f = f0 + i * RPN_T + t;
        if (f < lv.n) {
            const unsigned key = rpn_key(rpn_logit<FT>(lv, img, f));
            if (PASS == 0) {
                atomicAdd(&s_hist[key >> 21], 1);
            } else if (PASS == 1) {
                if ((key >> 21) == prefix) atomicAdd(&s_hist[(key >> 10) & 2047u], 1);
            } else {
                if ((key >> 10) == prefix) atomicAdd(&s_hist[key & 1023u], 1);
            }
        }
    }
    __syncthreads();
    for (int b = t; b < RPN_BINS; b += RPN_T)
        if (s_hist[b]) atomicAdd(&hist[PASS * RPN_BINS + b], s_hist[b]);
}

// the k-th largest key of the level and the number of keys above it, from the three finished histograms
__device__ __forceinline__ void rpn_threshold(const int* hist, int k, int* s_scan, int* s_out, unsigned* T, int* greater) {
    const int2 r0 = rpn_find_bin(hist, k, s_scan, s_out);
    const int2 r1 = rpn_find_bin(hist + RPN_BINS, k - r0.y, s_scan, s_out);
    const int2 r2 = rpn_find_bin(hist + 2 * RPN_BINS, k - r0.y - r1.y, s_scan, s_out);
    *T = ((unsigned)r0.x << 21) | ((unsigned)r1.x << 10) | (unsigned)r2.x;
    *greater = r0.y + r1.y + r2.y;
}

template <typename FT>
__global__ void __launch_bounds__(RPN_T) rpn_select_kernel(RpnArgs A) {
    __shared__ int s_scan[RPN_T];
    __shared__ int s_out[2];
    __shared__ int s_gt, s_eq, s_base;
    const int img = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    const int l = rpn_level_of(A, chunk);
    const RpnLevel lv = A.lv[l];
    const int il = img * A.L + l;
    unsigned T;
    int greater;
    rpn_threshold(A.hist + (size_t)il * 3 * RPN_BINS, lv.k, s_scan, s_out, &T, &greater);
    if (t == 0) s_gt = s_eq = 0;
    __syncthreads();
    const int f0 = (chunk - lv.chunk0) * RPN_CHUNK;
    unsigned keys[RPN_PER_THREAD];
    int ngt = 0, neq = 0;
#pragma unroll
    for (int i = 0; i < RPN_PER_THREAD; ++i) {
        const int f = f0 + i * RPN_T + t;
        keys[i] = 0u;
        if (f < lv.n) {
            keys[i] = rpn_key(rpn_logit<FT>(lv, img, f));
            ngt += keys[i] > T ? 1 : 0;
            neq += keys[i] == T ? 1 : 0;
        }
    }
    int off = ngt ? atomicAdd(&s_gt, ngt) : 0;
    if (neq) atomicAdd(&s_eq, neq);
    __syncthreads();
    if (t == 0) {
        s_base = s_gt ? atomicAdd(&A.sel_count[il], s_gt) : 0;
        A.chunk_ties[img * A.chunks + chunk] = s_eq;
    }
    __syncthreads();
    off += s_base;
    unsigned long long* sel = A.sel + (size_t)il * RPN_MAX_K;
#pragma unroll
    for (int i = 0; i < RPN_PER_THREAD; ++i) {
        const int f = f0 + i * RPN_T + t;
        if (f < lv.n && keys[i] > T) {
            if (off < RPN_MAX_K) sel[off] = ((unsigned long long)keys[i] << 32) | (unsigned)(~(unsigned)f);
            ++off;
        }
    }
}

template <typename FT>
__global__ void __launch_bounds__(RPN_T) rpn_ties_kernel(RpnArgs A) {
    __shared__ int s_scan[RPN_T];
    __shared__ int s_out[2];
    __shared__ int s_before;
    __shared__ int s_wave[RPN_T / 64];
    const int img = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    const int l = rpn_level_of(A, chunk);
    const RpnLevel lv = A.lv[l];
    const int il = img * A.L + l;
    unsigned T;
    int greater;
    rpn_threshold(A.hist + (size_t)il * 3 * RPN_BINS, lv.k, s_scan, s_out, &T, &greater);
    const int need = lv.k - greater;                           // >= 1 elements with key == T are selected
    if (t == 0) s_before = 0;
    __syncthreads();
    int mine = 0;
    for (int c = lv.chunk0 + t; c < chunk; c += RPN_T) mine += A.chunk_ties[img * A.chunks + c];
    if (mine) atomicAdd(&s_before, mine);
    __syncthreads();
    int before = s_before;                                     // ties in the chunks before this one
    if (before >= need || A.chunk_ties[img * A.chunks + chunk] == 0) return;     // workgroup-uniform
    const int f0 = (chunk - lv.chunk0) * RPN_CHUNK;
    const int lane = t & 63, wave = t >> 6;
    unsigned long long* sel = A.sel + (size_t)il * RPN_MAX_K;
    for (int i = 0; i < RPN_PER_THREAD; ++i) {
        const int f = f0 + i * RPN_T + t;
        const bool tie = f < lv.n && rpn_key(rpn_logit<FT>(lv, img, f)) == T;
        const unsigned long long b = __ballot(tie);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int pos = before + __popcll(b & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < RPN_T / 64; ++w) {
            pos += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (tie && pos < need && greater + pos < RPN_MAX_K)
            sel[greater + pos] = ((unsigned long long)T << 32) | (unsigned)(~(unsigned)f);
        before += total;
        __syncthreads();
        if (before >= need) break;                             // workgroup-uniform
    }
}

// sort, gather, decode, clip, filter: one workgroup per (image, level)
template <typename FT>
__global__ void __launch_bounds__(RPN_SORT_T) rpn_decode_kernel(RpnArgs A, RpnImages I) {
    __shared__ unsigned long long s_key[RPN_MAX_K];
    __shared__ int s_scan[RPN_SORT_T];
    const int il = blockIdx.x, t = threadIdx.x;
    const int img = il / A.L, l = il - img * A.L;
    const RpnLevel lv = A.lv[l];
    const int k = lv.k;
    int P = 2;
    while (P < k) P <<= 1;
    const unsigned long long* sel = A.sel + (size_t)il * RPN_MAX_K;
    for (int e = t; e < P; e += RPN_SORT_T) s_key[e] = e < k ? sel[e] : 0ull;
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int e = t; e < (P >> 1); e += RPN_SORT_T) {
                const int lo = 2 * e - (e & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long a = s_key[lo], b = s_key[hi];
                if ((a < b) == desc) {
                    s_key[lo] = b;
                    s_key[hi] = a;
                }
            }
        }
    }
    __syncthreads();
    const float* anchors = I.anchor[I.slot[il]];
    const FT* reg = reinterpret_cast<const FT*>(lv.reg) + (size_t)img * 4 * lv.n;
    const float clip_w = I.w[img] - 1.0f, clip_h = I.h[img] - 1.0f;
    float box[2][4], logit[2];
    int keep[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r = 2 * t + q;                               // rank: a thread's two rows are consecutive
        keep[q] = 0;
        if (r < k) {
            const int f = (int)min(~(unsigned)s_key[r], (unsigned)(lv.n - 1));    // (memory safety: never past the level)
            const int hw = f / lv.A, a = f - hw * lv.A;
            logit[q] = rpn_logit<FT>(lv, img, f);
            float d[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) d[c] = feat_ld<FT>(reg + (size_t)(4 * a + c) * lv.HW + hw);
            const float* an = anchors + (size_t)f * 4;
            const float x1 = an[0], y1 = an[1], x2 = an[2], y2 = an[3];
            // [UPSTREAM] BoxCoder.decode, as box_refine.hip writes it
            const float w = add_rn(sub_rn(x2, x1), 1.0f), h = add_rn(sub_rn(y2, y1), 1.0f);
            const float cx = add_rn(x1, mul_rn(0.5f, w)), cy = add_rn(y1, mul_rn(0.5f, h));
            const float dx = div_rn(d[0], A.wx), dy = div_rn(d[1], A.wy);
            const float dw = min_nan(div_rn(d[2], A.ww), A.xform_clip), dh = min_nan(div_rn(d[3], A.wh), A.xform_clip);
            const float pcx = add_rn(mul_rn(dx, w), cx), pcy = add_rn(mul_rn(dy, h), cy);
            const float pw = mul_rn(expf(dw), w), ph = mul_rn(expf(dh), h);
            float bx1 = sub_rn(pcx, mul_rn(0.5f, pw));
            float by1 = sub_rn(pcy, mul_rn(0.5f, ph));
            float bx2 = sub_rn(add_rn(pcx, mul_rn(0.5f, pw)), 1.0f);
            float by2 = sub_rn(add_rn(pcy, mul_rn(0.5f, ph)), 1.0f);
            const size_t row = (size_t)il * A.pre + r;
            A.cand_idx[row] = f;
            A.cand_logit[row] = logit[q];
            A.cand_box[row * 4 + 0] = bx1;
            A.cand_box[row * 4 + 1] = by1;
            A.cand_box[row * 4 + 2] = bx2;
            A.cand_box[row * 4 + 3] = by2;
            if (!A.amodal) {                                   // clip_to_image(remove_empty=False)
                bx1 = clamp_nan(bx1, 0.0f, clip_w);
                by1 = clamp_nan(by1, 0.0f, clip_h);
                bx2 = clamp_nan(bx2, 0.0f, clip_w);
                by2 = clamp_nan(by2, 0.0f, clip_h);
            }
            // remove_small_boxes: the xywh sides, both >= min_size (a NaN side drops the row)
            const float ws = add_rn(sub_rn(bx2, bx1), 1.0f), hs = add_rn(sub_rn(by2, by1), 1.0f);
            keep[q] = (ws >= A.min_size && hs >= A.min_size) ? 1 : 0;
            box[q][0] = bx1;
            box[q][1] = by1;
            box[q][2] = bx2;
            box[q][3] = by2;
        }
    }
    if (t == 0) A.cand_count[il] = k;
    // ordered compaction: survivors keep their order
    const int mine = keep[0] + keep[1];
    s_scan[t] = mine;
    __syncthreads();
    for (int off = 1; off < RPN_SORT_T; off <<= 1) {
        const int v = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    int pos = s_scan[t] - mine;
    if (t == RPN_SORT_T - 1) A.surv_count[il] = s_scan[t];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (keep[q]) {
            const size_t row = (size_t)il * A.pre + pos;
            A.surv_box[row * 4 + 0] = box[q][0];
            A.surv_box[row * 4 + 1] = box[q][1];
            A.surv_box[row * 4 + 2] = box[q][2];
            A.surv_box[row * 4 + 3] = box[q][3];
            A.surv_logit[row] = logit[q];
            ++pos;
        }
    }
}

// nms_mask_kernel of nms.hip over (image, level): blockIdx.y = il, blockIdx.x = (row tile, column tile)
__global__ void __launch_bounds__(NMS_T) rpn_nms_mask_kernel(RpnArgs A) {
    const int il = blockIdx.y;
    const int n = A.surv_count[il];
    const int rb = blockIdx.x / A.nblk, cb = blockIdx.x - rb * A.nblk;
    if (rb * NMS_T >= n || cb * NMS_T >= n) return;
    const float* boxes = A.surv_box + (size_t)il * A.pre * 4;
    unsigned long long* mask = A.mask + (size_t)il * A.pre * A.nblk;
    __shared__ float cbox[NMS_T * 4];
    const int ccount = min(n - cb * NMS_T, NMS_T);
    if ((int)threadIdx.x < ccount) {
        const float* src = boxes + (size_t)(cb * NMS_T + threadIdx.x) * 4;
        cbox[threadIdx.x * 4 + 0] = src[0];
        cbox[threadIdx.x * 4 + 1] = src[1];
        cbox[threadIdx.x * 4 + 2] = src[2];
        cbox[threadIdx.x * 4 + 3] = src[3];
    }
    __syncthreads();
    const int i = rb * NMS_T + threadIdx.x;
    if (i >= n) return;
    unsigned long long bits = 0ull;
    if (cb >= rb) {                                   // only later boxes can be suppressed by box i
        const float* me = boxes + (size_t)i * 4;
        const float b4[4] = {me[0], me[1], me[2], me[3]};
        const int j0 = (cb == rb) ? threadIdx.x + 1 : 0;
        for (int j = j0; j < ccount; ++j)
            if (iou_plus1(b4, cbox + j * 4) > A.thresh) bits |= 1ull << j;
    }
    mask[(size_t)i * A.nblk + cb] = bits;
}

// nms_scan_kernel of nms.hip per (image, level) (at most 2048 boxes: one `removed` word per lane), stopping at `post`
// kept boxes; the kept rows become the level's list
__global__ void __launch_bounds__(256) rpn_nms_scan_kernel(RpnArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long slab[];   // [64 rows][ne]
    __shared__ int s_kept[RPN_MAX_K];
    __shared__ int s_nkept;
    const int il = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.surv_count[il];
    const int ne = (n + NMS_T - 1) / NMS_T;                    // <= 32 words per row in use
    const unsigned long long* mask = A.mask + (size_t)il * A.pre * A.nblk;
    unsigned long long removed = 0ull;                         // wave 0: lane w holds word w
    int nkept = 0;
    if (tid == 0) s_nkept = 0;
    __syncthreads();
    for (int c = 0; c < ne; ++c) {
        const int rows = min(NMS_T, n - c * NMS_T);
        for (int e = tid; e < rows * ne; e += 256) {
            const int r = e / ne, w = e - r * ne;
            slab[e] = mask[(size_t)(c * NMS_T + r) * A.nblk + w];
        }
        __syncthreads();
        if (wave == 0) {
            const unsigned lo = __shfl((unsigned)removed, c), hi = __shfl((unsigned)(removed >> 32), c);
            unsigned long long r = ((unsigned long long)hi << 32) | lo;
            for (int j = 0; j < rows && nkept < A.post; ++j) {
                if (!((r >> j) & 1ull)) {                      // wave-uniform: kept
                    if (lane == 0) s_kept[nkept] = c * NMS_T + j;
                    ++nkept;
                    if (lane < ne) removed |= slab[j * ne + lane];
                    r |= slab[j * ne + c];
                }
            }
            if (lane == 0) s_nkept = nkept;
        }
        __syncthreads();
        if (s_nkept >= A.post) break;                          // workgroup-uniform
    }
    __syncthreads();
    const int total = s_nkept;
    if (tid == 0) A.lvl_count[il] = total;
    for (int p = tid; p < total; p += 256) {
        const size_t src = (size_t)il * A.pre + s_kept[p], dst = (size_t)il * A.post + p;
        A.lvl_box[dst * 4 + 0] = A.surv_box[src * 4 + 0];
        A.lvl_box[dst * 4 + 1] = A.surv_box[src * 4 + 1];
        A.lvl_box[dst * 4 + 2] = A.surv_box[src * 4 + 2];
        A.lvl_box[dst * 4 + 3] = A.surv_box[src * 4 + 3];
        A.lvl_logit[dst] = A.surv_logit[src];
    }
}

// number of keys of a descending list that are > key (STRICT) or >= key
template <bool STRICT>
__device__ __forceinline__ int rpn_count_above(const unsigned* list, int n, unsigned key) {
    int lo = 0, hi = n;                                        // first position whose key is not above
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const bool above = STRICT ? list[mid] > key : list[mid] >= key;
        if (above) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(RPN_SORT_T) rpn_merge_kernel(RpnArgs A) {
    extern __shared__ unsigned s_keys[];                       // [L][post]
    __shared__ int s_cnt[SMOT_MAX_LEVELS];
    const int img = blockIdx.x, t = threadIdx.x;
    float* ob = A.out_boxes + (size_t)img * A.fpn_post * 4;
    float* oo = A.out_obj + (size_t)img * A.fpn_post;
    if (t < A.L) s_cnt[t] = min(A.lvl_count[img * A.L + t], A.post);
    __syncthreads();
    int total = 0;
    for (int l = 0; l < A.L; ++l) total += s_cnt[l];
    const int count = min(total, A.fpn_post);
    const bool merge = A.L > 1;                                // upstream: select_over_all_levels only with several levels
    if (merge) {
        for (int e = t; e < A.L * A.post; e += RPN_SORT_T) {
            const int l = e / A.post, p = e - l * A.post;
            if (p < s_cnt[l]) s_keys[e] = rpn_key(A.lvl_logit[(size_t)(img * A.L + l) * A.post + p]);
        }
        __syncthreads();
    }
    for (int e = t; e < A.L * A.post; e += RPN_SORT_T) {
        const int l = e / A.post, p = e - l * A.post;
        if (p >= s_cnt[l]) continue;
        int rank = p;
        if (merge) {
            const unsigned key = s_keys[e];
            for (int m = 0; m < A.L; ++m) {
                if (m < l) rank += rpn_count_above<false>(s_keys + m * A.post, s_cnt[m], key);
                if (m > l) rank += rpn_count_above<true>(s_keys + m * A.post, s_cnt[m], key);
            }
        }
        if (rank < count) {
            const size_t src = (size_t)(img * A.L + l) * A.post + p;
            ob[rank * 4 + 0] = A.lvl_box[src * 4 + 0];
            ob[rank * 4 + 1] = A.lvl_box[src * 4 + 1];
            ob[rank * 4 + 2] = A.lvl_box[src * 4 + 2];
            ob[rank * 4 + 3] = A.lvl_box[src * 4 + 3];
            const float x = A.lvl_logit[src];
            oo[rank] = div_rn(1.0f, add_rn(1.0f, expf(-x)));    // the objectness field: sigmoid of the rows that are output
        }
    }
    for (int r = count + t; r < A.fpn_post; r += RPN_SORT_T) {
        ob[r * 4 + 0] = ob[r * 4 + 1] = ob[r * 4 + 2] = ob[r * 4 + 3] = 0.0f;
        oo[r] = 0.0f;
    }
    if (t == 0) A.out_count[img] = count;
}

// ---- workspace layout (4-byte words; every section starts at a multiple of 4 words) -------------------------------------
struct RpnLayout {
    size_t cand_count, cand_idx, cand_logit, cand_box;         // the public head (include/smot_emm.h)
    size_t hist, sel_count, zero_end, chunk_ties, sel, surv_count, surv_box, surv_logit, mask, lvl_count, lvl_box, lvl_logit, end;
};

static inline size_t rpn_al4(size_t w) { return (w + 3) & ~(size_t)3; }

static RpnLayout rpn_layout(int N, int L, int pre, int post, int chunks) {
    const size_t NL = (size_t)N * L, nblk = (size_t)(pre + NMS_T - 1) / NMS_T;
    RpnLayout o;
    size_t w = 0;
    o.cand_count = w; w += rpn_al4(NL);
    o.cand_idx = w; w += rpn_al4(NL * pre);
    o.cand_logit = w; w += rpn_al4(NL * pre);
    o.cand_box = w; w += rpn_al4(NL * pre * 4);
    o.hist = w; w += rpn_al4(NL * 3 * RPN_BINS);
    o.sel_count = w; w += rpn_al4(NL);
    o.zero_end = w;
    o.chunk_ties = w; w += rpn_al4((size_t)N * chunks);
    o.sel = w; w += rpn_al4(NL * RPN_MAX_K * 2);
    o.surv_count = w; w += rpn_al4(NL);
    o.surv_box = w; w += rpn_al4(NL * pre * 4);
    o.surv_logit = w; w += rpn_al4(NL * pre);
    o.mask = w; w += rpn_al4(NL * pre * nblk * 2);
    o.lvl_count = w; w += rpn_al4(NL);
    o.lvl_box = w; w += rpn_al4(NL * post * 4);
    o.lvl_logit = w; w += rpn_al4(NL * post);
    o.end = w;
    return o;
}

static int rpn_check_shapes(int num_images, int num_levels, const int* num_anchors, const int* heights, const int* widths,
                            int pre, int post, int fpn_post, int* chunks) {
    SMOT_REQUIRE(num_images >= 1 && num_images <= SMOT_MAX_IMAGES, "rpn_proposals: num_images=%d not in [1,%d]", num_images,
                 SMOT_MAX_IMAGES);
    SMOT_REQUIRE(num_levels >= 1 && num_levels <= SMOT_MAX_LEVELS, "rpn_proposals: num_levels=%d not in [1,%d]", num_levels,
                 SMOT_MAX_LEVELS);
    SMOT_REQUIRE(pre >= 1 && pre <= RPN_MAX_K, "rpn_proposals: pre_nms_top_n=%d not in [1,%d]", pre, RPN_MAX_K);
    SMOT_REQUIRE(post >= 1, "rpn_proposals: post_nms_top_n=%d", post);
    SMOT_REQUIRE(fpn_post >= 1 && fpn_post <= RPN_MAX_K, "rpn_proposals: fpn_post_nms_top_n=%d not in [1,%d]", fpn_post,
                 RPN_MAX_K);
    SMOT_REQUIRE(num_anchors && heights && widths, "rpn_proposals: null shape array");
    long long c = 0;
    for (int l = 0; l < num_levels; ++l) {
        SMOT_REQUIRE(num_anchors[l] >= 1 && heights[l] >= 1 && widths[l] >= 1, "rpn_proposals: level %d is %d x %d x %d", l,
                     num_anchors[l], heights[l], widths[l]);
        const long long n = (long long)num_anchors[l] * heights[l] * widths[l];
        SMOT_REQUIRE(n * 4 * num_images < (1ll << 31), "rpn_proposals: level %d has %lld anchors per image (x %d images)", l, n,
                     num_images);
        c += (n + RPN_CHUNK - 1) / RPN_CHUNK;
    }
    SMOT_REQUIRE(c <= 65535, "rpn_proposals: %lld chunks of %d anchors per image", c, RPN_CHUNK);
    *chunks = (int)c;
    return SMOT_OK;
}

template <typename FT>
static int rpn_launch(const RpnArgs& A, const RpnImages& I, hipStream_t st) {
    const dim3 grid(A.chunks, A.N);
    const int NL = A.N * A.L;
    hipLaunchKernelGGL((rpn_hist_kernel<FT, 0>), grid, dim3(RPN_T), 0, st, A);
    hipLaunchKernelGGL((rpn_hist_kernel<FT, 1>), grid, dim3(RPN_T), 0, st, A);
    hipLaunchKernelGGL((rpn_hist_kernel<FT, 2>), grid, dim3(RPN_T), 0, st, A);
    hipLaunchKernelGGL((rpn_select_kernel<FT>), grid, dim3(RPN_T), 0, st, A);
    hipLaunchKernelGGL((rpn_ties_kernel<FT>), grid, dim3(RPN_T), 0, st, A);
    int rc = check_launch("rpn_proposals select");
    if (rc) return rc;
    hipLaunchKernelGGL((rpn_decode_kernel<FT>), dim3(NL), dim3(RPN_SORT_T), 0, st, A, I);
    hipLaunchKernelGGL(rpn_nms_mask_kernel, dim3(A.nblk * A.nblk, NL), dim3(NMS_T), 0, st, A);
    hipLaunchKernelGGL(rpn_nms_scan_kernel, dim3(NL), dim3(256), (size_t)NMS_T * A.nblk * 8, st, A);
    hipLaunchKernelGGL(rpn_merge_kernel, dim3(A.N), dim3(RPN_SORT_T), (size_t)A.L * A.post * 4, st, A);
    return check_launch("rpn_proposals");
}

}  // namespace smot

extern "C" long long smot_rpn_proposals_ws_bytes(int num_images, int num_levels, const int* num_anchors, const int* heights,
                                                 const int* widths, int pre_nms_top_n, int post_nms_top_n) {
    int chunks = 0;
    if (smot::rpn_check_shapes(num_images, num_levels, num_anchors, heights, widths, pre_nms_top_n, post_nms_top_n, 1, &chunks))
        return -1;
    const int post = post_nms_top_n < pre_nms_top_n ? post_nms_top_n : pre_nms_top_n;
    return (long long)smot::rpn_layout(num_images, num_levels, pre_nms_top_n, post, chunks).end * 4;
}

extern "C" int smot_rpn_proposals_fwd(const void* const* objectness, const void* const* regression, int feat_type,
                                      const int* num_anchors, const int* heights, const int* widths, int num_levels,
                                      int num_images, const float* const* anchors, const float* image_wh,
                                      int pre_nms_top_n, int post_nms_top_n, int fpn_post_nms_top_n, float nms_thresh,
                                      float min_size, int amodal, float wx, float wy, float ww, float wh, float xform_clip,
                                      void* ws, float* out_boxes, float* out_objectness, int32_t* out_count,
                                      smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(feat_type == SMOT_FEAT_F32 || feat_type == SMOT_FEAT_F16 || feat_type == SMOT_FEAT_BF16,
                 "rpn_proposals: feat_type=%d (fp32, fp16 or bf16 NCHW tensors)", feat_type);
    int chunks = 0;
    int rc = rpn_check_shapes(num_images, num_levels, num_anchors, heights, widths, pre_nms_top_n, post_nms_top_n,
                              fpn_post_nms_top_n, &chunks);
    if (rc) return rc;
    SMOT_REQUIRE(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f, "rpn_proposals: regression weights must be positive");
    if (!(nms_thresh > 0.0f)) {
        set_error("rpn_proposals: nms_thresh=%g (upstream returns the level unsuppressed and untruncated there)", nms_thresh);
        return SMOT_ERR_UNSUPPORTED;
    }
    SMOT_REQUIRE(objectness && regression && anchors && image_wh && ws && out_boxes && out_objectness && out_count,
                 "rpn_proposals: null pointer");
    SMOT_REQUIRE(((uintptr_t)ws & 15) == 0, "rpn_proposals: ws must be 16-byte aligned");
    const int N = num_images, L = num_levels, pre = pre_nms_top_n;
    const int post = post_nms_top_n < pre ? post_nms_top_n : pre;
    // the merge keeps one key per (level, row) in LDS beside its 32 bytes of counters: 64 KiB in all without an opt-in
    if ((size_t)L * post * 4 + 64 > 64 * 1024) {
        set_error("rpn_proposals: %d levels x %d rows per level exceed the merge's LDS (levels x rows x 4 + 64 <= 65536)", L, post);
        return SMOT_ERR_UNSUPPORTED;
    }
    RpnArgs A = {};
    RpnImages I = {};
    int c0 = 0;
    for (int l = 0; l < L; ++l) {
        SMOT_REQUIRE(objectness[l] && regression[l], "rpn_proposals: null tensor at level %d", l);
        RpnLevel& v = A.lv[l];
        v.obj = objectness[l];
        v.reg = regression[l];
        v.A = num_anchors[l];
        v.HW = heights[l] * widths[l];
        v.n = v.A * v.HW;
        v.k = pre < v.n ? pre : v.n;
        v.chunk0 = c0;
        c0 += (v.n + RPN_CHUNK - 1) / RPN_CHUNK;
    }
    int distinct = 0;
    for (int e = 0; e < N * L; ++e) {
        SMOT_REQUIRE(anchors[e], "rpn_proposals: null anchor tensor (image %d, level %d)", e / L, e % L);
        int s = 0;
        while (s < distinct && I.anchor[s] != anchors[e]) ++s;
        if (s == distinct) {
            if (distinct == RPN_MAX_ANCHOR_PTRS) {
                set_error("rpn_proposals: more than %d distinct anchor tensors in one call", RPN_MAX_ANCHOR_PTRS);
                return SMOT_ERR_UNSUPPORTED;
            }
            I.anchor[distinct++] = anchors[e];
        }
        I.slot[e] = (unsigned char)s;
    }
    for (int i = 0; i < N; ++i) {
        I.w[i] = image_wh[2 * i];
        I.h[i] = image_wh[2 * i + 1];
    }
    const RpnLayout o = rpn_layout(N, L, pre, post, chunks);
    int* wi = reinterpret_cast<int*>(ws);
    float* wf = reinterpret_cast<float*>(ws);
    A.L = L;
    A.N = N;
    A.chunks = chunks;
    A.pre = pre;
    A.post = post;
    A.fpn_post = fpn_post_nms_top_n;
    A.nblk = (pre + NMS_T - 1) / NMS_T;
    A.amodal = amodal ? 1 : 0;
    A.thresh = nms_thresh;
    A.min_size = min_size;
    A.wx = wx;
    A.wy = wy;
    A.ww = ww;
    A.wh = wh;
    A.xform_clip = xform_clip;
    A.cand_count = wi + o.cand_count;
    A.cand_idx = wi + o.cand_idx;
    A.cand_logit = wf + o.cand_logit;
    A.cand_box = wf + o.cand_box;
    A.hist = wi + o.hist;
    A.sel_count = wi + o.sel_count;
    A.chunk_ties = wi + o.chunk_ties;
    A.sel = reinterpret_cast<unsigned long long*>(wi + o.sel);
    A.surv_count = wi + o.surv_count;
    A.surv_box = wf + o.surv_box;
    A.surv_logit = wf + o.surv_logit;
    A.mask = reinterpret_cast<unsigned long long*>(wi + o.mask);
    A.lvl_count = wi + o.lvl_count;
    A.lvl_box = wf + o.lvl_box;
    A.lvl_logit = wf + o.lvl_logit;
    A.out_boxes = out_boxes;
    A.out_obj = out_objectness;
    A.out_count = out_count;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(wi + o.hist, 0, (o.zero_end - o.hist) * 4, st);
    if (e != hipSuccess) {
        set_error("rpn_proposals: memset failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    if (feat_type == SMOT_FEAT_F32) return rpn_launch<float>(A, I, st);
    if (feat_type == SMOT_FEAT_F16) return rpn_launch<f16_t>(A, I, st);
    return rpn_launch<bf16_t>(A, I, st);
}
