// Box-head post-processing of the DETECTIONS — the device half of ROIBoxHead's PostProcessor that box_refine.hip leaves out.
//
// Replaces, for one image whose proposals are ALL detections (no `ids` field: every row has ids = -1, what the RPN hands the
// box head every frame): PostProcessor.forward + filter_results (reference siammot/modelling/box_head/inference.py:46-191:
// soft-max, BoxCoder.decode [UPSTREAM box_coder.py] of every foreground class's deltas, clip_to_image, and per class a
// nonzero, three mask gathers, `len(det) > 0`, an argsort, the NMS launch + its mask gather, `trk_idx.any()`, two
// cat_boxlist) — ~25 launches and three to four host synchronisations per class as stock torch.
//
// Here: FOUR launches and no memset, whatever the number of rows M, of classes K and the device-resident row count; a
// foreground class is a grid slice of the same launch (the structure of rpn_proposals.hip with classes for (image, level)
// pairs).  No host synchronisation, no atomics on global memory: two runs give the same bits.  Several images of a call
// (smot_box_detect_post_batched_fwd) are one more grid dimension of the same four kernels: the same four launches, every
// image's outputs bit for bit the single-image call's on that image's rows.
//
//   1  box_detect_cand_kernel, one workgroup per class j in [1, K): soft-max of the row's K logits (box_refine.hip's op
//      order), BoxCoder.decode of class j's deltas (class-agnostic: the last four columns), clip, candidates = rows with
//      p_j > score_thresh (a NaN score is none), bitonic sort in LDS on (score descending, row ascending) — the stable
//      descending argsort ops._nms_sorted runs today — and the class's sorted candidate list written.
//   2  box_detect_mask_kernel: the 64 x 64 tile bitmask of nms.hip over (class, row tile, column tile).
//   3  box_detect_scan_kernel, one workgroup per class: the one-wave greedy scan of nms.hip, then the kept candidates
//      put back into ascending PROPOSAL ROW order (what ops.nms and the reference's per-class loop return) by an ordered
//      compaction over the rows.
//   4  box_detect_write_kernel, one workgroup per class: the class's rows behind the prefix of the classes before it, the
//      counts, and the rows beyond the total zeroed (a share of the tail per workgroup).
//
// Rows >= min(*count, M) are never loaded.  DETECTIONS_PER_IMG is not applied (the reference does not apply it in this
// function either).  Non-finite inputs: a row whose soft-max is NaN in torch (a NaN or +inf among its logits) is a
// candidate of no class; a NaN among a candidate's deltas gives the NaN coordinates box_refine.hip documents, and such a
// box neither suppresses nor is suppressed (every comparison with its IoU is false).
#include "nms_common.h"
#include "roi_common.h"

namespace smot {

constexpr int BD_MAX_ROWS = 2048;
constexpr int BD_MAX_CLASSES = 128;
constexpr int BD_SORT_T = 1024;          // two rows per thread
constexpr int BD_T = 256;

struct BoxDetectArgs {
    const float* head;       // [M, ld] : columns [0, K) class logits, columns [K, K + 4*KR) box deltas
    int ld, K, KR, M, nblk;  // KR = K (per-class regression) or 2 (class-agnostic: the LAST four columns are used)
    const float* boxes;      // [M, 4] proposals
    const int* count;        // device: rows that exist
    float wx, wy, ww, wh, xform_clip;
    float clip_w, clip_h;    // image size, or 0: amodal (no clipping)
    float score_thresh, nms_thresh;
    int* cand_count;                 // [C]        C = K - 1 foreground classes, class j at c = j - 1
    int* cand_row;                   // [C][M]     proposal rows of the class's candidates, best score first
    float* cand_score;               // [C][M]
    float* cand_box;                 // [C][M][4]
    unsigned long long* mask;        // [C][M][nblk]
    int* keep_count;                 // [C]
    int* keep_rank;                  // [C][M]     ranks (positions in the candidate list) of the survivors, by ascending row
    float* out_boxes;                // [M*C][4]
    float* out_scores;               // [M*C]
    long long* out_labels;           // [M*C]
    int* out_rows;                   // [M*C]
    int* out_count;                  // [K]: total, then per class
};

// order-preserving image of a float: a > b  <=>  key(a) > key(b); -0 as +0
__device__ __forceinline__ unsigned bd_key(float x) {
    const unsigned u = (x == 0.0f) ? 0u : __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int bd_rows(const BoxDetectArgs& A) { return min(max(*A.count, 0), A.M); }

// ---- the four kernels' bodies: one text behind the single-image kernels (A = the call) and the batched ones (A = the view
// of one image of the call, bd_image below); `c` = the foreground class's slot ---------------------------------------------
__device__ __forceinline__ void bd_cand_body(const BoxDetectArgs& A, const int c) {
    __shared__ unsigned long long s_key[BD_MAX_ROWS];        // score key << 32 | ~row; 0: not a candidate
    __shared__ float4 s_box[BD_MAX_ROWS];                    // by row
    __shared__ float s_score[BD_MAX_ROWS];                   // by row
    __shared__ int s_cnt;
    const int j = c + 1, t = threadIdx.x;
    const int n = bd_rows(A);
    int P = 2;
    while (P < n) P <<= 1;
    if (t == 0) s_cnt = 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = t + q * BD_SORT_T;
        unsigned long long key = 0ull;
        if (i < n) {
            const float* row = A.head + (size_t)i * A.ld;
            // F.softmax(class_logits, -1): max, exp of the difference, sum in class order, divide
            float m = row[0];
            for (int k = 1; k < A.K; ++k) m = fmaxf(m, row[k]);
            float s = 0.0f, el = 0.0f;
            for (int k = 0; k < A.K; ++k) {
                const float e = expf(sub_rn(row[k], m));
                s = add_rn(s, e);
                if (k == j) el = e;
            }
            const float p = div_rn(el, s);
            // BoxCoder.decode on class j's four deltas (class-agnostic: the last four columns, inference.py:67-68)
            const float* d = row + A.K + ((A.KR == A.K) ? 4 * j : 4 * (A.KR - 1));
            const float x1 = A.boxes[i * 4 + 0], y1 = A.boxes[i * 4 + 1], x2 = A.boxes[i * 4 + 2], y2 = A.boxes[i * 4 + 3];
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
            if (A.clip_w > 0.0f) {                                           // clip_to_image(remove_empty=False)
                bx1 = clamp_nan(bx1, 0.0f, A.clip_w - 1.0f);
                by1 = clamp_nan(by1, 0.0f, A.clip_h - 1.0f);
                bx2 = clamp_nan(bx2, 0.0f, A.clip_w - 1.0f);
                by2 = clamp_nan(by2, 0.0f, A.clip_h - 1.0f);
            }
            s_box[i] = make_float4(bx1, by1, bx2, by2);
            s_score[i] = p;
            if (p > A.score_thresh)                                          // (NaN: false)
                key = ((unsigned long long)bd_key(p) << 32) | (unsigned)(~(unsigned)i);
        }
        if (i < P) s_key[i] = key;
    }
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            const int e = t;                                                 // P / 2 <= BD_SORT_T compare-exchanges per step
            if (e < (P >> 1)) {
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
    // candidate keys are never 0 (their low word is ~row with row < 2048): the list ends at the first 0
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = t + q * BD_SORT_T;
        if (e < P && s_key[e] != 0ull && (e + 1 == P || s_key[e + 1] == 0ull)) s_cnt = e + 1;
    }
    __syncthreads();
    const int nc = min(s_cnt, n);
    if (t == 0) A.cand_count[c] = nc;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = t + q * BD_SORT_T;
        if (e < nc) {
            const int i = (int)min(~(unsigned)s_key[e], (unsigned)(n - 1));  // (memory safety: never past the rows)
            const size_t dst = (size_t)c * A.M + e;
            const float4 b = s_box[i];
            A.cand_row[dst] = i;
            A.cand_score[dst] = s_score[i];
            A.cand_box[dst * 4 + 0] = b.x;
            A.cand_box[dst * 4 + 1] = b.y;
            A.cand_box[dst * 4 + 2] = b.z;
            A.cand_box[dst * 4 + 3] = b.w;
        }
    }
}

// nms_mask_kernel of nms.hip over the classes: c = class, tile = (row tile, column tile) < nblk * nblk
__device__ __forceinline__ void bd_mask_body(const BoxDetectArgs& A, const int c, const unsigned tile) {
    const int n = min(A.cand_count[c], A.M);
    const int rb = tile / A.nblk, cb = tile - rb * A.nblk;
    if (rb * NMS_T >= n || cb * NMS_T >= n) return;
    const float* boxes = A.cand_box + (size_t)c * A.M * 4;
    unsigned long long* mask = A.mask + (size_t)c * A.M * A.nblk;
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
            if (iou_plus1(b4, cbox + j * 4) > A.nms_thresh) bits |= 1ull << j;
    }
    mask[(size_t)i * A.nblk + cb] = bits;
}

// nms_scan_kernel of nms.hip per class (at most 2048 candidates: one `removed` word per lane of wave 0); the survivors
// leave in ascending proposal-row order
__device__ __forceinline__ void bd_scan_body(const BoxDetectArgs& A, const int c) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long slab[];   // [64 rows][ne]
    __shared__ int s_kept[BD_MAX_ROWS];                        // ranks of the kept candidates, in score order
    __shared__ int s_rank[BD_MAX_ROWS];                        // by proposal row: rank + 1 of a kept candidate, else 0
    __shared__ int s_scan[BD_T];
    __shared__ int s_nkept;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(A.cand_count[c], A.M);
    const int ne = (n + NMS_T - 1) / NMS_T;                    // <= 32 words per row in use
    const unsigned long long* mask = A.mask + (size_t)c * A.M * A.nblk;
    unsigned long long removed = 0ull;                         // wave 0: lane w holds word w
    int nkept = 0;
    if (tid == 0) s_nkept = 0;
    for (int r = tid; r < A.M; r += BD_T) s_rank[r] = 0;
    __syncthreads();
    for (int ch = 0; ch < ne; ++ch) {
        const int rows = min(NMS_T, n - ch * NMS_T);
        for (int e = tid; e < rows * ne; e += BD_T) {
            const int r = e / ne, w = e - r * ne;
            slab[e] = mask[(size_t)(ch * NMS_T + r) * A.nblk + w];
        }
        __syncthreads();
        if (wave == 0) {
            const unsigned lo = __shfl((unsigned)removed, ch), hi = __shfl((unsigned)(removed >> 32), ch);
            unsigned long long r = ((unsigned long long)hi << 32) | lo;
            for (int j = 0; j < rows; ++j) {
                if (!((r >> j) & 1ull)) {                      // wave-uniform: kept
                    if (lane == 0) s_kept[nkept] = ch * NMS_T + j;
                    ++nkept;
                    if (lane < ne) removed |= slab[j * ne + lane];
                    r |= slab[j * ne + ch];
                }
            }
            if (lane == 0) s_nkept = nkept;
        }
        __syncthreads();
    }
    const int total = s_nkept;
    for (int p = tid; p < total; p += BD_T) {
        const int rank = s_kept[p];
        const int row = min(max(A.cand_row[(size_t)c * A.M + rank], 0), A.M - 1);
        s_rank[row] = rank + 1;                                // (a row is a candidate of the class once)
    }
    __syncthreads();
    // ordered compaction over the proposal rows: a thread's rows are consecutive
    constexpr int PER = BD_MAX_ROWS / BD_T;
    int mine = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int r = tid * PER + q;
        mine += (r < A.M && s_rank[r] != 0) ? 1 : 0;
    }
    s_scan[tid] = mine;
    __syncthreads();
    for (int off = 1; off < BD_T; off <<= 1) {
        const int v = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int pos = s_scan[tid] - mine;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int r = tid * PER + q;
        if (r < A.M && s_rank[r] != 0) {
            A.keep_rank[(size_t)c * A.M + pos] = s_rank[r] - 1;
            ++pos;
        }
    }
    if (tid == 0) A.keep_count[c] = total;
}

__device__ __forceinline__ void bd_write_body(const BoxDetectArgs& A, const int c) {
    __shared__ int s_cnt[BD_MAX_CLASSES];
    const int t = threadIdx.x, C = A.K - 1;
    if (t < C) s_cnt[t] = min(max(A.keep_count[t], 0), A.M);
    __syncthreads();
    int base = 0, total = 0;
    for (int k = 0; k < C; ++k) {
        base += k < c ? s_cnt[k] : 0;
        total += s_cnt[k];
    }
    const int mine = s_cnt[c];
    for (int p = t; p < mine; p += BD_T) {
        const int rank = min(max(A.keep_rank[(size_t)c * A.M + p], 0), A.M - 1);
        const size_t src = (size_t)c * A.M + rank, dst = (size_t)base + p;
        A.out_boxes[dst * 4 + 0] = A.cand_box[src * 4 + 0];
        A.out_boxes[dst * 4 + 1] = A.cand_box[src * 4 + 1];
        A.out_boxes[dst * 4 + 2] = A.cand_box[src * 4 + 2];
        A.out_boxes[dst * 4 + 3] = A.cand_box[src * 4 + 3];
        A.out_scores[dst] = A.cand_score[src];
        A.out_labels[dst] = (long long)(c + 1);
        A.out_rows[dst] = A.cand_row[src];
    }
    const long long cap = (long long)A.M * C;
    for (long long r = (long long)total + (long long)c * BD_T + t; r < cap; r += (long long)C * BD_T) {
        A.out_boxes[r * 4 + 0] = A.out_boxes[r * 4 + 1] = A.out_boxes[r * 4 + 2] = A.out_boxes[r * 4 + 3] = 0.0f;
        A.out_scores[r] = 0.0f;
        A.out_labels[r] = 0ll;
        A.out_rows[r] = 0;
    }
    if (c == 0) {
        if (t == 0) A.out_count[0] = total;
        if (t < C) A.out_count[1 + t] = s_cnt[t];
    }
}

// ---- workspace layout (4-byte words; every section starts at a multiple of 4 words) -------------------------------------
struct BoxDetectLayout {
    size_t cand_count, cand_row, cand_score, cand_box, mask, keep_count, keep_rank, end;
};

__host__ __device__ static inline size_t bd_al4(size_t w) { return (w + 3) & ~(size_t)3; }

__host__ __device__ static inline BoxDetectLayout bd_layout(int M, int K) {
    const size_t C = (size_t)K - 1, nblk = (size_t)(M + NMS_T - 1) / NMS_T;
    BoxDetectLayout o;
    size_t w = 0;
    o.cand_count = w; w += bd_al4(C);
    o.cand_row = w; w += bd_al4(C * M);
    o.cand_score = w; w += bd_al4(C * M);
    o.cand_box = w; w += bd_al4(C * M * 4);
    o.mask = w; w += bd_al4(C * M * nblk * 2);
    o.keep_count = w; w += bd_al4(C);
    o.keep_rank = w; w += bd_al4(C * M);
    o.end = w;
    return o;
}

// the workspace sections of one image (or of the single-image call) behind `ws`
__host__ __device__ static inline void bd_set_workspace(BoxDetectArgs& A, void* ws) {
    const BoxDetectLayout o = bd_layout(A.M, A.K);
    int* wi = reinterpret_cast<int*>(ws);
    float* wf = reinterpret_cast<float*>(ws);
    A.cand_count = wi + o.cand_count;
    A.cand_row = wi + o.cand_row;
    A.cand_score = wf + o.cand_score;
    A.cand_box = wf + o.cand_box;
    A.mask = reinterpret_cast<unsigned long long*>(wi + o.mask);
    A.keep_count = wi + o.keep_count;
    A.keep_rank = wi + o.keep_rank;
}

// ---- one image -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BD_SORT_T) box_detect_cand_kernel(BoxDetectArgs A) { bd_cand_body(A, blockIdx.x); }
// blockIdx.y = class, blockIdx.x = (row tile, column tile)
__global__ void __launch_bounds__(NMS_T) box_detect_mask_kernel(BoxDetectArgs A) { bd_mask_body(A, blockIdx.y, blockIdx.x); }
__global__ void __launch_bounds__(BD_T) box_detect_scan_kernel(BoxDetectArgs A) { bd_scan_body(A, blockIdx.x); }
__global__ void __launch_bounds__(BD_T) box_detect_write_kernel(BoxDetectArgs A) { bd_write_body(A, blockIdx.x); }

// ---- several images: the image is one more grid dimension of the same four kernels -----------------------------------------
// A = the call (head / boxes / out_* at row 0 of image 0, count[0], out_count[0]; M, nblk and the workspace sections are
// per image and filled by bd_image), I = the validated row ranges, ws_off[b] = where image b's workspace segment starts (in
// 4-byte words; a multiple of 4).  A segment is laid out like the single-image call's workspace of M_b rows.
struct BoxDetectBatch {
    BoxDetectArgs A;
    int* ws;
    ImageRows I;
    unsigned long long ws_off[SMOT_MAX_IMAGES];
};

// the call as image b alone sees it: what smot_box_detect_post_fwd is given for that image's rows (b is workgroup-uniform:
// scalar loads from the kernel-argument segment)
__device__ __forceinline__ BoxDetectArgs bd_image(const BoxDetectBatch& B, const int b) {
    BoxDetectArgs A = B.A;
    const int r0 = B.I.row_start[b], C = A.K - 1;
    A.M = B.I.row_start[b + 1] - r0;
    A.nblk = (A.M + NMS_T - 1) / NMS_T;
    A.head += (size_t)r0 * A.ld;
    A.boxes += (size_t)r0 * 4;
    A.count += b;
    bd_set_workspace(A, B.ws + B.ws_off[b]);
    A.out_boxes += (size_t)r0 * C * 4;
    A.out_scores += (size_t)r0 * C;
    A.out_labels += (size_t)r0 * C;
    A.out_rows += (size_t)r0 * C;
    A.out_count += (size_t)b * A.K;
    return A;
}

// blockIdx.x = class, blockIdx.y = image
__global__ void __launch_bounds__(BD_SORT_T) box_detect_cand_batched_kernel(BoxDetectBatch B) {
    bd_cand_body(bd_image(B, blockIdx.y), blockIdx.x);
}
// blockIdx.x = (row tile, column tile) of the LARGEST image of the call, blockIdx.y = class, blockIdx.z = image
__global__ void __launch_bounds__(NMS_T) box_detect_mask_batched_kernel(BoxDetectBatch B) {
    const BoxDetectArgs A = bd_image(B, blockIdx.z);
    if ((int)blockIdx.x >= A.nblk * A.nblk) return;                  // (workgroup-uniform; an image without rows: nblk = 0)
    bd_mask_body(A, blockIdx.y, blockIdx.x);
}
__global__ void __launch_bounds__(BD_T) box_detect_scan_batched_kernel(BoxDetectBatch B) {
    bd_scan_body(bd_image(B, blockIdx.y), blockIdx.x);
}
__global__ void __launch_bounds__(BD_T) box_detect_write_batched_kernel(BoxDetectBatch B) {
    bd_write_body(bd_image(B, blockIdx.y), blockIdx.x);
}

static int bd_check_shapes(int M, int K) {
    SMOT_REQUIRE(M >= 1 && M <= BD_MAX_ROWS, "box_detect_post: M=%d not in [1,%d]", M, BD_MAX_ROWS);
    SMOT_REQUIRE(K >= 2 && K <= BD_MAX_CLASSES, "box_detect_post: num_classes=%d not in [2,%d]", K, BD_MAX_CLASSES);
    return SMOT_OK;
}

// the row ranges and per-image shapes of a batched call, checked before anything else; ws_off / *total: the images' workspace
// segments in 4-byte words
static int bd_check_batch(ImageRows* I, int num_images, const int* row_start, int M, int K, unsigned long long* ws_off,
                          unsigned long long* total, int* max_nblk) {
    int rc = fill_image_rows(I, num_images, row_start, M, "box_detect_post_batched");
    if (rc) return rc;
    unsigned long long w = 0;
    int nb = 0;
    for (int b = 0; b < num_images; ++b) {
        const int Mb = I->row_start[b + 1] - I->row_start[b];
        rc = bd_check_shapes(Mb > 0 ? Mb : 1, K);                    // (an image without rows is legal)
        if (rc) return rc;
        if (ws_off) ws_off[b] = w;
        w += bd_layout(Mb, K).end;
        nb = max(nb, (Mb + NMS_T - 1) / NMS_T);
    }
    if (ws_off)
        for (int b = num_images; b < SMOT_MAX_IMAGES; ++b) ws_off[b] = w;
    *total = w;
    *max_nblk = nb;
    return SMOT_OK;
}
}  // namespace smot

extern "C" long long smot_box_detect_post_ws_bytes(int M, int num_classes) {
    if (smot::bd_check_shapes(M, num_classes)) return -1;
    return (long long)smot::bd_layout(M, num_classes).end * 4;
}

extern "C" int smot_box_detect_post_fwd(const float* head_out, int ld, int num_classes, int reg_classes, const float* boxes,
                                        const int32_t* count, int M, float wx, float wy, float ww, float wh,
                                        float xform_clip, float clip_w, float clip_h, float score_thresh, float nms_thresh,
                                        void* ws, float* out_boxes, float* out_scores, int64_t* out_labels,
                                        int32_t* out_rows, int32_t* out_count, smot_stream_t stream) {
    using namespace smot;
    int rc = bd_check_shapes(M, num_classes);
    if (rc) return rc;
    SMOT_REQUIRE((reg_classes == num_classes || reg_classes == 2) && ld >= num_classes + 4 * reg_classes,
                 "box_detect_post: bad head shape K=%d KR=%d ld=%d", num_classes, reg_classes, ld);
    SMOT_REQUIRE(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f, "box_detect_post: regression weights must be positive");
    if (!(nms_thresh > 0.0f)) {
        set_error("box_detect_post: nms_thresh=%g (the reference's NMS returns the class unsuppressed there)", nms_thresh);
        return SMOT_ERR_UNSUPPORTED;
    }
    SMOT_REQUIRE(head_out && boxes && count && ws && out_boxes && out_scores && out_labels && out_rows && out_count,
                 "box_detect_post: null pointer");
    SMOT_REQUIRE(((uintptr_t)ws & 15) == 0, "box_detect_post: ws must be 16-byte aligned");
    BoxDetectArgs A;
    A.head = head_out;
    A.ld = ld;
    A.K = num_classes;
    A.KR = reg_classes;
    A.M = M;
    A.nblk = (M + NMS_T - 1) / NMS_T;
    A.boxes = boxes;
    A.count = count;
    A.wx = wx;
    A.wy = wy;
    A.ww = ww;
    A.wh = wh;
    A.xform_clip = xform_clip;
    A.clip_w = clip_w;
    A.clip_h = clip_h;
    A.score_thresh = score_thresh;
    A.nms_thresh = nms_thresh;
    bd_set_workspace(A, ws);
    A.out_boxes = out_boxes;
    A.out_scores = out_scores;
    A.out_labels = (long long*)out_labels;
    A.out_rows = out_rows;
    A.out_count = out_count;
    hipStream_t st = (hipStream_t)stream;
    const int C = num_classes - 1;
    hipLaunchKernelGGL(box_detect_cand_kernel, dim3(C), dim3(BD_SORT_T), 0, st, A);
    hipLaunchKernelGGL(box_detect_mask_kernel, dim3(A.nblk * A.nblk, C), dim3(NMS_T), 0, st, A);
    hipLaunchKernelGGL(box_detect_scan_kernel, dim3(C), dim3(BD_T), (size_t)NMS_T * A.nblk * 8, st, A);
    hipLaunchKernelGGL(box_detect_write_kernel, dim3(C), dim3(BD_T), 0, st, A);
    return check_launch("box_detect_post");
}

// ---- several images per call ---------------------------------------------------------------------------------------------
extern "C" long long smot_box_detect_post_batched_ws_bytes(int num_images, const int* row_start, int num_classes) {
    smot::ImageRows I;
    unsigned long long words = 0;
    int nb = 0;
    if (num_images < 1 || num_images > SMOT_MAX_IMAGES || row_start == nullptr) return -1;
    if (smot::bd_check_batch(&I, num_images, row_start, row_start[num_images], num_classes, nullptr, &words, &nb)) return -1;
    return (long long)words * 4;
}

extern "C" int smot_box_detect_post_batched_fwd(const float* head_out, int ld, int num_classes, int reg_classes,
                                                const float* boxes, const int32_t* count, int M, float wx, float wy, float ww,
                                                float wh, float xform_clip, float clip_w, float clip_h, float score_thresh,
                                                float nms_thresh, void* ws, float* out_boxes, float* out_scores,
                                                int64_t* out_labels, int32_t* out_rows, int32_t* out_count,
                                                smot_stream_t stream, int num_images, const int* row_start) {
    using namespace smot;
    BoxDetectBatch B;
    unsigned long long words = 0;
    int max_nblk = 0;
    int rc = bd_check_batch(&B.I, num_images, row_start, M, num_classes, B.ws_off, &words, &max_nblk);
    if (rc) return rc;
    SMOT_REQUIRE((reg_classes == num_classes || reg_classes == 2) && ld >= num_classes + 4 * reg_classes,
                 "box_detect_post_batched: bad head shape K=%d KR=%d ld=%d", num_classes, reg_classes, ld);
    SMOT_REQUIRE(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f,
                 "box_detect_post_batched: regression weights must be positive");
    if (!(nms_thresh > 0.0f)) {
        set_error("box_detect_post_batched: nms_thresh=%g (the reference's NMS returns the class unsuppressed there)",
                  nms_thresh);
        return SMOT_ERR_UNSUPPORTED;
    }
    SMOT_REQUIRE(count && ws && out_count && (M == 0 || (head_out && boxes && out_boxes && out_scores && out_labels && out_rows)),
                 "box_detect_post_batched: null pointer");
    SMOT_REQUIRE(((uintptr_t)ws & 15) == 0, "box_detect_post_batched: ws must be 16-byte aligned");
    BoxDetectArgs& A = B.A;
    A.head = head_out;
    A.ld = ld;
    A.K = num_classes;
    A.KR = reg_classes;
    A.M = 0;                         // (per image: bd_image)
    A.nblk = 0;
    A.boxes = boxes;
    A.count = count;
    A.wx = wx;
    A.wy = wy;
    A.ww = ww;
    A.wh = wh;
    A.xform_clip = xform_clip;
    A.clip_w = clip_w;
    A.clip_h = clip_h;
    A.score_thresh = score_thresh;
    A.nms_thresh = nms_thresh;
    A.cand_count = A.cand_row = A.keep_count = A.keep_rank = nullptr;
    A.cand_score = A.cand_box = nullptr;
    A.mask = nullptr;
    A.out_boxes = out_boxes;
    A.out_scores = out_scores;
    A.out_labels = (long long*)out_labels;
    A.out_rows = out_rows;
    A.out_count = out_count;
    B.ws = reinterpret_cast<int*>(ws);
    hipStream_t st = (hipStream_t)stream;
    const int C = num_classes - 1;
    const int tiles = max_nblk > 0 ? max_nblk * max_nblk : 1;       // (a call without rows still writes its counts)
    hipLaunchKernelGGL(box_detect_cand_batched_kernel, dim3(C, num_images), dim3(BD_SORT_T), 0, st, B);
    hipLaunchKernelGGL(box_detect_mask_batched_kernel, dim3(tiles, C, num_images), dim3(NMS_T), 0, st, B);
    hipLaunchKernelGGL(box_detect_scan_batched_kernel, dim3(C, num_images), dim3(BD_T), (size_t)NMS_T * max_nblk * 8, st, B);
    hipLaunchKernelGGL(box_detect_write_batched_kernel, dim3(C, num_images), dim3(BD_T), 0, st, B);
    return check_launch("box_detect_post_batched");
}
