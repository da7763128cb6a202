// K1+K2 fused — search-region pooling straight into the cross-correlation.
//
// Replaces, inside EMM.forward (reference EMM/track_core.py:49-53): TrackUtils.pad_feature
// (track_head/track_utils.py:87-107) -> SRPooler on the search regions (EMM/sr_pool.py:53-91, legacy
// ROIAlign [UPSTREAM]) -> xcorr_depthwise (EMM/xcorr.py:37-46).  The [N,C,30,30] search-region tensor
// (13.8 MB @30 tracks, written once and read once by the unfused path) never leaves the CU.
//
// Workgroup = (track, 8 channels); 4 waves, each owning 2 channels (planes).
//   1. The per-axis sample tables of the roi are built once per workgroup in LDS exactly as in
//      roi_align.hip (reference rounding sequence, padded extent, cells in the virtual border get
//      weight 0) together with the bounding window [ymin..ymax] x [xmin..xmax] of touched real cells.
//   2. Pooling is SEPARABLE: bin(ph,pw) = 1/g^2 * sum_iy sum_ix [ hx*col_iy(xlo) + lx*col_iy(xhi) ] with
//      col_iy(wx) = hy*V[ylo][wx] + ly*V[yhi][wx].  A lane owns window column wx: for every pooled row it
//      loads the (up to) four feature rows of the two y-samples — contiguous row segments, coalesced,
//      no LDS window — forms the two column values, and lane pw gathers its four column values with
//      ds_bpermute (cross-lane, no LDS storage).  Terms are added in the reference's (iy, ix) order; only
//      the factorisation (hy*hx)*v -> hx*(hy*v) differs: fp32 rounding level, held to (2 e32 + 2^-22) * sum w|v| of an
//      fp64 evaluation on the reference's own fp32 sample tables (e32: the fp32 reference's own error in that case,
//      <= 2^-21; measured here <= 2.4e-7 * sum w|v|: tests/test_roi_pool_edges.py).
//   3. The pooled 30x30 planes land in the same LDS image the xcorr kernel stages from HBM
//      (xcorr_patch2.h), the templates are staged next to them, and the FMA phase is the shared
//      xcorr_patch2_compute: responses are bit-identical to smot_xcorr_dw_fwd on the pooled planes.
// Windows wider than 64 columns (search regions far larger than their FPN level suggests: degenerate
// aspect ratios) take a workgroup-uniform slow path: per-bin gathers, same arithmetic as roi_align.hip.
#include "pool_launch.h"
#include "xcorr_patch2.h"
#include "xcorr_patch1.h"
#include "xcorr_f16x2.h"
#include "knobs.h"
#include <type_traits>

namespace smot {

constexpr int FX_CH = 8;          // channels per workgroup (2 per wave)

// EMM.extract_cache in one launch: the pool-only kernel also writes the next frame's search regions
// (update_boxes_in_pad_images + extend_bbox, reference track_utils.py:62-85,109-135; same arithmetic as
// search_region_kernel in roi_align.hip) from its (roi, channel-group 0) workgroup.
struct SrOut {
    float* sr;            // [R,4] or nullptr
    float pad, half_e, two_e, min_wh;
    long long* trace;     // phase trace (smot_debug_trace) or nullptr
    int abl;              // timing ablation of the generation-2 kernel (wrong results): 2 = no correlation phase
                          // (SMOT_FUSED_ABL=2).  A run-time switch around the row loads is NOT an option: the
                          // branch makes hipcc wait for every pair of loads (measured +2 us).
    const int* n_valid;   // device count of valid rois, or nullptr: rois >= *n_valid are skipped (the launch covers
                          // a CAPACITY when the count is still on the device — smot_emm_extract_cache_masked_fwd)
    int order;            // workgroup -> (roi, channel group) assignment: 0 = grid order, 1..3 = cost-sorted forms
                          // (fx_assign below; the measurement library can select any, SMOT_FUSED_ORDER)
    float* hint_out;      // pool-only kernel: write the cost-sorted roi list of the NEXT frame's search regions here
                          // (fx_write_hint below; [R] entries of SMOT_HINT_FLOATS floats) or nullptr
    const float* hint_in; // pooling + correlation kernel: such a list for ITS rois (written by the extraction that made
                          // them), read instead of ranking the rois again in every workgroup; or nullptr
    int hint_extra;       // hint writer with n_valid: the list ranks *n_valid + hint_extra rows — the rows the caller appended behind
                          // the valid ones before this launch (the tracking frame's carried dormant tracks: their boxes stand
                          // in `boxes` behind the active rows, and a dormant row's search region is search_region_of(its box),
                          // bit for bit what the extraction that created it wrote)
    int plan_pad[SMOT_MAX_LEVELS];   // hint writer: zero-pad cells per level of the NEXT frame's search-region pooling
                          // (the extraction itself pools un-padded maps); the finished sample tables in a hint entry are
                          // built against them
    float* plane_max;     // pooling + correlation kernel: the largest |response| of every plane [R][C], or nullptr — the tower
                          // kernel's split form scales a track's response by a power of two chosen from them (tower_wino.hip)
};
// One hint entry = SMOT_HINT_FLOATS dwords: {search region x1,y1,x2,y2, FPN level, roi index, 0, 0 | ymin, ymax, xmin, xmax of the
// touched window, pad cells / H / W of the level the tables were built against, 0 | y table [64] x int4 | x table [64] x int4}
// — since round 4 the FINISHED sample tables of the roi's 30x30 pooling ride along (exactly the entries the consumer's
// waves 0 / 1 would compute: reference rounding sequence, re-based rows / columns), so that a consumer workgroup loads 2 KB
// instead of ranking, dividing and building them.
constexpr int HINT_FLOATS = SMOT_HINT_FLOATS;
constexpr int HINT_BOUNDS = 8, HINT_GEOM = 12, HINT_YTAB = 16, HINT_XTAB = 16 + 256;
// ABI 12: behind the tables, entry x also carries the BY-ROI record of roi x (entries are sorted by rank, this record is
// not): {search region x1,y1,x2,y2 of roi x, its FPN level, the number of rois the list ranks, status word (entry 0's is
// THE status word of the list, zeroed by the writer), 0}.  The consumer verifies it against ITS `sr[x]` / `boxes[x]` / roi
// count (fx_verify_hint) — the list is a permutation of the rois it was made from by construction, so "every by-roi
// record equals the consumer's roi" is "the list describes exactly these rois".
constexpr int HINT_BYROI = HINT_XTAB + 256, HINT_STATUS = HINT_BYROI + 6;
static_assert(HINT_BYROI + 8 == HINT_FLOATS && (HINT_FLOATS * 4) % 32 == 0 && HINT_STATUS == SMOT_HINT_STATUS_WORD,
              "hint entry layout");

// base (wave-uniform, SGPR pair) + 32-bit unsigned BYTE offset: selects the `global_load v, v_off, s[base]`
// addressing form (one address VGPR per load instead of a 64-bit pair — 120 loads are in flight).
typedef const __attribute__((address_space(1))) char* gptr_t;
__device__ __forceinline__ float ld_off(gptr_t base, unsigned byte_off) {
    return *reinterpret_cast<const __attribute__((address_space(1))) float*>(base + byte_off);
}
// Launder a wave-uniform global pointer through an SGPR pair: stops loop-strength-reduction from turning
// "base(pl) + offset(s)" into one 64-bit per-lane pointer induction variable per load (60 of them spill).
__device__ __forceinline__ gptr_t uniform_base(const float* p) {
    unsigned long long a = reinterpret_cast<unsigned long long>(p);
    asm volatile("" : "+s"(a));
    return reinterpret_cast<gptr_t>(a);
}

#ifdef SMOT_DEBUG
#include "../../measure/csrc/sr_xcorr_gen2.inc"      // measurement library only (not product source)
#endif

// ---- third generation (default): sample tables in registers, wave-uniform addressing, gathers in bulk ------------
// What the phase traces of generation 2 showed (round-1 traces, ticks per workgroup @30 tracks):
// tables 4.3 k, pooling 14 k on average but 26 k for the 33..64-column windows, correlation 12 k.  The pooling was
// neither bandwidth- nor LDS-bound; it was a chain of dependent round trips: per pooled row one LDS read of the
// weights, four loads' waits, four ds_bpermute gathers waited for one by one — 15 rows x 2 batches x ~400 cycles —
// behind a load-issue phase that spent a quarter-rate v_mul_lo_u32 + add per load, behind an LDS table + barrier.
// This generation removes the chains:
//   * every wave builds BOTH sample tables itself, lane = sample, in registers (no LDS image, no barrier); the
//     window bounds come from one ballot per axis (the tables are monotone: first / last touched entry);
//   * row offsets and vertical weights are read with v_readlane (constant lane) into SGPRs: the 60 row loads of a
//     batch are buffer loads `voffset = lane column (+ plane), soffset = row` — no per-load VALU at all — and the
//     vertical taps are FMAs with an SGPR weight;
//   * all column sums of a batch are formed first, then all 60 gathers are issued back to back and waited for
//     ONCE, then the horizontal taps run — two LDS round trips per batch instead of thirty;
//   * windows <= 32 columns: a wave pools TWO planes side by side (plane = lane / 32, same rows and weights for
//     both halves, so everything stays wave-uniform) and the two waves of a plane pair split the pooled rows:
//     one batch of 60 loads per wave covers the pair; wider windows: one plane per wave, two batches, the second
//     batch's loads in flight while the first is gathered; windows wider than a wave are walked in 64-column
//     chunks by the same code (there is no separate slow path any more).
// Arithmetic per output is generation 2's, term by term (same fmaf chains), so results are bit-identical to it.
typedef int v4i_t __attribute__((ext_vector_type(4)));

// The row loads of the pooling by the maps' element type FT (sr_xcorr_fused9_body.h): one column per lane (4 or 2 bytes),
// or two adjacent columns (8 bytes at 4-byte alignment, or 4 bytes at 2-byte alignment: odd xmin, odd map width — the
// runtime runs the memory pipeline in its unaligned access mode).  The conversion to fp32 is exact (roi_common.h).
typedef int v2i_t __attribute__((ext_vector_type(2)));
template <typename FT>
struct fx_pair {
    typedef int type;
};
template <>
struct fx_pair<float> {
    typedef v2i_t type;
};
template <typename FT>
__device__ __forceinline__ typename fx_pair<FT>::type fx_load2(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, int soff) {
    if constexpr (sizeof(FT) == 4) {
        return __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, soff, 0);
    } else {
        return __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, soff, 0);
    }
}
template <typename FT>
__device__ __forceinline__ float fx_pair_elem(typename fx_pair<FT>::type v, int k) {
    if constexpr (sizeof(FT) == 4) {
        return __int_as_float(v[k]);
    } else {
        return k == 0 ? feat_of_pair<FT, 0>((unsigned)v) : feat_of_pair<FT, 1>((unsigned)v);
    }
}
template <typename FT>
__device__ __forceinline__ float fx_load1(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, int soff) {
    if constexpr (sizeof(FT) == 4) {
        return __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, soff, 0));
    } else {
        return feat_cvt<FT>((unsigned short)__builtin_amdgcn_raw_buffer_load_b16(rsrc, voff, soff, 0));
    }
}

__device__ __forceinline__ float rl_f(float v, int lane_const) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane_const));
}

// ---- row runs (sr_xcorr_fused9_body.h: the two-column pipeline of the 33 .. 64-column windows) -------------------------
// A batch of NE samples names 2 NE rows (lo_0, hi_0, lo_1, hi_1, ...) and loads each of them, although consecutive
// samples almost always share a row (hi(s) == lo(s + 1), or both rows when the sample step is below one row).  Where all
// rows of a batch lie within RMAX rows from its first entry's — a RUN — those consecutive rows are loaded ONCE into one
// register tuple, and every tap of the vertical FMA chain reads its row out of the tuple by its wave-uniform index.
// Same cells, same operands in the same order: bit-identical.
// How the uniform index selects a register (profiles/pool_row_runs_ab.json; the parent is at 52.82 us per step):
//   * chosen, 51.65 us: the GPR index mode on the FMA's own source operand (s_set_gpr_idx_on idx, SRC0 — the instruction
//     hipcc itself emits for a uniform dynamic index), one switch for the two columns of a lane — no vector instruction
//     beside the FMAs that were there already;
//   * measured and dropped, 54.34 us: the compiler's form of `rows[idx]`, the same mode around a v_mov_b32 per operand — 40
//     more vector instructions per batch beside its 40 FMAs, more than the 8 loads it saves;
//   * not built: a scalar-compare select chain (RMAX - 1 v_cndmask per operand: worse than the v_mov) and staging the rows
//     in the wave's own image rows (the taps then go through the LDS pipe, which the horizontal taps already load).
typedef float fx_rows_t __attribute__((ext_vector_type(32)));

// The vertical chains of a pooled row (G = 2: lo_0, hi_0, lo_1, hi_1) for the two adjacent columns of a lane, which are
// registers i and i + 1 of the tuple: c = fmaf(w3, r[i3], fmaf(w2, r[i2], fmaf(w1, r[i1], fmaf(w0, r[i0], 0)))), the registers
// read through the GPR index; the mode is off again behind the chains.
// The indexed operand must be written as the tuple's FIRST register, and inline assembly cannot name a sub-register of an
// operand: the tuple is therefore bound to v[32:63] by its constraint and the text says v32 / v33.  The constraint makes that
// correct whatever the allocator does; it puts the row loads straight into v[32:55] (no copies, read off the ISA).
__device__ __forceinline__ void fx_run_fma4x2(const fx_rows_t r, int i0, int i1, int i2, int i3, float w0, float w1, float w2, float w3,
                                              float* c0, float* c1) {
    float a, b;
    asm volatile("s_set_gpr_idx_on %3, gpr_idx(SRC0)\n\t"
                 "v_fma_f32 %0, v32, %7, 0\n\t"
                 "v_fma_f32 %1, v33, %7, 0\n\t"
                 "s_set_gpr_idx_on %4, gpr_idx(SRC0)\n\t"
                 "v_fma_f32 %0, v32, %8, %0\n\t"
                 "v_fma_f32 %1, v33, %8, %1\n\t"
                 "s_set_gpr_idx_on %5, gpr_idx(SRC0)\n\t"
                 "v_fma_f32 %0, v32, %9, %0\n\t"
                 "v_fma_f32 %1, v33, %9, %1\n\t"
                 "s_set_gpr_idx_on %6, gpr_idx(SRC0)\n\t"
                 "v_fma_f32 %0, v32, %10, %0\n\t"
                 "v_fma_f32 %1, v33, %10, %1\n\t"
                 "s_set_gpr_idx_off"
                 : "=&v"(a), "=&v"(b)
                 : "{v[32:63]}"(r), "s"(i0), "s"(i1), "s"(i2), "s"(i3), "s"(w0), "s"(w1), "s"(w2), "s"(w3));
    *c0 = a;
    *c1 = b;
}

// Do the NB batches of NE samples in `ye` (lane = sample: {row offset lo, hi, weight lo, hi}, offsets in bytes of an fp32
// map with rows of `row_bytes`) each lie within `rows` rows from their first entry's row?  Wave-uniform.  That is ALL a run
// needs: every entry then names a row of the loaded set, and the chain reads exactly the row it names.  (Rows that never
// step back and span at most `rows` are the common case; an order is not required — at a sample step below one row the
// entries of consecutive samples read 3, 4, 3, 4.)  Only the first n_real lanes are judged: the samples behind them belong to
// masked tail rows, whose sums are never stored.  Not a run: an entry re-based to the window's first row when that row lies
// before the batch's first (zero weight at the bottom border, or an integral coordinate), a bin more than two rows tall,
// a NaN weight.
template <int NE, int NB>
__device__ __forceinline__ int fx_run_base(const int4 ye, const int lane) {       // the first entry's row of the lane's batch
    int base = __builtin_amdgcn_readlane(ye.x, 0);
#pragma unroll
    for (int b = 1; b < NB; ++b) base = lane >= b * NE ? __builtin_amdgcn_readlane(ye.x, b * NE) : base;
    return base;
}
template <int NE, int NB>
__device__ __forceinline__ bool fx_run_within(const int rows, const int4 ye, const int lane, const int n_real, const unsigned row_bytes) {
    static_assert(NE * NB <= 64, "one lane per sample");
    const int base = fx_run_base<NE, NB>(ye, lane);
    const unsigned dl = (unsigned)(ye.x - base), dh = (unsigned)(ye.y - base), far = (unsigned)(rows - 1) * row_bytes;   // (a row before the base wraps)
    const float wl = __int_as_float(ye.z), wh = __int_as_float(ye.w);
    const bool ok = (dl <= far) & (dh <= far) & (wl == wl) & (wh == wh);
    // (row_bytes: the bound under which fx_run_index's quotient is exact)
    return row_bytes <= (1u << 18) && n_real > 0 && __ballot((lane < n_real) & !ok) == 0ull;
}
// The tuple indices of a run's entries: the row relative to the batch's first entry, times NV registers per row; 0 for the
// unjudged lanes.  Offsets are whole multiples of row_bytes and below 2^23: the rounded quotient is exact.
template <int NE, int NB, int NV>
__device__ __forceinline__ void fx_run_index(const int4 ye, const int lane, const int n_real, const unsigned row_bytes, int* il, int* ih) {
    const int base = fx_run_base<NE, NB>(ye, lane);
    const float inv = __builtin_amdgcn_rcpf((float)row_bytes);
    *il = lane < n_real ? NV * (int)((float)(unsigned)(ye.x - base) * inv + 0.5f) : 0;
    *ih = lane < n_real ? NV * (int)((float)(unsigned)(ye.y - base) * inv + 0.5f) : 0;
}

// update_boxes_in_pad_images + extend_bbox (track_utils.py:62-85,109-135) for one box: the next frame's search region.
__device__ __forceinline__ float4 search_region_of(float b0, float b1, float b2, float b3, const SrOut& S) {
    const float bx1 = add_rn(b0, S.pad), by1 = add_rn(b1, S.pad);
    const float bx2 = add_rn(b2, S.pad), by2 = add_rn(b3, S.pad);
    const float bw = add_rn(sub_rn(bx2, bx1), 1.0f), bh = add_rn(sub_rn(by2, by1), 1.0f);
    const float w_ext = max_nan(div_rn(sub_rn(S.min_wh, bw), S.two_e), mul_rn(bw, S.half_e));
    const float h_ext = max_nan(div_rn(sub_rn(S.min_wh, bh), S.two_e), mul_rn(bh, S.half_e));
    return make_float4(sub_rn(bx1, w_ext), sub_rn(by1, h_ext), add_rn(bx2, w_ext), add_rn(by2, h_ext));
}

// The pooling + correlation kernel of the NEXT frame ranks its rois by cost class in every one of its workgroups
// (fx_assign below: ~6.5 k cycles at the head of each, two vector-memory round trips on lines all CUs want at once).
// The extraction that creates those rois knows everything the ranking needs one frame earlier: one wave of one extra
// workgroup of the template-pooling launch ranks them ONCE and writes the sorted list — entry k = the roi of rank k
// with its search region and FPN level — so that a consumer workgroup needs one scalar load of its own entry.
// Same classes and the same order as fx_assign order 1 (class descending, roi ascending); the consumer's results do
// not depend on it (any permutation of the rois is a valid assignment).
// Workgroup x of the extraction launch's extra row writes the entry of roi x: both of its first two waves rank the rois
// (lane = roi, three ballots per 64 rois: the rank of roi x is read out of its lane), wave 0 builds the y table and wave 1
// the x table of the roi's NEXT-frame search region exactly as the consumer's waves 0 / 1 would (same code, same rounding
// sequence), against the pad cells the next frame's pooling uses.
template <int RXN, int G>
__device__ __forceinline__ void fx_write_hint(const LevelParams& P, const float* __restrict__ boxes, const SrOut& S,
                                              const int* n_valid, float* hint_out, int NT, int x, int wave, int lane) {
    if (NT > 256 || wave >= 2) return;                         // (the consumer keeps grid order beyond 256 rois)
    const int nv = (n_valid != nullptr) ? min(*n_valid + S.hint_extra, NT) : NT;
    if (x >= nv) return;
    unsigned long long mask[4][3];
    int cnt[3] = {0, 0, 0};
    int cl[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int t = lane + 64 * p;
        cl[p] = -1;
        if (64 * p < nv && t < nv) {
            const float4 b4 = *reinterpret_cast<const float4*>(boxes + (size_t)t * 4);
            int lvl = 0;
            if (P.num_levels > 1) lvl = map_level(boxes + (size_t)t * 4, P.k_min, P.k_max);
            float scale = P.scale[0];
#pragma unroll
            for (int l = 1; l < SMOT_MAX_LEVELS; ++l) scale = (lvl == l) ? P.scale[l] : scale;
            const float4 srb = search_region_of(b4.x, b4.y, b4.z, b4.w, S);
            const float ww = (srb.z - srb.x) * scale;                                    // window width in cells
            cl[p] = ww <= 30.0f ? 0 : (ww <= 62.0f ? 1 : 2);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mask[p][c] = __ballot(cl[p] == c);
            cnt[c] += __popcll(mask[p][c]);
        }
    }
    const int px = x >> 6, lx = x & 63;
    int cx = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
        if (p == px) cx = __builtin_amdgcn_readlane(cl[p], lx);
    int rank = cx == 2 ? 0 : (cx == 1 ? cnt[2] : cnt[2] + cnt[1]);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const unsigned long long mk = cx == 2 ? mask[p][2] : (cx == 1 ? mask[p][1] : mask[p][0]);
        if (p < px) rank += __popcll(mk);
        if (p == px) rank += __popcll(mk & ((1ull << lx) - 1ull));
    }
    // the roi itself (wave-uniform scalar loads)
    const float* bx = boxes + (size_t)x * 4;
    const float4 roi = search_region_of(bx[0], bx[1], bx[2], bx[3], S);
    int lvl = 0;
    if (P.num_levels > 1) lvl = map_level(bx, P.k_min, P.k_max);
    lvl = __builtin_amdgcn_readfirstlane(lvl);
    const int H = P.H[lvl], W = P.W[lvl], pad = S.plan_pad[lvl];
    const float scale = P.scale[lvl];
    const float x1 = mul_rn(roi.x, scale), y1 = mul_rn(roi.y, scale);
    const float x2 = mul_rn(roi.z, scale), y2 = mul_rn(roi.w, scale);
    const float bin_h = div_rn(fmaxf(sub_rn(y2, y1), 1.0f), (float)RXN);
    const float bin_w = div_rn(fmaxf(sub_rn(x2, x1), 1.0f), (float)RXN);
    int* ent = reinterpret_cast<int*>(hint_out) + (size_t)rank * HINT_FLOATS;
    int lo = 0, hi = 0;
    float wl = 0.0f, wh = 0.0f;
    if (lane < RXN * G) {
        if (wave == 0) {
            axis_sample(y1, bin_h, G, lane, H, pad, &lo, &hi, &wl, &wh);
        } else {
            axis_sample(x1, bin_w, G, lane, W, pad, &lo, &hi, &wl, &wh);
        }
    }
    int mn = 0x7fffffff, mx = -1;
    const unsigned long long m = __ballot(wl != 0.0f || wh != 0.0f);
    if (m != 0ull) {
        mn = __builtin_amdgcn_readlane((wl != 0.0f) ? lo : hi, __ffsll((long long)m) - 1);
        mx = __builtin_amdgcn_readlane((wh != 0.0f) ? hi : lo, 63 - __clzll((long long)m));
    }
    const int rl = (wl != 0.0f) ? lo : mn, rh = (wh != 0.0f) ? hi : mn;
    int4 e;
    if (wave == 0) {
        e.x = (int)((unsigned)(rl * W) * 4u);
        e.y = (int)((unsigned)(rh * W) * 4u);
    } else {
        e.x = (wl != 0.0f) ? lo - mn : 0;
        e.y = (wh != 0.0f) ? hi - mn : 0;
    }
    e.z = __float_as_int(wl);
    e.w = __float_as_int(wh);
    *reinterpret_cast<int4*>(ent + (wave == 0 ? HINT_YTAB : HINT_XTAB) + 4 * lane) = e;
    if (lane == 0) {
        ent[HINT_BOUNDS + 2 * wave] = mn;
        ent[HINT_BOUNDS + 2 * wave + 1] = mx;
        if (wave == 0) {
            float4* o = reinterpret_cast<float4*>(ent);
            o[0] = roi;
            o[1] = make_float4(__int_as_float(lvl), __int_as_float(x), 0.f, 0.f);
            ent[HINT_GEOM + 0] = pad;
            ent[HINT_GEOM + 1] = H;
            ent[HINT_GEOM + 2] = W;
            ent[HINT_GEOM + 3] = __float_as_int(scale);           // (the tables were built with this scale: part of the stamp)
            // the by-roi record of roi x, in entry x (not entry `rank`): what the consumer verifies against its own tensors
            int* rec = reinterpret_cast<int*>(hint_out) + (size_t)x * HINT_FLOATS + HINT_BYROI;
            float4* r4 = reinterpret_cast<float4*>(rec);
            r4[0] = roi;
            rec[4] = lvl;
            rec[5] = nv;
            rec[6] = 0;                                            // status word (entry 0's is the list's)
            rec[7] = 0;
        }
    }
}

// The consumer's check of an order hint (VERDICT r4 "next" #2: detect, not trust).  A workgroup of grid row 0 verifies the
// by-roi record of ITS grid column x against the launch's own tensors: sr[x] bit for bit, the FPN level recomputed from
// boxes[x], and the number of rois.  Every address is known at kernel start, so the loads travel beside the entry's own
// (no dependent round trip), one dword per lane, and the comparison runs in a wave that would otherwise wait at the table
// barrier: no cost on the workgroup's chain.  A mismatch raises the list's status word (entry 0): the decode kernel of the
// same head then writes NaN boxes and scores for every row (smot_emm_track_fwd), the solver's record counts them, and the
// tracking loop raises — a stale hint is reported, never silently used.
__device__ __forceinline__ void fx_verify_hint(const LevelParams& P, const float* __restrict__ sr,
                                               const float* __restrict__ boxes, const float* hint, int x, int NT, int lane) {
    const int* rec = reinterpret_cast<const int*>(hint) + (size_t)x * HINT_FLOATS + HINT_BYROI;
    int v = 0;
    if (lane < 4) {
        v = __float_as_int(sr[(size_t)x * 4 + lane]);
    } else if (lane < 8) {
        v = __float_as_int(boxes[(size_t)x * 4 + lane - 4]);
    } else if (lane < 14) {
        v = rec[lane - 8];
    }
    const int up = __shfl_up(v, 8);                              // lanes 8..11: the consumer's sr[x] beside the record's
    float b4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) b4[i] = __int_as_float(__builtin_amdgcn_readlane(v, 4 + i));
    int lvl = 0;
    if (P.num_levels > 1) lvl = map_level(b4, P.k_min, P.k_max);
    const bool bad = (lane >= 8 && lane < 12 && up != v) || (lane == 12 && v != lvl) || (lane == 13 && v != NT);
    if (__ballot(bad) != 0ull && lane == 0)
        atomicOr(reinterpret_cast<int*>(const_cast<float*>(hint)) + HINT_STATUS, 1);
}

// Which (roi, channel group) a workgroup takes.  The grid is (rois, channel groups) and the hardware dispatches
// workgroups in linear order (x fastest), L and L + 256 onto the same CU while the launch fits the chip; a roi whose
// window is wider than 32 columns costs about twice a narrow one (two row blocks per plane), so the order in which
// rois appear in the caller's tensor decided how evenly the CUs were loaded (measure/debug/pairing_probe.py: the same 30
// boxes, 18.9 us in the benchmark's size-cycling order, 17.6 us sorted by width; 49.2 vs 42.5 us at 100).  Every
// workgroup therefore ranks the rois by a cost class itself — lane = roi, three ballots per 64 rois, all wave-uniform
// — and takes its item from the cost-sorted list; results do not depend on the assignment (it is a bijection).
//   order 1: item i = L of the list sorted by (class descending, roi, channel group)
//   order 2: the first 256 workgroups take the list from the front, the next 256 from the back (expensive with cheap
//            on a CU), the rest the middle in descending order
//   order 3: grid position x -> the roi of rank x (channel group = grid y, as in grid order)
// Rois at or past *n_valid keep their own index (they return at once).  More than 256 rois: grid order.
// Returns true when the roi's box and FPN level are handed back as well (read out of the lane that ranked it: the
// workgroup's own roi loads — a second dependent memory round trip — are then not needed).
__device__ __forceinline__ bool fx_assign(const LevelParams& P, const float* __restrict__ sr,
                                          const float* __restrict__ boxes, const int* __restrict__ n_valid, int order,
                                          int by, int ny, const float* __restrict__ hint, int NT, int lane, int* n_out,
                                          int* cg_out, float4* roi_out, int* lvl_out, int* k_out) {
    // (by, ny): the workgroup's row and the number of rows of the (roi, channel group) grid — blockIdx.y / gridDim.y
    // less the hint row of an extraction launch; NT = gridDim.x (a kernel argument: see FX_LEAD_PARAMS)
    int n = blockIdx.x, cg = by;
    *n_out = n;
    *cg_out = cg;
    if (order == 0 || NT > 256 || NT < 2) return false;
    const int T = NT * ny, L = by * NT + blockIdx.x;
    if (hint != nullptr && order == 1 && n_valid == nullptr) {
        // the list was made when the rois were (fx_write_hint): one scalar load of this workgroup's entry
        const int k = L / ny;
        *cg_out = L - k * ny;
        *k_out = k;
        // through the constant address space: a wave-uniform address there is a scalar load (one s_load_dwordx8 per
        // wave through the scalar cache; as a plain global pointer hipcc issues vector loads — it cannot see that
        // nothing writes the list during this launch)
        typedef int v8i_t __attribute__((ext_vector_type(8)));
        const v8i_t e = *reinterpret_cast<const __attribute__((address_space(4))) v8i_t*>(
            reinterpret_cast<unsigned long long>(hint) + (unsigned long long)k * (HINT_FLOATS * 4));
        roi_out->x = __int_as_float(e[0]);
        roi_out->y = __int_as_float(e[1]);
        roi_out->z = __int_as_float(e[2]);
        roi_out->w = __int_as_float(e[3]);
        *lvl_out = min(max(e[4], 0), P.num_levels - 1);        // (a stale list must not index out of range)
        *n_out = min(max(e[5], 0), NT - 1);
        return true;
    }
    const int nv = (n_valid != nullptr) ? min(*n_valid, NT) : NT;
    constexpr int SLOTS = 256;                       // CUs: one workgroup each per dispatch round
    int i = L;
    if (order == 2) {
        const int r = L / SLOTS, q = L - r * SLOTS;
        if (r == 1) {
            i = T - 1 - q;
        } else if (r >= 2) {
            i = SLOTS + (L - 2 * SLOTS);
        }
    }
    int k;
    if (order == 3) {
        k = blockIdx.x;
    } else {
        k = i / ny;
        cg = i - k * ny;
    }
    *cg_out = cg;
    if (k >= nv) {
        *n_out = k;
        return false;
    }
    unsigned long long mask[4][3];
    int cnt[3] = {0, 0, 0};
    float rbx[4], rby[4], rbz[4], rbw[4];
    int rl[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        int cls = -1;
        const int t = lane + 64 * p;
        rbx[p] = rby[p] = rbz[p] = rbw[p] = 0.0f;
        rl[p] = 0;
        if (64 * p < nv && t < nv) {
            int lvl = 0;
            if (P.num_levels > 1) lvl = map_level(boxes + (size_t)t * 4, P.k_min, P.k_max);
            float scale = P.scale[0];
#pragma unroll
            for (int l = 1; l < SMOT_MAX_LEVELS; ++l) scale = (lvl == l) ? P.scale[l] : scale;
            const float4 b4 = *reinterpret_cast<const float4*>(sr + (size_t)t * 4);
            rbx[p] = b4.x;
            rby[p] = b4.y;
            rbz[p] = b4.z;
            rbw[p] = b4.w;
            rl[p] = lvl;
            const float ww = (b4.z - b4.x) * scale;                                         // window width in cells
            cls = ww <= 30.0f ? 0 : (ww <= 62.0f ? 1 : 2);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mask[p][c] = __ballot(cls == c);
            cnt[c] += __popcll(mask[p][c]);
        }
    }
    int m = k, csel = 2;
    if (m >= cnt[2]) {
        m -= cnt[2];
        csel = 1;
        if (m >= cnt[1]) {
            m -= cnt[1];
            csel = 0;
        }
    }
    int psel = 0;
    bool done = false;
    unsigned long long msel = 0ull;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const unsigned long long mk = csel == 2 ? mask[p][2] : (csel == 1 ? mask[p][1] : mask[p][0]);
        const int pc = __popcll(mk);
        if (!done) {
            if (m < pc) {
                psel = p;
                msel = mk;
                done = true;
            } else {
                m -= pc;
            }
        }
    }
    const unsigned long long below = msel & ((1ull << lane) - 1ull);
    const bool hit = ((msel >> lane) & 1ull) != 0ull && __popcll(below) == m;
    const unsigned long long b = __ballot(hit);
    if (b == 0ull) return false;                                  // (cannot happen: k < nv)
    const int ln = __ffsll((long long)b) - 1;
    *n_out = ln + 64 * psel;
    float sx = rbx[0], sy = rby[0], sz = rbz[0], sw = rbw[0];
    int lsel = rl[0];
#pragma unroll
    for (int p = 1; p < 4; ++p)
        if (psel == p) {                                         // wave-uniform
            sx = rbx[p];
            sy = rby[p];
            sz = rbz[p];
            sw = rbw[p];
            lsel = rl[p];
        }
    roi_out->x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sx), ln));
    roi_out->y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sy), ln));
    roi_out->z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sz), ln));
    roi_out->w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sw), ln));
    *lvl_out = __builtin_amdgcn_readlane(lsel, ln);
    return true;
}

// MM: the correlation on the matrix pipe (xcorr_f16x2.h) — the product's form since round 6.  A plane's slot then holds its
// image (fp32, later the two fp16 half images in place) and the even / odd Toeplitz rows of its template instead of the fp32
// template: 9,024 B instead of 6,080 per plane, TWO workgroups per CU instead of three (76 KB of LDS each).
// MM == 2: the LEAN layout of the same (xl_*: 5,760 B per plane) — three workgroups per CU again.
// The kernel's body is in sr_xcorr_fused9_body.h (shared with the batched form below).

// Argument order, for every form of the kernel.  The leading 14 dwords arrive in user SGPRs with the wave (kernel-argument
// preload, build.py), everything behind them through the kernel-argument segment; ordered by first use:
//   hint     the order hint: the list this launch honours (XCORR: SrOut::hint_in) or writes (pool-only: SrOut::hint_out) — the
//            consumer's entry, tables and by-roi record are its first loads, the writer's row its first branch;
//   n_valid  the masked form's count (a scalar load and the first early return);
//   sr, boxes  the rois (fx_assign / fx_verify_hint, the extraction's own roi);
//   trace    the phase tracer's null test is the kernel's first instruction;
//   order, grid_nx, grid_ny  the assignment; grid_nx / grid_ny = gridDim.x / gridDim.y, which were reads through the
//            implicit-argument pointer (behind the segment, in front of the hint entry's address);
//   C        the channel tail.
// The template pointer, the outputs (search regions and templates of the extraction role: SrOut::sr, x_debug) and the structs
// do not fit the user SGPRs: their first use is behind the assignment's round trip.  SrOut keeps its members of the same
// names for the host code and the generation-2 kernel; the kernels here read the leading arguments.
#define FX_LEAD_PARAMS                                                                                                  \
    float *hint, const int *n_valid, const float *__restrict__ sr, const float *__restrict__ boxes,                     \
        long long *__restrict__ trace, int order, int grid_nx, int grid_ny, int C
#define FX_TAIL_PARAMS                                                                                                  \
    const float *__restrict__ z, float *__restrict__ resp, float *__restrict__ x_debug, int32_t *__restrict__ levels_out, \
        LevelParams P, SrOut S
template <int RX, int RZ, int G, bool XCORR, int NCH = FX_CH, bool P2 = false, int MM = 0>
__global__ void __launch_bounds__(64 * NCH, (P2 || MM == 1) ? 4 : 6) // <= 80 VGPRs: THREE workgroups (24 waves) per CU (LDS allows three)
sr_xcorr_fused9_kernel(FX_LEAD_PARAMS, FX_TAIL_PARAMS) {
    constexpr bool BATCHED = false;
    constexpr NoImages I{};
    using FT = float;
    constexpr bool NHWC = false;
#include "sr_xcorr_fused9_body.h"
}

// A batch of images (smot_emm_*_batched_fwd): rows, outputs and the order hint as for one image of ΣN rois; every workgroup
// adds its roi's image (I.row_start) to the level's 64-bit base address.
template <int RX, int RZ, int G, bool XCORR, int NCH = FX_CH, int MM = 0>
__global__ void __launch_bounds__(64 * NCH, MM == 1 ? 4 : 6)
sr_xcorr_fused9_batched_kernel(FX_LEAD_PARAMS, FX_TAIL_PARAMS, ImageRows I) {
    constexpr bool BATCHED = true;
    constexpr bool P2 = false;
    using FT = float;
    constexpr bool NHWC = false;
#include "sr_xcorr_fused9_body.h"
}

// The same two kernels on fp16 / bf16 maps (FT = f16_t / bf16_t; smot_*_typed_fwd): P.feat[] is read as `const FT*`, the
// image offset of the batched form is in elements of FT.  Only the product's forms exist (no A/B variants).
template <typename FT, int RX, int RZ, int G, bool XCORR, int MM = 0>
__global__ void __launch_bounds__(64 * FX_CH, MM == 1 ? 4 : 6)
sr_xcorr_fused9_half_kernel(FX_LEAD_PARAMS, FX_TAIL_PARAMS) {
    static_assert(sizeof(FT) == 2, "fp16 / bf16 maps");
    constexpr bool BATCHED = false;
    constexpr NoImages I{};
    constexpr int NCH = FX_CH;
    constexpr bool P2 = false;
    constexpr bool NHWC = false;
#include "sr_xcorr_fused9_body.h"
}
template <typename FT, int RX, int RZ, int G, bool XCORR, int MM = 0>
__global__ void __launch_bounds__(64 * FX_CH, MM == 1 ? 4 : 6)
sr_xcorr_fused9_half_batched_kernel(FX_LEAD_PARAMS, FX_TAIL_PARAMS, ImageRows I) {
    static_assert(sizeof(FT) == 2, "fp16 / bf16 maps");
    constexpr bool BATCHED = true;
    constexpr int NCH = FX_CH;
    constexpr bool P2 = false;
    constexpr bool NHWC = false;
#include "sr_xcorr_fused9_body.h"
}

// The product's forms on CHANNELS-LAST maps of every element type (SMOT_FEAT_CHANNELS_LAST; FT = float / f16_t / bf16_t):
// the body's pooling stage is sr_pool_nhwc_stage.h, everything else — assignment, order hint, sample tables, LDS images,
// correlation, write-out — is the NCHW kernels' text, and the static LDS is theirs (76,176 B for the 30 / 15 matrix form).
// One kernel per form: a single image is a batch of one.  (The stage keeps a row's 8 channels of column sums and taps in
// registers: 128 VGPRs, two workgroups of eight waves per CU, for every form.)
template <typename FT, int RX, int RZ, int G, bool XCORR, int MM = 0>
__global__ void __launch_bounds__(64 * FX_CH, 4)
sr_xcorr_fused9_nhwc_kernel(FX_LEAD_PARAMS, FX_TAIL_PARAMS, ImageRows I) {
    constexpr bool BATCHED = true;
    constexpr int NCH = FX_CH;
    constexpr bool P2 = false;
    constexpr bool NHWC = true;
#include "sr_xcorr_fused9_body.h"
}

}  // namespace smot


// Launch the pooling(+correlation) kernel: generation 3 in the product library; the measurement library can
// select generation 2 (SMOT_FUSED_GEN=2) for A/B runs.
namespace smot {
constexpr int FX_ORDER_DEFAULT = 1;
static inline int fused_order() {          // SMOT_FUSED_ORDER: 0 = default, 1..3 = a form of fx_assign, 4 = grid order
    const int k = knobs().fused_order;
    return k == 0 ? FX_ORDER_DEFAULT : (k == 4 ? 0 : k);
}
// An order hint is written / honoured for this many rois (fx_write_hint / fx_assign: one wave ranks up to 256 rois; the
// list has the default order's form; the measurement library's generation-2 kernel knows nothing of it).
static inline bool order_hint_rois(int N, bool consumer) {
    if (knobs().fused_gen == 2 || knobs().no_hint >= (consumer ? 1 : 2)) return false;      // (constant false: product)
    return N >= 2 && N <= 256 && fused_order() == 1;
}
static inline bool half_maps() { return feat_type() != SMOT_FEAT_F32; }

// The ONE launch site of the kernel: pooling alone (XCORR = false: RX = 7, 15 or 30 bins) or feeding the correlation
// (XCORR = true: RX = 30, on the matrix pipe — MM = 1).  The wrapper by (channels_last(), feat_type(), I): I = the row ranges
// of a batch, or nullptr for one image of grid.x rois (the channels-last kernels then take it as a batch of one).
template <int RX, bool XCORR>
static void launch_fused(dim3 grid, hipStream_t st, const LevelParams& P, int C, const float* rois, const float* boxes,
                         const float* z, float* resp, float* out, int32_t* levels_out, const SrOut& S, const ImageRows* I) {
    constexpr int MM = (RX == 30 && XCORR) ? 1 : 0;
    // (the batched wrappers and the channels-last ones take row ranges behind the single-image wrappers' arguments)
    float* const hint = XCORR ? const_cast<float*>(S.hint_in) : S.hint_out;      // (the kernels' leading arguments: FX_LEAD_PARAMS)
    auto launch = [&](auto kernel, size_t smem, const auto&... rows) {
        SMOT_LAUNCH(kernel, grid, dim3(512), smem, st, hint, S.n_valid, rois, boxes, S.trace, S.order, (int)grid.x, (int)grid.y,
                    C, z, resp, out, levels_out, P, S, rows...);
    };
    if (channels_last()) {
        with_feat_type([&](auto ft) {
            launch(sr_xcorr_fused9_nhwc_kernel<decltype(ft), RX, 15, 2, XCORR, MM>, 0, I ? *I : one_image_rows((int)grid.x));
        });
        return;
    }
    if (half_maps()) {
        SMOT_HALF_TYPES(if (I) launch(sr_xcorr_fused9_half_batched_kernel<FT, RX, 15, 2, XCORR, MM>, 0, *I);
                        else launch(sr_xcorr_fused9_half_kernel<FT, RX, 15, 2, XCORR, MM>, 0))
        return;
    }
    if (I) {
        launch(sr_xcorr_fused9_batched_kernel<RX, 15, 2, XCORR, FX_CH, MM>, 0, *I);
        return;
    }
#ifdef SMOT_DEBUG
    // A/B switches of the measurement library: fp32 NCHW maps of one image only
    if constexpr (RX != 7) {
        if (knobs().fused_gen == 2 && S.n_valid == nullptr) {      // (generation 2 has no masked form)
            hipLaunchKernelGGL((sr_xcorr_fused8_kernel<RX, 15, 2, XCORR>), grid, dim3(512), 0, st, P, C, rois, boxes, z, resp,
                               out, levels_out, S);
            return;
        }
    }
    if constexpr (MM == 1) {
        if (knobs().fused_abl == 8 || knobs().fused_abl == 9) {
            // SMOT_FUSED_ABL=8: the fp32 FMA correlation of rounds 2-5; 9: the same with 26 KB of unused dynamic LDS, i.e. at
            // TWO workgroups per CU like the matrix form (what the third workgroup is worth)
            launch(sr_xcorr_fused9_kernel<RX, 15, 2, XCORR>, knobs().fused_abl == 9 ? 26000 : 0);
            return;
        }
        if (knobs().fused_abl == 10) {
            // SMOT_FUSED_ABL=10: the matrix form's LEAN layout (5,760 B per plane, three workgroups per CU).  Measured,
            // same session, hinted: 15.66 vs 15.35 us at 30 tracks, 38.8 vs 39.65 at 100 — the third workgroup buys back what
            // the extra reads and funnel shifts cost (correlation phase 7.5 k vs 5.8 k cycles per workgroup) and no more.
            launch(sr_xcorr_fused9_kernel<RX, 15, 2, XCORR, FX_CH, false, 2>, 0);
            return;
        }
    }
#endif
    launch(sr_xcorr_fused9_kernel<RX, 15, 2, XCORR, FX_CH, false, MM>, 0);
}
// (the pool-only forms by pooled size: 7, 15 or 30)
static void launch_pool(int out_size, dim3 grid, hipStream_t st, const LevelParams& P, int C, const float* rois,
                        const float* boxes, float* out, int32_t* levels_out, const SrOut& S, const ImageRows* I) {
    if (out_size == 30) launch_fused<30, false>(grid, st, P, C, rois, boxes, nullptr, nullptr, out, levels_out, S, I);
    else if (out_size == 7) launch_fused<7, false>(grid, st, P, C, rois, boxes, nullptr, nullptr, out, levels_out, S, I);
    else launch_fused<15, false>(grid, st, P, C, rois, boxes, nullptr, nullptr, out, levels_out, S, I);
}

// Separable stand-alone pooling for the EMM pooler shapes and the box head's 7x7 (box_head.py:46, roi_heads.py:60-84): what
// roi_align_levels_impl routes here, and box_refine.hip's pooler.
int launch_roi_pool_separable(const LevelParams& P, int C, const float* rois, const float* level_boxes, int R,
                              int out_size, float* out, int32_t* levels_out, hipStream_t st, const ImageRows* I) {
    dim3 grid(R, (C + FX_CH - 1) / FX_CH);
    SrOut none = {nullptr, 0.f, 0.f, 0.f, 0.f, g_trace, 0, nullptr, fused_order(), nullptr, nullptr, 0};
    launch_pool(out_size, grid, st, P, C, rois, level_boxes, out, levels_out, none, I);
    return check_launch(I ? "roi_pool_separable_batched" : "roi_pool_separable");
}

// EMM.extract_cache in one launch: the templates (rz = 15, or 7: the second yaml family's, DLA_34_FPN_EMM_AOT.yaml:52-63) and
// the next frame's search regions, of one image or a batch.  n_valid: the masked form (one image: rows >= *n_valid return at
// once).  The hint writer row is the same for a batch (it reads only boxes).
int launch_extract_cache(const float* const* feats, const int* heights, const int* widths, const float* scales,
                         int num_levels, int C, const float* boxes, int N, int rz, float pad_pixels, float half_e,
                         float two_e, float min_wh, float* templates, float* sr, const int* n_valid, float* order_hint,
                         hipStream_t st, int hint_extra_rows, const ImageRows* I) {
    const char* who = I ? "emm_extract_cache_batched" : "emm_extract_cache";
    LevelParams P;
    const int rc = fill_level_params(&P, feats, heights, widths, nullptr, scales, num_levels, who, C);
    if (rc) return rc;
    SMOT_REQUIRE(boxes && templates && sr, "%s: null pointer", who);
    if (!order_hint_rois(N, false) || rz != 15) order_hint = nullptr;     // (the hint's consumer is the 30/15 head)
    SMOT_REQUIRE(order_hint == nullptr || ((((uintptr_t)order_hint) & 31) == 0 && (((uintptr_t)boxes) & 15) == 0),
                 "%s: the order hint must be 32-byte aligned (and the boxes 16-byte aligned)", who);
    // with a hint to write: one extra row of workgroups in front, of which the first ranks the rois (fx_write_hint)
    dim3 grid(N, (C + FX_CH - 1) / FX_CH + (order_hint != nullptr ? 1 : 0));
    SrOut S = {sr, pad_pixels, half_e, two_e, min_wh, g_trace, 0, n_valid, fused_order(), order_hint, nullptr,
               n_valid != nullptr ? hint_extra_rows : 0};
    // the next frame's search-region pooling runs on maps zero-padded by int(pad_pixels / stride) cells per level
    // (track_utils.py:94-96); the hint's finished tables are built against exactly that
    for (int l = 0; l < num_levels && l < SMOT_MAX_LEVELS; ++l) S.plan_pad[l] = (int)(pad_pixels * scales[l]);
    launch_pool(rz, grid, st, P, C, boxes, boxes, templates, nullptr, S, I);
    return check_launch(who);
}

#ifdef SMOT_DEBUG
// measure/csrc/sr_xcorr_plan.hip (measurement library only): the round-4 plan-driven, barrier-free generation
int launch_roi_plans(const LevelParams& P, const float* sr, const float* boxes, int N, float* plans, hipStream_t st);
int launch_fused10(const LevelParams& P, int C, const float* plans, const float* z, int N, float* resp, float* x_debug,
                   hipStream_t st);
int fused10_plan_floats();
#endif

// Pooling + correlation of one image or a batch, with an optional order hint for its rois (smot_emm_track_fwd and its batched
// twin; the stand-alone operator smot_sr_xcorr_fused_fwd passes none), honoured and verified by the kernel.
int sr_xcorr_fused_impl(const float* const* feats, const int* heights, const int* widths, const int* pad_cells,
                        const float* scales, int num_levels, int C, const float* boxes, const float* sr,
                        const float* templates, int N, float* resp, float* x_debug, const float* order_hint,
                        hipStream_t st, const int** hint_status, float* plane_max, const ImageRows* I) {
    const char* who = I ? "sr_xcorr_fused_batched" : "sr_xcorr_fused";
    LevelParams P;
    const int rc = fill_level_params(&P, feats, heights, widths, pad_cells, scales, num_levels, who, C);
    if (rc) return rc;
    if (!order_hint_rois(N, true)) order_hint = nullptr;
    // the status word of a hint this launch honours (and verifies: fx_verify_hint) — for the head's decode kernel
    if (hint_status != nullptr)
        *hint_status = order_hint != nullptr ? reinterpret_cast<const int*>(order_hint) + HINT_STATUS : nullptr;
    SMOT_REQUIRE(order_hint == nullptr || (((uintptr_t)order_hint) & 31) == 0, "%s: the order hint must be 32-byte aligned", who);
    dim3 grid(N, (C + FX_CH - 1) / FX_CH);
#ifdef SMOT_DEBUG
    if (I == nullptr && knobs().fused_gen == 10 && !channels_last()) {   // stage 1 (measurement library): generation 4 with a stand-alone plan launch
        static float* plans = nullptr;
        if (plans == nullptr && hipMalloc(&plans, (size_t)4096 * fused10_plan_floats() * 4) != hipSuccess) return SMOT_ERR_BAD_ARG;
        SMOT_REQUIRE(N <= 4096, "fused10 debug: at most 4096 rois");
        int rcp = launch_roi_plans(P, sr, boxes, N, plans, st);
        if (rcp) return rcp;
        timer_mark(0, 0, st);
        rcp = launch_fused10(P, C, plans, templates, N, resp, x_debug, st);
        timer_mark(0, 1, st);
        if (rcp == SMOT_OK && plane_max != nullptr) rcp = launch_plane_absmax(resp, N * C, 256, plane_max, st);
        return rcp;
    }
#endif
    timer_mark(0, 0, st);
    // (the timing ablations of the measurement library: one image only)
    SrOut none = {nullptr, 0.f, 0.f, 0.f, 0.f, g_trace, I ? 0 : knobs().fused_abl, nullptr, fused_order(), nullptr, order_hint, 0};
    none.plane_max = plane_max;
#ifdef SMOT_DEBUG
    if (I == nullptr && plane_max != nullptr && (knobs().fused_gen == 2 || knobs().fused_abl == 5)) {      // kernels that do not write them
        none.plane_max = nullptr;
        launch_fused<30, true>(grid, st, P, C, sr, boxes, templates, resp, x_debug, nullptr, none, nullptr);
        timer_mark(0, 1, st);
        const int rcl = check_launch("sr_xcorr_fused");
        return rcl ? rcl : launch_plane_absmax(resp, N * C, 256, plane_max, st);
    }
    // A/B (measurement library, SMOT_FUSED_ABL=4): four channels per workgroup, twice the workgroups (960 of four waves at
    // 30 tracks: finer balance, twice the table builds).  Bit-identical; 17.7 vs 17.7 us at 30 tracks, 39.0 vs 39.7 at 100
    // (measure/fused_ab.py): not worth a second configuration.
    if (I == nullptr && knobs().fused_abl == 5) {       // A/B: the correlation on plane pairs with 4x2 patches (half the LDS read volume)
        hipEvent_t e0_, e1_;
        if (timer_take(&e0_, &e1_)) {
            hipExtLaunchKernelGGL((sr_xcorr_fused9_kernel<30, 15, 2, true, 8, true>), grid, dim3(512), 0, st, e0_, e1_, 0,
                                  const_cast<float*>(none.hint_in), none.n_valid, sr, boxes, none.trace, none.order, (int)grid.x,
                                  (int)grid.y, C, templates, resp, x_debug, (int32_t*)nullptr, P, none);
        } else {
            hipLaunchKernelGGL((sr_xcorr_fused9_kernel<30, 15, 2, true, 8, true>), grid, dim3(512), 0, st,
                               const_cast<float*>(none.hint_in), none.n_valid, sr, boxes, none.trace, none.order, (int)grid.x,
                               (int)grid.y, C, templates, resp, x_debug, (int32_t*)nullptr, P, none);
        }
        timer_mark(0, 1, st);
        return check_launch("sr_xcorr_fused");
    }
    if (I == nullptr && knobs().fused_abl == 4) {
        hipLaunchKernelGGL((sr_xcorr_fused9_kernel<30, 15, 2, true, 4>), dim3(N, (C + 3) / 4), dim3(256), 0, st,
                           const_cast<float*>(none.hint_in), none.n_valid, sr, boxes, none.trace, none.order, N, (C + 3) / 4, C,
                           templates, resp, x_debug, (int32_t*)nullptr, P, none);
        timer_mark(0, 1, st);
        return check_launch("sr_xcorr_fused");
    }
#endif
    launch_fused<30, true>(grid, st, P, C, sr, boxes, templates, resp, x_debug, nullptr, none, I);
    timer_mark(0, 1, st);
    return check_launch(who);
}
}  // namespace smot

#ifdef SMOT_DEBUG
// measurement library only: the stand-alone pooling + correlation launch WITH an order hint (phase traces / A/B runs of
// the kernel alone; the product passes hints through smot_emm_track_fwd)
extern "C" int smot_debug_sr_xcorr_fused_hint_fwd(const float* const* feats, const int* heights, const int* widths,
                                                  const int* pad_cells, const float* scales, int num_levels, int C,
                                                  const float* boxes, const float* sr, const float* templates, int N,
                                                  float* resp, const float* order_hint, smot_stream_t stream) {
    return smot::sr_xcorr_fused_impl(feats, heights, widths, pad_cells, scales, num_levels, C, boxes, sr, templates, N,
                                     resp, nullptr, order_hint, (hipStream_t)stream, nullptr, nullptr, nullptr);
}
#endif

extern "C" int smot_emm_order_hint_status(const float* order_hint, int* status_host, smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(order_hint != nullptr && status_host != nullptr, "order_hint_status: null pointer");
    const hipError_t e = hipMemcpyAsync(status_host, reinterpret_cast<const int*>(order_hint) + HINT_STATUS, sizeof(int),
                                        hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e != hipSuccess) {
        set_error("order_hint_status: hipMemcpyAsync: %s", hipGetErrorString(e));
        return (int)e;
    }
    return SMOT_OK;
}

extern "C" long long smot_emm_order_hint_floats(int N, int rz, int sampling_ratio) {
    using namespace smot;
    if (!(rz == 15 && sampling_ratio == 2) || knobs().roi_generic || !order_hint_rois(N, false)) return 0;
    return (long long)N * HINT_FLOATS;
}

extern "C" int smot_sr_xcorr_fused_fwd(const float* const* feats, const int* heights, const int* widths,
                                       const int* pad_cells, const float* scales, int num_levels, int C,
                                       const float* boxes, const float* sr, const float* templates, int N, int rx,
                                       int rz, int sampling_ratio, float* resp, float* x_debug,
                                       smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(N >= 0 && C > 0, "sr_xcorr_fused: bad sizes N=%d C=%d", N, C);
    if (!(rx == 30 && rz == 15 && sampling_ratio == 2)) {
        set_error("sr_xcorr_fused: only Rx=30, Rz=15, sampling_ratio=2 is fused (got %d, %d, %d); use "
                  "smot_roi_align_levels_fwd + smot_xcorr_dw_fwd", rx, rz, sampling_ratio);
        return SMOT_ERR_UNSUPPORTED;
    }
    if (N == 0) return SMOT_OK;
    SMOT_REQUIRE(boxes && sr && templates && resp, "sr_xcorr_fused: null pointer");
    return sr_xcorr_fused_impl(feats, heights, widths, pad_cells, scales, num_levels, C, boxes, sr, templates, N, resp,
                               x_debug, nullptr, (hipStream_t)stream, nullptr, nullptr, nullptr);
}

// fp16 / bf16 maps (include/smot_emm.h, "fp16 / bf16 FEATURE MAPS")
extern "C" int smot_sr_xcorr_fused_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                             const int* pad_cells, const float* scales, int num_levels, int C,
                                             const float* boxes, const float* sr, const float* templates, int N, int rx,
                                             int rz, int sampling_ratio, float* resp, float* x_debug, smot_stream_t stream) {
    const int rc = smot::check_feat_type(feat_type, "sr_xcorr_fused_typed");
    if (rc) return rc;
    smot::FeatTypeScope scope(feat_type);
    return smot_sr_xcorr_fused_fwd(reinterpret_cast<const float* const*>(feats), heights, widths, pad_cells, scales, num_levels,
                                   C, boxes, sr, templates, N, rx, rz, sampling_ratio, resp, x_debug, stream);
}
