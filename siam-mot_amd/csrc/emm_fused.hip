// One-call entry points for the two halves of a frame pair (host-side fusion: one FFI crossing and
// one argument validation per call instead of five; the kernels are the ones in the other files and
// run back-to-back on `stream`).
//
//   smot_emm_track_fwd         == the inference branch of EMM.forward          (reference EMM/track_core.py:28-79)
//   smot_emm_extract_cache_fwd == EMM.extract_cache                             (reference EMM/track_core.py:81-98)
#include "pool_launch.h"
#include "knobs.h"

#include "tower_common.h"

// whether the towers that follow will launch the split form and so want the response's plane maxima from the pooling +
// correlation kernel (the launchers' own choice: tower_wino.hip; a bad group count is refused by predictor_impl later)
static inline bool towers_want_plane_max(int N, int C, int ho, int gn_groups, const float* packed) {
    return packed != nullptr && gn_groups > 0 && C % gn_groups == 0 && smot::tower_split_form(N, C, ho, C / gn_groups);
}

extern "C" long long smot_emm_track_ws_floats(int N, int C, int rx, int rz) {
    if (N < 0 || C <= 0 || rz <= 0 || rx < rz) return -1;
    const long long ho = rx - rz + 1;
    const long long n = N > 0 ? N : 1;
    // x | response | tower workspace | logits | decode candidates (8-byte aligned: all terms even)
    return n * C * rx * rx + n * C * ho * ho + n * 2 * C * ho * ho + n * 8 * ho * ho +
           n * smot_emm_decode_ws_floats((int)ho, 16);
}

// The head of smot_emm_track_fwd (I == nullptr) and of its batched twin (I = the validated row ranges of the batch): the
// pooling launches take the batch's image of every row, the towers and the decode are per row and the same.
static int emm_track_impl(const float* const* feats, const int* heights, const int* widths,
                          const int* pad_cells, const float* scales, int num_levels, int C,
                          const float* boxes, const float* sr, const float* templates, int N, int rx,
                          int rz, int sampling_ratio, const float* const* predictor_params, int gn_groups,
                          float gn_eps, const float* hann, int up, float pad_pixels,
                          float one_minus_sigma, float sigma, int use_centerness, float clip_w,
                          float clip_h, float* ws, float* bb, float* conf, int64_t* idx,
                          const float* order_hint, smot_stream_t stream, const smot::ImageRows* I) {
    using namespace smot;
    SMOT_REQUIRE(predictor_params && ws && boxes && sr && templates, "emm_track: null pointer");
    SMOT_REQUIRE(((uintptr_t)ws & 15) == 0, "emm_track: workspace must be 16-byte aligned");
    const int ho = rx - rz + 1;
    float* x = ws;
    float* resp = x + (size_t)N * C * rx * rx;
    float* tower = resp + (size_t)N * C * ho * ho;
    float* logits = tower + (size_t)N * 2 * C * ho * ho;
    float* cand = logits + (size_t)N * 8 * ho * ho;       // 7 planes used; 8 keeps the 8-byte alignment
    int rc;
    // the response's plane maxima [N][C] for the tower kernel's split form: in the head of the logits buffer, which nothing
    // reads before the towers and the decode kernel writes after them; nullptr = the predictor makes them itself
    const float* plane_max = nullptr;
    const int* poison = nullptr;
    const bool no_fuse = knobs().no_fuse;             // A/B: measurement library only (constant false otherwise)
    if (rx == 30 && rz == 15 && sampling_ratio == 2 && !no_fuse) {
        // pooling feeds the correlation inside one kernel: the search-region tensor never reaches HBM
        // (a hint the kernel honours is VERIFIED against `boxes` / `sr` by it; `poison` = the list's status word)
        float* pm = (C <= 7 * ho * ho && towers_want_plane_max(N, C, ho, gn_groups, predictor_params[12])) ? logits : nullptr;
        rc = sr_xcorr_fused_impl(feats, heights, widths, pad_cells, scales, num_levels, C, boxes, sr, templates, N, resp, nullptr,
                                 order_hint, (hipStream_t)stream, &poison, pm, I);
        if (rc) return rc;
        plane_max = pm;
    } else if (rx == 35 && rz == 7 && sampling_ratio == 2 && !no_fuse) {
        // the second yaml family's shape: gathers + correlation in one kernel (sr_xcorr_small.hip), same arithmetic
        float* pm = (C <= 7 * ho * ho && towers_want_plane_max(N, C, ho, gn_groups, predictor_params[12])) ? logits : nullptr;
        rc = sr_xcorr_gather_impl(feats, heights, widths, pad_cells, scales, num_levels, C, boxes, sr, templates, N, resp,
                                  (hipStream_t)stream, pm, I);
        if (rc) return rc;
        plane_max = pm;
    } else {
        rc = roi_align_levels_impl(feats, heights, widths, pad_cells, scales, num_levels, C, sr, boxes, N, rx, rx, sampling_ratio,
                                   x, nullptr, (hipStream_t)stream, I, I ? "roi_align_batched" : "roi_align");
        if (rc) return rc;
        rc = smot_xcorr_dw_fwd(x, templates, resp, N, C, rx, rz, stream);
        if (rc) return rc;
    }
    const float* const* p = predictor_params;
    // towers only: when the matrix-core path applies the per-tile partial head sums stay in `tower` and the
    // decode kernels sum them while loading (no combine launch, no logits round trip)
    int tiles = 0;
    bool tickets_zeroed = false;           // the Winograd tower kernel zeroes the decode kernel's tickets on its way
    rc = predictor_impl(resp, N, C, ho, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11],
                        gn_groups, gn_eps, p[12], tower, logits, stream, &tiles, decode_tickets(cand, N, ho),
                        &tickets_zeroed, plane_max);
    if (rc) return rc;
    LogitSrc L;
    L.logits = tiles > 0 ? nullptr : logits;
    L.part = tower;
    L.tpt = tiles;
    L.cls_b = p[7];
    L.center_b = p[9];
    L.reg_b = p[11];
    L.logits_out = logits;
    return decode_impl(L, sr, boxes, hann, N, ho, up, rx, rz, pad_pixels, one_minus_sigma, sigma, use_centerness,
                       clip_w, clip_h, cand, bb, conf, idx, tickets_zeroed, (hipStream_t)stream, poison);
}

extern "C" int smot_emm_track_fwd(const float* const* feats, const int* heights, const int* widths,
                                  const int* pad_cells, const float* scales, int num_levels, int C,
                                  const float* boxes, const float* sr, const float* templates, int N, int rx,
                                  int rz, int sampling_ratio, const float* const* predictor_params, int gn_groups,
                                  float gn_eps, const float* hann, int up, float pad_pixels,
                                  float one_minus_sigma, float sigma, int use_centerness, float clip_w,
                                  float clip_h, float* ws, float* bb, float* conf, int64_t* idx,
                                  const float* order_hint, smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(N >= 0 && C > 0 && rz > 0 && rx >= rz, "emm_track: bad sizes N=%d C=%d rx=%d rz=%d", N, C, rx, rz);
    if (N == 0) return SMOT_OK;
    return emm_track_impl(feats, heights, widths, pad_cells, scales, num_levels, C, boxes, sr, templates, N, rx, rz,
                          sampling_ratio, predictor_params, gn_groups, gn_eps, hann, up, pad_pixels, one_minus_sigma, sigma,
                          use_centerness, clip_w, clip_h, ws, bb, conf, idx, order_hint, stream, nullptr);
}

// A batch of images in one set of launches (include/smot_emm.h): the row ranges are checked before anything is launched.
extern "C" int smot_emm_track_batched_fwd(const float* const* feats, const int* heights, const int* widths,
                                          const int* pad_cells, const float* scales, int num_levels, int C,
                                          const float* boxes, const float* sr, const float* templates, int N, int rx,
                                          int rz, int sampling_ratio, const float* const* predictor_params, int gn_groups,
                                          float gn_eps, const float* hann, int up, float pad_pixels,
                                          float one_minus_sigma, float sigma, int use_centerness, float clip_w,
                                          float clip_h, float* ws, float* bb, float* conf, int64_t* idx,
                                          const float* order_hint, smot_stream_t stream, int num_images,
                                          const int* row_start) {
    using namespace smot;
    SMOT_REQUIRE(N >= 0 && C > 0 && rz > 0 && rx >= rz, "emm_track_batched: bad sizes N=%d C=%d rx=%d rz=%d", N, C, rx, rz);
    ImageRows I;
    const int rc = fill_image_rows(&I, num_images, row_start, N, "emm_track_batched");
    if (rc) return rc;
    if (N == 0) return SMOT_OK;
    return emm_track_impl(feats, heights, widths, pad_cells, scales, num_levels, C, boxes, sr, templates, N, rx, rz,
                          sampling_ratio, predictor_params, gn_groups, gn_eps, hann, up, pad_pixels, one_minus_sigma, sigma,
                          use_centerness, clip_w, clip_h, ws, bb, conf, idx, order_hint, stream, &I);
}

// EMM.extract_cache behind all of its entry points: one image (I == nullptr) or the rows of a batch; n_valid != nullptr = the
// masked form (N is a capacity, the count is on the device; hint_extra_rows: SrOut::hint_extra).  `who` names the entry point.
static int emm_extract_cache_impl(const float* const* feats, const int* heights, const int* widths, const float* scales,
                                  int num_levels, int C, const float* boxes, int N, int rz, int sampling_ratio,
                                  float pad_pixels, float search_expansion, float min_search_wh, float* templates, float* sr,
                                  float* order_hint, smot_stream_t stream, const smot::ImageRows* I, const int* n_valid,
                                  int hint_extra_rows, const char* who) {
    using namespace smot;
    SMOT_REQUIRE(N >= 0 && num_levels >= 1 && num_levels <= SMOT_MAX_LEVELS, "%s: bad sizes", who);
    if (N == 0) return SMOT_OK;
    const bool separable = (rz == 15 || rz == 7) && sampling_ratio == 2;
    if (separable && (n_valid != nullptr || !knobs().roi_generic)) {
        // one launch: separable template pooling, with the search regions written by the same kernel
        // (the reference forms e/2 and e*2 in Python double before they meet the fp32 tensors)
        const float half_e = (float)((double)search_expansion / 2.0);
        const float two_e = (float)((double)search_expansion * 2.0);
        return launch_extract_cache(feats, heights, widths, scales, num_levels, C, boxes, N, rz, pad_pixels, half_e, two_e,
                                    min_search_wh, templates, sr, n_valid, order_hint, (hipStream_t)stream, hint_extra_rows, I);
    }
    if (n_valid != nullptr) {
        set_error("%s: the masked extraction needs Rz=15 or 7, sampling_ratio=2 (got %d, %d); use smot_emm_extract_cache_fwd "
                  "with the count on the host", who, rz, sampling_ratio);
        return SMOT_ERR_UNSUPPORTED;
    }
    const int rc = roi_align_levels_impl(feats, heights, widths, nullptr, scales, num_levels, C, boxes, boxes, N, rz, rz,
                                         sampling_ratio, templates, nullptr, (hipStream_t)stream, I,
                                         I ? "roi_align_batched" : "roi_align");
    if (rc) return rc;
    return smot_search_region_fwd(boxes, N, pad_pixels, search_expansion, min_search_wh, sr, stream);
}

extern "C" int smot_emm_extract_cache_fwd(const float* const* feats, const int* heights, const int* widths,
                                          const float* scales, int num_levels, int C, const float* boxes, int N,
                                          int rz, int sampling_ratio, float pad_pixels, float search_expansion,
                                          float min_search_wh, float* templates, float* sr, float* order_hint,
                                          smot_stream_t stream) {
    return emm_extract_cache_impl(feats, heights, widths, scales, num_levels, C, boxes, N, rz, sampling_ratio, pad_pixels,
                                  search_expansion, min_search_wh, templates, sr, order_hint, stream, nullptr, nullptr, 0,
                                  "emm_extract_cache");
}

// EMM.extract_cache over a batch of images (include/smot_emm.h): the row ranges are checked before anything is launched.
extern "C" int smot_emm_extract_cache_batched_fwd(const float* const* feats, const int* heights, const int* widths,
                                                  const float* scales, int num_levels, int C, const float* boxes, int N,
                                                  int rz, int sampling_ratio, float pad_pixels, float search_expansion,
                                                  float min_search_wh, float* templates, float* sr, float* order_hint,
                                                  smot_stream_t stream, int num_images, const int* row_start) {
    using namespace smot;
    SMOT_REQUIRE(N >= 0 && num_levels >= 1 && num_levels <= SMOT_MAX_LEVELS, "emm_extract_cache_batched: bad sizes");
    ImageRows I;
    const int rc = fill_image_rows(&I, num_images, row_start, N, "emm_extract_cache_batched");
    if (rc) return rc;
    return emm_extract_cache_impl(feats, heights, widths, scales, num_levels, C, boxes, N, rz, sampling_ratio, pad_pixels,
                                  search_expansion, min_search_wh, templates, sr, order_hint, stream, &I, nullptr, 0,
                                  "emm_extract_cache_batched");
}

// EMM.extract_cache over a CAPACITY of boxes of which only the first *n_valid (a device-resident count, e.g. word 1
// of smot_track_solve_fwd's record) are real: the launch is enqueued before the host knows the count, workgroups
// of the other rows return at once and their output rows stay unwritten.  The tracker's frame then needs no host
// synchronisation between the solver and the template extraction.
extern "C" int smot_emm_extract_cache_masked_fwd(const float* const* feats, const int* heights, const int* widths,
                                                 const float* scales, int num_levels, int C, const float* boxes,
                                                 int capacity, const int* n_valid, int rz, int sampling_ratio,
                                                 float pad_pixels, float search_expansion, float min_search_wh,
                                                 float* templates, float* sr, float* order_hint,
                                                 smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(capacity >= 0 && num_levels >= 1 && num_levels <= SMOT_MAX_LEVELS, "emm_extract_cache_masked: bad sizes");
    SMOT_REQUIRE(n_valid != nullptr, "emm_extract_cache_masked: null count pointer");
    return emm_extract_cache_impl(feats, heights, widths, scales, num_levels, C, boxes, capacity, rz, sampling_ratio, pad_pixels,
                                  search_expansion, min_search_wh, templates, sr, order_hint, stream, nullptr, n_valid, 0,
                                  "emm_extract_cache_masked");
}


// One tracking frame behind one call (include/smot_emm.h, smot_frame_args): the four stages' existing entry points in
// sequence on one stream — no new arithmetic, one FFI crossing instead of four and no host work between the launches.
extern "C" int smot_track_frame_fwd(const smot_frame_args* a, smot_stream_t stream) {
    using namespace smot;
    SMOT_REQUIRE(a != nullptr, "track_frame: null argument block");
    const int stages = a->stages == 0 ? (SMOT_STAGE_HEAD | SMOT_STAGE_REFINE | SMOT_STAGE_SOLVE | SMOT_STAGE_EXTRACT) : a->stages;
    SMOT_REQUIRE(a->n_trk >= 0, "track_frame: n_trk=%d", a->n_trk);
    int rc;
    if ((stages & SMOT_STAGE_HEAD) && a->n_trk > 0) {
        rc = smot_emm_track_fwd(a->feats, a->heights, a->widths, a->pad_cells, a->scales, a->num_levels, a->C, a->tpl_boxes,
                                a->sr, a->templates, a->n_trk, a->rx, a->rz, a->sampling_ratio, a->predictor_params,
                                a->gn_groups, a->gn_eps, a->hann, a->up, a->pad_pixels, a->one_minus_sigma, a->sigma,
                                a->use_centerness, a->clip_w, a->clip_h, a->head_ws, a->trk_boxes, a->trk_conf, nullptr,
                                a->order_hint, stream);
        if (rc) return rc;
    }
    if (!(stages & (SMOT_STAGE_REFINE | SMOT_STAGE_SOLVE | SMOT_STAGE_EXTRACT))) return SMOT_OK;
    SMOT_REQUIRE(a->n_det >= 0 && a->n_trk + a->n_det > 0, "track_frame: n_trk=%d n_det=%d", a->n_trk, a->n_det);
    // what the solver reads as its track segment: the head's output, or the refinement's (refine != 0)
    const float* trk_boxes = nullptr;
    float* trk_scores = nullptr;
    const int64_t* trk_ids = nullptr;
    const int64_t* trk_labels = nullptr;
    float bias = 1.0f;
    if (a->n_trk > 0) {
        trk_boxes = a->trk_boxes;
        trk_scores = a->trk_conf;
        trk_ids = a->trk_ids;
        trk_labels = a->trk_labels;
        if (a->refine) {
            if (stages & SMOT_STAGE_REFINE) {
                rc = smot_box_refine_fwd(a->feats, a->heights, a->widths, a->scales, a->num_levels, a->C, a->box_pooled,
                                         a->box_sampling_ratio, a->trk_boxes, a->trk_labels, a->trk_ids, a->trk_conf,
                                         a->n_trk, a->fc6_w, a->fc6_b, a->dim6, a->fc7_w, a->fc7_b, a->dim7, a->cls_w,
                                         a->cls_b, a->num_classes, a->reg_w, a->reg_b, a->reg_classes, a->box_wx,
                                         a->box_wy, a->box_ww, a->box_wh, a->box_xform_clip, a->clip_w, a->clip_h,
                                         a->tracktor, a->refine_ws, a->ref_boxes, a->ref_scores, a->ref_ids,
                                         a->ref_labels, stream);
                if (rc) return rc;
            }
            trk_boxes = a->ref_boxes;
            trk_scores = a->ref_scores;
            trk_ids = a->ref_ids;
            trk_labels = a->ref_labels;
            bias = 0.0f;                       // the refined scores are in the (1, 2] band already
        }
    }
    if (stages & SMOT_STAGE_SOLVE) {
        const int carry = (stages & SMOT_STAGE_CARRY) ? a->carry_rows : 0;
        rc = smot_track_solve_carry_fwd(a->det_boxes, a->det_scores, a->det_ids, a->det_labels, a->n_det, trk_boxes, trk_scores,
                                        trk_ids, trk_labels, a->n_trk, bias, a->track_thresh, a->start_thresh,
                                        a->resume_thresh, a->nms_thresh, a->max_dormant_frames, a->pool_state,
                                        a->pool_capacity, a->out_boxes, a->out_scores, a->out_ids, a->out_labels,
                                        a->act_boxes, a->act_ids, a->act_labels, a->act_scores, a->record,
                                        a->carry_templates, a->carry_boxes, a->carry_sr, a->carry_ids, a->carry_labels,
                                        a->carry_scores, a->carry_src_row0, carry, a->carry_dst_row0, a->next_templates,
                                        a->next_sr, a->C * a->rz * a->rz, stream);
        if (rc) return rc;
    }
    if (!(stages & SMOT_STAGE_EXTRACT)) return SMOT_OK;
    // = smot_emm_extract_cache_masked_fwd, whose order hint also ranks the dormant rows the solver's launch has just put
    // behind the active ones (SMOT_STAGE_CARRY: their boxes stand in act_boxes behind the count): a memory with dormant
    // tracks — most frames of a MOT sequence — keeps its hint
    return emm_extract_cache_impl(a->feats, a->heights, a->widths, a->scales, a->num_levels, a->C, a->act_boxes,
                                  a->n_det + a->n_trk, a->rz, a->sampling_ratio, a->pad_pixels, a->search_expansion,
                                  a->min_search_wh, a->next_templates, a->next_sr, a->next_order_hint, stream, nullptr,
                                  a->pool_state + 4, (stages & SMOT_STAGE_CARRY) ? a->carry_rows : 0, "track_frame");
}


// ---- fp16 / bf16 maps (include/smot_emm.h, "fp16 / bf16 FEATURE MAPS"): the element type is checked, set for the call's
// duration (FeatTypeScope: the launch sites of the kernels that read the maps pick their instantiation by it) and the fp32
// entry point's host code runs — towers, decode and solver never see the maps ------------------------------------------------
extern "C" int smot_emm_track_typed_fwd(const void* const* feats, int feat_type, const int* heights, const int* widths,
                                        const int* pad_cells, const float* scales, int num_levels, int C,
                                        const float* boxes, const float* sr, const float* templates, int N, int rx,
                                        int rz, int sampling_ratio, const float* const* predictor_params, int gn_groups,
                                        float gn_eps, const float* hann, int up, float pad_pixels,
                                        float one_minus_sigma, float sigma, int use_centerness, float clip_w,
                                        float clip_h, float* ws, float* bb, float* conf, int64_t* idx,
                                        const float* order_hint, smot_stream_t stream, int num_images,
                                        const int* row_start) {
    const int rc = smot::check_feat_type(feat_type, "emm_track_typed");
    if (rc) return rc;
    smot::FeatTypeScope scope(feat_type);
    return smot_emm_track_batched_fwd(reinterpret_cast<const float* const*>(feats), heights, widths, pad_cells, scales,
                                      num_levels, C, boxes, sr, templates, N, rx, rz, sampling_ratio, predictor_params,
                                      gn_groups, gn_eps, hann, up, pad_pixels, one_minus_sigma, sigma, use_centerness, clip_w,
                                      clip_h, ws, bb, conf, idx, order_hint, stream, num_images, row_start);
}

extern "C" int smot_emm_extract_cache_typed_fwd(const void* const* feats, int feat_type, const int* heights,
                                                const int* widths, const float* scales, int num_levels, int C,
                                                const float* boxes, int N, int rz, int sampling_ratio, float pad_pixels,
                                                float search_expansion, float min_search_wh, float* templates, float* sr,
                                                float* order_hint, smot_stream_t stream, int num_images,
                                                const int* row_start, const int* n_valid) {
    using namespace smot;
    const int rc = check_feat_type(feat_type, "emm_extract_cache_typed");
    if (rc) return rc;
    FeatTypeScope scope(feat_type);
    const float* const* f = reinterpret_cast<const float* const*>(feats);
    if (n_valid == nullptr)
        return smot_emm_extract_cache_batched_fwd(f, heights, widths, scales, num_levels, C, boxes, N, rz, sampling_ratio,
                                                  pad_pixels, search_expansion, min_search_wh, templates, sr, order_hint,
                                                  stream, num_images, row_start);
    // the masked form: N is a capacity, the count is on the device — one image only
    SMOT_REQUIRE(num_images == 1, "emm_extract_cache_typed: n_valid needs num_images == 1 (got %d)", num_images);
    ImageRows I;
    const int rci = fill_image_rows(&I, num_images, row_start, N, "emm_extract_cache_typed");
    if (rci) return rci;
    return smot_emm_extract_cache_masked_fwd(f, heights, widths, scales, num_levels, C, boxes, N, n_valid, rz, sampling_ratio,
                                             pad_pixels, search_expansion, min_search_wh, templates, sr, order_hint, stream);
}

extern "C" int smot_track_frame_typed_fwd(const smot_frame_args* a, int feat_type, smot_stream_t stream) {
    const int rc = smot::check_feat_type(feat_type, "track_frame_typed");
    if (rc) return rc;
    smot::FeatTypeScope scope(feat_type);
    return smot_track_frame_fwd(a, stream);
}
