// The body of the pooling (+ correlation) kernel, shared by its single-image and batched forms (sr_xcorr.hip): included
// inside each kernel's braces, which define BATCHED and the kernel arguments (I = the batch's ImageRows, or NoImages).
// One text in two kernels instead of one inlined device function: the single-image kernels compile to the same code as
// before batching existed (an inlined body schedules differently).
// FT (defined by the kernel as well) is the maps' element type: float, or f16_t / bf16_t in the *_half_* kernels, which
// load 2-byte elements and convert them right behind the load (fx_load1 / fx_load2 / fx_pair_elem); everything else,
// the sample tables and the order hint's row BYTE offsets of an fp32 map included, is the same text.
// NHWC (defined by the kernel too; false in every NCHW kernel): the maps are channels-last and the pooling stage is
// sr_pool_nhwc_stage.h; tables, hint, assignment, LDS images and the correlation are the same text.
    constexpr int HO = XCORR ? RX - RZ + 1 : 16;
    constexpr int NS = RX * G;                   // samples per axis
    // LDS image of the one-plane-per-wave correlation (xcorr_patch1.h): row stride 40, one plane per slot
    // P2: the correlation runs on plane PAIRS with 4x2 output patches per lane (xcorr_patch2.h: half the LDS read volume
    // per FMA of the one-plane form) by waves 0..NCH/2-1; the image then has that phase's strides
    constexpr int XS = P2 ? XP2_XS : (MM == 2 ? XL_XS : XP1_XS), XP = P2 ? XP2_XP : (MM == 2 ? 30 * XL_XS : 32 * XP1_XS), ZS = XP1_ZS,
                  ZP = MM == 1 ? XH_TZ_FLOATS : (MM == 2 ? XL_TZ_FLOATS : RZ * XP1_ZS);
    static_assert(MM == 0 || (XCORR && !P2 && RX == 30 && RZ == 15), "the matrix-pipe correlation is the 30 / 15 head's");
    static_assert(MM != 2 || ((XP * 4) % 128 == 0 && ((2 * XP + 2 * ZP) * 4) % 128 == 0), "lean layout: 128-byte aligned plane images");
    constexpr int RH = (RX + 1) / 2;             // pooled rows per batch
    static_assert((!XCORR || RX - RZ + 1 == 16) && RX <= 32 && G == 2 && RX * XS <= XP && 2 * RH * G <= 64,
                  "specialised for pooled sizes <= 32, g = 2 (and the 30/15/16 correlation geometry)");
    __shared__ __attribute__((aligned(128))) float sm[(NCH / 2) * (2 * XP + 2 * ZP)];
    __shared__ __attribute__((aligned(16))) int4 tab[2][64 + 2 * RH * G];   // y / x sample tables (+ zero pad)
    __shared__ int wbound[4];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0..7
    // (the leading kernel arguments — FX_LEAD_PARAMS in sr_xcorr.hip — under the names the text below uses)
    const float* const hint_in = XCORR ? hint : nullptr;
    float* const hint_out = XCORR ? nullptr : hint;
    const long long t_start = trace ? (long long)__builtin_amdgcn_s_memtime() : 0ll;
    // pooled sizes <= 15 keep grid order (fx_assign: n = blockIdx.x): the workgroup's roi is requested now, beside the masked
    // form's count, and used where the loads stood
    float roi_early[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (RX <= 15) {
#pragma unroll
        for (int k = 0; k < 4; ++k) roi_early[k] = sr[(size_t)blockIdx.x * 4 + k];
    }
    // The level's map size, padding, scale and base pointer are read from the kernel-argument segment with a DYNAMIC index
    // once the level is known: scalar loads that DEPEND on the workgroup's first memory round trip and — at a kernel's start,
    // with the scalar cache and the XCD's L2 freshly invalidated — may miss all the way to memory.  Their three 64-byte lines
    // (pointers; H, W; pad, scale) are requested here, with the first round trip; the values are "used" behind it (SMOT_KA_USE).
    const int ka_h = P.H[0], ka_w = P.W[0], ka_p = P.pad[0];
    const float ka_s = P.scale[0];
    const unsigned long long ka_f = reinterpret_cast<unsigned long long>(P.feat[0]);
#define SMOT_KA_USE() asm volatile("" ::"s"(ka_h), "s"(ka_w), "s"(ka_p), "s"(ka_s), "s"(ka_f))
    // batched: the row ranges' lines likewise (one value per 16 dwords covers all of them); used by image_of_row behind it
    int ka_i[6] = {0, 0, 0, 0, 0, 0};
    if constexpr (BATCHED) {
        ka_i[0] = I.num_images;
#pragma unroll
        for (int k = 1; k < 6; ++k) ka_i[k] = I.row_start[min(16 * k - 1, SMOT_MAX_IMAGES)];
    }
#ifdef SMOT_DEBUG
    // experiment (measurement library, SMOT_FUSED_ABL = 100 + k): workgroups of the second dispatch wave start 512*k
    // cycles late, so that the two workgroups of a CU pool (LDS crossbar) and correlate (VALU) in anti-phase.
    // Measured: 17.0 us at no delay, 17.05-17.2 us for delays of 2 k .. 8 k cycles, 18.0 at 16 k — the late workgroup
    // catches up exactly: a CU's time is the SUM of its workgroups' instruction issue (1,500 vector instructions per
    // wave, 900 of them the correlation's FMAs), not a chain of latencies that a phase shift could overlap.
    if (S.abl >= 100 && (int)(blockIdx.y * grid_nx + blockIdx.x) >= 256) {
        for (int d = 0; d < S.abl - 100; ++d) __builtin_amdgcn_s_sleep(8);
    }
#endif
    int n_assigned, cg_assigned, lvl_assigned = 0;
    float4 roi_assigned = make_float4(0.f, 0.f, 0.f, 0.f);
    // The ranking costs ~3 k cycles per box tensor at the head of every workgroup: one vector-memory round trip on
    // lines that all 256 CUs request at the same moment (the workgroup's own roi used to arrive through the scalar
    // cache in half that).  The 30x30 kernels earn it back (fused: 18.7 -> 17.4 us at 30 rois, 49 -> 42 us at 100);
    // the small template pooler does not (7.1 -> 7.3 us) and keeps grid order.  Measured and dropped: ranking in wave
    // 0 only with an LDS broadcast (same time: the cost is latency, not VALU contention); ranking from the search
    // regions alone with the level estimated (one tensor fewer, but the workgroup's exact level then costs a
    // dependent scalar load: 17.8 -> 18.4 us); the boxes through the scalar cache (sixteen s_load_dwordx4 per wave,
    // parked in LDS for the lanes: 106 SGPRs cost the kernel its occupancy target, 18.4 us).
    // Also measured and dropped for the 33..64-column windows that set the makespan: three 10-row blocks per plane with
    // the next block's row loads issued before the current block's gathers (96 VGPRs, two workgroups per CU):
    // bit-identical, 17.0 instead of 16.75 us at 30 rois, 12.9 instead of 12.3 at 16 (profiles/r02_fused_pipelined_wide.jsonl).
    int grid_row = blockIdx.y, grid_rows = grid_ny;
    if constexpr (!XCORR) {
        if (hint_out != nullptr) {                 // extraction launch with one extra row in front: the hint writer
            if (grid_row == 0) {
                fx_write_hint<30, G>(P, boxes, S, n_valid, hint_out, grid_nx, blockIdx.x, wave, lane);     // (the consumer's shape: 30x30 bins)
                return;
            }
            grid_row -= 1;
            grid_rows -= 1;
        }
    }
    // With a hint the entry's finished tables and its geometry stamp are requested NOW, beside fx_assign's own scalar load
    // of the entry: everything a hinted workgroup needs before its first feature load is ONE memory round trip.
    int4 tab_early = make_int4(0, 0, 0, 0);
    int4 ye_early = make_int4(0, 0, 0, 0), xe_early[2] = {make_int4(0, 0, 0, 0), make_int4(0, 0, 0, 0)};
    typedef int v8h_t __attribute__((ext_vector_type(8)));
    v8h_t g8 = {0, 0, 0, 0, -1, -1, -1, 0};
    if constexpr (XCORR && RX == 30) {
        if (hint_in != nullptr && order == 1 && n_valid == nullptr && grid_nx >= 2 && grid_nx <= 256) {
            const int k0 = (int)(blockIdx.y * grid_nx + blockIdx.x) / grid_ny;        // = fx_assign's rank k
            const int* ent = reinterpret_cast<const int*>(hint_in) + (size_t)k0 * HINT_FLOATS;
            g8 = *reinterpret_cast<const __attribute__((address_space(4))) v8h_t*>(
                reinterpret_cast<unsigned long long>(ent) + 4ull * HINT_BOUNDS);
            if (wave < 2) tab_early = *reinterpret_cast<const int4*>(ent + (wave == 0 ? HINT_YTAB : HINT_XTAB) + 4 * lane);
            if constexpr (MM == 1) {
                // (round 6) ... and EVERY wave requests the entries it will use itself — the y entries of its own 15 pooled
                // rows (plane-pair form: the two waves of a pair split the rows), the two x entries of its lane's pooled column —
                // so that a hinted workgroup with a window of <= 64 columns needs neither the tables' image in LDS nor the
                // barrier behind it (`fast` below): the row loads go out ~1.2 k cycles earlier.
                ye_early = *reinterpret_cast<const int4*>(ent + HINT_YTAB + 4 * min(lane + (wave & 1) * RH * G, 63));
                const int pwl = (lane & 31) < RX ? (lane & 31) : 0;
                xe_early[0] = *reinterpret_cast<const int4*>(ent + HINT_XTAB + 4 * (pwl * G));
                xe_early[1] = *reinterpret_cast<const int4*>(ent + HINT_XTAB + 4 * (pwl * G + 1));
            }
        }
    }
    if constexpr (XCORR && RX == 30) {
        if (hint_in != nullptr && order == 1 && n_valid == nullptr && grid_nx >= 2 && grid_nx <= 256 &&
            blockIdx.y == 0 && wave == 2
#ifdef SMOT_DEBUG
            && S.abl != 6                 // A/B (measurement library, SMOT_FUSED_ABL=6): the round-4 kernel that trusted the hint
#endif
        )
            fx_verify_hint(P, sr, boxes, hint_in, blockIdx.x, grid_nx, lane);
    }
    int k_assigned = -1;
    const bool have_roi = fx_assign(P, sr, boxes, n_valid, RX > 15 ? order : 0, grid_row, grid_rows,
                                    XCORR ? hint_in : nullptr, grid_nx, lane, &n_assigned, &cg_assigned, &roi_assigned,
                                    &lvl_assigned, &k_assigned);
    SMOT_KA_USE();
#undef SMOT_KA_USE
    if constexpr (BATCHED)
        asm volatile("" ::"s"(ka_i[0]), "s"(ka_i[1]), "s"(ka_i[2]), "s"(ka_i[3]), "s"(ka_i[4]), "s"(ka_i[5]));
    const int n = __builtin_amdgcn_readfirstlane(n_assigned);
    const int cgrp = __builtin_amdgcn_readfirstlane(cg_assigned);
    if (n_valid != nullptr && n >= *n_valid) return;         // workgroup-uniform (scalar load)
    int img = 0;                                                 // the roi's image (batched form)
    if constexpr (BATCHED) img = image_of_row(I, n);
    // (trace rows are indexed by the item, not by the workgroup that happened to take it)
#define FX_TRACE(SLOT)                                                                      \
    if (trace && tid == 0)                                                                  \
        trace[((size_t)n * grid_rows + cgrp) * 8 + (SLOT)] = (long long)__builtin_amdgcn_s_memtime();
    if (trace && tid == 0) trace[((size_t)n * grid_rows + cgrp) * 8 + 0] = t_start;
    FX_TRACE(5)                                   // after the assignment

    float roi0 = roi_assigned.x, roi1 = roi_assigned.y, roi2 = roi_assigned.z, roi3 = roi_assigned.w;
    int lvl = lvl_assigned;
    if (!have_roi) {                             // workgroup-uniform
        if constexpr (RX <= 15) {                // (n == blockIdx.x)
            roi0 = roi_early[0];
            roi1 = roi_early[1];
            roi2 = roi_early[2];
            roi3 = roi_early[3];
        } else {
            roi0 = sr[(size_t)n * 4 + 0];
            roi1 = sr[(size_t)n * 4 + 1];
            roi2 = sr[(size_t)n * 4 + 2];
            roi3 = sr[(size_t)n * 4 + 3];
        }
        lvl = 0;
        if (P.num_levels > 1) lvl = map_level(boxes + (size_t)n * 4, P.k_min, P.k_max);
    }
    const float roi[4] = {roi0, roi1, roi2, roi3};
    lvl = __builtin_amdgcn_readfirstlane(lvl);
    if (levels_out != nullptr && cgrp == 0 && tid == 0) levels_out[n] = lvl;
    if (!XCORR && S.sr != nullptr && cgrp == 0 && tid == 0) {
        const float4 o = search_region_of(roi[0], roi[1], roi[2], roi[3], S);
        S.sr[n * 4 + 0] = o.x;
        S.sr[n * 4 + 1] = o.y;
        S.sr[n * 4 + 2] = o.z;
        S.sr[n * 4 + 3] = o.w;
    }
    const int H = P.H[lvl], W = P.W[lvl], pad = P.pad[lvl];
    const float scale = P.scale[lvl];
    const float x1 = mul_rn(roi[0], scale), y1 = mul_rn(roi[1], scale);
    const float x2 = mul_rn(roi[2], scale), y2 = mul_rn(roi[3], scale);
    const float bin_h = div_rn(fmaxf(sub_rn(y2, y1), 1.0f), (float)RX);
    const float bin_w = div_rn(fmaxf(sub_rn(x2, x1), 1.0f), (float)RX);
    FX_TRACE(6)                                   // (level parameters and bin sizes known)
    // (Measured and dropped, profiles/r02x: one workgroup per (roi, FOUR channels) for rois whose window is wider
    // than 32 columns — two waves per plane, so that they do not set the makespan — with narrow rois using every
    // second workgroup: per-workgroup spans became equal (25-32 k cycles instead of 26 k / 48 k) but 608 working
    // workgroups no longer fit the chip's 512 resident slots (two rounds: 18.7 -> 24 us), and at three workgroups
    // per CU — 74 VGPRs with the one-plane correlation below — the kernel still took 23.0 us.)
    constexpr int nplanes = NCH;
    const int c0 = cgrp * NCH;
    // template of this wave's plane: issue the loads now, park them in LDS after the tables
    const bool owns = (wave < nplanes && c0 + wave < C);  // channel tails / four-plane workgroups: no plane here
    const int plane = n * C + c0 + wave;
    constexpr int NZ = XCORR ? (RZ * RZ + 63) / 64 : 1;
    float zreg[NZ];
    float zq[4] = {0.0f, 0.0f, 0.0f, 0.0f}, isz = 1.0f;
    if constexpr (MM != 0) {
        if (owns) xh_template_load(z + (size_t)plane * (RZ * RZ), lane, zq);
    } else if (XCORR && owns) {
        const float* __restrict__ zg = z + (size_t)plane * (RZ * RZ);
#pragma unroll
        for (int t = 0; t < NZ; ++t) zreg[t] = zg[min(lane + 64 * t, RZ * RZ - 1)];
    }

    // ---- sample tables: wave 0 builds the y axis, wave 1 the x axis (lane = sample), one barrier ------------------
    // (Every wave building both tables itself was measured: eight waves x two tables of ~150 VALU instructions each
    // cost more issue slots on the CU than the barrier they saved: 5.1 k instead of 4.3 k ticks.)
    // Entries are stored re-based and packed (16 bytes): y = {row byte offset lo, hi, weight lo, hi}, x = {window
    // column lo, hi, weight lo, hi}; consumers fetch an entry with one ds_read_b128.
    // With a hint entry the tables arrive FINISHED (fx_write_hint built them when the roi was made, one frame earlier):
    // waves 0 / 1 copy 1 KB each instead of ~150 vector instructions and two IEEE divisions; the entry's geometry stamp
    // must match this launch's level (another pad / map size: the tables are rebuilt here, the assignment stands).
    const bool hent = XCORR && RX == 30 && k_assigned >= 0 && g8[4] == pad && g8[5] == H && g8[6] == W &&
                      g8[7] == __float_as_int(scale);
    const int hb[4] = {g8[0], g8[1], g8[2], g8[3]};
    // the entries every wave fetched for itself are enough (no LDS tables, no barrier): a verified-geometry hint and a window
    // the plane-pair forms take (workgroup-uniform)
    const bool fast = !NHWC && MM == 1 && hent && hb[3] - hb[2] + 1 <= 64
#ifdef SMOT_DEBUG
                      && S.abl != 3 && S.abl != 12        // (3: the one-plane-per-wave A/B form reads the LDS tables; 12: A/B of this path)
#endif
        ;
    if (fast) {
    } else if (wave < 2 && hent) {
        tab[wave][lane] = tab_early;
        if (lane < 2 * RH * G) tab[wave][64 + lane] = make_int4(0, 0, 0, 0);      // the pad behind the table
    } else if (wave < 2) {
        int lo = 0, hi = 0;
        float wl = 0.0f, wh = 0.0f;
        if (lane < NS) {
            if (wave == 0) {
                axis_sample(y1, bin_h, G, lane, H, pad, &lo, &hi, &wl, &wh);
            } else {
                axis_sample(x1, bin_w, G, lane, W, pad, &lo, &hi, &wl, &wh);
            }
        }
        // Bounding window of the touched real cells.  Cell indices are non-decreasing in the sample index and a
        // zero low weight means "outside" (1 - frac is never 0), so the first touched entry holds the minimum and
        // the last the maximum: one ballot + two readlanes instead of a 6-step wave reduction.
        int mn = 0x7fffffff, mx = -1;
        const unsigned long long m = __ballot(wl != 0.0f || wh != 0.0f);
        if (m != 0ull) {
            mn = __builtin_amdgcn_readlane((wl != 0.0f) ? lo : hi, __ffsll((long long)m) - 1);
            mx = __builtin_amdgcn_readlane((wh != 0.0f) ? hi : lo, 63 - __clzll((long long)m));
        }
        // re-base: zero-weight entries point at a safe cell; rows become byte offsets inside a plane, columns
        // become window-relative
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
        tab[wave][lane] = e;
        if (lane < 2 * RH * G) tab[wave][64 + lane] = make_int4(0, 0, 0, 0);      // the pad behind the table
        if (lane == 0) {
            wbound[2 * wave] = mn;
            wbound[2 * wave + 1] = mx;
        }
    }
    FX_TRACE(7)                                   // (wave 0 at the table barrier)
    if (!fast) __syncthreads();
    const int ymin = hent ? hb[0] : wbound[0], ymax = hent ? hb[1] : wbound[1];
    const int xmin = hent ? hb[2] : wbound[2], xmax = hent ? hb[3] : wbound[3];
    if (ymax < ymin || xmax < xmin) {
        // every sample in the virtual zero border: pooled planes are exact zeros -> zero response
        if (owns) {
            if (XCORR) {
                for (int e = lane; e < HO * HO; e += 64) resp[(size_t)plane * HO * HO + e] = 0.0f;
                if (S.plane_max != nullptr && lane == 0) S.plane_max[plane] = 0.0f;
            }
            if (x_debug != nullptr)
                for (int e = lane; e < RX * RX; e += 64) x_debug[(size_t)plane * RX * RX + e] = 0.0f;
        }
        return;
    }
    const int ww = xmax - xmin + 1;
    // (Measured and dropped, round 4: s_setprio 1..3 for the waves of wide-window workgroups — twice a narrow one's pooling,
    // they set the kernel's makespan: 15.3-15.6 us at every priority against 15.3-15.4 without, 36.9 vs 36.9 at 100 tracks,
    // measure/gpu_r04_prio.sh.  Issue arbitration is not what holds them back.)
    FX_TRACE(1)

    if constexpr (MM != 0) {
        // (the template's Toeplitz rows are built inside the pooling, behind the issue of its first batch of row loads)
    } else if (XCORR && owns) {
        float* zs = sm + (wave >> 1) * (2 * XP + 2 * ZP) + 2 * XP + (wave & 1) * ZP;    // this wave's template
#pragma unroll
        for (int t = 0; t < NZ; ++t) {
            const int e = lane + 64 * t;
            if (e < RZ * RZ) {
                const int u = e / RZ;
                zs[u * ZS + (e - u * RZ)] = zreg[t];
            }
        }
    }
    FX_TRACE(2)

    // ---- pooling ----------------------------------------------------------------------------------------------
    const FT* __restrict__ fbase = reinterpret_cast<const FT*>(P.feat[lvl]);
    // batched: the image's offset goes into the 64-bit base (a batch of maps passes 4 GiB; lane offsets stay 32-bit)
    if constexpr (BATCHED) fbase += (size_t)img * ((size_t)C * H * W);
    const unsigned plane_bytes = (unsigned)(H * W) * (unsigned)sizeof(FT);
    // the tables (and a hint's) hold row offsets in bytes of an fp32 map: 2-byte maps halve them where they are used
    constexpr int ROW_SHIFT = sizeof(FT) == 2 ? 1 : 0;
    // (row runs, fx_run_within: a row and the window's last row in the tables' unit)
    const unsigned row_bytes = (unsigned)W * 4u, last_row = (unsigned)(ymax * W) * 4u;
    // One batch = ROWS pooled rows of one plane (or of a plane pair side by side).  `PAIR`: lanes 32..63 pool the
    // wave's second plane and the two waves of the pair split the pooled rows; `CHUNKED`: windows wider than 64
    // columns (rare: small batches keep its loop-carried accumulators out of the register peak).
    auto pool = [&](auto pair_tag, auto chunk_tag, auto x2_tag, auto rows_tag) {
        constexpr bool PAIR = decltype(pair_tag)::value;
        constexpr bool CHUNKED = decltype(chunk_tag)::value;
        constexpr bool X2 = decltype(x2_tag)::value;           // a lane loads TWO adjacent window columns (33..64-column windows)
        constexpr int ROWS = decltype(rows_tag)::value;
        constexpr int NV = X2 ? 2 : 1;
        static_assert(!X2 || (PAIR && !CHUNKED), "two columns per lane is a form of the plane-pair mode");
        const int half = PAIR ? (lane >> 5) : 0;
        const int col = PAIR ? (lane & 31) : lane;
        const int pw = col < RX ? col : 0;
        // this wave's plane(s) and destination(s) in the LDS image of the correlation
        const int pl0 = PAIR ? 2 * (wave >> 1) : wave;                 // first plane within the workgroup
        const bool has0 = (c0 + pl0 < C);
        const bool has1 = PAIR && (c0 + pl0 + 1 < C);
        if (!has0) return;
        const bool mine = PAIR ? (half == 0 || has1) : true;           // this lane's plane exists
        const unsigned lane_plane = (PAIR && half == 1 && has1) ? plane_bytes : 0u;
        float* xdst = sm + ((pl0 + half) >> 1) * (2 * XP + 2 * ZP) + ((pl0 + half) & 1) * XP;
        // buffer resource of the (first) plane: wave-uniform base, offsets are 32-bit
        const FT* pbase = fbase + (size_t)(c0 + pl0) * H * W;
        unsigned long long pa = reinterpret_cast<unsigned long long>(pbase);
        const unsigned pa_lo = __builtin_amdgcn_readfirstlane((unsigned)pa);
        const unsigned pa_hi = __builtin_amdgcn_readfirstlane((unsigned)(pa >> 32));
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<void*>(((unsigned long long)pa_hi << 32) | pa_lo), 0, 0x7fffffff, 0x00020000);
        // horizontal taps of this lane's pooled column: entries 2*pw, 2*pw+1 of the x table
        int sxl[G], sxh[G];
        float hxw[G], lxw[G];
#pragma unroll
        for (int ix = 0; ix < G; ++ix) {
            const int4 e = fast ? xe_early[ix] : tab[1][pw * G + ix];
            sxl[ix] = e.x;
            sxh[ix] = e.y;
            hxw[ix] = __int_as_float(e.z);
            lxw[ix] = __int_as_float(e.w);
        }
        const int row0 = PAIR ? (wave & 1) * RH : 0;           // first pooled row of this wave (wave-uniform)
        const int nrows = PAIR ? RH : RX;
        const int nchunk = CHUNKED ? (ww + 63) >> 6 : 1;
        if constexpr (X2 && MM == 1) {
            // 33..64-column windows, matrix form (two workgroups per CU: 128 registers): the batches of a wave in a TWO-STAGE
            // PIPELINE — the next batch's row loads are issued as soon as this batch's vertical taps have consumed its load
            // registers, so that their memory round trip runs beside this batch's staging and horizontal taps instead of
            // behind them: ONE exposed round trip per wave instead of one per batch.  Three batches of five rows (40 load
            // registers in flight; two of eight rows spilled 30 registers).  Same loads, same FMA chains: bit-identical.
            constexpr int GR = (ROWS + 1) / 2, SW = 64;
            static_assert(RH % ROWS == 0 && GR * SW <= ROWS * XS, "full batches; staging fits a batch's own rows");
            const int wcol = min(2 * col, ww - 2);
            const unsigned voff = (unsigned)(xmin + wcol) * (unsigned)sizeof(FT) + lane_plane;
            typename fx_pair<FT>::type vl[ROWS][G], vh[ROWS][G];
            // (fast: the wave's own 30 y entries sit in ye_early, batch b's at lanes 10 b ..; else a batch's entries from LDS)
            int4 ye = fast ? ye_early : tab[0][min(lane + row0 * G, 63 + 2 * RH * G)];
            int yoff = 0;
            // the staged horizontal taps of a batch's column sums and the store of its pooled rows (both loops below)
            auto htaps = [&](const float (&cs)[ROWS][NV], const int r0) {
                float acc[ROWS];
                float* stage = xdst + r0 * XS;
#pragma unroll
                for (int g0 = 0; g0 < ROWS; g0 += GR) {
#pragma unroll
                    for (int b = g0; b < g0 + GR && b < ROWS; ++b)
#pragma unroll
                        for (int k = 0; k < NV; ++k) stage[(b - g0) * SW + wcol + k] = cs[b][k];
                    float p[GR][G][2];
#pragma unroll
                    for (int b = g0; b < g0 + GR && b < ROWS; ++b)
#pragma unroll
                        for (int ix = 0; ix < G; ++ix) {
                            p[b - g0][ix][0] = stage[(b - g0) * SW + sxl[ix]];
                            p[b - g0][ix][1] = stage[(b - g0) * SW + sxh[ix]];
                        }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int b = g0; b < g0 + GR && b < ROWS; ++b)
#pragma unroll
                        for (int ix = 0; ix < G; ++ix) {
                            acc[b] = fmaf(hxw[ix], p[b - g0][ix][0], ix == 0 ? 0.0f : acc[b]);
                            acc[b] = fmaf(lxw[ix], p[b - g0][ix][1], acc[b]);
                        }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int b = 0; b < ROWS; ++b) {
                    const int ph = r0 + b;
                    if (col < RX && ph < row0 + nrows && ph < RX && mine) xdst[ph * XS + col] = acc[b] * (1.0f / (float)(G * G));
                }
            };
            // ROW RUNS (fx_run_within, sr_xcorr.hip).  A batch's 10 samples name 20 rows and loaded each of them; in a 65-row
            // window they are 11 or 12 DISTINCT rows.  `ye` holds all of the wave's 30 entries here, with or without a hint: where
            // each of its three batches lies within RMAX = 12 rows from its first entry's, a batch loads those 12 consecutive rows
            // once (clamped to the window's last row) into one register tuple and the vertical chains read their rows out of it by
            // wave-uniform index (fx_run_fma4x2): 12 loads and 24 registers in flight per batch instead of 20 and 40, the same
            // cells into the same FMA chains — bit-identical.  The decision is taken once for the wave, not per batch: the
            // pipeline carries a batch's load registers round the loop, and a loop that could take either form per batch would
            // carry both sets.  A wave with one batch that is not a run (entries re-based to a row before the batch's first: the
            // bottom border, integral coordinates; a bin more than two rows tall; NaN tables) takes today's loop below, unchanged.
            // Measured (profiles/pool_row_runs_ab.json, seven alternating pairs, two sessions): 52.82 -> 51.65 and 52.54 -> 51.73 us
            // per step, this form's pooling 9.5 k -> 8.4 k ticks (profiles/pool_row_runs_before.md: the address unit was issuing
            // for ~80 % of that phase).
            // Measured and dropped: the same for the one-column forms below (windows <= 32 columns: 30 samples, RMAX 32, loads
            // of 20 / 28 / 32 rows by the rows the batch needs; the extraction: 16 samples, RMAX 18) — bit-identical, but their
            // pooling got SLOWER (7.2 k -> 8.0 k, extraction 3.2 k -> 4.0 k ticks, 52.98 us per step): a one-column load costs the
            // address unit half of a two-column one, and every tap pays a switch of the register index, which two columns share
            // here.  Also dropped: the compiler's own form of a uniformly indexed register (54.34 us, see fx_run_fma4x2).
            constexpr int NE = ROWS * G, RMAX = NE + 2;
            static_assert(RMAX * NV <= 32, "a run fits the register tuple");
            if (fx_run_within<NE, RH / ROWS>(RMAX, ye, lane, RH * G, row_bytes)) {
                int il, ih;
                fx_run_index<NE, RH / ROWS, NV>(ye, lane, RH * G, row_bytes, &il, &ih);
                fx_rows_t rr;
#define SMOT_FX_ISSUE_RUN()                                                                                         \
                {                                                                                                   \
                    const unsigned rb_ = (unsigned)__builtin_amdgcn_readlane(ye.x, yoff);                           \
                    _Pragma("unroll") for (int j = 0; j < RMAX; ++j) {                                              \
                        const auto v2_ = fx_load2<FT>(rsrc, voff, (int)(min(rb_ + j * row_bytes, last_row) >> ROW_SHIFT)); \
                        rr[NV * j] = fx_pair_elem<FT>(v2_, 0);                                                      \
                        rr[NV * j + 1] = fx_pair_elem<FT>(v2_, 1);                                                  \
                    }                                                                                               \
                }
                SMOT_FX_ISSUE_RUN()
                __builtin_amdgcn_sched_barrier(0);
                if (owns) {
                    unsigned char* tzw = reinterpret_cast<unsigned char*>(sm + (wave >> 1) * (2 * XP + 2 * ZP) + 2 * XP + (wave & 1) * ZP);
                    isz = xh_template_store(zq, tzw, lane);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
                for (int r0 = row0; r0 < row0 + nrows; r0 += ROWS) {
                    const float wl = __int_as_float(ye.z), wh = __int_as_float(ye.w);
                    float cs[ROWS][NV];
#pragma unroll
                    for (int b = 0; b < ROWS; ++b) {
                        const int e = yoff + b * G;
                        const int i0 = __builtin_amdgcn_readlane(il, e), i1 = __builtin_amdgcn_readlane(ih, e);
                        const int i2 = __builtin_amdgcn_readlane(il, e + 1), i3 = __builtin_amdgcn_readlane(ih, e + 1);
                        fx_run_fma4x2(rr, i0, i1, i2, i3, rl_f(wl, e), rl_f(wh, e), rl_f(wl, e + 1), rl_f(wh, e + 1), &cs[b][0], &cs[b][1]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (r0 + ROWS < row0 + nrows) {                  // (wave-uniform) the next batch's run
                        yoff += NE;
                        SMOT_FX_ISSUE_RUN()
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    htaps(cs, r0);
                }
#undef SMOT_FX_ISSUE_RUN
                return;
            }
            ye.x = (int)((unsigned)ye.x >> ROW_SHIFT);
            ye.y = (int)((unsigned)ye.y >> ROW_SHIFT);
#define SMOT_FX_ISSUE()                                                                                           \
            _Pragma("unroll") for (int b = 0; b < ROWS; ++b)                                                        \
                _Pragma("unroll") for (int iy = 0; iy < G; ++iy) {                                                  \
                    vl[b][iy] = fx_load2<FT>(rsrc, voff, __builtin_amdgcn_readlane(ye.x, yoff + b * G + iy));         \
                    vh[b][iy] = fx_load2<FT>(rsrc, voff, __builtin_amdgcn_readlane(ye.y, yoff + b * G + iy));         \
                }
            SMOT_FX_ISSUE()
            __builtin_amdgcn_sched_barrier(0);
            if (owns) {
                unsigned char* tzw = reinterpret_cast<unsigned char*>(sm + (wave >> 1) * (2 * XP + 2 * ZP) + 2 * XP + (wave & 1) * ZP);
                isz = xh_template_store(zq, tzw, lane);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
            for (int r0 = row0; r0 < row0 + nrows; r0 += ROWS) {
                const float wl = __int_as_float(ye.z), wh = __int_as_float(ye.w);
                float cs[ROWS][NV];
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        float c_ = 0.0f;
#pragma unroll
                        for (int iy = 0; iy < G; ++iy) {
                            const int e = yoff + b * G + iy;
                            c_ = fmaf(rl_f(wl, e), fx_pair_elem<FT>(vl[b][iy], k), c_);
                            c_ = fmaf(rl_f(wh, e), fx_pair_elem<FT>(vh[b][iy], k), c_);
                        }
                        cs[b][k] = c_;
                    }
                __builtin_amdgcn_sched_barrier(0);
                if (r0 + ROWS < row0 + nrows) {                      // (wave-uniform) the next batch's entries and row loads
                    if (fast) yoff += ROWS * G;
                    else {
                        ye = tab[0][min(lane + (r0 + ROWS) * G, 63 + 2 * RH * G)];
                        ye.x = (int)((unsigned)ye.x >> ROW_SHIFT);
                        ye.y = (int)((unsigned)ye.y >> ROW_SHIFT);
                    }
                    SMOT_FX_ISSUE()
                }
                __builtin_amdgcn_sched_barrier(0);
                htaps(cs, r0);
            }
#undef SMOT_FX_ISSUE
            return;
        }
#pragma unroll 1
        for (int r0 = row0; r0 < row0 + nrows; r0 += ROWS) {
            // this block's y entries: entry (b, iy) into lane b*G + iy (constant-lane readlanes below); entries past
            // the table (masked tail rows) read the zero pad: weight 0, offset 0
            // (fast: only the narrow plane-pair form comes here — ONE batch at r0 == row0, the entries ye_early holds)
            const int4 ye = (fast && PAIR && !CHUNKED) ? ye_early : tab[0][min(lane + r0 * G, 63 + 2 * RH * G)];
            const unsigned ol = (unsigned)ye.x >> ROW_SHIFT, oh = (unsigned)ye.y >> ROW_SHIFT;
            const float wl = __int_as_float(ye.z), wh = __int_as_float(ye.w);
            float acc[ROWS];
            if (CHUNKED) {
#pragma unroll
                for (int b = 0; b < ROWS; ++b) acc[b] = 0.0f;
            }
#pragma unroll 1
            for (int ch = 0; ch < nchunk; ++ch) {
                const int cbase = ch << 6;                                   // first window column of the chunk
                // first window column this lane loads.  X2: columns (wcol, wcol + 1); the last pair of an odd-width
                // window is (ww-2, ww-1) — lanes past the window repeat it (same values to the same staging slots)
                const int wcol = CHUNKED ? min(cbase + col, ww - 1) : (X2 ? min(2 * col, ww - 2) : min(col, ww - 1));
                const unsigned voff = (unsigned)(xmin + wcol) * (unsigned)sizeof(FT) + lane_plane;
                float v[ROWS][G][2][NV];
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int iy = 0; iy < G; ++iy) {
                        const int e = b * G + iy;
                        if constexpr (X2) {
                            const auto l2 = fx_load2<FT>(rsrc, voff, __builtin_amdgcn_readlane((int)ol, e));
                            const auto h2 = fx_load2<FT>(rsrc, voff, __builtin_amdgcn_readlane((int)oh, e));
                            v[b][iy][0][0] = fx_pair_elem<FT>(l2, 0);
                            v[b][iy][0][NV - 1] = fx_pair_elem<FT>(l2, 1);
                            v[b][iy][1][0] = fx_pair_elem<FT>(h2, 0);
                            v[b][iy][1][NV - 1] = fx_pair_elem<FT>(h2, 1);
                        } else {
                            v[b][iy][0][0] = fx_load1<FT>(rsrc, voff, __builtin_amdgcn_readlane((int)ol, e));
                            v[b][iy][1][0] = fx_load1<FT>(rsrc, voff, __builtin_amdgcn_readlane((int)oh, e));
                        }
                    }
                // fences: hipcc otherwise sinks the loads to their first use (4 loads, wait, use, next 4 loads ...)
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (MM != 0) {
                    // the template's Toeplitz rows, while the first batch of row loads is in flight (the template's own loads
                    // were issued at the kernel's start: ~1 k cycles of conversion and LDS stores off the workgroup's chain)
                    if (r0 == row0 && ch == 0 && owns) {
                        unsigned char* tzw = reinterpret_cast<unsigned char*>(sm + (wave >> 1) * (2 * XP + 2 * ZP) + 2 * XP + (wave & 1) * ZP);
                        isz = MM == 2 ? xl_template_store(zq, tzw, lane) : xh_template_store(zq, tzw, lane);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                float cs[ROWS][NV];
#pragma unroll
                for (int b = 0; b < ROWS; ++b)
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        float c_ = 0.0f;
#pragma unroll
                        for (int iy = 0; iy < G; ++iy) {
                            const int e = b * G + iy;
                            c_ = fmaf(rl_f(wl, e), v[b][iy][0][k], c_);
                            c_ = fmaf(rl_f(wh, e), v[b][iy][1][k], c_);
                        }
                        cs[b][k] = c_;
                    }
                __builtin_amdgcn_sched_barrier(0);
                // Horizontal taps.  A lane (= pooled column) needs the column sums of up to four window columns (other
                // lanes' values).  ds_bpermute_b32 cost 10.6 LDS cycles per wave instruction here (SQ_LDS_IDX_ACTIVE,
                // profiles/r02aa_pmc_counters.md: two thirds of the LDS pipe's busy time) — so the sums of a group of
                // rows are staged in LDS instead (one ds_write per row, 2 array cycles) and every tap is a plain
                // ds_read_b32 (2 cycles): 10 instead of 42 LDS cycles per pooled row.  The staging rows are this
                // wave's own not-yet-written rows of the plane image (the batch's results are stored after its last
                // gather; LDS operations of one wave execute in order, so neither a wait nor a barrier is needed).
                // Rows are processed in two groups to keep the register peak (column sums + gathered taps + tables)
                // where the correlation phase is scheduled for.  Same values, same FMA order: bit-identical.
                constexpr int GR = ((P2 || MM == 2) && X2) ? 3 : (ROWS + 1) / 2;
                if constexpr (!CHUNKED) {
                    constexpr int SW = (X2 || !PAIR) ? 64 : 32;                      // staged floats per row (and plane)
                    static_assert(GR * SW <= (RH - (RH / ROWS) * ROWS == 0 ? ROWS : RH - (RH / ROWS) * ROWS) * XS,
                                  "staging fits the image rows of the wave's LAST batch");
                    float* stage = xdst + r0 * XS;
#pragma unroll
                    for (int g0 = 0; g0 < ROWS; g0 += GR) {
#pragma unroll
                        for (int b = g0; b < g0 + GR && b < ROWS; ++b)
#pragma unroll
                            for (int k = 0; k < NV; ++k) stage[(b - g0) * SW + wcol + k] = cs[b][k];
                        float p[GR][G][2];
#pragma unroll
                        for (int b = g0; b < g0 + GR && b < ROWS; ++b)
#pragma unroll
                            for (int ix = 0; ix < G; ++ix) {
                                p[b - g0][ix][0] = stage[(b - g0) * SW + sxl[ix]];
                                p[b - g0][ix][1] = stage[(b - g0) * SW + sxh[ix]];
                            }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int b = g0; b < g0 + GR && b < ROWS; ++b)
#pragma unroll
                            for (int ix = 0; ix < G; ++ix) {
                                // (acc[b] is not live across the loads here: first written in this group)
                                acc[b] = fmaf(hxw[ix], p[b - g0][ix][0], ix == 0 ? 0.0f : acc[b]);
                                acc[b] = fmaf(lxw[ix], p[b - g0][ix][1], acc[b]);
                            }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
                    // windows wider than 64 columns (rare): cross-lane gathers per 64-column chunk, two groups of rows
                    int al[G], ah[G];
                    bool inl[G], inh[G];
#pragma unroll
                    for (int ix = 0; ix < G; ++ix) {
                        const int tl = sxl[ix] - cbase, th = sxh[ix] - cbase;
                        inl[ix] = (unsigned)tl < 64u;
                        inh[ix] = (unsigned)th < 64u;
                        al[ix] = (tl & 63) << 2;                                  // ds_bpermute takes byte addresses
                        ah[ix] = (th & 63) << 2;
                    }
#pragma unroll
                    for (int g0 = 0; g0 < ROWS; g0 += GR) {
                        float p[GR][G][2];
#pragma unroll
                        for (int b = g0; b < g0 + GR && b < ROWS; ++b)
#pragma unroll
                            for (int ix = 0; ix < G; ++ix) {
                                p[b - g0][ix][0] = __int_as_float(__builtin_amdgcn_ds_bpermute(al[ix], __float_as_int(cs[b][0])));
                                p[b - g0][ix][1] = __int_as_float(__builtin_amdgcn_ds_bpermute(ah[ix], __float_as_int(cs[b][0])));
                            }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int b = g0; b < g0 + GR && b < ROWS; ++b)
#pragma unroll
                            for (int ix = 0; ix < G; ++ix) {
                                // a tap outside the chunk adds nothing (not even 0 * garbage)
                                acc[b] = inl[ix] ? fmaf(hxw[ix], p[b - g0][ix][0], acc[b]) : acc[b];
                                acc[b] = inh[ix] ? fmaf(lxw[ix], p[b - g0][ix][1], acc[b]) : acc[b];
                            }
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < ROWS; ++b) {
                const int ph = r0 + b;
                if (col < RX && ph < row0 + nrows && ph < RX && mine) xdst[ph * XS + col] = acc[b] * (1.0f / (float)(G * G));   // exact: /4
            }
        }
    };
    // <= 32 columns: a wave pools two planes side by side (lane = plane half x column), the two waves of a plane
    // pair split the pooled rows: ONE batch of 60 row loads per wave.  33..64 columns: the same plane-pair form with
    // TWO adjacent columns per lane (8-byte loads), two batches of 8 rows: a wide window now costs the load
    // instructions of a narrow one (it was one plane per wave in two batches of 15 rows — twice the load, FMA and
    // tap instructions per plane, and those workgroups set the kernel's makespan: 25 k vs 12 k cycles of pooling).
    // Wider than 64 (degenerate aspect ratios): one plane per wave in 64-column chunks.
    if constexpr (NHWC) {
        // channels-last maps: one stage for every window width, same plane images (sr_pool_nhwc_stage.h)
#include "sr_pool_nhwc_stage.h"
    } else
    if (ww <= 32) {
        pool(std::true_type{}, std::false_type{}, std::false_type{}, std::integral_constant<int, RH>{});
#ifdef SMOT_DEBUG
    } else if (ww <= 64 && S.abl == 3 && MM != 2) {      // A/B (measurement library, SMOT_FUSED_ABL=3): one plane per wave, two batches
        if constexpr (MM != 2) pool(std::false_type{}, std::false_type{}, std::false_type{}, std::integral_constant<int, RH>{});
#endif
    } else if (ww <= 64) {
        if constexpr (MM == 1) pool(std::true_type{}, std::false_type{}, std::true_type{}, std::integral_constant<int, RH / 3>{});
        else pool(std::true_type{}, std::false_type{}, std::true_type{}, std::integral_constant<int, (RH + 1) / 2>{});
    } else {
        pool(std::false_type{}, std::true_type{}, std::false_type{}, std::integral_constant<int, (RH + 2) / 3>{});
    }
    FX_TRACE(3)
    __syncthreads();                                      // every plane of the workgroup pooled (pairs share rows)
    if (x_debug != nullptr && owns) {
        const float* xs = sm + (wave >> 1) * (2 * XP + 2 * ZP) + (wave & 1) * XP;
        for (int e = lane; e < RX * RX; e += 64) {
            const int r = e / RX;
            x_debug[(size_t)plane * RX * RX + e] = xs[r * XS + (e - r * RX)];
        }
    }
    if constexpr (XCORR) {
#ifdef SMOT_DEBUG
        if (S.abl == 2) return;                           // timing ablation: measurement library only
#endif
        // every wave correlates its own plane (2x2 output patches per lane): all eight waves work, and the phase
        // needs few enough registers for three workgroups per CU
        if constexpr (P2) {
            if (wave < nplanes / 2 && c0 + 2 * wave < C) {
                const float* xs2 = sm + wave * (2 * XP + 2 * ZP);
                xcorr_patch2_compute<RX, RZ, 0>(xs2, xs2 + 2 * XP, lane, resp, n * C + c0 + 2 * wave, n * C + min(C, c0 + NCH));
            }
        } else if (owns) {
            float* xs1 = sm + (wave >> 1) * (2 * XP + 2 * ZP) + (wave & 1) * XP;
            const float* zs1 = sm + (wave >> 1) * (2 * XP + 2 * ZP) + 2 * XP + (wave & 1) * ZP;
            if constexpr (MM == 1) xh_correlate<RX, RZ>(xs1, reinterpret_cast<const unsigned char*>(zs1), isz, lane, resp, plane, S.plane_max);
            else if constexpr (MM == 2) xl_correlate<RX, RZ>(xs1, reinterpret_cast<const unsigned char*>(zs1), isz, lane, resp, plane, S.plane_max);
            else xcorr_patch1_compute<RX, RZ, true>(xs1, zs1, lane, resp, plane, S.plane_max);
        }
    }
    FX_TRACE(4)
#undef FX_TRACE
