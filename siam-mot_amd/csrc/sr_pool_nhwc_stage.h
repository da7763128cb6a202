// The pooling stage of the pooling (+ correlation) kernel on CHANNELS-LAST maps ([B, H, W, C] in memory; include/smot_emm.h,
// "CHANNELS-LAST FEATURE MAPS"): included by sr_xcorr_fused9_body.h in place of the NCHW row loads, between the sample tables
// (in LDS: the fast hinted path is off here) and the barrier in front of the correlation.  It leaves the same fp32 plane
// images in LDS, bit for bit: per element the NCHW stage's arithmetic in the NCHW stage's order —
//   column sum  c = fma(wl, v_lo, c); c = fma(wh, v_hi, c)        over the bin's two y samples, from 0
//   taps        acc = fma(hxw, c[x_lo], acc); acc = fma(lxw, c[x_hi], acc)   over its two x samples, from 0; windows wider
//               than 64 columns apply them per 64-column chunk like the NCHW chunked form (a zero-weight tap sits at window
//               column 0, i.e. in chunk 0, whatever its sample)
//   bin         acc * 1/(G*G)
// Decomposition: the workgroup's 8 channels are ONE run of 32 (fp32) or 16 (fp16 / bf16) bytes per pixel.  A lane takes a
// window column with the 8 channels in registers; the two halves of a wave take two pooled rows, the waves split the rows
// (pooled row = r0 + 2 * wave + half, r0 = 0, 16); windows are walked in 32-column chunks.  The column sums of a chunk are
// staged in the row's own 32 floats of each plane image (XS >= 32; the row's results are written behind its last gather —
// LDS operations of one wave execute in order), the four taps of a pooled column are gathered from there chunk by chunk
// and applied once all are in.  NOTE: lanes hand the column sums to each other through LDS WITHOUT a barrier — a store of
// srow[col] followed by another lane's load of srow[tl] — which holds only because both are issued by ONE wave in program
// order (the NCHW stage stages its sums the same way); never split a pooled row's columns over two waves.  Rows past RX (the second half of the
// last wave) run on the tables' zero-weight tail entries and the image's spare rows, and write nothing.
{
    static_assert(NCH == 8 && G == 2 && !P2 && MM != 2 && XS >= 32 && 32 * XS <= XP && RX <= 32,
                  "channels-last pooling: 8 channels per workgroup, 2x2 samples, a 32-float staging row per plane");
    if constexpr (MM != 0) {
        if (owns) {
            unsigned char* tzw = reinterpret_cast<unsigned char*>(sm + (wave >> 1) * (2 * XP + 2 * ZP) + 2 * XP + (wave & 1) * ZP);
            isz = xh_template_store(zq, tzw, lane);
        }
    }
    const int half = lane >> 5, col = lane & 31;
    const int pw = col < RX ? col : 0;
    int sxl[G], sxh[G];
    float hxw[G], lxw[G];
#pragma unroll
    for (int ix = 0; ix < G; ++ix) {
        const int4 e = tab[1][pw * G + ix];
        sxl[ix] = e.x;
        sxh[ix] = e.y;
        hxw[ix] = __int_as_float(e.z);
        lxw[ix] = __int_as_float(e.w);
    }
    const FT* __restrict__ crun = fbase + c0;                  // the workgroup's channel run of pixel 0
    const int nch64 = ww > 64 ? (ww + 63) >> 6 : 1;
#pragma unroll 1
    for (int r0 = 0; r0 + 2 * wave < RX; r0 += 16) {           // (wave-uniform)
        const int ph = r0 + 2 * wave + half;                   // <= 31: entries 2 ph, 2 ph + 1 exist (zero weights past the table)
        const int4 ye0 = tab[0][ph * G], ye1 = tab[0][ph * G + 1];
        // the tables (and a hint's) hold row offsets in BYTES of an fp32 NCHW row: pixels of the row's start here
        const unsigned ro[2 * G] = {(unsigned)ye0.x >> 2, (unsigned)ye0.y >> 2, (unsigned)ye1.x >> 2, (unsigned)ye1.y >> 2};
        const float wy[2 * G] = {__int_as_float(ye0.z), __int_as_float(ye0.w), __int_as_float(ye1.z), __int_as_float(ye1.w)};
        float* srow = sm + ph * XS;                            // + plane slot: this row of plane k's image
        float pv[G][2][NCH];
#pragma unroll
        for (int ix = 0; ix < G; ++ix)
#pragma unroll
            for (int k = 0; k < NCH; ++k) pv[ix][0][k] = pv[ix][1][k] = 0.0f;
#pragma unroll 1
        for (int cb = 0; cb < ww; cb += 32) {
            const int wcol = min(cb + col, ww - 1);            // lanes past the window repeat its last column (unused slots)
            float v[2 * G][NCH];
#pragma unroll
            for (int t = 0; t < 2 * G; ++t) feat_ld8<FT>(crun + (size_t)(ro[t] + (unsigned)(xmin + wcol)) * (size_t)C, v[t]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                float c_ = 0.0f;
#pragma unroll
                for (int t = 0; t < 2 * G; ++t) c_ = fmaf(wy[t], v[t][k], c_);
                srow[(k >> 1) * (2 * XP + 2 * ZP) + (k & 1) * XP + col] = c_;
            }
#pragma unroll
            for (int ix = 0; ix < G; ++ix) {
                const int tl = sxl[ix] - cb, th = sxh[ix] - cb;
                if ((unsigned)tl < 32u) {
#pragma unroll
                    for (int k = 0; k < NCH; ++k) pv[ix][0][k] = srow[(k >> 1) * (2 * XP + 2 * ZP) + (k & 1) * XP + tl];
                }
                if ((unsigned)th < 32u) {
#pragma unroll
                    for (int k = 0; k < NCH; ++k) pv[ix][1][k] = srow[(k >> 1) * (2 * XP + 2 * ZP) + (k & 1) * XP + th];
                }
            }
        }
        float acc[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) acc[k] = 0.0f;
#pragma unroll 1
        for (int ch = 0; ch < nch64; ++ch) {
#pragma unroll
            for (int ix = 0; ix < G; ++ix) {
                const bool inl = nch64 == 1 || (sxl[ix] >> 6) == ch;
                const bool inh = nch64 == 1 || (sxh[ix] >> 6) == ch;
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    acc[k] = inl ? fmaf(hxw[ix], pv[ix][0][k], acc[k]) : acc[k];
                    acc[k] = inh ? fmaf(lxw[ix], pv[ix][1][k], acc[k]) : acc[k];
                }
            }
        }
        if (col < RX && ph < RX) {
#pragma unroll
            for (int k = 0; k < NCH; ++k)
                srow[(k >> 1) * (2 * XP + 2 * ZP) + (k & 1) * XP + col] = acc[k] * (1.0f / (float)(G * G));
        }
    }
}
