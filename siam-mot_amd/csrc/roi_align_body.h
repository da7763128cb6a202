// The body of the generic level-routed ROIAlign kernel, shared by its single-image and batched forms (roi_align.hip):
// included inside each kernel's braces, which define BATCHED and I (the batch's ImageRows, or NoImages) — one text in two
// kernels, so that the single-image kernel compiles to the same code as before batching existed.
// FT (defined by the kernel as well) is the maps' element type: float, or f16_t / bf16_t in the *_half_* kernels, which
// convert every cell to fp32 where it is loaded (the staged window in LDS is fp32 for every type).
// NHWC (defined by the kernel too; false in the NCHW kernels): channels-last maps — only the staging of the window and the
// addressing of the unstaged fallback differ; the pooling behind them is the same text.
    // num_images == 0: rois are [R,4] on the one image of the call (the level-routed pooler).
    // num_images >= 1: rois are [R,5] = (image index, x1, y1, x2, y2) as upstream's _C.roi_align_forward takes them,
    //                  P.feat[0] is [num_images, C, H, W]; a row whose index is out of range pools to zeros.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int wbound[4];              // ymin, ymax, xmin, xmax of the cells with non-zero weight
    const int ny = PH * G, nx = PW * G;
    float* win = reinterpret_cast<float*>(smem);
    int* y_lo = reinterpret_cast<int*>(win + RA_CH * RA_WIN_FLOATS);
    int* y_hi = y_lo + ny;
    float* wy_lo = reinterpret_cast<float*>(y_hi + ny);
    float* wy_hi = wy_lo + ny;
    int* x_lo = reinterpret_cast<int*>(wy_hi + ny);
    int* x_hi = x_lo + nx;
    float* wx_lo = reinterpret_cast<float*>(x_hi + nx);
    float* wx_hi = wx_lo + nx;

    const int r = blockIdx.x;
    const float* roi = num_images ? rois + (size_t)r * 5 + 1 : rois + (size_t)r * 4;
    // (a batched launch passes [R,4] rois and num_images 0; its rows' images come from I)
    const int image = BATCHED ? image_of_row(I, r) : (num_images ? (int)rois[(size_t)r * 5] : 0);
    int lvl = 0;
    if (P.num_levels > 1) lvl = map_level(level_boxes + (size_t)r * 4, P.k_min, P.k_max);
    if (levels_out != nullptr && blockIdx.y == 0 && threadIdx.x == 0) levels_out[r] = lvl;

    const int H = P.H[lvl], W = P.W[lvl], pad = P.pad[lvl];
    const float scale = P.scale[lvl];
    const float x1 = mul_rn(roi[0], scale), y1 = mul_rn(roi[1], scale);
    const float x2 = mul_rn(roi[2], scale), y2 = mul_rn(roi[3], scale);
    const float roi_w = fmaxf(sub_rn(x2, x1), 1.0f);
    const float roi_h = fmaxf(sub_rn(y2, y1), 1.0f);
    const float bin_h = div_rn(roi_h, (float)PH);
    const float bin_w = div_rn(roi_w, (float)PW);

    if (threadIdx.x == 0) {
        wbound[0] = 0x7fffffff;
        wbound[1] = -1;
        wbound[2] = 0x7fffffff;
        wbound[3] = -1;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < ny + nx; s += blockDim.x) {
        int lo, hi;
        float wl, wh;
        if (s < ny) {
            axis_sample(y1, bin_h, G, s, H, pad, &lo, &hi, &wl, &wh);
            y_lo[s] = lo;
            y_hi[s] = hi;
            wy_lo[s] = wl;
            wy_hi[s] = wh;
        } else {
            const int sx = s - ny;
            axis_sample(x1, bin_w, G, sx, W, pad, &lo, &hi, &wl, &wh);
            x_lo[sx] = lo;
            x_hi[sx] = hi;
            wx_lo[sx] = wl;
            wx_hi[sx] = wh;
        }
        const int b = (s < ny) ? 0 : 2;
        if (wl != 0.0f) {
            atomicMin(&wbound[b], lo);
            atomicMax(&wbound[b + 1], lo);
        }
        if (wh != 0.0f) {
            atomicMin(&wbound[b], hi);
            atomicMax(&wbound[b + 1], hi);
        }
    }
    __syncthreads();
    const int ymin = wbound[0], ymax = wbound[1], xmin = wbound[2], xmax = wbound[3];
    const int c0 = blockIdx.y * ch_per_block;
    const int c1 = min(C, c0 + ch_per_block);
    const int bins = PH * PW;
    const FT* __restrict__ f = reinterpret_cast<const FT*>(P.feat[lvl]) + (size_t)image * C * H * W;
    if (ymax < ymin || xmax < xmin || image < 0 || image >= (BATCHED ? I.num_images : max(num_images, 1))) {
        // every sample lies in the virtual zero border (or outside the padded map): exact zeros
        for (int c = c0; c < c1; ++c)
            for (int t = threadIdx.x; t < bins; t += blockDim.x) out[((size_t)r * C + c) * bins + t] = 0.0f;
        return;
    }
    const int wh_ = ymax - ymin + 1, ww = xmax - xmin + 1;
    const bool staged = (wh_ * ww <= RA_WIN_FLOATS);     // workgroup-uniform
    // re-base the tables: window-relative when staged, map-relative row offsets otherwise
    __syncthreads();
    for (int s = threadIdx.x; s < ny + nx; s += blockDim.x) {
        if (s < ny) {
            const int lo = (wy_lo[s] != 0.0f) ? y_lo[s] : ymin;
            const int hi = (wy_hi[s] != 0.0f) ? y_hi[s] : ymin;
            y_lo[s] = staged ? (lo - ymin) * ww : lo * W;
            y_hi[s] = staged ? (hi - ymin) * ww : hi * W;
        } else {
            const int sx = s - ny;
            const int lo = (wx_lo[sx] != 0.0f) ? x_lo[sx] : xmin;
            const int hi = (wx_hi[sx] != 0.0f) ? x_hi[sx] : xmin;
            x_lo[sx] = staged ? lo - xmin : lo;
            x_hi[sx] = staged ? hi - xmin : hi;
        }
    }
    __syncthreads();

    const int nch = c1 - c0;
    if (staged) {
        // ---- stage the (wh x ww) windows of all channels of this workgroup.  Wave w takes rows
        // w, w+4, ...; lanes take columns (contiguous, coalesced row segments).  All loads of a pass
        // (up to 16 rows x RA_CH channels per lane) are issued before the first LDS store, so one
        // memory round trip covers the whole pass; co-resident workgroups cover the rest. ----
        if constexpr (NHWC) {
            // channels-last maps: lanes run along the window's pixels (row-major, as the LDS image is), each takes the run of
            // the workgroup's RA_CH channels of its pixel in one 16-byte (fp32) or 8-byte (fp16 / bf16) load and writes it
            // into the same per-channel LDS images; four pixels per lane are in flight before the first LDS store
            static_assert(RA_CH == 4, "a channel run of 16 / 8 bytes");
            const FT* __restrict__ fr = f + c0;
            const int npix = wh_ * ww;
            for (int p0 = 0; p0 < npix; p0 += 4 * 256) {
                float tmp[4][RA_CH];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int p = min(p0 + 256 * k + (int)threadIdx.x, npix - 1);
                    const int row = p / ww, col = p - row * ww;
                    feat_ld_run<FT, RA_CH>(fr + ((size_t)(ymin + row) * W + xmin + col) * C, tmp[k]);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int p = p0 + 256 * k + (int)threadIdx.x;
                    if (p < npix) {
#pragma unroll
                        for (int cl = 0; cl < RA_CH; ++cl) win[cl * RA_WIN_FLOATS + p] = tmp[k][cl];
                    }
                }
            }
        } else {
        const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
        for (int col0 = 0; col0 < ww; col0 += 64) {
            const int col = col0 + tx;
            for (int row0 = 0; row0 < wh_; row0 += 64) {
                float tmp[RA_CH][16];
#pragma unroll
                for (int cl = 0; cl < RA_CH; ++cl) {
                    const FT* __restrict__ fc = f + (size_t)(c0 + min(cl, nch - 1)) * H * W;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int row = row0 + ty + 4 * k;
                        tmp[cl][k] = (row < wh_ && col < ww) ? feat_ld<FT>(fc + ((ymin + row) * W + xmin + col)) : 0.0f;
                    }
                }
#pragma unroll
                for (int cl = 0; cl < RA_CH; ++cl) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int row = row0 + ty + 4 * k;
                        if (row < wh_ && col < ww) win[cl * RA_WIN_FLOATS + row * ww + col] = tmp[cl][k];
                    }
                }
            }
        }
        }
        __syncthreads();
    }
    // channels-last maps read in place (windows past the LDS budget): cell (y, x) of channel c at ((y * W + x) * C + c)
    const int cell = NHWC ? (staged ? 1 : C) : 1;
    if constexpr (sizeof(FT) == 4) {
    // bins outer (tables of one bin in registers), channels inner
    for (int t = threadIdx.x; t < bins; t += 256) {
        const int ph = t / PW;
        const int pw = t - ph * PW;
        int ylo[G], yhi[G], xlo[G], xhi[G];
        float wyl[G], wyh[G], wxl[G], wxh[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            ylo[i] = y_lo[ph * G + i];
            yhi[i] = y_hi[ph * G + i];
            wyl[i] = wy_lo[ph * G + i];
            wyh[i] = wy_hi[ph * G + i];
            xlo[i] = x_lo[pw * G + i];
            xhi[i] = x_hi[pw * G + i];
            wxl[i] = wx_lo[pw * G + i];
            wxh[i] = wx_hi[pw * G + i];
        }
        for (int cl = 0; cl < nch; ++cl) {
            // window larger than the LDS budget (degenerate aspect ratios): gather straight from the map
            const float* __restrict__ src = staged ? (const float*)(win + cl * RA_WIN_FLOATS)
                                                   : reinterpret_cast<const float*>(f + (NHWC ? (size_t)(c0 + cl) : (size_t)(c0 + cl) * H * W));
            float acc = 0.0f;
#pragma unroll
            for (int iy = 0; iy < G; ++iy) {
#pragma unroll
                for (int ix = 0; ix < G; ++ix) {
                    const float v1 = src[(ylo[iy] + xlo[ix]) * cell];
                    const float v2 = src[(ylo[iy] + xhi[ix]) * cell];
                    const float v3 = src[(yhi[iy] + xlo[ix]) * cell];
                    const float v4 = src[(yhi[iy] + xhi[ix]) * cell];
                    const float w1 = wyl[iy] * wxl[ix], w2 = wyl[iy] * wxh[ix];
                    const float w3 = wyh[iy] * wxl[ix], w4 = wyh[iy] * wxh[ix];
                    acc += w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
                }
            }
            out[((size_t)r * C + c0 + cl) * bins + t] = acc / (float)(G * G);
        }
    }
    } else {
    // 2-byte maps: the same loop over `src_of(cl)`, where channel cl's cells are read — the staged window (fp32) or the map
    // itself (converted cell by cell); which one is workgroup-uniform, so the two sources get a loop each
    auto pool_bins = [&](auto src_of) __attribute__((always_inline)) {
    for (int t = threadIdx.x; t < bins; t += 256) {
        const int ph = t / PW;
        const int pw = t - ph * PW;
        int ylo[G], yhi[G], xlo[G], xhi[G];
        float wyl[G], wyh[G], wxl[G], wxh[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            ylo[i] = y_lo[ph * G + i];
            yhi[i] = y_hi[ph * G + i];
            wyl[i] = wy_lo[ph * G + i];
            wyh[i] = wy_hi[ph * G + i];
            xlo[i] = x_lo[pw * G + i];
            xhi[i] = x_hi[pw * G + i];
            wxl[i] = wx_lo[pw * G + i];
            wxh[i] = wx_hi[pw * G + i];
        }
        for (int cl = 0; cl < nch; ++cl) {
            const auto* __restrict__ src = src_of(cl);
            float acc = 0.0f;
#pragma unroll
            for (int iy = 0; iy < G; ++iy) {
#pragma unroll
                for (int ix = 0; ix < G; ++ix) {
                    const float v1 = feat_ld(src + (ylo[iy] + xlo[ix]) * cell);
                    const float v2 = feat_ld(src + (ylo[iy] + xhi[ix]) * cell);
                    const float v3 = feat_ld(src + (yhi[iy] + xlo[ix]) * cell);
                    const float v4 = feat_ld(src + (yhi[iy] + xhi[ix]) * cell);
                    const float w1 = wyl[iy] * wxl[ix], w2 = wyl[iy] * wxh[ix];
                    const float w3 = wyh[iy] * wxl[ix], w4 = wyh[iy] * wxh[ix];
                    acc += w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
                }
            }
            out[((size_t)r * C + c0 + cl) * bins + t] = acc / (float)(G * G);
        }
    }
    };
    if (staged) {
        pool_bins([&](int cl) { return (const float*)(win + cl * RA_WIN_FLOATS); });
    } else {
        pool_bins([&](int cl) { return f + (NHWC ? (size_t)(c0 + cl) : (size_t)(c0 + cl) * H * W); });
    }
    }
