"""Deterministic inputs, reference answers, bounds and mutants for tests/test_roi_pool_edges.py: the ROIAlign family
(csrc/roi_align_body.h, csrc/sr_xcorr_fused9_body.h, csrc/sr_xcorr_gather_body.h, the one-launch extraction) at the
edges of its geometry:

  * border    sample coordinates exactly at -1, 0, size - 1 and size, one fp32 below -1 and above size, in (-1, 0) and
              in (size - 1, size], on both axes and both ends, without and with a virtual pad of 8 cells;
  * integral  every sample coordinate an integer (every high weight exactly 0, the first and last entry included);
  * window    touched windows 1, 2, 31, 32, 33, 63, 64, 65 cells wide and as wide as the map, xmin even and odd, map widths
              even and odd, windows on column 0, on column W - 1 and on the last cell of a level; 64 x 64 and 64 x 65 cells
              (the generic kernel's staging budget of 4096 cells) at 1 .. 4 samples per bin;
  * tiny / outside / huge   zero-size and sub-cell rois, x2 < x1, y2 < y1, rois beyond each side, half outside,
              -1000 .. 2000 px and 1e6 px;
  * pad       virtual padding ``int(pad_pixels / stride)`` for 512 and 100 px, sample pairs straddling the real / pad
              border on all four sides in both directions;
  * levels    level boxes (separate from the rois) with sqrt(area) exactly 112 / 224 / 448, the nearest fp32 sizes on both
              sides at which ``O.level_mapper`` changes its answer, a 1 x 1 and a 1e4 box.

A case is (pyramid, channel count, rois, level boxes, pooled size, samples per bin, pad pixels).  Its reference answers
for a pooled shape and a sampling ratio (``reference``):

  ref32   ``O.sr_pool`` / ``O.roi_align`` / ``O.level_mapper`` in fp32 on ``O.pad_features`` (physical padding);
  ref64   the same operation with the sample tables of ``O._axis_samples(..., torch.float32)`` (validity, cells and weights
          are the reference's own fp32 roundings, widened) and every product and sum in fp64;
  den     the same evaluation on |feat|: ``sum w |v|`` per output;
  e32     max |ref32 - ref64| / den over the outputs with den > 0.

``bound`` = ``(2 e32 + 2^-22) * den``: two fp32 evaluations in different summation orders are each within the operation's
own rounding of the truth, 2^-22 covers the final division and store.  ``violates`` is THE criterion of the GPU tests
(levels, exact zeros where den == 0, the bound), and ``mutant`` restates the reference with one rule changed so that
the CPU tests can show that a wrong kernel breaks it.  Nothing here touches a device."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import emm_oracle as O

F32 = np.float32
SCALES4 = (0.25, 0.125, 0.0625, 0.03125)
PYRAMIDS = {"A": ((56, 88), (28, 44), (14, 22), (7, 11)),
            "B": ((57, 89), (29, 45), (15, 23), (7, 11)),          # the odd-width twin
            "S": ((72, 96),)}                                      # one level, scale 1/4
MARGIN = 2.0 ** -22
E32_MAX = 2.0 ** -21
OLD_TOL = 1e-5                                                     # atol = rtol of the earlier pooling tests
MUTANTS = ("ge_size_invalid", "le_m1_invalid", "no_clamp0", "aligned", "no_side_clamp", "pad_replicate", "pad_untruncated",
           "level_no_plus1", "level_no_eps", "coord_order", "drop_last_high")


def scales_of(pyr):
    return SCALES4[:len(PYRAMIDS[pyr])]


@functools.lru_cache(maxsize=None)
def maps(pyr, C, images=1):
    """``randn * 3`` plus a constant per plane (and image), so that a wrong plane shows: tuple of [images, C, H, W] fp32."""
    out = []
    for l, (h, w) in enumerate(PYRAMIDS[pyr]):
        g = torch.Generator().manual_seed(7000 + 131 * C + 17 * l + ord(pyr))
        m = torch.randn((images, C, h, w), generator=g) * 3.0
        m = m + (torch.arange(C, dtype=torch.float32) * 0.75 - 2.0)[None, :, None, None]
        m = m + (torch.arange(images, dtype=torch.float32) * 0.375)[:, None, None, None]
        out.append(m.contiguous())
    return tuple(out)


def pad_cells(case):
    return [O.pad_cells(case["pad_pixels"], l) for l in range(len(PYRAMIDS[case["pyr"]]))]


# ---- the reference's sample tables, and what the tests read off them ------------------------------------------------
def roi_axes(roi, scale, ph, pw, clamp_side=True):
    """(y start, y bin, x start, x bin) of a roi as ``O.roi_align`` forms them (fp32 tensors)."""
    x1, y1, x2, y2 = [roi[k].to(torch.float32) * scale for k in range(4)]
    w, h = x2 - x1, y2 - y1
    if clamp_side:
        w, h = torch.clamp(w, min=1.0), torch.clamp(h, min=1.0)
    return y1, h / ph, x1, w / pw


def sample_coords(start, bin_size, n_bins, grid, order="reference"):
    """The sample coordinates in fp32, in ``O._axis_samples``' rounding sequence (or one sequence away)."""
    p = torch.arange(n_bins, dtype=torch.float32).repeat_interleave(grid)
    i = torch.arange(grid, dtype=torch.float32).repeat(n_bins)
    if order == "reference":
        return start + p * bin_size + (i + 0.5) * bin_size / grid
    return start + (p + (i + 0.5) / grid) * bin_size


def mutant_tables(start, bin_size, n_bins, grid, size, mut):
    """``O._axis_samples`` in fp32 with one rule changed."""
    c = sample_coords(start, bin_size, n_bins, grid, "other" if mut == "coord_order" else "reference")
    if mut == "aligned":
        c = c - 0.5
    low_bad = (c <= -1.0) if mut == "le_m1_invalid" else (c < -1.0)
    high_bad = (c >= size) if mut == "ge_size_invalid" else (c > size)
    valid = ~(low_bad | high_bad)
    if mut != "no_clamp0":
        c = torch.clamp(c, min=0)
    low = torch.clamp(c, min=0, max=2.0 ** 30).to(torch.int64)
    at_edge = low >= size - 1
    low = torch.where(at_edge, torch.full_like(low, size - 1), low)
    high = torch.where(at_edge, low, low + 1)
    c = torch.where(at_edge, low.to(torch.float32), c)
    l = c - low.to(torch.float32)
    h = 1.0 - l
    if mut == "drop_last_high":                      # window bound from the low cells only: the last high cell is never loaded
        wl, wh = h * valid, l * valid
        lows, highs = low[wl != 0], high[wh != 0]
        if highs.numel() and (lows.numel() == 0 or int(highs.max()) > int(lows.max())):
            l = torch.where(high == highs.max(), torch.zeros_like(l), l)
    return valid, low, high, l, h


def tables(start, bin_size, n_bins, grid, size, mut=None):
    if mut in (None, "no_side_clamp", "pad_replicate", "pad_untruncated", "level_no_plus1", "level_no_eps"):
        return O._axis_samples(start, bin_size, n_bins, grid, size, torch.float32)
    return mutant_tables(start, bin_size, n_bins, grid, size, mut)


def touched(tab):
    """(first, last) touched cell of an axis from its table (weights that are not 0), or None."""
    valid, low, high, l, h = tab
    cells = torch.cat((low[(h * valid) != 0], high[(l * valid) != 0]))
    return (int(cells.min()), int(cells.max())) if cells.numel() else None


def touched_real(tab, pad, size):
    """``touched`` in cells of the real map under a virtual pad of ``pad`` cells (cells of the pad hold zeros: not touched)."""
    valid, low, high, l, h = tab
    cells = torch.cat((low[(h * valid) != 0], high[(l * valid) != 0])) - pad
    cells = cells[(cells >= 0) & (cells < size)]
    return (int(cells.min()), int(cells.max())) if cells.numel() else None


def case_tables(c, r, g=None, ph=None):
    """(y table, x table, level, pad cells, H, W) of row ``r`` of a case: the reference's own tables against the padded map."""
    g = c["g"] if g is None else g
    ph = c["out_size"] if ph is None else ph
    scales = scales_of(c["pyr"])
    lb = c["rois"] if c["level_boxes"] is None else c["level_boxes"]
    lvl = int(O.level_mapper(torch.from_numpy(lb[r:r + 1]), k_min=2, k_max=5)[0]) if len(scales) > 1 else 0
    H, W = PYRAMIDS[c["pyr"]][lvl]
    p = O.pad_cells(c["pad_pixels"], lvl)
    y1, bh, x1, bw = roi_axes(torch.from_numpy(c["rois"][r]), scales[lvl], ph, ph)
    ty = O._axis_samples(y1, bh, ph, g, H + 2 * p, torch.float32)
    tx = O._axis_samples(x1, bw, ph, g, W + 2 * p, torch.float32)
    return ty, tx, lvl, p, H, W, (sample_coords(y1, bh, ph, g), sample_coords(x1, bw, ph, g))


def _axis_matrix(tab, n_bins, grid, size):
    """[n_bins, size] fp64: the summed weights of an axis' samples per cell."""
    valid, low, high, l, h = tab
    rows = torch.arange(n_bins * grid)
    m = torch.zeros((n_bins * grid, size), dtype=torch.float64)
    m.index_put_((rows, low), h.double() * valid.double(), accumulate=True)
    m.index_put_((rows, high), l.double() * valid.double(), accumulate=True)
    return m.reshape(n_bins, grid, size).sum(1)


def pool64(fmap, roi, scale, ph, pw, g, mut=None):
    """One roi on one (physically padded) map [C, H, W]: (values, den) in fp64 with the fp32 tables."""
    f = fmap.double()
    H, W = f.shape[-2:]
    y1, bh, x1, bw = roi_axes(roi, scale, ph, pw, clamp_side=(mut != "no_side_clamp"))
    my = _axis_matrix(tables(y1, bh, ph, g, H, mut), ph, g, H)
    mx = _axis_matrix(tables(x1, bw, pw, g, W, mut), pw, g, W)
    val = torch.einsum("ph,chw,qw->cpq", my, f, mx) / (g * g)
    den = torch.einsum("ph,chw,qw->cpq", my.abs(), f.abs(), mx.abs()) / (g * g)
    return val, den


def level_mapper(boxes, k_min, k_max, mut=None):
    if mut not in ("level_no_plus1", "level_no_eps"):
        return O.level_mapper(boxes, k_min=k_min, k_max=k_max)
    one = 0.0 if mut == "level_no_plus1" else 1.0
    eps = 0.0 if mut == "level_no_eps" else 1e-6
    s = torch.sqrt((boxes[:, 2] - boxes[:, 0] + one) * (boxes[:, 3] - boxes[:, 1] + one))
    lvl = torch.floor(4.0 + torch.log2(s / 224.0 + eps))
    lvl = torch.nan_to_num(lvl, nan=float(k_min))
    return torch.clamp(lvl, min=k_min, max=k_max).to(torch.int64) - k_min


def _padded(feats, pad_pixels, mut=None):
    """Physical padding (``O.pad_features``); the mutants replicate the border, or pad by ``pad_pixels * scale`` cells without
    truncation (returned as a whole number of cells plus the shift of the roi that makes up the difference)."""
    if mut == "pad_replicate":
        out = []
        for l, f in enumerate(feats):
            p = O.pad_cells(pad_pixels, l)
            out.append(F.pad(f, [p, p, p, p], mode="replicate") if p else f)
        return tuple(out), [0.0] * len(feats)
    if mut == "pad_untruncated":
        out, shift = [], []
        for l, f in enumerate(feats):
            exact = pad_pixels * SCALES4[l]
            p = int(np.ceil(exact))
            out.append(F.pad(f, [p, p, p, p]))
            shift.append((p - exact) / SCALES4[l])                 # pixels
        return tuple(out), shift
    return O.pad_features(feats, pad_pixels), [0.0] * len(feats)


def evaluate(case, ph, pw, g, mut=None, rois=None, level_boxes=None, image=0):
    """(levels [R] int64, values [R, C, ph, pw] fp64, den) of a case with the fp32 tables, fp64 products and sums."""
    feats = tuple(m[image:image + 1] for m in maps(case["pyr"], case["C"], case.get("images", 1)))
    scales = scales_of(case["pyr"])
    rois = torch.from_numpy(case["rois"] if rois is None else rois)
    lb = case["level_boxes"] if level_boxes is None else level_boxes
    lb = rois if lb is None else torch.from_numpy(lb)
    if len(scales) == 1:
        levels = torch.zeros(len(rois), dtype=torch.int64)
    else:
        levels = level_mapper(lb, 2, 5, mut)
    padded, shift = _padded(feats, case["pad_pixels"], mut)
    val = torch.zeros((len(rois), case["C"], ph, pw), dtype=torch.float64)
    den = torch.zeros_like(val)
    for r in range(len(rois)):
        l = int(levels[r])
        val[r], den[r] = pool64(padded[l][0], rois[r] + F32(shift[l]), scales[l], ph, pw, g, mut)
    return levels, val, den


def ref32_of(case, ph, pw, g, rois=None, level_boxes=None, image=0):
    feats = tuple(m[image:image + 1] for m in maps(case["pyr"], case["C"], case.get("images", 1)))
    scales = scales_of(case["pyr"])
    rois = torch.from_numpy(case["rois"] if rois is None else rois)
    lb = case["level_boxes"] if level_boxes is None else level_boxes
    lb = rois if lb is None else torch.from_numpy(lb)
    padded = O.pad_features(feats, case["pad_pixels"])
    if ph == pw:
        return O.sr_pool(padded, lb, rois, ph, scales, g)
    assert len(scales) == 1
    r5 = torch.cat((rois.new_zeros((len(rois), 1)), rois), 1)
    return O.roi_align(padded[0], r5, scales[0], ph, pw, g)


def reference_eval(case, ph, pw, g, rois=None, level_boxes=None, image=0):
    levels, f64, den = evaluate(case, ph, pw, g, None, rois, level_boxes, image)
    f32 = ref32_of(case, ph, pw, g, rois, level_boxes, image)
    pos = den > 0
    e32 = float(((f32.double() - f64).abs()[pos] / den[pos]).max()) if bool(pos.any()) else 0.0
    return dict(levels=levels, f32=f32, f64=f64, den=den, e32=e32)


@functools.lru_cache(maxsize=None)
def reference(name, ph=None, pw=None, g=None, boxes_as_rois=False):
    """Reference answers of case ``name`` at a pooled shape and sampling ratio (default: the case's own).  ``boxes_as_rois``:
    the extraction's reading, the level boxes are the rois."""
    c = cases()[name]
    ph = c["out_size"] if ph is None else ph
    pw = ph if pw is None else pw
    g = c["g"] if g is None else g
    if boxes_as_rois:
        b = extraction_boxes(c)
        return reference_eval(dict(c, pad_pixels=0), ph, pw, g, rois=b, level_boxes=b)
    return reference_eval(c, ph, pw, g)


def extraction_boxes(c):
    """What the one-launch extraction is given of a case: boxes that are roi and level box at once (the level boxes of the
    ``levels`` family, the rois of every other).  Rows with (w + 1)(h + 1) <= 0 are left out: ``O.level_mapper`` has no
    answer for them (the square root of a negative area), they belong to the non-finite test."""
    b = c["level_boxes"] if c["family"] == "levels" else c["rois"]
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    return np.ascontiguousarray(b[area > 0])


def bound(ref):
    return (2.0 * ref["e32"] + MARGIN) * ref["den"]


def violates(ref, levels, out):
    """THE criterion of the GPU tests: a description of the first violation, or None."""
    if [int(v) for v in levels] != ref["levels"].tolist():
        return "levels %s, the reference has %s" % ([int(v) for v in levels], ref["levels"].tolist())
    out = torch.as_tensor(out).double()
    if tuple(out.shape) != tuple(ref["f64"].shape):
        return "shape %s" % (tuple(out.shape),)
    zero = ref["den"] == 0
    if bool((out[zero] != 0).any()) or bool(torch.isnan(out).any()):
        return "%d outputs without a weighted cell are not 0.0 (or NaN)" % int((out[zero] != 0).sum())
    err = (out - ref["f64"]).abs()
    bad = err > bound(ref)
    if bool(bad.any()):
        k = int(torch.argmax((err / ref["den"].clamp_min(1e-300)) * (~zero)))
        idx = np.unravel_index(k, tuple(out.shape))
        return "%d of %d outputs beyond (2 * %.3e + 2^-22) * den; worst at %s: %.9g, fp64 %.9g, den %.6g, error %.3e den" % (
            int(bad.sum()), bad.numel(), ref["e32"], idx, float(out[idx]), float(ref["f64"][idx]), float(ref["den"][idx]),
            float(err[idx] / ref["den"][idx]))
    return None


def kernel_error(ref, out):
    """Largest |out - ref64| / den over den > 0, and the share of outputs bit-identical to ref32."""
    out = torch.as_tensor(out).cpu()
    pos = ref["den"] > 0
    e = float(((out.double() - ref["f64"]).abs()[pos] / ref["den"][pos]).max()) if bool(pos.any()) else 0.0
    same = float((out.float().view(torch.int32) == ref["f32"].view(torch.int32)).double().mean())
    return e, same


def passes_old_tolerance(ref, out):
    out = torch.as_tensor(out).double()
    return bool(((out - ref["f32"].double()).abs() <= OLD_TOL + OLD_TOL * ref["f32"].double().abs()).all())


def mutant(name, mut, ph=None, pw=None, g=None):
    """(levels, values rounded to fp32) of the reference restated with rule ``mut`` changed."""
    c = cases()[name]
    ph = c["out_size"] if ph is None else ph
    levels, val, _ = evaluate(c, ph, ph if pw is None else pw, c["g"] if g is None else g, mut)
    return levels, val.float()


# ---- generators -----------------------------------------------------------------------------------------------------
def _case(family, pyr, C, rois, out_size, g=2, pad_pixels=0, level_boxes=None, rows=None, gs=None):
    rois = np.ascontiguousarray(rois, F32).reshape(-1, 4)
    assert 1 <= len(rois) <= 16
    if level_boxes is not None:
        level_boxes = np.ascontiguousarray(level_boxes, F32).reshape(-1, 4)
        assert level_boxes.shape == rois.shape
    return dict(family=family, pyr=pyr, C=C, rois=rois, level_boxes=level_boxes, out_size=out_size, g=g, pad_pixels=pad_pixels,
                rows=rows or {}, gs=gs or (g,))


LEVEL_BOX = ((10.0, 10.0, 69.0, 69.0), (10.0, 10.0, 159.0, 159.0), (10.0, 10.0, 309.0, 309.0), (10.0, 10.0, 609.0, 609.0))


def _next(v, up, k=1):
    v = F32(v)
    for _ in range(k):
        v = np.nextafter(v, F32(np.inf if up else -np.inf))
    return v


def _edge_axis(P, b, size_p, kind):
    """(start, end) in cells of an axis whose first sample is exactly -1 ("low") or one fp32 below it ("low_out"), or whose
    last sample is exactly ``size_p`` ("high") or one fp32 above it ("high_out"); found by trying neighbours of the dyadic
    solution and checked on the reference's coordinates."""
    g = 2
    if kind in ("low", "low_out"):
        base, target = -1.0 - b / 4, (F32(-1.0) if kind == "low" else _next(-1.0, False))
    else:
        base, target = size_p - P * b + b / 4, (F32(size_p) if kind == "high" else _next(size_p, True))
    for k1 in (0, 1, -1, 2, -2, 3, -3):
        s = _next(base, k1 > 0, abs(k1))
        for k2 in (0, 1, -1, 2, -2, 3, -3):
            e = _next(F32(base + P * b), k2 > 0, abs(k2))
            roi = torch.tensor([s * 4, 0.0, e * 4, 4.0])
            _, _, x1, bw = roi_axes(roi, 0.25, P, P)
            c = sample_coords(x1, bw, P, g)
            if float(bw) == b and float(c[0 if kind.startswith("low") else -1]) == float(target):
                return float(s), float(e)
    raise AssertionError("no fp32 roi puts a sample at %r" % target)


def _border(P, b, pad, C):
    """Rows 0 .. 7 on map S (scale 1/4): see ``BORDER_ROWS``; coordinates in padded-image pixels."""
    H, W = PYRAMIDS["S"][0]
    Hp, Wp = H + 2 * pad, W + 2 * pad
    inner_y = (10.25 + pad, 10.25 + pad + P * b)
    inner_x = (13.5 + pad, 13.5 + pad + P * b)
    ax = lambda size_p, kind: _edge_axis(P, b, size_p, kind)
    spec = (("low", "low"), ("low_out", None), (None, "low_out"), ("high", "high"), ("high_out", None), (None, "high_out"),
            ("low", "high"), ("high", "low"))
    rois = []
    for kx, ky in spec:
        x = inner_x if kx is None else ax(Wp, kx)
        y = inner_y if ky is None else ax(Hp, ky)
        rois.append((x[0] * 4, y[0] * 4, x[1] * 4, y[1] * 4))
    return _case("border", "S", C, rois, P, pad_pixels=pad * 4, rows=dict(spec=spec, bin=b))


def _integral(pyr, P, C, starts):
    """Every sample an integer: bin 2, start a - 1/2 (samples a + 2 p and a + 2 p + 1), on both axes."""
    scale = SCALES4[0]
    rois = [((ax - 0.5) / scale, (ay - 0.5) / scale, (ax - 0.5 + 2 * P) / scale, (ay - 0.5 + 2 * P) / scale) for ax, ay in starts]
    lb = [LEVEL_BOX[0]] * len(rois) if len(PYRAMIDS[pyr]) > 1 else None
    return _case("integral", pyr, C, rois, P, level_boxes=lb, rows=dict(starts=starts))


def _span(a, n, P=30):
    """(start, end) in cells of an axis whose touched window is [a, a + n - 1], n >= 3: first sample in (a, a + 1), last in
    (a + n - 2, a + n - 1) for 1 .. 4 samples per bin when P >= n / 2."""
    assert n >= 3
    return a + 0.01, a + n - 1 - 0.01


def _window_case(pyr, C, parity, pad_pixels=0):
    """Level-0 windows of the widths the pooling + correlation kernel switches forms at, xmin of one parity; then a window
    of each coarser level's whole width; the last row holds the last cell of the last plane of level 0."""
    H, W = PYRAMIDS[pyr][0]
    s = SCALES4[0]
    rois, want = [], []

    def add(x, y, lvl=0):                                      # (real cells -> padded-image pixels)
        sc, p = SCALES4[lvl], O.pad_cells(pad_pixels, lvl)
        rois.append(((x[0] + p) / sc, (y[0] + p) / sc, (x[1] + p) / sc, (y[1] + p) / sc))

    # width 1: only a clamp makes it (samples in [-1, 0] -> column 0; samples in [W - 1, W] -> column W - 1; the others invalid)
    add((-2.0, -0.02), (3.3, 20.1))
    want.append((0, 0))
    add((W - 0.95, W + 1.0), (5.7, 25.2))
    want.append((W - 1, W - 1))
    a0 = 4 + parity
    add((a0 + 0.004, a0 + 0.6), (7.1, 30.9))                  # narrower than a cell: its clamped side of 1 stays inside cell a0 -> 2 columns
    want.append((a0, a0 + 1))
    for n in (31, 32, 33, 63, 64, 65):
        a = a0 + (2 if n % 2 else 0)
        add(_span(a, n), _span(3 + (n % 5), 20 + n % 7))
        want.append((a, a + n - 1))
    add(_span(0, W, 60), _span(H - 12, 12))                    # the whole width, down to the last row (column 0 and W - 1)
    want.append((0, W - 1))
    n = 33 if (W - 33) % 2 == parity else 34
    add(_span(W - n, n), _span(H - 9, 9))                      # ends on the last cell of the plane
    want.append((W - n, W - 1))
    lb = [LEVEL_BOX[0]] * len(rois)
    for lvl in (1, 2, 3):
        h, w = PYRAMIDS[pyr][lvl]
        add(_span(0, w, 60), _span(0, h, 60), lvl)
        want.append((0, w - 1))
        lb.append(LEVEL_BOX[lvl])
    return _case("window", pyr, C, rois, 30, pad_pixels=pad_pixels, level_boxes=lb, rows=dict(xwin=want, parity=parity))


def _window_staging():
    """Map S, pooled 40 x 40 (the generic kernel), 1 .. 4 samples per bin: windows of 64 x 64 cells (4096: staged in LDS), 64 rows
    x 65 columns and 65 x 64 (4160: gathered from the map), 63 x 65 (4095), with odd and even corners, one on the last cell."""
    H, W = PYRAMIDS["S"][0]
    spec = ((3, 4, 64, 64), (8, 5, 64, 65), (2, 31, 65, 64), (H - 63, W - 65, 63, 65), (H - 64, W - 64, 64, 64), (0, 0, 64, 65))
    rois = []
    for y, x, nh, nw in spec:
        xs, ys = _span(x, nw, 40), _span(y, nh, 40)
        rois.append((xs[0] * 4, ys[0] * 4, xs[1] * 4, ys[1] * 4))
    return _case("window", "S", 5, rois, 40, rows=dict(win=spec), gs=(1, 2, 3, 4))


def _tiny():
    rois = ((40.0, 40.0, 40.0, 40.0),                 # zero size: the side clamps to 1 cell
            (41.0, 41.0, 42.0, 43.0),                 # narrower than a cell, inside cell (10, 10) of level 0
            (164.5, 82.0, 165.0, 83.5),               # ... and of level 2
            (100.0, 50.0, 80.0, 90.0),                # x2 < x1
            (100.0, 90.0, 140.0, 50.0),               # y2 < y1
            (200.0, 120.0, 150.0, 60.0),              # both
            (351.0, 223.0, 351.0, 223.0),             # zero size on the last pixel
            (0.0, 0.0, 0.0, 0.0))
    lb = (LEVEL_BOX[0], LEVEL_BOX[0], LEVEL_BOX[2], LEVEL_BOX[0], LEVEL_BOX[1], LEVEL_BOX[3], LEVEL_BOX[1], LEVEL_BOX[2])
    return _case("tiny", "A", 12, rois, 15, level_boxes=lb)


def _outside(pad_pixels, C):
    """352 x 224 px image (pyramid A): rows 0 .. 3 wholly beyond the left, right, top, bottom side (of the padded map), rows
    4 .. 7 half outside, at level 0 and 2."""
    p = pad_pixels
    Wpx, Hpx = 352 + 2 * p, 224 + 2 * p
    rois = ((-200.0, 40.0, -50.0, 120.0), (Wpx + 40.0, 40.0, Wpx + 200.0, 120.0), (40.0, -300.0, 200.0, -40.0),
            (40.0, Hpx + 40.0, 200.0, Hpx + 160.0),
            (-60.0, 40.0 + p, p + 60.0, 120.0 + p), (Wpx - p - 50.0, 40.0 + p, Wpx + 70.0, 120.0 + p),
            (40.0 + p, -80.0, 200.0 + p, p + 80.0), (40.0 + p, Hpx - p - 60.0, 200.0 + p, Hpx + 90.0))
    lb = [LEVEL_BOX[0], LEVEL_BOX[2]] * 4
    return _case("outside", "A", C, rois, 30, pad_pixels=p, level_boxes=lb)


def _huge():
    rois = ((-1000.0, -1000.0, 2000.0, 2000.0), (-1000.0, -1000.0, 2000.0, 2000.0), (-5e5, -5e5, 5e5, 5e5), (-5e5, -5e5, 5e5, 5e5),
            (-1e6, 100.0, 1e6, 140.0), (100.0, -1e6, 180.0, 1e6))
    lb = (LEVEL_BOX[0], LEVEL_BOX[3], LEVEL_BOX[1], LEVEL_BOX[3], LEVEL_BOX[0], LEVEL_BOX[2])
    return _case("huge", "A", 5, rois, 7, level_boxes=lb)


def _pad_case(pyr, C, pad_pixels):
    """Per level one roi across each side's real / pad border, narrow bins, so that sample pairs sit low-in-pad / high-real
    (left, top) and low-real / high-in-pad (right, bottom)."""
    rois, lb = [], []
    for lvl in range(4):
        sc = SCALES4[lvl]
        p = O.pad_cells(pad_pixels, lvl)
        h, w = PYRAMIDS[pyr][lvl]
        cx0, cx1 = p + 0.37 * w, p + 0.37 * w + min(6.3, 0.5 * w)
        cy0, cy1 = p + 0.21 * h, p + 0.21 * h + min(5.1, 0.5 * h)
        sides = (((p - 2.3, p + 3.9), (cy0, cy1)), ((p + w - 4.1, p + w + 2.6), (cy0, cy1)), ((cx0, cx1), (p - 3.2, p + 2.7)),
                 ((cx0, cx1), (p + h - 3.3, p + h + 1.9)))
        for x, y in sides:
            rois.append((x[0] / sc, y[0] / sc, x[1] / sc, y[1] / sc))
            lb.append(LEVEL_BOX[lvl])
    return _case("pad", pyr, C, rois, 30, pad_pixels=pad_pixels, level_boxes=lb)


# -- level boxes at the mapper's boundaries
def _level32(d):
    b = torch.tensor([[100.0, 60.0, 100.0, 60.0]]) + torch.tensor([[0.0, 0.0, 1.0, 1.0]]) * torch.tensor(d, dtype=torch.float32)
    return int(O.level_mapper(b, k_min=2, k_max=5)[0])


def level_is_robust(box):
    """The floor does not depend on the last bit of ``log2``: ``4 + log2(x)`` evaluated in fp64 from the same fp32 argument
    ``x = s / 224 + 1e-6f`` and rounded to fp32 has the same floor."""
    b = torch.as_tensor(box, dtype=torch.float32).reshape(1, 4)
    s = torch.sqrt((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1))
    x = s / 224.0 + 1e-6
    f32 = torch.floor(4.0 + torch.log2(x))
    f64 = torch.floor((4.0 + torch.log2(x.double())).float())
    return bool(f32 == f64)


@functools.lru_cache(maxsize=None)
def level_boundaries():
    """Per boundary 112 / 224 / 448: the largest fp32 side d (box [100, 60, 100 + d, 60 + d], sqrt(area) = d + 1 up to
    rounding) with the lower level and the smallest with the upper one, stepped outwards past candidates that are not
    robust; and how many candidates were stepped over (dropped)."""
    out, dropped = {}, 0
    for s in (112, 224, 448):
        lo, hi = F32(s - 1) * F32(0.999), F32(s - 1) * F32(1.001)
        l_lo, l_hi = _level32(lo), _level32(hi)
        assert l_hi == l_lo + 1
        a, b = int(lo.view(np.int32)), int(hi.view(np.int32))
        while b - a > 1:                                     # bisect on the bit pattern: d is positive
            m = (a + b) // 2
            if _level32(np.int32(m).view(F32)) == l_lo:
                a = m
            else:
                b = m
        below, above = np.int32(a).view(F32), np.int32(b).view(F32)
        for side, v, up in (("below", below, False), ("above", above, True)):
            for _ in range(20):
                box = (100.0, 60.0, float(F32(100.0) + v), float(F32(60.0) + v))
                if level_is_robust(box):
                    break
                dropped += 1
                v = np.nextafter(v, F32(np.inf if up else -np.inf))
            else:
                raise AssertionError("no robust box near sqrt(area) = %d" % s)
            out[(s, side)] = box
    return out, dropped


def _levels_cases():
    nb, _ = level_boundaries()
    exact, near = [], []
    for s in (112, 224, 448):
        exact.append((100.0, 60.0, 100.0 + s - 1, 60.0 + s - 1))
        for f in (1 - 1e-4, 1 + 1e-4):
            exact.append((100.0, 60.0, 100.0 + s * f - 1, 60.0 + s * f - 1))
        near += [nb[(s, "below")], nb[(s, "above")]]
        # a non-square box with the same area on the boundary: (w + 1)(h + 1) = s^2 exactly
        near.append((30.0, 20.0, 30.0 + 2 * s - 1, 20.0 + s / 2 - 1))
    exact += [(50.0, 50.0, 50.0, 50.0), (-4000.0, -4000.0, 5999.0, 5999.0)]     # 1 x 1 (k_min), 1e4 (k_max)
    rs = np.random.RandomState(77)

    def rois(n):
        xy = rs.uniform(0.0, 1.0, (n, 2)) * (200.0, 120.0)
        return np.concatenate((xy, xy + rs.uniform(30.0, 110.0, (n, 2))), 1)
    return (_case("levels", "A", 8, rois(len(exact)), 15, level_boxes=exact),
            _case("levels", "B", 16, rois(len(near)), 7, level_boxes=near))


def _ordinary():
    """Ordinary geometry, as the earlier pooling tests used: boxes of 30 .. 140 px inside the image on levels 1 .. 3.  Here the
    reference with its coordinate formed one rounding sequence away still passes 1e-5."""
    rs = np.random.RandomState(2)
    xy = rs.uniform(0, 1, (8, 2)) * (200.0, 120.0)
    rois = np.concatenate((xy, xy + rs.uniform(30, 140, (8, 2))), 1)
    return _case("ordinary", "A", 8, rois, 15, level_boxes=[LEVEL_BOX[(1, 2, 3)[i % 3]] for i in range(8)])


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["border_p7_pad0"] = _border(7, 1.0, 0, 5)
    c["border_p15_pad8"] = _border(15, 1.0, 8, 8)
    c["border_p30_pad0"] = _border(30, 0.5, 0, 12)
    c["border_p30_pad8"] = _border(30, 0.5, 8, 16)
    c["integral_p7"] = _integral("S", 7, 5, ((0, 0), (3, 58), (82, 5), (82, 58)))
    c["integral_p15"] = _integral("B", 15, 8, ((0, 0), (7, 27), (59, 3), (59, 27)))
    c["integral_p30"] = _integral("S", 30, 16, ((0, 0), (36, 12), (11, 7)))
    c["window_A_even"] = _window_case("A", 8, 0)
    c["window_A_odd"] = _window_case("A", 5, 1)
    c["window_B_even"] = _window_case("B", 12, 0)
    c["window_B_odd"] = _window_case("B", 16, 1, pad_pixels=100)
    c["window_S_staging"] = _window_staging()
    c["tiny_A"] = _tiny()
    c["outside_pad0"] = _outside(0, 8)
    c["outside_pad100"] = _outside(100, 5)
    c["huge_A"] = _huge()
    c["pad_512_A"] = _pad_case("A", 16, 512)
    c["pad_100_A"] = _pad_case("A", 8, 100)
    c["pad_100_B"] = _pad_case("B", 12, 100)
    c["pad_512_B"] = _pad_case("B", 5, 512)
    c["levels_exact"], c["levels_nearest"] = _levels_cases()
    c["ordinary_A"] = _ordinary()
    return c


CASE_NAMES = ("border_p7_pad0", "border_p15_pad8", "border_p30_pad0", "border_p30_pad8", "integral_p7", "integral_p15",
              "integral_p30", "window_A_even", "window_A_odd", "window_B_even", "window_B_odd", "window_S_staging", "tiny_A",
              "outside_pad0", "outside_pad100", "huge_A", "pad_512_A", "pad_100_A", "pad_100_B", "pad_512_B", "levels_exact",
              "levels_nearest", "ordinary_A")
SINGLE_LEVEL = tuple(n for n in CASE_NAMES if n.startswith(("border_", "integral_p7", "integral_p30", "window_S")))


# ---- non-finite and inverted rows (no reference contract) ---------------------------------------------------------------
DIRTY_KINDS = ("roi_x1_nan", "roi_y2_nan", "roi_x2_pinf", "roi_y1_ninf", "roi_at_pinf", "roi_at_ninf", "box_nan", "box_pinf",
               "box_ninf", "box_inverted")


def nonfinite_rows(pad_pixels=0):
    """(rois, level boxes) dirty and clean, and {kind: row}: 16 rows on pyramid A, the dirty ones among clean ones.  A dirty
    value in a roi coordinate leaves the level box finite and the other way round; ``roi_at_*``: both corners at the same
    infinity (every sample invalid: exact zeros); ``box_inverted``: w + 1 < 0 <= h + 1."""
    rs = np.random.RandomState(4242)
    xy = rs.uniform(0.0, 1.0, (16, 2)) * (240.0, 140.0) + pad_pixels
    rois = np.concatenate((xy, xy + rs.uniform(20.0, 100.0, (16, 2))), 1).astype(F32)
    lb = np.asarray([LEVEL_BOX[i % 4] for i in range(16)], F32)
    dirty_r, dirty_b = rois.copy(), lb.copy()
    at = {k: 1 + i + (i // 3) for i, k in enumerate(DIRTY_KINDS)}          # rows 1, 2, 3, 5, 6, 7, 9, ...: clean rows between
    inf, nan = F32(np.inf), F32(np.nan)
    dirty_r[at["roi_x1_nan"], 0] = nan
    dirty_r[at["roi_y2_nan"], 3] = nan
    dirty_r[at["roi_x2_pinf"], 2] = inf
    dirty_r[at["roi_y1_ninf"], 1] = -inf
    dirty_r[at["roi_at_pinf"]] = (inf, 50.0, inf, 90.0)
    dirty_r[at["roi_at_ninf"]] = (40.0, -inf, 90.0, -inf)
    dirty_b[at["box_nan"], 2] = nan
    dirty_b[at["box_pinf"], 3] = inf
    dirty_b[at["box_ninf"], 0] = -inf
    dirty_b[at["box_inverted"]] = (300.0, 10.0, 100.0, 200.0)
    return dict(rois=dirty_r, level_boxes=dirty_b), dict(rois=rois, level_boxes=lb), at
