"""The NCHW pooling of csrc/sr_xcorr_fused9_body.h where it loads a batch's window rows once (a RUN: fx_run_within in
csrc/sr_xcorr.hip) and where it must not: small cases on both sides of every condition of the run decision, judged by
tests/roi_pool_edge_cases.py's criterion (``E.violates``: levels exact, outputs without a weighted cell exactly 0.0, every
other output within ``(2 e32 + 2^-22) * den`` of the fp64 evaluation on the reference's own fp32 sample tables — derived
per case from the reference, never from a kernel).  Every roi of every case is judged; nothing is excused.

A batch is ROWS pooled rows of a wave: ``2 * G * ROWS`` table entries lo_0, hi_0, lo_1, hi_1, ... (row of the low and of the
high cell of every sample; an entry whose weight is 0 is re-based to the window's first row).  It is a run when every one of
those rows lies within RMAX = ROWS * G + 2 rows from the first entry's (``is_run``: rows that never step back and span at
most RMAX, but without asking for an order — below a step of one row consecutive samples name 3, 4, 3, 4 — since the kernel
reads each entry's own row out of the loaded set).  ``run_model`` restates that decision in Python on
the REFERENCE's tables (``O._axis_samples`` through ``E.case_tables``) for the kernel's batch shapes:

    pooled 30, 33 .. 64 columns, pooling + correlation form   two waves x three batches of 5 rows, RMAX 12, all three or none
    every other form (one column per lane: windows <= 32 columns; the pool-only kernels at 30 and 15; chunked windows
    wider than 64 columns; channels-last maps)                never a run: measured slower there, see the kernel body

and the CPU tests assert which batches of each case are runs, so that a change of RMAX or of the batch shapes that turns
the cases into all-fallback (or all-run) fails here, not silently.  The regimes (every case holds windows of <= 32 columns,
which keep their loads, and of 33 .. 64 columns, which the column to the right speaks of):

  1 step_below_one   17 / 21 / 33 / 41-row windows: consecutive samples share rows                      -> runs
  2 step_above_one   65-row windows for 60 samples: hi(s) == lo(s + 1) mostly, a skipped row now and then -> runs (span <= 12)
  3 tall_bin         96-row windows: a bin more than two rows tall                                      -> never a run
  4 top_cut          cut by the top border: zero-weight entries at the START, re-based to the window's first row, which IS
                     the batch's first                                                                  -> runs
  5 bottom_cut       cut by the bottom border: re-based entries step BACK before the batch's first row  -> fallback in that wave
    bottom_cut_inf   the same rois on a map with +inf in the window's first row, outside the sampled columns, and in the
                     row above the window: equal to the clean map's output bit for bit, never NaN
  6 one_row_col      a one-row and a one-column window
  7 widths           windows of exactly 32, 33, 64 and 65 (chunked) columns

each at C = 8 and C = 10 (a channel tail), pooled 30 through the pooling + correlation form (pooled planes through its debug
output, response against the fp64 correlation of those planes within tests/test_hip_parity.py's bound) and through
``roi_align_levels``, pooled 15 through ``roi_align_levels`` and the one-launch extraction; fp16 / bf16 maps equal the fp32
call on the upcast maps bitwise; NCHW equals channels-last (the untouched stage) bitwise on cases 1, 2, 4, 5.
"""
import functools
import os

import numpy as np
import pytest
import torch

import roi_pool_edge_cases as E
from oracle import emm_oracle as O

DEV = "cuda:0"
G = 2
E.PYRAMIDS.setdefault("T", ((96, 96),))              # one level at scale 1/4, tall enough for a 96-row window
CHANNELS = (8, 10)


def _roi(x, y):
    """Cells (x0, x1), (y0, y1) at scale 1/4 -> a roi in pixels."""
    return (x[0] * 4, y[0] * 4, x[1] * 4, y[1] * 4)


def _geometry():
    H, W = E.PYRAMIDS["S"][0]                        # 72 x 96
    sp = E._span
    g = {}
    g["step_below_one"] = ("S", [_roi(sp(5, 16), sp(3, 17)), _roi(sp(8, 20), sp(6, 21)), _roi(sp(11, 25), sp(20, 33)),
                                 _roi(sp(30, 33), sp(9, 41)), _roi(sp(40, 40), sp(30, 33)), _roi(sp(3, 64), sp(25, 41))])
    g["step_above_one"] = ("S", [_roi(sp(6, 20), sp(4, 65)), _roi(sp(21, 40), sp(3, 65)), _roi(sp(30, 33), sp(7, 65)),
                                 _roi(sp(2, 32), sp(5, 65))])
    g["tall_bin"] = ("T", [_roi(sp(10, 20), sp(0, 96)), _roi(sp(33, 40), sp(0, 96)), _roi(sp(1, 33), sp(0, 96))])
    g["top_cut"] = ("S", [_roi(sp(6, 20), (-10.3, 24.7)), _roi(sp(41, 40), (-12.6, 27.2)), _roi(sp(30, 33), (-30.2, 33.4)),
                          _roi(sp(3, 28), (-6.13, 12.31))])
    g["bottom_cut"] = ("S", [_roi(sp(6, 20), (H - 24.7, H + 10.3)), _roi(sp(41, 40), (H - 27.2, H + 12.6)),
                             _roi(sp(30, 33), (H - 33.4, H + 30.2)), _roi(sp(60, 28), (H - 12.31, H + 6.13))])
    g["one_row_col"] = ("S", [_roi(sp(7, 20), (-2.0, -0.02)), _roi(sp(35, 40), (-2.0, -0.02)), _roi((-2.0, -0.02), sp(9, 33)),
                              _roi((W - 0.95, W + 1.0), sp(4, 41)), _roi((-2.0, -0.02), (H - 0.95, H + 1.0))])
    g["widths"] = ("S", [_roi(sp(3, 32), sp(5, 33)), _roi(sp(4, 33), sp(11, 33)), _roi(sp(7, 64), sp(20, 33)),
                         _roi(sp(10, 65), sp(30, 33)), _roi(sp(31, 65), sp(2, 65))])
    return g


NAMES = ("step_below_one", "step_above_one", "tall_bin", "top_cut", "bottom_cut", "one_row_col", "widths")
LAYOUT_CASES = ("step_below_one", "step_above_one", "top_cut", "bottom_cut")


@functools.lru_cache(maxsize=None)
def case(name, C):
    pyr, rois = _geometry()[name]
    return E._case("runs", pyr, C, rois, 30)


@functools.lru_cache(maxsize=None)
def reference(name, C, P):
    return E.reference_eval(case(name, C), P, P, G)


# ---- the run decision, restated on the reference's tables -----------------------------------------------------------------
def y_entries(c, r, P):
    """Per sample (row of lo, row of hi, weight lo, weight hi) as the kernel's y table holds them — zero-weight entries re-based
    to the first touched row — and the touched x window's width; None when nothing is touched."""
    ty, tx, lvl, p, H, W, _ = E.case_tables(c, r, g=G, ph=P)
    assert p == 0 and lvl == 0
    valid, low, high, l, h = ty
    wl, wh = (h * valid).tolist(), (l * valid).tolist()
    ywin, xwin = E.touched(ty), E.touched(tx)
    if ywin is None or xwin is None:
        return None, 0
    mn = ywin[0]
    ent = [(int(low[s]) if wl[s] != 0 else mn, int(high[s]) if wh[s] != 0 else mn, wl[s], wh[s]) for s in range(P * G)]
    return ent, xwin[1] - xwin[0] + 1


def is_run(ent, rmax):
    """Every row the batch names lies within rmax rows from its FIRST entry's (no weight NaN).  Rows that never step back and
    span at most rmax are the common case, but an order is not what the kernel needs, and it is not there below a step of one
    row (3, 4, 3, 4): the chain reads the row an entry names out of the loaded set, so all it needs is that the row is in it."""
    seq = [v for e in ent for v in e[:2]]
    finite = all(w == w for e in ent for w in e[2:])
    return bool(ent) and rmax > 0 and finite and all(0 <= v - seq[0] <= rmax - 1 for v in seq)


def wave_batches(P, ww, form):
    """[(wave, [(first sample, samples judged, RMAX), ...], decided per wave)] of the kernel's forms (module docstring)."""
    RH = (P + 1) // 2
    if ww > 64:
        return []
    per_wave = ww > 32 and P == 30 and form == "fused"
    rows = RH if ww <= 32 else (5 if per_wave else (RH + 1) // 2)
    rmax = rows * G + 2 if per_wave else 0
    out = []
    for wave in (0, 1):
        row0, bs = wave * RH, []
        for r0 in range(row0, row0 + RH, rows):
            real = min(rows, min(row0 + RH, P) - r0)
            if real > 0:
                bs.append((r0 * G, real * G, rmax))
        out.append((wave, bs, per_wave))
    return out


def run_model(c, r, P, form):
    """{(wave, first sample): is a run} of one roi; {} where the kernel pools nothing or walks chunks."""
    ent, ww = y_entries(c, r, P)
    if ent is None:
        return {}
    out = {}
    for wave, bs, per_wave in wave_batches(P, ww, form):
        runs = [is_run(ent[s0:s0 + n], rmax) for s0, n, rmax in bs]
        if per_wave:
            runs = [all(runs)] * len(runs)
        out.update({(wave, s0): v for (s0, _, _), v in zip(bs, runs)})
    return out


def _summary(name, P, form):
    c = case(name, 8)
    return [sorted(run_model(c, r, P, form).values()) for r in range(len(c["rois"]))]


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_cases_are_small():
    for name in NAMES:
        for C in CHANNELS:
            c = case(name, C)
            assert len(c["rois"]) <= 8 and len(E.PYRAMIDS[c["pyr"]]) == 1 and c["pad_pixels"] == 0
            h, w = E.PYRAMIDS[c["pyr"]][0]
            assert h <= 96 and w <= 96


def test_the_model_uses_the_kernel_s_constants():
    """RMAX and the batch shapes above are the source's: if these lines change, the model changes with them."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "siam-mot_amd", "csrc")
    body = open(os.path.join(root, "sr_xcorr_fused9_body.h")).read()
    assert "constexpr int NE = ROWS * G, RMAX = NE + 2;" in body and body.count("fx_run_within<") == 1
    assert "if (fx_run_within<NE, RH / ROWS>(RMAX, ye, lane, RH * G, row_bytes)) {" in body
    assert "if constexpr (MM == 1) pool(std::true_type{}, std::false_type{}, std::true_type{}, std::integral_constant<int, RH / 3>{});" in body
    assert "typedef float fx_rows_t __attribute__((ext_vector_type(32)));" in open(os.path.join(root, "sr_xcorr.hip")).read()


@pytest.mark.parametrize("name", NAMES)
def test_case_is_in_its_regime(name):
    """Read off the reference's tables alone.  If one fails the generator is to change, not this test."""
    c = case(name, 8)
    H, W = E.PYRAMIDS[c["pyr"]][0]
    R = len(c["rois"])
    ents = [y_entries(c, r, 30) for r in range(R)]
    wins = [E.touched(E.case_tables(c, r, g=G, ph=30)[0]) for r in range(R)]
    widths = [ww for _, ww in ents]
    mono = lambda e: all(a <= b for a, b in zip([v for x in e for v in x[:2]], [v for x in e for v in x[:2]][1:]))
    rising = lambda e: all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(e, e[1:])) and all(x[0] <= x[1] <= x[0] + 1 for x in e)
    if name == "step_below_one":
        assert [w[1] - w[0] + 1 for w in wins] == [17, 21, 33, 41, 33, 41] and widths == [16, 20, 25, 33, 40, 64]
        for e, _ in ents:
            assert rising(e) and not mono(e) and all(b[0] in (a[0], a[1]) for a, b in zip(e, e[1:]))   # shares a row with its predecessor
            assert sum(a[:2] == b[:2] for a, b in zip(e, e[1:])) >= 15                          # ... and often both
    if name == "step_above_one":
        assert [w[1] - w[0] + 1 for w in wins] == [65] * 4 and widths == [20, 40, 33, 32]
        for e, _ in ents:
            steps = [b[0] - a[1] for a, b in zip(e, e[1:])]
            assert mono(e) and set(steps) == {0, 1} and 1 <= steps.count(1) <= 8                # a skipped row now and then
            assert all(x[1] == x[0] + 1 for x in e)
    if name == "tall_bin":
        assert [w[1] - w[0] + 1 for w in wins] == [96] * 3 and widths == [20, 40, 33]
        y1, bh, _, _ = E.roi_axes(torch.from_numpy(c["rois"][0]), 0.25, 30, 30)
        assert float(bh) > 2.0
    if name == "top_cut":
        for (e, _), w in zip(ents, wins):
            zero = [x[2] == 0 and x[3] == 0 for x in e]
            k = zero.index(False)
            assert w[0] == 0 and k >= 4 and all(zero[:k]) and not any(zero[k:])                 # zero weights at the start only
            assert all(x[:2] == (0, 0) for x in e[:k]) and rising(e)
        assert widths == [20, 40, 33, 28]
    if name == "bottom_cut":
        for (e, _), w in zip(ents, wins):
            zero = [x[2] == 0 and x[3] == 0 for x in e]
            k = zero.index(True)
            assert w[1] == H - 1 and 60 - k >= 4 and all(zero[k:]) and not any(zero[:k])        # ... at the end only
            part = [x[2] == 0 or x[3] == 0 for x in e]                                           # (in [H - 1, H]: only hi is re-based)
            k2 = part.index(True)
            assert all(x[:2] == (w[0], w[0]) for x in e[k:]) and all(part[k2:]) and rising(e[:k2])
            assert min(e[k2][:2]) == w[0] < e[k2 - 1][0]                                         # ... and step back to the first row
        assert widths == [20, 40, 33, 28]
    if name == "one_row_col":
        assert [w[1] - w[0] + 1 for w in wins] == [1, 1, 33, 41, 1] and widths == [20, 40, 1, 1, 1]
        assert wins[4] == (H - 1, H - 1)
    if name == "widths":
        assert widths == [32, 33, 64, 65, 65]


# which batches are runs: per roi one letter per batch (R = run, F = fallback; sorted; two waves x 1, 2 or 3 batches; "" = chunked)
EXPECTED = {
    ("step_below_one", 30, "fused"): ["FF", "FF", "FF", "RRRRRR", "RRRRRR", "RRRRRR"],
    ("step_above_one", 30, "fused"): ["FF", "RRRRRR", "RRRRRR", "FF"],
    ("tall_bin", 30, "fused"): ["FF", "FFFFFF", "FFFFFF"],
    ("top_cut", 30, "fused"): ["FF", "RRRRRR", "RRRRRR", "FF"],
    ("bottom_cut", 30, "fused"): ["FF", "FFFRRR", "FFFRRR", "FF"],
    ("one_row_col", 30, "fused"): ["FF", "RRRRRR", "FF", "FF", "FF"],
    ("widths", 30, "fused"): ["FF", "RRRRRR", "RRRRRR", "", ""],
    ("step_below_one", 30, "pool"): ["FF", "FF", "FF", "FFFF", "FFFF", "FFFF"],
    ("step_below_one", 15, "pool"): ["FF", "FF", "FF", "FFFF", "FFFF", "FFFF"],
}


@pytest.mark.parametrize("key", sorted(EXPECTED))
def test_which_batches_are_runs(key):
    name, P, form = key
    assert ["".join("RF"[not v] for v in roi) for roi in _summary(name, P, form)] == EXPECTED[key]


def test_both_paths_are_exercised():
    for P, form in ((30, "fused"),):
        seen = [v for name in NAMES for roi in _summary(name, P, form) for v in roi]
        assert seen.count(True) >= 10 and seen.count(False) >= 10, (P, form)
        widths = {2 if ww > 32 else 1 for name in NAMES for r in range(len(case(name, 8)["rois"]))
                  for _, ww in [y_entries(case(name, 8), r, P)] if 0 < ww <= 64}
        assert widths == {1, 2}


def test_the_run_model_on_hand_made_tables():
    e = lambda lo, hi, wl=0.5, wh=0.5: (lo, hi, wl, wh)
    assert is_run([e(3, 4), e(4, 5), e(5, 6)], 4) and not is_run([e(3, 4), e(4, 5), e(5, 6)], 3)       # span
    assert is_run([e(3, 4), e(3, 4), e(4, 5)], 4) and is_run([e(3, 4), e(5, 6)], 4)                    # shared rows, a skipped row
    assert not is_run([e(4, 5), e(5, 3, 0.5, 0.0)], 8) and not is_run([e(5, 6), e(3, 3, 0.0, 0.0)], 8)   # re-based to a row before the first
    assert is_run([e(3, 3, 0.0, 0.0), e(3, 3, 0.0, 0.5), e(3, 4)], 8)                                 # ... to the first row itself
    assert is_run([e(3, 4), e(4, 5), e(5, 3, 0.5, 0.0)], 8)                                           # (the row it names is loaded)
    assert not is_run([e(3, 4, float("nan"), 0.5)], 8) and not is_run([], 8) and not is_run([e(3, 4)], 0)
    assert [len(b) for _, b, _ in wave_batches(30, 40, "fused")] == [3, 3] and wave_batches(30, 65, "fused") == []
    assert all(rmax == 12 for _, b, _ in wave_batches(30, 40, "fused") for _, _, rmax in b)
    assert wave_batches(15, 20, "pool")[1][1] == [(16, 14, 0)]                                        # (the masked row is not counted)
    assert all(rmax == 0 for P, ww, f in ((30, 40, "pool"), (30, 20, "fused"), (15, 40, "pool")) for _, b, _ in wave_batches(P, ww, f) for _, _, rmax in b)


# ---- GPU --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _maps(c, dtype=None, channels_last=False, planted=None):
    m = E.maps(c["pyr"], c["C"])[0] if planted is None else planted
    m = m.to(DEV)
    if dtype is not None:
        m = m.to(dtype)
    if channels_last:
        m = m.contiguous(memory_format=torch.channels_last)
    return [m]


def _judge(form, name, C, ref, out):
    out = out.detach().cpu()
    err, same = E.kernel_error(ref, out)
    print("row-runs %-18s %-15s C %2d e32 %.3e kernel %.3e identical %.4f" % (form, name, C, ref["e32"], err, same))
    why = E.violates(ref, ref["levels"].tolist(), out)
    assert why is None, "%s, %s, C = %d: %s" % (form, name, C, why)


def _fused(ops, c, feats, seed=99):
    rois = _t(c["rois"]).to(DEV)
    z = torch.randn((len(rois), c["C"], 15, 15), generator=torch.Generator().manual_seed(seed)).to(DEV)
    resp, pooled = ops.sr_xcorr_fused(feats, rois, rois, z, 30, 15, E.scales_of(c["pyr"]), G, 0, return_pooled=True)
    torch.cuda.synchronize()
    return resp, pooled, z


def _levels(ops, c, feats, P):
    out, lv = ops.roi_align_levels(feats, _t(c["rois"]).to(DEV), None, P, E.scales_of(c["pyr"]), G, [0], return_levels=True)
    torch.cuda.synchronize()
    return out, lv


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("name", NAMES)
def test_pooling_and_correlation_on_row_runs(ops, name, C):
    """Pooled 30 through the pooling + correlation form: its pooled planes against the bound, its response against the fp64
    correlation of those planes."""
    from test_hip_parity import _assert_response_is_the_correlation
    c = case(name, C)
    resp, pooled, z = _fused(ops, c, _maps(c))
    _judge("fused 30/15", name, C, reference(name, C, 30), pooled)
    _assert_response_is_the_correlation(resp, pooled, z, "%s C = %d" % (name, C))


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("P", (30, 15))
@pytest.mark.parametrize("name", NAMES)
def test_pool_only_kernels_on_row_runs(ops, name, P, C):
    """``roi_align_levels`` at both pooled sizes, and at 15 the one-launch extraction (the case's rois as boxes)."""
    c = case(name, C)
    ref = reference(name, C, P)
    out, lv = _levels(ops, c, _maps(c), P)
    assert lv.cpu().tolist() == ref["levels"].tolist()
    _judge("levels %d" % P, name, C, ref, out)
    if P == 15:
        z, sr, _ = ops.emm_extract_cache(_maps(c), _t(c["rois"]).to(DEV), 15, E.scales_of(c["pyr"]), G, 512.0, 1.0, 0.0, hint=True)
        torch.cuda.synchronize()
        _judge("extract 15", name, C, ref, z)
        assert torch.equal(z.view(torch.int32), out.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
@pytest.mark.parametrize("name", ("step_below_one", "step_above_one", "bottom_cut"))
def test_half_maps_equal_the_fp32_call_on_the_upcast_maps(ops, name, dtype):
    c = case(name, 10)
    half = _maps(c, dtype=dtype)
    up = [m.float() for m in half]
    for what, call in (("fused", lambda f: torch.cat([t.reshape(len(c["rois"]), -1) for t in _fused(ops, c, f)[:2]], 1)),
                       ("levels 30", lambda f: _levels(ops, c, f, 30)[0]), ("levels 15", lambda f: _levels(ops, c, f, 15)[0])):
        a, b = call(half), call(up)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s, %s: %s maps differ from the fp32 call on the upcast maps" % (name, what, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_nchw_equals_channels_last(ops, name):
    """The channels-last stage (csrc/sr_pool_nhwc_stage.h) loads per sample as before: a differential check inside one library."""
    c = case(name, 8)
    cl = _maps(c, channels_last=True)
    assert not cl[0].is_contiguous()
    for what, call in (("fused", lambda f: torch.cat([t.reshape(len(c["rois"]), -1) for t in _fused(ops, c, f)[:2]], 1)),
                       ("levels 30", lambda f: _levels(ops, c, f, 30)[0]), ("levels 15", lambda f: _levels(ops, c, f, 15)[0])):
        a, b = call(_maps(c)), call(cl)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s, %s: NCHW differs from channels-last" % (name, what)


def _planted(c):
    """The case's map with +inf where no sample of any roi has a weighted cell AND the kernel loads nothing: in every roi's
    first window row, the columns outside every roi's touched columns; and the row above the topmost window."""
    m = E.maps(c["pyr"], c["C"])[0].clone()
    H, W = m.shape[-2:]
    cols, first_rows = torch.zeros(W, dtype=torch.bool), []
    for r in range(len(c["rois"])):
        ty, tx, *_ = E.case_tables(c, r, g=G, ph=30)
        xw, yw = E.touched(tx), E.touched(ty)
        cols[xw[0]:xw[1] + 1] = True
        first_rows.append(yw[0])
    free = torch.nonzero(~cols).flatten()
    assert len(free) >= 4
    for y in first_rows:
        m[0, :, y, free] = float("inf")
    m[0, :, min(first_rows) - 1, :] = float("inf")
    return m, first_rows, free


def test_the_planted_cells_carry_no_weight():
    c = case("bottom_cut", 10)
    m, first_rows, free = _planted(c)
    ref = reference("bottom_cut", 10, 30)
    assert bool(torch.isinf(m).any()) and min(first_rows) >= 1
    for P in (30, 15):
        for r in range(len(c["rois"])):
            ty, tx, *_ = E.case_tables(c, r, g=G, ph=P)
            assert E.touched(ty)[0] >= min(first_rows) and not set(range(E.touched(tx)[0], E.touched(tx)[1] + 1)) & set(free.tolist())
    assert bool(torch.isfinite(ref["f32"]).all())


@pytest.mark.gpu
def test_bottom_cut_with_inf_in_the_first_window_row(ops):
    """Entries re-based to the window's first row multiply the cell they were re-based to by 0: the kernel must read the cell
    today's loads read (finite) there.  The planted map's outputs equal the clean map's bit for bit and meet the bound."""
    c = case("bottom_cut", 10)
    m, _, _ = _planted(c)
    for what, call, P in (("fused", lambda f: _fused(ops, c, f)[1], 30), ("levels 30", lambda f: _levels(ops, c, f, 30)[0], 30),
                          ("levels 15", lambda f: _levels(ops, c, f, 15)[0], 15)):
        clean, dirty = call(_maps(c)), call(_maps(c, planted=m))
        assert not bool(torch.isnan(dirty).any()), what
        assert torch.equal(clean.view(torch.int32), dirty.view(torch.int32)), what
        _judge(what + " +inf", "bottom_cut", 10, reference("bottom_cut", 10, P), dirty)
    resp = _fused(ops, c, _maps(c, planted=m))[0]
    assert bool(torch.isfinite(resp).all())
