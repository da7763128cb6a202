"""The ROIAlign family against a reference that is not itself, at the edges of its geometry: the generic level-routed
kernel (csrc/roi_align_body.h: staged and unstaged, 1 .. 4 samples per bin, [R, 4] and [R, 5] rois), the separable kernel
of the pooled sizes 7 / 15 / 30 and its pooling + correlation form (csrc/sr_xcorr_fused9_body.h: plane-pair,
two-columns-per-lane and chunked windows), the 35 / 7 gather kernel (csrc/sr_xcorr_gather_body.h) and the one-launch
template extraction, on fp32 / fp16 / bf16 maps, NCHW and channels-last, one image and a batch.

Inputs, references, the bound and the mutants come from tests/roi_pool_edge_cases.py (computed once per case and pooled
shape, shared).  The chain of custody, asserted by the CPU tests: ``ref32`` (``O.sr_pool`` on ``O.pad_features``) equals
the compiled C restatement ``O.roi_align_c`` bit for bit; ``ref64`` (the reference's own fp32 sample tables, fp64
products and sums) is within ``e32 * den`` of it with ``e32 <= 2^-21`` in every case; every case is in the regime it is
named for, read off the reference's tables alone; and the reference restated with one rule changed (eleven mutants)
breaks the GPU tests' own criterion in named cases — the coordinate formed as ``start + (p + (i + .5) / G) * bin``, one
rounding sequence away, passes the earlier 1e-5 on ordinary geometry (ordinary_A) and fails the bound there.

The GPU tests' criterion (``E.violates``): levels exactly ``O.level_mapper``'s; outputs with ``den == 0`` exactly 0.0;
every other output within ``(2 e32 + 2^-22) * den`` of ``ref64`` — derived per case from the reference, never from a
kernel.  Form identities (fp16 / bf16 call = fp32 call on the upcast maps, channels-last = NCHW, batched = per image)
are bitwise.

Non-finite and inverted rows have no reference contract (``O.level_mapper`` yields a garbage level for w + 1 < 0 <= h + 1,
``_axis_samples`` indexes with the integer conversion of NaN), but the tracking loop feeds them.  Established by reading,
before the test ran, that no kernel body forms a cell index outside the map from such a row:
  * ``map_level`` (roi_common.h): ``fminf(fmaxf(lvl, k_min), k_max)`` returns the non-NaN operand, so a NaN / inf / negative
    area gives a level in [0, num_levels - 1] (NaN -> 0);
  * ``axis_sample``: a NaN coordinate fails both comparisons of the validity test and ``c <= 0``, the conversion
    ``(int)c`` is the saturating v_cvt_i32_f32 (NaN -> 0, +inf -> INT_MAX), and ``l >= size_p - 1`` clamps what is left: l, h
    are in [0, size_p - 1] for every c; the real-cell mask (``lr >= 0 && lr < size_real``) turns everything else into cell 0
    with weight 0.0, so a table entry is (real cell, weight) or (0, 0.0) whatever the coordinate — only WEIGHTS can be NaN;
  * a table of one axis is all finite, or all NaN / +-inf (start or bin non-finite: ``p * inf`` is NaN for p = 0, so no finite
    entry survives); its NaN entries all name cells (0, 1) of the padded axis and its inf entries are invalid, so the
    touched entries stay monotone and the ballot bound (first / last touched entry) and the atomicMin / atomicMax bound of
    the generic and gather kernels hold what the tables name (``w != 0.0f`` is true for a NaN weight: a NaN entry is counted);
  * the re-basing writes ``lo - mn`` / ``rl * W`` of touched entries and ``mn`` / 0 of the others: inside the window;
  * the column clamps ``min(col, ww - 1)``, ``min(2 * col, ww - 2)`` (only for ww >= 33), ``min(cbase + col, ww - 1)`` and the
    channels-last stage's ``min(cb + col, ww - 1)`` bound every lane's load by xmax whatever the tables hold;
  * ``fx_assign`` / ``fx_write_hint`` class a NaN width as 2 (both ``<=`` fail): the assignment stays a bijection;
  * the [R, 5] form converts the image index with the same saturating conversion and pools an index outside [0, B) to zeros.
So every form is in test_non_finite_rows_leave_the_clean_rows_alone.

Measured on an MI355X (largest value per family over its launches; errors in units of den; "identical" = smallest share
of a launch's outputs bit-identical to ref32).  "separable" = the 7 / 15 / 30 kernel through ``roi_align_levels``, the
pooled planes of the pooling + correlation form and the extraction's templates; "generic" = the generic kernel at every
pooled shape (7 / 15 / 30 through its switch, 35, 40, 5 x 9), 1 .. 4 samples per bin, [R, 4] and [R, 5] rois:

    family     kernel      largest e32  kernel error  identical   launches (cases)
    border     separable   1.67e-07     1.98e-07      >= 0.511     8 (4)
    border     generic     2.26e-07     2.26e-07      1.000       20 (4)
    integral   separable   1.38e-07     1.04e-07      >= 0.666     3 (3)
    integral   generic     2.08e-07     2.08e-07      1.000        9 (3)
    window     separable   1.84e-07     1.88e-07      >= 0.350    19 (5)
    window     generic     3.20e-07     3.20e-07      1.000       16 (5)
    tiny       separable   1.71e-07     1.95e-07      >= 0.551     3 (1)
    tiny       generic     1.71e-07     1.71e-07      1.000        1 (1)
    outside    separable   1.73e-07     1.58e-07      >= 0.881     2 (2)
    outside    generic     1.73e-07     1.73e-07      1.000        2 (2)
    huge       separable   5.73e-08     5.73e-08      >= 0.997     1 (1)
    huge       generic     5.73e-08     5.73e-08      1.000        1 (1)
    pad        separable   1.91e-07     2.33e-07      >= 0.635     8 (4)
    pad        generic     1.97e-07     1.97e-07      1.000        8 (4)
    levels     separable   1.84e-07     1.89e-07      >= 0.452     6 (2)
    levels     generic     1.64e-07     1.64e-07      1.000        2 (2)
    ordinary   separable   1.55e-07     2.04e-07      >= 0.447     1 (1)
    ordinary   generic     1.55e-07     1.55e-07      1.000        1 (1)

so the bounds came out at 3.5e-07 .. 8.8e-07 of den.  The generic kernel (and with it the 35 / 7 gather kernel, which equals
it bit for bit) returned ref32's bits in every one of its 60 judged launches: its coordinate chain, weights and summation order
ARE the reference's rounding sequence.  The separable kernel's factorisation ``hx * (hy * v)`` leaves up to two thirds of a
launch's outputs a rounding away; its largest error (2.33e-07, pad_512_A) is 1.3 times the fp32 reference's own.  Every
level equalled ``O.level_mapper``'s, every form identity held bit for bit and the non-finite test passed at its first run:
the suite exposed no kernel bug.
"""
import numpy as np
import pytest
import torch

import roi_pool_edge_cases as E
from oracle import emm_oracle as O

DEV = "cuda:0"
SEPARABLE = (7, 15, 30)
FUSED_CASES = tuple(n for n in E.CASE_NAMES if n.startswith(("pad_", "window_", "border_")))
EXTRACT_CASES = tuple(n for n in E.CASE_NAMES if n.startswith(("levels_", "tiny_", "window_")))
# a by-roi record of the order hint (csrc/sr_xcorr.hip: HINT_BYROI): {search region, level, rois ranked, status, 0}
HINT_BYROI_FROM_END = 8


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- CPU: the chain of custody ------------------------------------------------------------------------------------
def test_case_list_is_complete_and_small():
    c = E.cases()
    assert tuple(c) == E.CASE_NAMES and len(c) <= 40
    assert all(len(v["rois"]) <= 16 for v in c.values())
    assert {v["C"] for v in c.values()} == {5, 8, 12, 16} and {v["pyr"] for v in c.values()} == {"A", "B", "S"}
    assert {v["out_size"] for v in c.values()} >= {7, 15, 30} and {v["pad_pixels"] for v in c.values()} == {0, 32, 100, 512}
    assert {v["family"] for v in c.values()} == {"border", "integral", "window", "tiny", "outside", "huge", "pad", "levels", "ordinary"}
    assert {v["out_size"] for v in c.values() if v["family"] == "integral"} == {7, 15, 30}
    assert E.PYRAMIDS["A"][0][1] % 2 == 0 and E.PYRAMIDS["B"][0][1] % 2 == 1
    for pyr, C in {(v["pyr"], v["C"]) for v in c.values()}:
        for m in E.maps(pyr, C):
            assert m.numel() * 4 < 512 * 1024
        means = E.maps(pyr, C)[0].mean((0, 2, 3))
        assert bool((means[1:] - means[:-1] > 0.5).all())                         # a wrong plane shows


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_ref32_equals_the_c_restatement_bitwise(name):
    if O.roi_align_c_library() is None:
        pytest.fail("oracle/_build/libroi_align_cpu.so is not built (python oracle/build_c.py)")
    c = E.cases()[name]
    feats = O.pad_features(E.maps(c["pyr"], c["C"]), c["pad_pixels"])
    rois = _t(c["rois"])
    lb = rois if c["level_boxes"] is None else _t(c["level_boxes"])
    for g in c["gs"]:
        ref = E.reference(name, g=g)
        assert bool(torch.isfinite(ref["f32"]).all())
        got = O.sr_pool(feats, lb, rois, c["out_size"], E.scales_of(c["pyr"]), g, roi_align=O.roi_align_c)
        assert torch.equal(got.view(torch.int32), ref["f32"].view(torch.int32)), (name, g)


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_ref64_is_the_same_operation_in_higher_precision(name):
    c = E.cases()[name]
    for g in c["gs"]:
        r = E.reference(name, g=g)
        assert r["e32"] <= E.E32_MAX, (name, g, r["e32"])
        # (the fp32 reference is at most e32 * den from ref64 by definition; rounding ref64 to fp32 moves it by at most
        # half a spacing of the result)
        f64r = r["f64"].float()
        slack = r["e32"] * r["den"] + 0.5 * torch.from_numpy(np.spacing(np.abs(f64r.numpy()))).double()
        assert bool(((f64r.double() - r["f32"].double()).abs() <= slack).all())
        zero = r["den"] == 0
        assert not bool(r["f32"][zero].any()) and not bool(r["f64"][zero].any())
        assert E.violates(r, r["levels"], r["f32"]) is None                       # the bound can be met
        assert r["levels"].dtype == torch.int64 and 0 <= int(r["levels"].min()) and int(r["levels"].max()) < len(E.PYRAMIDS[c["pyr"]])


def _axis(c, r, axis, **kw):
    ty, tx, lvl, p, H, W, (cy, cx) = E.case_tables(c, r, **kw)
    return (ty, cy, H + 2 * p, p, H) if axis == "y" else (tx, cx, W + 2 * p, p, W)


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_generated_case_is_in_its_regime(name):
    """Conditions on the INPUTS, from the reference's tables alone.  If one fails the generator is to change, not this test."""
    c = E.cases()[name]
    fam, R, P = c["family"], len(c["rois"]), c["out_size"]
    ref = E.reference(name)
    below_m1, above = np.nextafter(np.float32(-1), np.float32(-2)), lambda s: np.nextafter(np.float32(s), np.float32(np.inf))
    for r in range(R):                                   # the tables' validity is the strict / non-strict rule on the coordinates
        for axis in "yx":
            (valid, low, high, l, h), co, size_p, p, size = _axis(c, r, axis)
            assert torch.equal(valid, ~((co < -1.0) | (co > size_p)))
            assert bool(((low >= 0) & (high <= size_p - 1) & (l >= 0) & (l < 1) & (h > 0)).all())
    if fam == "border":
        assert c["pyr"] == "S" and c["pad_pixels"] in (0, 32)
        seen = set()
        for r, kinds in enumerate(c["rows"]["spec"]):
            for axis, kind in zip("xy", kinds):
                (valid, low, high, l, h), co, size_p, p, size = _axis(c, r, axis)
                seen.add((axis, kind))
                if kind == "low":
                    assert float(co[0]) == -1.0 and bool(valid[0]) and int(low[0]) == 0 and float(l[0]) == 0.0
                    inside = (co > -1) & (co < 0)
                    assert bool(inside.any()) and bool(valid[inside].all()) and not bool(low[inside].any()) and not bool(l[inside].any())
                    assert bool((co == 0).any())
                elif kind == "low_out":
                    assert float(co[0]) == float(below_m1) and not bool(valid[0]) and bool(valid[1:].all())
                elif kind == "high":
                    assert float(co[-1]) == size_p and bool(valid[-1]) and int(low[-1]) == int(high[-1]) == size_p - 1
                    assert float(l[-1]) == 0.0 and float(h[-1]) == 1.0
                    assert bool((co == size_p - 1).any())
                    inside = (co > size_p - 1) & (co < size_p)
                    assert bool(inside.any()) and bool(valid[inside].all()) and bool((low[inside] == size_p - 1).all())
                    assert bool((high[inside] == size_p - 1).all()) and not bool(l[inside].any())
                elif kind == "high_out":
                    assert float(co[-1]) == float(above(size_p)) and not bool(valid[-1]) and bool(valid[:-1].all())
                else:
                    assert bool(valid.all()) and bool((l > 0).any())
        assert seen >= {(a, k) for a in "xy" for k in ("low", "low_out", "high", "high_out")}
    if fam == "integral":
        cols, rows_ = set(), set()
        for r in range(R):
            ty, tx, lvl, p, H, W, _ = E.case_tables(c, r)
            for tab, size, acc in ((ty, H, rows_), (tx, W, cols)):
                valid, low, high, l, h = tab
                assert bool(valid.all()) and not bool(l.any()) and bool((h == 1).all())       # first and last entry included
                win = E.touched(tab)
                assert win[1] - win[0] + 1 == 2 * P and win == (int(low[0]), int(low[-1]))
                acc.update(win)
            assert lvl == 0
        H, W = E.PYRAMIDS[c["pyr"]][0]
        assert 0 in cols and 0 in rows_ and W - 1 in cols and H - 1 in rows_
    if fam == "window" and c["pyr"] != "S":
        H0, W0 = E.PYRAMIDS[c["pyr"]][0]
        widths, corner = set(), False
        for r, want in enumerate(c["rows"]["xwin"]):
            ty, tx, lvl, p, H, W, _ = E.case_tables(c, r)
            xw, yw = E.touched_real(tx, p, W), E.touched_real(ty, p, H)
            assert xw == tuple(want), (r, xw, want)
            if lvl == 0:
                widths.add(xw[1] - xw[0] + 1)
                if 2 <= xw[1] - xw[0] + 1 <= 65:
                    assert xw[0] % 2 == c["rows"]["parity"]
                corner = corner or (xw[1] == W - 1 and yw[1] == H - 1)
            else:
                assert xw == (0, W - 1) and yw == (0, H - 1)
        assert widths >= {1, 2, 31, 32, 33, 63, 64, 65, W0} and corner
        assert ref["levels"].tolist() == [0] * 11 + [1, 2, 3]
    if fam == "window" and c["pyr"] == "S":
        cells = set()
        for g in c["gs"]:
            for r, (y, x, nh, nw) in enumerate(c["rows"]["win"]):
                ty, tx, lvl, p, H, W, _ = E.case_tables(c, r, g=g)
                assert E.touched(ty) == (y, y + nh - 1) and E.touched(tx) == (x, x + nw - 1), (g, r)
                cells.add(nh * nw)
        assert cells == {4096, 4160, 4095} and c["gs"] == (1, 2, 3, 4) and P not in SEPARABLE
        assert any(y + nh == 72 and x + nw == 96 for y, x, nh, nw in c["rows"]["win"])
    if fam == "tiny":
        b = c["rois"]
        assert (b[0, 2] == b[0, 0]) and (b[0, 3] == b[0, 1]) and b[3, 2] < b[3, 0] and b[4, 3] < b[4, 1] and b[5, 2] < b[5, 0] and b[5, 3] < b[5, 1]
        assert np.floor(b[1, 0] * 0.25) == np.floor(b[1, 2] * 0.25) and 0 < (b[1, 2] - b[1, 0]) * 0.25 < 1
        for r, axes in ((0, "xy"), (1, "xy"), (3, "x"), (4, "y"), (5, "xy"), (6, "xy")):
            lvl = int(ref["levels"][r])
            y1, bh, x1, bw = E.roi_axes(_t(c["rois"][r]), E.SCALES4[lvl], P, P)
            for a in axes:
                assert float(bh if a == "y" else bw) == float(np.float32(1.0) / np.float32(P))      # the side clamped to 1
        assert not np.array_equal(c["rois"], c["level_boxes"]) and len(set(ref["levels"].tolist())) == 4
    if fam == "outside":
        for r, axis in enumerate("xxyy"):
            assert not bool(_axis(c, r, axis)[0][0].any()) and not bool(ref["den"][r].any()) and not bool(ref["f32"][r].any())
        for r, axis in zip(range(4, 8), "xxyy"):
            valid = _axis(c, r, axis)[0][0]
            assert bool(valid.any()) and not bool(valid.all())
            assert bool((ref["den"][r] == 0).any()) and bool((ref["den"][r] > 0).any())
    if fam == "huge":
        w = c["rois"][:, 2:] - c["rois"][:, :2]
        assert (w.max(1) >= 3000).all() and (w.max(1) >= 1e6).sum() >= 4
        for r in range(R):
            frac = [float(_axis(c, r, a)[0][0].double().mean()) for a in "yx"]
            assert min(frac) < 0.5 and bool((ref["den"][r] == 0).any())
    if fam == "pad":
        pads = E.pad_cells(c)
        assert pads == ([128, 64, 32, 16] if c["pad_pixels"] == 512 else [25, 12, 6, 3])
        if c["pad_pixels"] == 100:
            assert [100 * s == int(100 * s) for s in E.SCALES4] == [True, False, False, False]      # truncates differently per level
        for r in range(R):
            side = r % 4
            (valid, low, high, l, h), co, size_p, p, size = _axis(c, r, "xxyy"[side])
            assert int(ref["levels"][r]) == r // 4 and p == pads[r // 4]
            frac = valid & (l > 0)
            if side in (0, 2):                           # low in the pad, high real
                assert bool((frac & (low == p - 1) & (high == p)).any())
            else:                                        # low real, high in the pad
                assert bool((frac & (low == p + size - 1) & (high == p + size)).any())
            assert bool((ref["den"][r] == 0).any()) and bool((ref["den"][r] > 0).any())
    if fam == "levels":
        lb = _t(c["level_boxes"])
        s = torch.sqrt((lb[:, 2] - lb[:, 0] + 1) * (lb[:, 3] - lb[:, 1] + 1))
        assert not np.array_equal(c["rois"], c["level_boxes"]) and all(E.level_is_robust(b) for b in c["level_boxes"])
        if name == "levels_exact":
            assert s[0::3][:3].tolist() == [112.0, 224.0, 448.0]
            assert ref["levels"].tolist() == [1, 0, 1, 2, 1, 2, 3, 2, 3, 0, 3]                 # ... 1 x 1 -> k_min, 1e4 -> k_max
            assert float(s[-2]) == 1.0 and float(s[-1]) == 1e4
        else:
            nb, dropped = E.level_boundaries()
            kept = sum(len(v["rois"]) for v in E.cases().values() if v["family"] == "levels")
            assert 10 * dropped <= kept + dropped
            assert ref["levels"].tolist() == [0, 1, 1, 1, 2, 2, 2, 3, 3]
            assert s[2::3].tolist() == [112.0, 224.0, 448.0]                                 # the non-square boundary boxes
            for k, sq in enumerate((112, 224, 448)):
                lo, hi = nb[(sq, "below")], nb[(sq, "above")]
                assert 0 < np.float32(hi[2]) - np.float32(lo[2]) <= 24 * np.spacing(np.float32(lo[2])) and abs(lo[2] - 100 + 1 - sq) < 1e-3 * sq


# ---- CPU: a wrong kernel cannot pass ----------------------------------------------------------------------------------
CAUGHT_BY = {"ge_size_invalid": ("border_p7_pad0", "border_p30_pad0"),
             "le_m1_invalid": ("border_p7_pad0", "border_p30_pad0"),
             "no_clamp0": ("border_p7_pad0", "border_p30_pad0", "window_A_even"),
             "aligned": E.CASE_NAMES,
             "no_side_clamp": ("tiny_A", "window_A_odd"),
             "pad_replicate": ("pad_512_A", "pad_100_B", "border_p15_pad8", "outside_pad100"),
             "pad_untruncated": ("pad_100_A", "pad_100_B", "window_B_odd"),
             "level_no_plus1": ("levels_exact", "levels_nearest"),
             "level_no_eps": ("levels_nearest",),
             "coord_order": ("ordinary_A", "levels_exact", "pad_512_A", "window_S_staging"),
             "drop_last_high": ("window_A_even", "window_B_odd", "window_S_staging", "border_p30_pad0", "pad_100_A")}


@pytest.mark.parametrize("mut", E.MUTANTS)
def test_the_reference_with_one_rule_changed_breaks_the_criterion(mut):
    assert set(CAUGHT_BY) == set(E.MUTANTS)
    for name in CAUGHT_BY[mut]:
        ref = E.reference(name)
        levels, out = E.mutant(name, mut)
        assert E.violates(ref, levels, out) is not None, (mut, name)
    if mut.startswith("level_"):
        name = CAUGHT_BY[mut][-1]
        assert E.mutant(name, mut)[0].tolist() != E.reference(name)["levels"].tolist()
    if mut == "pad_untruncated":                         # 512 px is a whole number of cells on every level: nothing to see there
        assert E.violates(E.reference("pad_512_A"), *E.mutant("pad_512_A", mut)) is None


def test_the_rounding_sequence_mutant_passes_the_old_tolerance_and_fails_the_bound():
    """``start + (p + (i + .5) / G) * bin`` instead of ``start + p * bin + (i + .5) * bin / G``: on ordinary geometry every
    output is within atol = rtol = 1e-5 of ref32, and 15 times the bound away from ref64."""
    ref = E.reference("ordinary_A")
    levels, out = E.mutant("ordinary_A", "coord_order")
    assert levels.tolist() == ref["levels"].tolist() and E.passes_old_tolerance(ref, out)
    assert E.violates(ref, levels, out) is not None
    err, _ = E.kernel_error(ref, out)
    assert err > 10 * (2 * ref["e32"] + E.MARGIN)
    # on dyadic geometry the two sequences are the same numbers
    assert E.violates(E.reference("border_p30_pad0"), *E.mutant("border_p30_pad0", "coord_order")) is None


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


def _maps(c, images=1, dtype=None, channels_last=False):
    out = []
    for m in E.maps(c["pyr"], c["C"], images):
        m = m.to(DEV)
        if dtype is not None:
            m = m.to(dtype)
        if channels_last:
            m = m.contiguous(memory_format=torch.channels_last)
        out.append(m)
    return out


def _boxes(c):
    rois = _t(c["rois"]).to(DEV)
    return rois, (None if c["level_boxes"] is None else _t(c["level_boxes"]).to(DEV))


def _pool(ops, c, feats, out_size=None, g=None, rois=None, lb=None):
    r0, l0 = _boxes(c)
    rois, lb = (r0 if rois is None else rois), (l0 if lb is None else lb)
    out, lv = ops.roi_align_levels(feats, rois, lb, c["out_size"] if out_size is None else out_size, E.scales_of(c["pyr"]),
                                   c["g"] if g is None else g, E.pad_cells(c), return_levels=True)
    torch.cuda.synchronize()
    return out, lv


def _judge(form, name, ref, levels, out):
    """THE comparison of this module (``E.violates``); prints e32, the kernel's error and the bit-identical share."""
    out = out.detach().cpu()
    levels = [int(v) for v in (levels.cpu().tolist() if isinstance(levels, torch.Tensor) else levels)]
    err, same = E.kernel_error(ref, out)
    print("roi-edge %-22s %-18s family %-8s e32 %.3e kernel %.3e identical %.4f" % (form, name, E.cases()[name]["family"], ref["e32"], err, same))
    why = E.violates(ref, levels, out)
    assert why is None, "%s, %s: %s" % (form, name, why)


LEVELS_RUNS = [(n, "product") for n in E.CASE_NAMES] + [(n, "generic") for n in E.CASE_NAMES if E.cases()[n]["out_size"] in SEPARABLE]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel", LEVELS_RUNS)
def test_roi_align_levels_edge_case(ops, name, kernel):
    """``ops.roi_align_levels`` at the case's pooled size: the separable kernel at 7 / 15 / 30 with two samples per bin, the
    generic kernel otherwise ("product"), and the generic kernel at the separable sizes through SMOT_ROI_GENERIC."""
    c = E.cases()[name]
    feats = _maps(c)
    for g in c["gs"]:
        if kernel == "generic":
            with ops.debug_library(SMOT_ROI_GENERIC=1):
                out, lv = _pool(ops, c, feats, g=g)
        else:
            out, lv = _pool(ops, c, feats, g=g)
        form = "levels/%s g%d" % ("separable" if (kernel == "product" and c["out_size"] in SEPARABLE and g == 2) else "generic", g)
        _judge(form, name, E.reference(name, g=g), lv, out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.SINGLE_LEVEL)
def test_roi_align_with_image_indices_edge_case(ops, name):
    """``ops.roi_align`` ([R, 5] rois) on a batch of three different images at 5 x 9 bins, three samples per bin; the case's
    rows go round the images, and a row with image index 3 pools to zeros."""
    c = dict(E.cases()[name], images=3)
    feats = _maps(c, images=3)[0]
    R = len(c["rois"])
    img = np.arange(R) % 3
    rois5 = np.concatenate((img[:, None].astype(np.float32), c["rois"]), 1)
    rois5 = np.concatenate((rois5, np.concatenate(([3.0], c["rois"][0]))[None].astype(np.float32)), 0)
    out = ops.roi_align(feats, _t(rois5).to(DEV), 0.25, 5, 9, 3, E.pad_cells(c)[0])
    torch.cuda.synchronize()
    assert tuple(out.shape) == (R + 1, c["C"], 5, 9) and not bool(out[R].any())
    for b in range(3):
        rows = np.flatnonzero(img == b)
        ref = E.reference_eval(c, 5, 9, 3, rois=c["rois"][rows], image=b)
        _judge("rois5 5x9 g3 image %d" % b, name, ref, [0] * len(rows), out[_t(rows).to(DEV)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED_CASES)
def test_pooling_and_correlation_edge_case(ops, name):
    """``ops.sr_xcorr_fused`` at 30 / 15 with its pooled planes against the bound and its response against the correlation of
    those planes; the 35 / 7 family through ``ops.roi_align_levels(35)`` against the bound, and its one-kernel entry bit for
    bit against the correlation of those planes (as test_fused_gather_kernel_of_the_second_yaml_family_... has it)."""
    from test_hip_parity import _assert_response_is_the_correlation
    c = E.cases()[name]
    feats = _maps(c)
    rois, lb = _boxes(c)
    boxes = rois if lb is None else lb
    R, C = len(c["rois"]), c["C"]
    g = torch.Generator().manual_seed(99)
    z = torch.randn((R, C, 15, 15), generator=g).to(DEV)
    resp, pooled = ops.sr_xcorr_fused(feats, boxes, rois, z, 30, 15, E.scales_of(c["pyr"]), 2, c["pad_pixels"], return_pooled=True)
    torch.cuda.synchronize()
    ref = E.reference(name, 30, 30, 2)
    _judge("fused 30/15 pooled", name, ref, ref["levels"], pooled)
    _assert_response_is_the_correlation(resp, pooled, z, name)
    x35, lv = _pool(ops, c, feats, out_size=35, g=2)
    _judge("levels/generic 35", name, E.reference(name, 35, 35, 2), lv, x35)
    z7 = torch.randn((R, C, 7, 7), generator=g).to(DEV)
    got = ops.sr_xcorr_fused(feats, boxes, rois, z7, 35, 7, E.scales_of(c["pyr"]), 2, c["pad_pixels"])
    want = ops.xcorr_depthwise(x35, z7)
    assert torch.equal(got, want), "%s: 35 / 7 entry, max diff %g" % (name, float((got - want).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("rz", [15, 7])
@pytest.mark.parametrize("name", EXTRACT_CASES)
def test_template_extraction_edge_case(ops, name, rz):
    """``ops.emm_extract_cache(hint=True)``: templates against the bound, search regions bit-equal to ``O.search_region``, the
    levels in the hint's by-roi records the reference's."""
    c = E.cases()[name]
    boxes = E.extraction_boxes(c)
    ref = E.reference(name, rz, rz, 2, boxes_as_rois=True)
    scales = E.scales_of(c["pyr"])
    z, sr, oh = ops.emm_extract_cache(_maps(c), _t(boxes).to(DEV), rz, scales, 2, 512.0, 1.0, 0.0, hint=True)
    torch.cuda.synchronize()
    _judge("extract rz%d" % rz, name, ref, ref["levels"], z)
    want = O.search_region(_t(boxes), 512.0, 1.0, 0.0)
    assert torch.equal(sr.cpu().view(torch.int32), want.view(torch.int32))
    assert (oh is not None) == (rz == 15 and len(boxes) >= 2)
    if oh is not None:
        rec = oh.cpu()[:, ops.HINT_FLOATS - HINT_BYROI_FROM_END:].contiguous().view(torch.int32)
        assert rec[:, 4].tolist() == ref["levels"].tolist() and rec[:, 5].tolist() == [len(boxes)] * len(boxes)
        assert torch.equal(rec[:, :4], want.view(torch.int32)) and ops.order_hint_status(oh) == 0


def _forms(call, c, what):
    """The project's stated identities of a map-reading call ``call(feats)`` -> tensor, bitwise."""
    base = call(_maps(c))
    for dt in (torch.float16, torch.bfloat16):
        half = _maps(c, dtype=dt)
        a, b = call(half), call([m.float() for m in half])
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: %s maps differ from the fp32 call on the upcast maps" % (what, dt)
        if c["C"] % 8 == 0:
            a_cl = call(_maps(c, dtype=dt, channels_last=True))
            assert torch.equal(a_cl.view(torch.int32), a.view(torch.int32)), "%s: channels-last %s maps" % (what, dt)
    if c["C"] % 8 == 0:
        cl = _maps(c, channels_last=True)
        assert not cl[0].is_contiguous()
        assert torch.equal(call(cl).view(torch.int32), base.view(torch.int32)), "%s: channels-last fp32 maps" % what
    return base


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_forms_are_bitwise_identical_at_the_edges(ops, name):
    """fp16 / bf16 call = fp32 call on the upcast maps; channels-last (C = 8, 16) = NCHW; batched = per image (three images:
    none, the case's rows, the case's last four rows)."""
    c = E.cases()[name]
    rois, lb = _boxes(c)
    scales, pads, P, g = E.scales_of(c["pyr"]), E.pad_cells(c), c["out_size"], c["g"]
    _forms(lambda f: ops.roi_align_levels(f, rois, lb, P, scales, g, pads), c, name + " roi_align_levels")
    if name in FUSED_CASES:
        boxes = rois if lb is None else lb
        z = torch.randn((len(rois), c["C"], 15, 15), generator=torch.Generator().manual_seed(5)).to(DEV)
        _forms(lambda f: torch.cat([t.reshape(len(rois), -1) for t in ops.sr_xcorr_fused(
            f, boxes, rois, z, 30, 15, scales, 2, c["pad_pixels"], return_pooled=True)], 1).contiguous(), c, name + " sr_xcorr_fused")
    R = len(rois)
    k = min(4, R)                                        # (window_*: the row on level 0's last cell and the whole maps of levels 1 .. 3)
    rows = [0, R, k]
    rois_b = torch.cat((rois, rois[R - k:]), 0).contiguous()
    lb_b = None if lb is None else torch.cat((lb, lb[R - k:]), 0).contiguous()
    for kw in ({}, {"dtype": torch.float16}, {"channels_last": True}):
        if kw.get("channels_last") and c["C"] % 8:
            continue
        feats = _maps(c, images=3, **kw)
        got = ops.roi_align_levels_batched(feats, rois_b, lb_b, rows, P, scales, g, pads)
        one = lambda b, r_, l_: ops.roi_align_levels([f[b:b + 1] for f in feats], r_, l_, P, scales, g, pads)
        want = torch.cat((one(1, rois, lb), one(2, rois_b[R:], None if lb_b is None else lb_b[R:])), 0)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "%s: batched %s" % (name, kw)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_non_finite_rows_leave_the_clean_rows_alone(ops):
    """One launch per form with NaN, +inf, -inf in a roi coordinate or in a level box and an inverted level box among clean
    rows (see the module docstring for why no form can leave the map): every clean row is bit-identical to the same launch
    with the dirty rows made finite, the dirty rows' levels are in range, a roi at +-inf pools to exact zeros."""
    c = dict(E.cases()["pad_100_A"])
    scales, pads = E.scales_of("A"), E.pad_cells(c)
    feats = _maps(c)
    dirty, clean, at = E.nonfinite_rows(c["pad_pixels"])
    dev = lambda d: (_t(d["rois"]).to(DEV), _t(d["level_boxes"]).to(DEV))
    (dr, db), (cr, cb) = dev(dirty), dev(clean)
    R = len(dirty["rois"])
    keep = torch.ones(R, dtype=torch.bool)
    keep[list(at.values())] = False
    zero_rows = [at["roi_at_pinf"], at["roi_at_ninf"]]
    g = torch.Generator().manual_seed(11)
    z15, z7 = torch.randn((R, c["C"], 15, 15), generator=g).to(DEV), torch.randn((R, c["C"], 7, 7), generator=g).to(DEV)

    def levels_form(out_size, gs, generic=False):
        def run(r_, b_):
            if generic:
                with ops.debug_library(SMOT_ROI_GENERIC=1):
                    return ops.roi_align_levels(feats, r_, b_, out_size, scales, gs, pads, return_levels=True)
            return ops.roi_align_levels(feats, r_, b_, out_size, scales, gs, pads, return_levels=True)
        return run

    forms = {"separable 30": levels_form(30, 2), "separable 15": levels_form(15, 2), "separable 7": levels_form(7, 2),
             "generic 15 g2": levels_form(15, 2, True), "generic 9 g3": levels_form(9, 3),
             "fused 30/15": lambda r_, b_: ops.sr_xcorr_fused(feats, b_, r_, z15, 30, 15, scales, 2, c["pad_pixels"], return_pooled=True)[::-1],
             "gather 35/7": lambda r_, b_: (ops.sr_xcorr_fused(feats, b_, r_, z7, 35, 7, scales, 2, c["pad_pixels"]), None)}
    for what, run in forms.items():
        got, lv = run(dr, db)
        base, lv0 = run(cr, cb)
        torch.cuda.synchronize()
        got, base = got.cpu(), base.cpu()
        assert torch.equal(got[keep].view(torch.int32), base[keep].view(torch.int32)), "%s: a clean row changed" % what
        assert not bool(got[zero_rows].any()) and not bool(torch.isnan(got[zero_rows]).any()), "%s: roi at +-inf" % what
        if what.startswith(("separable", "generic")):
            lv, lv0 = lv.cpu(), lv0.cpu()
            assert torch.equal(lv[keep], lv0[keep]) and int(lv.min()) >= 0 and int(lv.max()) <= 3, (what, lv.tolist())
        elif what == "fused 30/15":                      # (the second output is the response)
            assert torch.equal(lv.cpu()[keep].view(torch.int32), lv0.cpu()[keep].view(torch.int32)), "%s: response" % what
            assert not bool(lv.cpu()[zero_rows].any())
    # the one-launch extraction: a box is roi and level box at once
    boxes_d, boxes_c = clean["rois"].copy() - c["pad_pixels"], clean["rois"].copy() - c["pad_pixels"]
    kinds = {1: (0, np.nan), 3: (3, np.nan), 5: (2, np.inf), 7: (1, -np.inf)}
    for r, (k, v) in kinds.items():
        boxes_d[r, k] = v
    boxes_d[9] = (np.inf, 50.0, np.inf, 90.0)
    boxes_d[11] = (40.0, -np.inf, 90.0, -np.inf)
    boxes_d[13] = (300.0, 10.0, 100.0, 200.0)
    keep = torch.ones(R, dtype=torch.bool)
    keep[[1, 3, 5, 7, 9, 11, 13]] = False
    for rz in (15, 7):
        zd, srd, ohd = ops.emm_extract_cache(feats, _t(boxes_d).to(DEV), rz, scales, 2, 512.0, 1.0, 0.0, hint=True)
        zc, src, ohc = ops.emm_extract_cache(feats, _t(boxes_c).to(DEV), rz, scales, 2, 512.0, 1.0, 0.0, hint=True)
        torch.cuda.synchronize()
        assert torch.equal(zd.cpu()[keep].view(torch.int32), zc.cpu()[keep].view(torch.int32)), "extraction rz %d: a clean row changed" % rz
        assert torch.equal(srd.cpu()[keep].view(torch.int32), src.cpu()[keep].view(torch.int32))
        assert not bool(zd.cpu()[[9, 11]].any()) and not bool(torch.isnan(zd.cpu()[[9, 11]]).any())
        if ohd is not None:
            rec = ohd.cpu()[:, ops.HINT_FLOATS - HINT_BYROI_FROM_END:].contiguous().view(torch.int32)
            rec0 = ohc.cpu()[:, ops.HINT_FLOATS - HINT_BYROI_FROM_END:].contiguous().view(torch.int32)
            assert int(rec[:, 4].min()) >= 0 and int(rec[:, 4].max()) <= 3 and torch.equal(rec[keep], rec0[keep])
