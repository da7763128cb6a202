"""The depthwise cross-correlation K2 (csrc/xcorr.hip ``smot_xcorr_dw_fwd``) and the head's general path (the ``else``
branch of ``emm_track_impl`` and the non-separable branch of ``emm_extract_cache_impl``, csrc/emm_fused.hip) against CPU
references at the shapes where their kernels change behaviour.  Every other test runs ``ops.xcorr_depthwise`` at the two
yaml shapes only (30/15: ``xcorr_dw_patch2_kernel``, 35/7: ``xcorr_dw_rowpatch_kernel``) on ``randn`` data, never
compares ``xcorr_dw_generic_kernel`` with anything, and runs the general path at (20, 9) only, batched against unbatched.

Inputs, references and the assertions themselves come from tests/xcorr_edge_cases.py.

Part A, the three correlation kernels.  Yardstick: ``ref64``, the explicit fp64 sum over taps (pinned on the CPU to
``oracle.emm_oracle.xcorr_depthwise`` and to grouped ``F.conv2d`` in fp64); ``mag = ref64(|x|, |z|)``.
  1. exact grid (x, z in k / 64): every fp32 fmaf is exact in any order, so ``torch.equal(out, ref64.float())`` — no
     tolerance; per-plane seeds, and per kernel a delta template with one live tap per plane (the four corners included);
  2. ``randn`` data and data with twelve decades of range inside a plane: |out - ref64| <= rz^2 * 2^-24 * mag (+ 1e-30), the
     a-priori bound of an rz^2-step fp32 fmaf chain; on ``randn`` data with at most 225 taps also the project's 1e-6 * mag;
  3. one NaN, +inf and -inf in x, a NaN and an inf in z, in different planes at corner, edge and interior cells: the NaN
     mask and the +-inf cells are ref64's (inf * 0 = NaN included), every other output meets the bound, untouched planes
     are bit-equal to the call without planted values;
  4. all-zero planes and templates of both signs give exact +0 planes;
and determinism, the empty call, the 64 KiB LDS opt-in of the generic kernel and its 160 KiB refusal.  The CPU part shows
the conditions of kind 1 from the references alone and rehearses the assertions of kinds 1-3 on a correct fp32 stand-in
(torch's grouped convolution: passes all) and on six mutants of it (each fails one).

Part B, the general path at (rx, rz) = (18, 3), (29, 1), (20, 9), (45, 15), (21, 7), 30/15 with one sample per bin and 35/7
with three, and (18, 3) at C = 64: the one-call entry points equal the operator composition, ``siammot_amd.emm.EMM`` and
the batched entry points bit for bit; every stage is held to the oracle evaluated on the product's own previous stage with
the project's existing measures (pooling 1e-5 abs + rel, search regions bit-equal, response 1e-6 * mag, logits 1e-4 / 2e-4
of the channel scale, decode by ``decode_edge_cases.adjudicate`` with its cap of excused tracks); at Ho 16 / 29
``ops.tower_form`` must report a Winograd form.

What these tests found.  (1) The head at (rx, rz) = (45, 15) did not run at all: Ho = 31 takes the scalar predictor, whose
entry guard admits 1024 positions (Ho <= 32) while its heads kernel stages 16 haloed planes in LDS — 69,696 B at Ho = 31 —
and refused everything above 64 KiB ("Ho=31 too large for the heads kernel").  ``predictor_impl`` opts in to the larger
LDS now (``ensure_lds_optin``), and Ho = 30, 31, 32 are held to the oracle here.  (2) The generic correlation kernel
admitted up to 160 KiB of dynamic LDS without that opt-in; ``smot_xcorr_dw_fwd`` makes it now — before any launch above
64 KiB was ever tried on the device, so whether the runtime would have refused it is not known — and the (128, 3) case
holds it to the exact sum.  (3) At (45, 15) the response of the generic kernel, then ONE fmaf chain over all 225 taps,
was off by 1.062e-06 * mag from the fp64 sum of the pooled planes, above the 1e-6 the project states for this operator
(an exact emulation of that chain on the CPU gives the same figure: no defect of the kernel's code, the accuracy of the
form).  The generic kernel now keeps one chain per template row and adds the row sums: 2 rz rounding steps instead of rz^2,
2.7e-07 at (45, 15).  The 30/15 and 35/7 kernels are unchanged.  Everything else is exact, within its bound or bit-equal
as stated.
Measured figures: profiles/xcorr_edges_parity.md."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_edge_cases as D
import golden_inputs as gi
import predictor_edge_cases as P
import xcorr_edge_cases as E
from oracle import emm_oracle as O

DEV = "cuda:0"


# =========================================================================================================================
# CPU: the references, the cases' conditions, the rehearsal
# =========================================================================================================================
def test_ref64_is_the_oracles_correlation_and_the_grouped_convolution():
    rs = np.random.RandomState(5)
    for rx, rz in ((30, 15), (35, 7), (18, 3), (29, 1), (33, 32), (1, 1)):
        x = torch.from_numpy(rs.standard_normal((2, 3, rx, rx)))
        z = torch.from_numpy(rs.standard_normal((2, 3, rz, rz)))
        ref = E.ref64(x, z)
        scale = float(E.mag(x, z).max())
        assert ref.dtype == torch.float64 and tuple(ref.shape) == (2, 3, rx - rz + 1, rx - rz + 1)
        assert float((ref - O.xcorr_depthwise(x, z)).abs().max()) <= 1e-13 * scale
        conv = F.conv2d(x.reshape(1, 6, rx, rx), z.reshape(6, 1, rz, rz), groups=6).reshape(ref.shape)
        assert float((ref - conv).abs().max()) <= 1e-13 * scale
    # fp32 inputs are widened, not rounded; inf * 0 is NaN and reaches only the outputs whose window covers it
    x = torch.ones((1, 1, 4, 4))
    x[0, 0, 0, 0] = float("inf")
    z = torch.tensor([[[[0.0, 1.0], [1.0, 1.0]]]])
    ref = E.ref64(x, z)
    assert bool(torch.isnan(ref[0, 0, 0, 0])) and int(torch.isnan(ref).sum()) == 1 and float(ref[0, 0, 1, 1]) == 3.0
    z[0, 0, 0, 0] = -2.0
    assert float(E.ref64(x, z)[0, 0, 0, 0]) == float("-inf")


def test_cases_cover_the_kernels_and_their_edges():
    kinds = {}
    for c in E.CASES.values():
        kinds.setdefault(E.kernel_of(c["rx"], c["rz"]), set()).add(c["kind"])
    assert kinds == {k: {"exact", "normal", "range", "nfzero", "nfnonzero", "zeros", "delta"}
                     for k in (E.PATCH2, E.ROWPATCH, E.GENERIC)}
    assert E.PLANES[(30, 15)] == (1, 2, 3, 7, 45) and E.PLANES[(35, 7)] == (1, 5, 33)
    assert set(E.GENERIC_SHAPES) == {(1, 1), (15, 15), (16, 1), (18, 3), (29, 1), (20, 9), (21, 7), (45, 15), (33, 32), (64, 7)}
    assert all(E.PLANES[s] == (1, 5) for s in E.GENERIC_SHAPES)
    ho = {s: s[0] - s[1] + 1 for s in E.GENERIC_SHAPES}
    assert ho[(15, 15)] == 1 and ho[(16, 1)] == 16 and ho[(33, 32)] == 2 and ho[(64, 7)] == 58
    assert ho[(45, 15)] ** 2 == 961 and 3 * 256 < 961 < 4 * 256          # four passes of the output loop, the last partial
    assert max(rz * rz for _, rz in E.SHAPES) == 1024
    for (rx, rz), p in E.DELTA_SHAPES.items():                           # the four corners and interior taps, all distinct
        taps = [E.delta_tap(rz, k) for k in range(p)]
        assert len(set(taps)) == p and set(taps[:4]) == {(0, 0), (0, rz - 1), (rz - 1, 0), (rz - 1, rz - 1)}
        assert any(0 < u < rz - 1 and 0 < v < rz - 1 for u, v in taps[4:])
    assert max(c["planes"] * c["rx"] ** 2 for c in E.CASES.values()) == 45 * 30 * 30
    assert E.lds_bytes(*E.LDS_OPTIN) == 65572 > 65536 >= E.lds_bytes(127, 3)
    assert E.lds_bytes(*E.LDS_REFUSED) == 164872 > 160 * 1024 >= E.lds_bytes(202, 3)


@pytest.mark.parametrize("name", E.EXACT_CASES)
def test_exact_grid_case_is_exact_in_fp32(name):
    """What makes kind 1 a test without a tolerance: the fp64 sum is an fp32 number and the absolute sum stays below 2^10,
    so every partial sum of multiples of 2^-12, in any order, fits the 24-bit significand."""
    c, ref = E.CASES[name], E.reference(name)
    x, z = E.inputs(name)
    for t in (x, z):
        assert bool((t * 64 == (t * 64).round()).all()) and float(t.abs().max()) <= 1.0
    assert torch.equal(ref["ref"].float().double(), ref["ref"])
    assert float(ref["mag"].max()) < 2 ** 10
    planes = torch.cat((x.reshape(c["planes"], -1), z.reshape(c["planes"], -1)), 1)
    assert len({tuple(p.tolist()) for p in planes}) == c["planes"], "planes share data"
    if c["kind"] == "delta":                                             # the result is the shifted crop times the live tap
        ho = c["rx"] - c["rz"] + 1
        xf, zf, rf = x.reshape(-1, c["rx"], c["rx"]), z.reshape(-1, c["rz"], c["rz"]), ref["ref"].reshape(-1, ho, ho)
        for k in range(c["planes"]):
            u, v = E.delta_tap(c["rz"], k)
            assert int((zf[k] != 0).sum()) == 1 and float(zf[k, u, v]) != 0
            assert torch.equal(rf[k], xf[k, u:u + ho, v:v + ho].double() * zf[k, u, v].double())
        assert len({float(zf[k].sum()) for k in range(c["planes"])}) == c["planes"]
    elif ref["ref"].numel() >= 100:
        assert float((ref["ref"] != 0).double().mean()) > 0.9


@pytest.mark.parametrize("name", E.NF_CASES)
def test_non_finite_case_plants_what_it_says(name):
    c, ref = E.CASES[name], E.reference(name)["ref"]
    x, z = E.planted(name)
    p, rx, rz = c["planes"], c["rx"], c["rz"]
    xf, zf, rf = x.reshape(p, rx, rx), z.reshape(p, rz, rz), ref.reshape(p, -1)
    pos = E.nf_positions(c)
    assert sorted(v[0] for v in pos.values()) == [0, 1, 2, 4, 5] and all(k not in E.NF_CLEAN for k, _, _ in pos.values())
    assert int((~torch.isfinite(x)).sum()) == 3 and int((~torch.isfinite(z)).sum()) == 2
    assert bool(torch.isnan(xf[pos["x_nan"]])) and float(xf[pos["x_pinf"]]) == float("inf")
    assert float(xf[pos["x_ninf"]]) == float("-inf") and bool(torch.isnan(zf[pos["z_nan"]]))
    for k in E.NF_CLEAN:
        assert bool(torch.isfinite(rf[k]).all())
    assert bool(torch.isnan(rf[0]).any()) and bool(torch.isnan(rf[4]).all())
    assert bool(torch.isinf(rf[5]).all()) or bool(torch.isnan(rf[5]).any())
    if rz > 1 and rx - rz >= 11:                                         # both signs of the inf in z, by the sign of x
        assert bool(torch.isposinf(rf[5]).any()) and bool(torch.isneginf(rf[5]).any())
    taps = zf[1]
    if c["kind"] == "nfzero":                                            # a zero tap meets the +inf: NaN exactly there
        assert float(taps[E.nf_zero_tap(c)]) == 0 and int(torch.isnan(rf[1]).sum()) == 1
        assert rz == 1 or rx == rz or bool(torch.isinf(rf[1]).any())
    else:                                                                # only non-zero taps meet it: +-inf, never NaN
        assert bool((taps != 0).all()) and not bool(torch.isnan(rf[1]).any()) and bool(torch.isinf(rf[1]).any())
    if rx - rz >= 8:                                                     # ... and only the outputs whose window covers a value move
        for k in (0, 1, 2):
            assert bool(torch.isfinite(rf[k]).any())


def test_rehearsal_the_correct_stand_in_passes_every_assertion():
    names = E.EXACT_CASES + E.BOUND_CASES + E.NF_CASES
    assert E.run_checks(E.standin, names) == []
    print("xcorr-edge rehearsal: torch fp32 grouped conv, max err / mag " + ", ".join(
        "%s %.2e" % (n, E.check_bound(E.standin, n)) for n in ("normal_30x15_p45", "normal_33x32_p5", "normal_45x15_p5")))


@pytest.mark.parametrize("mutant", sorted(E.MUTANTS))
def test_rehearsal_every_mutant_fails_an_assertion(mutant):
    """The assertions of kinds 1-3 are strong enough to see each of these wrong kernels, on small cases of every kernel."""
    names = [n for n in E.EXACT_CASES + E.BOUND_CASES + E.NF_CASES
             if (E.CASES[n]["rx"], E.CASES[n]["rz"]) in ((30, 15), (35, 7), (18, 3), (20, 9)) and E.CASES[n]["planes"] <= 7]
    failed = E.run_checks(E.MUTANTS[mutant], names)
    print("xcorr-edge rehearsal: %-32s fails %d of %d cases" % (mutant, len(failed), len(names)))
    assert failed, "the mutant '%s' passes every assertion" % mutant
    per_kernel = {E.kernel_of(E.CASES[n]["rx"], E.CASES[n]["rz"]) for n in failed}
    assert per_kernel == {E.PATCH2, E.ROWPATCH, E.GENERIC}, per_kernel
    kinds = {E.CASES[n]["kind"] for n in failed}
    if mutant == "inf * 0 skipped":                                      # ... seen by the zero-tap cases and by nothing else
        assert kinds == {"nfzero"}
    else:
        assert "exact" in kinds or "delta" in kinds


# ---- part B: the head cases' conditions, from the oracle alone -----------------------------------------------------------
@pytest.mark.parametrize("name", E.HEAD_NAMES)
def test_head_case_meets_its_conditions(name):
    """Conditions on the INPUTS of part B.  If one fails, the seed is to be changed, not this test."""
    cfg, orc = E.head_cfg(name), E.head_oracle(name)
    rx, ho = E.HEAD_SHAPES[name]
    assert (cfg.rx, cfg.rx - cfg.rz + 1) == (rx, ho), "(rx, Ho) = (%d, %d)" % (cfg.rx, cfg.rx - cfg.rz + 1)
    separable_extract = cfg.rz in (15, 7) and cfg.sampling_ratio == 2
    fused = (cfg.rx, cfg.rz) in ((30, 15), (35, 7)) and cfg.sampling_ratio == 2
    assert not fused, "the case takes a fused kernel, not the general path"
    assert separable_extract == (name in ("45_15", "21_7"))               # (their extraction is the separable kernel's)
    # the predictor's conditions (test_predictor_edges)
    assert float(orc["pred_scale"].min()) >= 1e-3, "an output channel's fp64 scale is %.3e" % float(orc["pred_scale"].min())
    assert orc["pred_err32"] <= 2e-5, "fp32 oracle vs fp64: %.3e" % orc["pred_err32"]
    # the decode's: the fp32 oracle's cells against the fp64 oracle by the rule of decode_edge_cases
    verdicts = D.adjudicate(orc["decode64"], orc["decode32"]["idx"])
    failed = [v for v in verdicts if v[0] == "fail"]
    excused = [v for v in verdicts if v[0] == "excused"]
    assert not failed and len(excused) <= E.TRACKS // D.EXCUSED_PER_TRACKS, verdicts
    assert np.array_equal(orc["decode32"]["idx"], orc["decode32"]["idx_torch"])
    assert bool(torch.isfinite(orc["f32"]["bb"]).all()) and bool(torch.isfinite(orc["f32"]["conf"]).all())
    # search regions: at least one crosses the image border, at least one lies inside
    sr = orc["f32"]["sr"].numpy() - cfg.pad_pixels
    W, H = E.IMAGE_WH
    inside = (sr[:, 0] >= 0) & (sr[:, 1] >= 0) & (sr[:, 2] <= W - 1) & (sr[:, 3] <= H - 1)
    meets = (sr[:, 2] > 0) & (sr[:, 3] > 0) & (sr[:, 0] < W - 1) & (sr[:, 1] < H - 1)
    assert int(inside.sum()) >= 1 and int((meets & ~inside).sum()) >= 1, (inside, meets)
    b = E.head_boxes(name)
    assert int(((b[:, 0] < 0) | (b[:, 1] < 0) | (b[:, 2] > W - 1) | (b[:, 3] > H - 1)).sum()) >= 2     # boxes partly outside
    # the batched test compares image by image bit for bit: the towers' form must not depend on the row count
    c = E.HEAD_CASES[name][3]
    if ho == 29:
        assert len({P.blocked_tiles(n, c) for n in E.BATCH_ROWS + (E.TRACKS,) if n}) == 1
    assert sum(E.BATCH_ROWS) == E.TRACKS and 0 in E.BATCH_ROWS


@pytest.mark.parametrize("name", E.HEAD_NAMES)
def test_head_case_fp32_chain_on_the_oracles_pooled_planes(name):
    """What the kernels' fp32 accumulation gives on the oracle's pooled planes of a case, from the CPU alone (an emulation,
    ``E.fma_chain32``): one fmaf chain over all taps — inside its a-priori bound everywhere, but AT the project's 1e-6 for the
    225 taps of (45, 15) — and one chain per template row with the row sums added, the generic kernel's form, which must
    keep a factor two to that 1e-6 in every case so that the GPU test's bound is no coin toss."""
    orc = E.head_oracle(name)
    x, z = orc["f32"]["inter"]["sr_features"], orc["f32"]["z"]
    ref, m = E.ref64(x, z), E.mag(x, z)
    live = m > 0
    assert float(live.double().mean()) > 0.5
    one = (E.fma_chain32(x, z).double() - ref).abs()
    rows = (E.fma_chain32(x, z, rows=True).double() - ref).abs()
    assert bool((one <= E.bound(x, z)).all()) and bool((rows <= E.bound(x, z)).all())
    r_one, r_rows = float((one[live] / m[live]).max()), float((rows[live] / m[live]).max())
    print("xcorr-edge head %-13s on the oracle's planes: one fmaf chain %.3e, row chains %.3e (a-priori %.3e, project %.1e)" % (
        name, r_one, r_rows, z.shape[-1] ** 2 * E.U24, E.PROJECT_RATIO))
    if E.kernel_of(x.shape[-1], z.shape[-1]) == E.GENERIC:
        assert r_rows <= 0.5 * E.PROJECT_RATIO, "row chains %.3e" % r_rows


def test_head_cases_are_the_general_path_shapes():
    assert {k: (E.head_cfg(k).rz, E.head_cfg(k).rx, E.head_cfg(k).sampling_ratio) for k in E.HEAD_NAMES} == {
        "18_3": (3, 18, 2), "29_1": (1, 29, 2), "20_9": (9, 20, 2), "45_15": (15, 45, 2), "21_7": (7, 21, 2),
        "30_15_ratio1": (15, 30, 1), "35_7_ratio3": (7, 35, 3), "18_3_c64": (3, 18, 2)}
    assert O.EMMConfig(rz=9, search_region=E.HEAD_CASES["20_9"][1]).rx == 20
    assert set(E.WINOGRAD_HEADS) == {"18_3", "29_1", "30_15_ratio1", "35_7_ratio3", "18_3_c64"}
    assert E.HEAD_CASES["18_3_c64"][3] == 64 and all(v[3] == 32 for k, v in E.HEAD_CASES.items() if k != "18_3_c64")
    for k in E.WINOGRAD_HEADS:                                            # what predictor_impl picks for them
        assert P.family(E.HEAD_CASES[k][3], E.GN_GROUPS, E.HEAD_SHAPES[k][1], True) in ("wino16", "wino29")
    for k in set(E.HEAD_NAMES) - set(E.WINOGRAD_HEADS):
        assert P.family(E.HEAD_CASES[k][3], E.GN_GROUPS, E.HEAD_SHAPES[k][1], True) == "scalar"


# =========================================================================================================================
# GPU, part A
# =========================================================================================================================
@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.fixture(scope="module")
def xcorr(ops):
    def run(x, z):
        out = ops.xcorr_depthwise(x.to(DEV), z.to(DEV))
        torch.cuda.synchronize()
        return out.cpu()
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.EXACT_CASES)
def test_xcorr_exact_grid(xcorr, name):
    E.check_exact(xcorr, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.BOUND_CASES)
def test_xcorr_within_the_fma_chain_bound(xcorr, name):
    c = E.CASES[name]
    ratio = E.check_bound(xcorr, name)
    print("xcorr-edge %-22s %-8s max err / mag %.3e (bound %.3e)" % (name, E.kernel_of(c["rx"], c["rz"]), ratio,
                                                                     c["rz"] ** 2 * E.U24))


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.NF_CASES)
def test_xcorr_non_finite_cells_reach_their_windows_only(xcorr, name):
    c = E.CASES[name]
    ratio = E.check_nonfinite(xcorr, name)
    print("xcorr-edge %-22s %-8s max err / mag %.3e over the finite outputs" % (name, E.kernel_of(c["rx"], c["rz"]), ratio))


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.ZERO_CASES)
def test_xcorr_zero_planes_and_templates_give_positive_zeros(xcorr, name):
    E.check_zeros(xcorr, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["range_30x15_p45", "range_35x7_p33", "range_45x15_p5", "nfzero_64x7_p7"])
def test_xcorr_is_deterministic(ops, name):
    x, z = (E.planted if E.CASES[name]["kind"] == "nfzero" else E.inputs)(name)
    x, z = x.to(DEV), z.to(DEV)
    a, b = ops.xcorr_depthwise(x, z), ops.xcorr_depthwise(x, z)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("rx,rz", [(30, 15), (35, 7), (20, 9), (1, 1)])
def test_xcorr_of_no_tracks(ops, rx, rz):
    out = ops.xcorr_depthwise(torch.zeros((0, 8, rx, rx), device=DEV), torch.zeros((0, 8, rz, rz), device=DEV))
    assert tuple(out.shape) == (0, 8, rx - rz + 1, rx - rz + 1) and out.dtype == torch.float32 and out.is_cuda


# ---- part C ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_generic_kernel_above_64_kib_of_lds(xcorr):
    """(128, 3): 65,572 B of dynamic LDS, the smallest square plane above the default limit of a launch; exact-grid data."""
    x, z = E.lds_inputs()
    ref = E.ref64(x, z)
    assert torch.equal(ref.float().double(), ref) and float(E.mag(x, z).max()) < 2 ** 10
    out = xcorr(x, z)
    assert tuple(out.shape) == (1, 1, 126, 126)
    assert torch.equal(out, ref.float()), "%d of %d outputs differ" % (int((out != ref.float()).sum()), out.numel())


@pytest.mark.gpu
def test_generic_kernel_refuses_a_plane_beyond_160_kib_and_goes_on(ops, xcorr):
    rx, rz = E.LDS_REFUSED
    with pytest.raises(RuntimeError, match="plane too large for LDS"):
        ops.xcorr_depthwise(torch.zeros((1, 1, rx, rx), device=DEV), torch.zeros((1, 1, rz, rz), device=DEV))
    E.check_exact(xcorr, "exact_20x9_p5")
    x, z = E.lds_inputs()
    assert torch.equal(xcorr(x, z), E.ref64(x, z).float())


# ---- the scalar predictor at the largest maps its entry guard admits (found by the (45, 15) head case) ----------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ho", [30, 31, 32])
def test_scalar_predictor_up_to_the_1024_positions_its_guard_admits(ops, ho):
    """``predictor_impl`` admits Ho^2 <= 1024; the heads kernel stages 16 haloed planes in LDS: 65,536 B at Ho = 30, 69,696 B
    at 31 and 73,984 B at 32, which a launch gets only after the opt-in.  Against O.predictor with the bounds of
    test_predictor_vs_oracle."""
    rs = np.random.RandomState(3100 + ho)
    params = gi.predictor_params(rs, 32, P.BOXES)
    resp = torch.from_numpy((rs.standard_normal((2, 32, ho, ho)) * 15.0).astype(np.float32))
    assert 16 * (ho + 2) ** 2 * 4 == {30: 65536, 31: 69696, 32: 73984}[ho]
    out = ops.emm_predictor(resp.to(DEV), {k: _dev(v) for k, v in params.items()}, gn_groups=E.GN_GROUPS).cpu()
    r64, r32, scale = E.predictor_refs(resp, params)
    e64, e32 = P.scaled_error(out, r64, scale), P.scaled_error(out, r32, scale)
    print("xcorr-edge predictor Ho %d (scalar kernels): vs fp64 %.3e  vs fp32 %.3e" % (ho, e64, e32))
    assert float(scale.min()) >= 1e-3 and e64 < P.TOL64 and e32 < P.TOL32, (e64, e32)


@pytest.mark.gpu
def test_predictor_refuses_more_than_1024_positions(ops):
    rs = np.random.RandomState(3133)
    params = {k: _dev(v) for k, v in gi.predictor_params(rs, 32, P.BOXES).items()}
    with pytest.raises(RuntimeError, match="Ho=33 too large"):
        ops.emm_predictor(torch.zeros((1, 32, 33, 33), device=DEV), params)


# =========================================================================================================================
# GPU, part B
# =========================================================================================================================
def _image(feats, b):
    return [f[b:b + 1] for f in feats]


_heads = {}


def _head(ops, name):
    """The product on image 0 of a case, stage by stage and in one call, computed once and shared by the tests below."""
    if name in _heads:
        return _heads[name]
    cfg, inp = E.head_cfg(name), E.head_inputs(name)
    fa3, fb3 = [_dev(f) for f in inp["features_a"]], [_dev(f) for f in inp["features_b"]]
    fa, fb = _image(fa3, 0), _image(fb3, 0)
    boxes = _dev(inp["boxes"])
    params = {k: _dev(v) for k, v in inp["params"].items()}
    pad_cells = [O.pad_cells(cfg.pad_pixels, i) for i in range(len(cfg.scales))]
    kw = dict(sigma=cfg.sigma, use_centerness=cfg.use_centerness, clip_wh=E.IMAGE_WH)
    h = dict(cfg=cfg, fa3=fa3, fb3=fb3, fa=fa, fb=fb, boxes=boxes, params=params, kw=kw)
    h["z1"], h["sr1"] = ops.emm_extract_cache(fa, boxes, cfg.rz, cfg.scales, cfg.sampling_ratio, cfg.pad_pixels,
                                              cfg.search_expansion, cfg.min_search_wh)
    h["z"] = ops.roi_align_levels(fa, boxes, boxes, cfg.rz, cfg.scales, cfg.sampling_ratio)
    h["sr"] = ops.search_region(boxes, cfg.pad_pixels, cfg.search_expansion, cfg.min_search_wh)
    h["x"] = ops.roi_align_levels(fb, h["sr"], boxes, cfg.rx, cfg.scales, cfg.sampling_ratio, pad_cells)
    h["resp"] = ops.xcorr_depthwise(h["x"], h["z"])
    h["logits"] = ops.emm_predictor(h["resp"], params, gn_groups=E.GN_GROUPS, gn_eps=E.GN_EPS)
    h["bb"], h["conf"], h["idx"] = ops.emm_decode(h["logits"], h["sr"], boxes, cfg.rx, cfg.rz, cfg.pad_pixels,
                                                  return_index=True, **kw)
    h["one"] = ops.emm_track(fb, boxes, h["sr"], h["z"], params, cfg.rx, cfg.rz, cfg.scales, cfg.sampling_ratio,
                             cfg.pad_pixels, gn_groups=E.GN_GROUPS, gn_eps=E.GN_EPS, return_index=True, **kw)
    torch.cuda.synchronize()
    _heads[name] = h
    return h


def _eq(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.HEAD_NAMES)
def test_general_path_one_call_equals_the_operator_composition(ops, name):
    """``emm_track`` = roi_align_levels -> xcorr_depthwise -> emm_predictor -> emm_decode and ``emm_extract_cache`` =
    roi_align_levels + search_region, bit for bit (test_one_call_entry_points_equal_operator_composition, off the fused
    family).  At Ho = 16 the one call decodes from the towers' partial sums and lets the predictor make the plane maxima."""
    h = _head(ops, name)
    assert _eq(h["z1"], h["z"]), "emm_extract_cache templates differ from roi_align_levels"
    assert _eq(h["sr1"], h["sr"]), "emm_extract_cache search regions differ from search_region"
    bb, conf, idx = h["one"]
    assert bool(torch.isfinite(bb).all()) and bool(torch.isfinite(conf).all())
    assert torch.equal(idx, h["idx"]), "cells %s vs %s" % (idx.tolist(), h["idx"].tolist())
    assert _eq(bb, h["bb"]) and _eq(conf, h["conf"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.HEAD_NAMES)
def test_general_path_module_equals_the_one_call_entry_points(ops, name, monkeypatch):
    """``siammot_amd.emm.EMM`` built for the shape: extract_cache and forward equal the ops calls; at Ho 16 / 29 both go
    through an ``ops.PairPlan`` (counted), elsewhere none is built."""
    from siammot_amd.config import get_default_cfg
    from siammot_amd.emm import EMM
    from siammot_amd.structures import BoxList
    from siammot_amd.track_utils import build_track_utils
    h = _head(ops, name)
    cfg = h["cfg"]
    rz, region, ratio, channels = E.HEAD_CASES[name]
    mc = get_default_cfg(channels=channels)
    th = mc.MODEL.TRACK_HEAD
    th.POOLER_RESOLUTION, th.SEARCH_REGION, th.POOLER_SAMPLING_RATIO = rz, region, ratio
    th.PAD_PIXELS, th.MINIMUM_SREACH_REGION, th.POOLER_SCALES = cfg.pad_pixels, cfg.min_search_wh, cfg.scales
    th.EMM.USE_CENTERNESS, th.EMM.COSINE_WINDOW_WEIGHT = cfg.use_centerness, cfg.sigma
    mc.INPUT.AMODAL = False
    emm = EMM(mc, build_track_utils(mc)).to(DEV).eval()
    emm.predictor.load_state_dict({k: torch.from_numpy(v) for k, v in E.head_inputs(name)["params"].items()})
    assert (emm.rx, emm.rz) == (cfg.rx, cfg.rz)
    calls = dict(plans=0, track=0, extract=0)
    init, track, extract = ops.PairPlan.__init__, ops.PairPlan.track, ops.PairPlan.extract

    def counted_init(self, *a, **k):
        init(self, *a, **k)
        calls["plans"] += 1

    def counted_track(self, *a, **k):
        out = track(self, *a, **k)
        calls["track"] += out is not None
        return out

    def counted_extract(self, *a, **k):
        out = extract(self, *a, **k)
        calls["extract"] += out is not None
        return out
    monkeypatch.setattr(ops.PairPlan, "__init__", counted_init)
    monkeypatch.setattr(ops.PairPlan, "track", counted_track)
    monkeypatch.setattr(ops.PairPlan, "extract", counted_extract)
    det = BoxList(h["boxes"], E.IMAGE_WH, mode="xyxy")
    det.add_field("ids", torch.arange(E.TRACKS, device=DEV))
    det.add_field("labels", torch.ones(E.TRACKS, dtype=torch.int64, device=DEV))
    with torch.no_grad():
        z, sr, det_out = emm.extract_cache(tuple(h["fa"]), det)
        _, result, _ = emm(tuple(h["fb"]), det_out, sr, template_features=z)
        z2, sr2, _ = emm.extract_cache(tuple(h["fa"]), det)                 # (the module plans its extraction after a forward)
    torch.cuda.synchronize()
    bb, conf, _ = h["one"]
    for zz, ss in ((z, sr), (z2, sr2)):
        assert _eq(zz, h["z"]) and _eq(ss[0].bbox, h["sr"])
    assert _eq(result[0].bbox, bb) and _eq(result[0].get_field("scores"), conf)
    if name in E.WINOGRAD_HEADS:
        assert calls == dict(plans=1, track=1, extract=1), calls
    else:
        assert calls == dict(plans=0, track=0, extract=0), calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.HEAD_NAMES)
def test_general_path_batched_equals_one_image_calls(ops, name):
    """Rows [2, 0, 4] over three images through ``emm_extract_cache_batched`` / ``emm_track_batched`` against one-image calls
    on each image's maps, bit for bit."""
    h = _head(ops, name)
    cfg, boxes, params, kw = h["cfg"], h["boxes"], h["params"], h["kw"]
    rows = list(E.BATCH_ROWS)
    ho = cfg.rx - cfg.rz + 1
    channels = E.HEAD_CASES[name][3]
    assert len({ops.tower_form(n, channels, ho) for n in rows + [E.TRACKS] if n}) == 1
    z, sr = ops.emm_extract_cache_batched(h["fa3"], boxes, rows, cfg.rz, cfg.scales, cfg.sampling_ratio, cfg.pad_pixels,
                                          cfg.search_expansion, cfg.min_search_wh)
    bb, conf, idx = ops.emm_track_batched(h["fb3"], boxes, sr, z, rows, params, cfg.rx, cfg.rz, cfg.scales,
                                          cfg.sampling_ratio, cfg.pad_pixels, gn_groups=E.GN_GROUPS, gn_eps=E.GN_EPS,
                                          return_index=True, **kw)
    torch.cuda.synchronize()
    assert _eq(sr, h["sr"])
    n0 = 0
    for b, r in enumerate(rows):
        if r:
            bx = boxes[n0:n0 + r].contiguous()
            z1, sr1 = ops.emm_extract_cache(_image(h["fa3"], b), bx, cfg.rz, cfg.scales, cfg.sampling_ratio, cfg.pad_pixels,
                                            cfg.search_expansion, cfg.min_search_wh)
            bb1, conf1, idx1 = ops.emm_track(_image(h["fb3"], b), bx, sr1, z1, params, cfg.rx, cfg.rz, cfg.scales,
                                             cfg.sampling_ratio, cfg.pad_pixels, gn_groups=E.GN_GROUPS, gn_eps=E.GN_EPS,
                                             return_index=True, **kw)
            torch.cuda.synchronize()
            assert _eq(z[n0:n0 + r], z1) and _eq(sr[n0:n0 + r], sr1), "image %d: extraction differs" % b
            assert torch.equal(idx[n0:n0 + r], idx1), "image %d: cells %s vs %s" % (b, idx[n0:n0 + r].tolist(), idx1.tolist())
            assert _eq(bb[n0:n0 + r], bb1) and _eq(conf[n0:n0 + r], conf1), "image %d: results differ" % b
        n0 += r
    assert _eq(z[:2], h["z"][:2])                                         # image 0's rows are the one-image case's first two


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.HEAD_NAMES)
def test_general_path_stages_against_the_oracle(ops, name):
    """Every stage against the oracle evaluated on the product's own previous stage: errors do not compound, only the
    decode can flip.  Measures and bounds are the project's existing ones."""
    _assert_close = E.assert_close
    h, orc, inp = _head(ops, name), E.head_oracle(name), E.head_inputs(name)
    cfg = h["cfg"]
    ho = cfg.rx - cfg.rz + 1
    channels = E.HEAD_CASES[name][3]
    if name in E.WINOGRAD_HEADS:          # generic correlation + Winograd towers (+ at Ho 16 the partial-sum decode), not the scalar kernels
        form = ops.tower_form(E.TRACKS, channels, ho)
        assert form in (1, 2, 3), "tower form %d: %s" % (form, ops.TOWER_FORMS.get(form))
        assert form == P.reported_form(E.TRACKS, channels, ho, True)
    # pooling
    fb = [torch.from_numpy(f[:1]) for f in inp["features_b"]]
    boxes = torch.from_numpy(inp["boxes"])
    _assert_close(h["z"], orc["f32"]["z"], 1e-5, 1e-5, name + ": templates vs O.extract_cache")
    assert torch.equal(h["sr"].cpu(), orc["f32"]["sr"]), name + ": search regions vs O.search_region"
    x_ref = O.sr_pool(O.pad_features(fb, cfg.pad_pixels), boxes, h["sr"].cpu(), cfg.rx, cfg.scales, cfg.sampling_ratio)
    _assert_close(h["x"], x_ref, 1e-5, 1e-5, name + ": search planes vs O.sr_pool of the padded maps")
    assert float(h["x"].abs().max()) > 0.1
    resp = h["resp"].cpu()
    # towers and heads on the product's own response
    r64, r32, scale = E.predictor_refs(resp, inp["params"])
    logits = h["logits"].cpu()
    e64, e32 = P.scaled_error(logits, r64, scale), P.scaled_error(logits, r32, scale)
    assert float(scale.min()) >= 1e-3
    # decode of the product's own logits
    lg = logits.numpy()
    d = dict(cls=lg[:, :2], center=lg[:, 2:3], reg=lg[:, 3:], boxes=inp["boxes"], sr=h["sr"].cpu().numpy())
    dorc = D.oracle_eval(d, E.decode_cfg(cfg), E.IMAGE_WH)
    verdicts = D.adjudicate(dorc, h["idx"].cpu().numpy())
    print("xcorr-edge head %-13s Ho %2d  logits vs fp64 %.3e  vs fp32 %.3e  decode identical %d / %d, "
          "excused %d, failed %d" % (name, ho, e64, e32, sum(v[0] == "same" for v in verdicts), len(verdicts),
                                     sum(v[0] == "excused" for v in verdicts), sum(v[0] == "fail" for v in verdicts)))
    assert e64 < P.TOL64, "%s: logits vs fp64 %.3e" % (name, e64)
    assert e32 < P.TOL32, "%s: logits vs fp32 %.3e" % (name, e32)
    E.judge(name, dorc, h["bb"].cpu().numpy(), h["conf"].cpu().numpy(), h["idx"].cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.HEAD_NAMES)
def test_general_path_response_against_ref64_of_the_pooled_planes(ops, name):
    """The response against ``ref64`` of the product's own pooled planes with the project's bound, 1e-6 * mag
    (test_hip_parity._xcorr_check), next to an emulation of the launched kernel's accumulation on the same planes.

    With ONE fmaf chain over all taps in the generic kernel [45_15] missed this bound: 1.062e-06 on the MI355X, and the
    same 1.062e-06 from the emulated chain on the same planes (1.057e-06 on the oracle's planes, which torch's fp32
    grouped convolution gives too; 8.3e-07 .. 1.03e-06 over seven other seeds).  The generic kernel accumulates per
    template row since."""
    h = _head(ops, name)
    x, z, resp = h["x"].cpu(), h["z"].cpu(), h["resp"].cpu()
    ref, m = E.ref64(x, z), E.mag(x, z)
    err = (resp.double() - ref).abs()
    live = m > 0
    ratio = float((err[live] / m[live]).max())
    generic = E.kernel_of(x.shape[-1], z.shape[-1]) == E.GENERIC
    chain = float(((E.fma_chain32(x, z, rows=generic).double() - ref).abs()[live] / m[live]).max())
    print("xcorr-edge head %-13s response max err / mag %.3e (the kernel's accumulation emulated on the CPU on the same planes: "
          "%.3e; a-priori bound %.3e)" % (name, ratio, chain, z.shape[-1] ** 2 * E.U24))
    assert bool(torch.isfinite(resp).all())
    assert float(resp[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0
    assert bool((err <= E.bound(x, z)).all()), "%s: response beyond the a-priori bound of the chain: %.3e" % (name, ratio)
    assert bool((err <= E.PROJECT_RATIO * m + 1e-30).all()), (
        "%s: response max err / mag %.3e, the emulated accumulation on the same planes %.3e" % (name, ratio, chain))
