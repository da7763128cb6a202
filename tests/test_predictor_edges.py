"""The predictor (csrc/predictor.hip ``predictor_impl`` and the tower kernels behind it) against the CPU oracle over group
sizes, channel counts and map sizes.  predictor_impl picks one of five kernel families from (C, Ho, C / gn_groups, packed
filters present) — Winograd 16 x 16 on two-part fp16 operands, the direct fp32 matrix-core tower, blocked Winograd for
29 x 29 (one tile fp32 or two tiles fp16 x 2), the direct 29 x 29 kernel, the scalar kernels — and every other predictor
test calls it with 32 groups, eps 1e-5 and gamma in [0.5, 1.5].

The inputs, the oracle's answers (computed once per case and shared) and the restated dispatch come from
tests/predictor_edge_cases.py.  Yardstick: ``oracle.emm_oracle.predictor`` on the CPU in fp64 and fp32.  Measure: the
project's own, max |out - ref| / max_channel |ref64| (test_hip_parity.test_predictor_vs_oracle).  Bounds: that test's, 1e-4
against fp64 and 2e-4 against fp32, for every family.  The CPU tests assert from the oracle alone what keeps those bounds
meaningful: every channel scale >= 1e-3, the fp32 oracle within 2e-5 of fp64, every case in the variance regime it is
named for.

What these tests found: for C % 32 == 0 that is no power of two (or above 512) at Ho = 29 the blocked launcher picks the
split form by workgroup count while the plane maxima it needs were provided by a predicate that knows powers of two only —
``emm_predictor(resp[1, 96, 29, 29], gn_groups=24)`` and the whole head at rx 35 / rz 7 failed with a bad-argument error;
and a refused shape (C = 64, 2 groups, Ho = 29) had the plane maxima written into its output buffer before the refusal.
Both are one predicate now (csrc/tower_wino.hip ``tower_split_form``).  Measured errors: INTEGRATION.md."""
import ctypes

import numpy as np
import pytest
import torch

import golden_inputs as gi
import predictor_edge_cases as E
from oracle import emm_oracle as O

DEV = "cuda:0"


# ---- CPU: the cases' conditions, from the oracle alone -------------------------------------------------------------------
@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_generated_case_meets_its_conditions(name):
    """Conditions on the INPUTS of this module.  If one fails, the seed is to be changed, not this test."""
    c, orc = E.CASES[name], E.oracle(name)
    assert 1 <= c["n"] <= 9 and c["c"] % c["groups"] == 0
    assert float(orc["scale"].min()) >= 1e-3, "an output channel's fp64 scale is %.3e" % float(orc["scale"].min())
    e = E.scaled_error(orc["ref32"], orc["ref64"], orc["scale"])
    assert e <= 2e-5, "fp32 oracle vs fp64: %.3e" % e
    var = E.group_variances(name)
    if c["variant"] == "zerotrack":
        assert float(var[E.ZERO_TRACK].max()) == 0.0
        var = var[[k for k in range(c["n"]) if k != E.ZERO_TRACK]]
    if c["variant"] == "eps1":
        assert c["eps"] == 1.0 and float(var.max()) < c["eps"], "largest group variance %.3e" % float(var.max())
    else:
        assert float(var.min()) > 100 * c["eps"], "smallest group variance %.3e" % float(var.min())
    if c["variant"] == "affine":
        _, params = E.inputs(name)
        for t in ("cls_tower", "reg_tower"):
            ga = params[t + ".1.weight"].reshape(c["groups"], c["cpg"])
            assert ((ga == 0).any(1) & (ga < 0).any(1) & (ga > 0).any(1)).all()      # mixed within EVERY group
            assert float(params[t + ".1.bias"].std()) > 2.0
    if c["tiles"] is not None:
        assert c["ho"] == 29 and E.blocked_tiles(c["n"], c["c"]) == c["tiles"]


def test_cases_cover_the_families_group_sizes_and_loops():
    runs = [(E.family(c["c"], c["groups"], c["ho"], w), c) for name, w in E.RUNS for c in (E.CASES[name],)]
    for fam in E.MATRIX_FAMILIES:
        assert {c["cpg"] for f, c in runs if f == fam} == set(E.MATRIX_CPG), fam
    # the 16 x 16 epilogue: the read-lane path (cpg 4) with the generic K loop, the LDS path with the unrolled one (C = 128)
    w16 = [c for f, c in runs if f == "wino16"]
    assert any(c["cpg"] == 4 and c["c"] == 64 for c in w16)
    assert {c["cpg"] for c in w16 if c["c"] == 128} >= {1, 2, 8, 16}
    assert {c["cpg"] for c in w16 if c["c"] != 128} >= {1, 4, 8, 16}
    assert {c["n"] for c in w16 if c["c"] == 512} == {1, 2}
    # blocked Winograd: both forms at every group size, at a C that is no power of two, and above 512
    w29 = [c for f, c in runs if f == "wino29"]
    for tiles in (1, 2):
        assert {c["cpg"] for c in w29 if E.blocked_tiles(c["n"], c["c"]) == tiles} == set(E.MATRIX_CPG)
        assert any(c["c"] & (c["c"] - 1) for c in w29 if E.blocked_tiles(c["n"], c["c"]) == tiles)
    assert (E.blocked_tiles(8, 64), E.blocked_tiles(9, 64), E.blocked_tiles(1, 96), E.blocked_tiles(9, 96)) == (1, 2, 2, 1)
    assert any(c["c"] > 512 for c in w29) and any(c["c"] == 512 for c in w29)
    assert {c["c"] for f, c in runs if f == "direct29" and c["c"] % 32} == {16, 48}
    sc = [c for f, c in runs if f == "scalar"]
    assert {c["cpg"] for c in sc} >= {3, 6, 32} and {c["ho"] for c in sc} >= {1, 2, 15, 16, 17}
    # the odd K-block count (C / 32 = 3, 5: one block per trip) and the even ones of the split form's generic loop
    split = [c["c"] // 32 for c in w29 if E.blocked_tiles(c["n"], c["c"]) == 2]
    assert {3, 5, 6, 18} <= set(split)
    assert {E.family(c, g, ho, w) for c, g, ho, _, w in E.MEMBERSHIP} == set(E.MATRIX_FAMILIES)
    assert {c // g for c, g, *_ in E.MEMBERSHIP} == {1, 4, 16}


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _dev_params(params):
    return {k: _dev(v) for k, v in params.items()}


_outputs = {}


def _run(ops, name, winograd):
    """The product's logits of a case (on the CPU), computed once per (case, form) and shared by the tests below."""
    key = (name, winograd)
    if key not in _outputs:
        c = E.CASES[name]
        resp, params = E.inputs(name)
        out = ops.emm_predictor(_dev(resp), _dev_params(params), gn_groups=c["groups"], gn_eps=c["eps"], winograd=winograd)
        torch.cuda.synchronize()
        _outputs[key] = out.cpu()
    return _outputs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name,winograd", E.RUNS)
def test_predictor_edge_case_against_the_oracle(ops, name, winograd):
    c, orc = E.CASES[name], E.oracle(name)
    want = E.reported_form(c["n"], c["c"], c["ho"], winograd)
    if want is not None:
        assert ops.tower_form(c["n"], c["c"], c["ho"]) == want
    out = _run(ops, name, winograd)
    assert tuple(out.shape) == (c["n"], 7, c["ho"], c["ho"]) and bool(torch.isfinite(out).all())
    e64 = E.scaled_error(out, orc["ref64"], orc["scale"])
    e32 = E.scaled_error(out, orc["ref32"], orc["scale"])
    print("predictor-edge %-28s %-8s cpg %2d  vs fp64 %.3e  vs fp32 %.3e" % (
        name, E.family(c["c"], c["groups"], c["ho"], winograd), c["cpg"], e64, e32))
    assert e64 < E.TOL64, "%s (winograd=%s): max scaled err vs fp64 %.3e" % (name, winograd, e64)
    assert e32 < E.TOL32, "%s (winograd=%s): max scaled err vs fp32 %.3e" % (name, winograd, e32)
    if c["variant"] == "zerotrack":                       # a zero track is relu(beta) through the heads, whatever its neighbours
        alone = ops.emm_predictor(_dev(E.inputs(name)[0][E.ZERO_TRACK:E.ZERO_TRACK + 1]), _dev_params(E.inputs(name)[1]),
                                  gn_groups=c["groups"], gn_eps=c["eps"], winograd=winograd).cpu()
        if E.family(c["c"], c["groups"], c["ho"], winograd) != "wino29":     # (the blocked form's tiles depend on N)
            assert torch.equal(alone[0], out[E.ZERO_TRACK])


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.PAIRS)
def test_winograd_and_direct_forms_agree(ops, name):
    """Where a Winograd and a direct form exist they differ in rounding order only: the project's existing bounds, 2e-5 at
    16 x 16 (test_tower_pack_cache_follows_the_weights) and 5e-5 at 29 x 29 (test_blocked_winograd_towers_...), relative to
    the channel scale of the direct result."""
    c = E.CASES[name]
    wino, direct = _run(ops, name, True), _run(ops, name, False)
    scale = direct.abs().amax(dim=(0, 2, 3), keepdim=True)
    err = float(((wino - direct).abs() / scale).max())
    print("predictor-edge %-28s winograd vs direct %.3e" % (name, err))
    assert err < E.AGREE[c["ho"]], "%s: %.3e" % (name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.SPLIT_CASES)
def test_split_form_keeps_the_fp32_forms_accuracy_at_the_new_group_sizes(ops, name):
    """The existing relation of test_tower_two_tile_workgroups_equal_one_tile_workgroups, against fp64:
    e_split <= 1.25 e_fp32form + 2e-7, the fp32 form being the measurement library's SMOT_TOWER_OCT=2, SMOT_TOWER_BF3=0."""
    c, orc = E.CASES[name], E.oracle(name)
    resp, params = E.inputs(name)
    resp, params = _dev(resp), _dev_params(params)
    with ops.debug_library(SMOT_TOWER_OCT=2, SMOT_TOWER_BF3=0):
        f32 = ops.emm_predictor(resp, params, gn_groups=c["groups"], gn_eps=c["eps"]).cpu()
    with ops.debug_library(SMOT_TOWER_OCT=2, SMOT_TOWER_BF3=1):
        runs = [ops.emm_predictor(resp, params, gn_groups=c["groups"], gn_eps=c["eps"]).cpu() for _ in range(2)]
    assert torch.equal(runs[0], runs[1]), "%s: the split form differs between launches" % name
    if c["ho"] == 16 or E.blocked_tiles(c["n"], c["c"]) == 2:
        assert torch.equal(runs[0], _run(ops, name, True)), "%s: the product does not compute the split form" % name
    e_split = E.scaled_error(runs[0], orc["ref64"], orc["scale"])
    e_f32 = E.scaled_error(f32, orc["ref64"], orc["scale"])
    print("predictor-edge %-28s split %.3e  fp32 form %.3e" % (name, e_split, e_f32))
    assert e_split <= 1.25 * e_f32 + 2e-7, "%s: split form %.3e vs fp32 form %.3e" % (name, e_split, e_f32)


@pytest.mark.gpu
@pytest.mark.parametrize("tower", [0, 1])
@pytest.mark.parametrize("c,groups,ho,grp,winograd", E.MEMBERSHIP)
def test_group_membership_is_exact(ops, c, groups, ho, grp, winograd, tower):
    """With the heads reading group ``grp`` of one tower only, negating the tower filter of the channel just below or just
    above the group must leave that tower's logits value-equal (a group's statistics see its own channels only), and
    negating the group's first or last channel must change them."""
    resp, base, variants = E.membership_inputs(c, groups, ho, grp, tower)
    resp = _dev(resp)
    ch = slice(0, 3) if tower == 0 else slice(3, 7)

    def run(p):
        return ops.emm_predictor(resp, _dev_params(p), gn_groups=groups, winograd=winograd)[:, ch].cpu()
    ref = run(base)
    assert bool(torch.isfinite(ref).all()) and float(ref.std()) > 0
    for k in ("below", "above"):
        got = run(variants[k])
        assert torch.equal(got, ref), "%s: a channel %s group %d moved the group's logits by %.3e" % (
            E.family(c, groups, ho, winograd), k, grp, float((got - ref).abs().max()))
    for k in ("first", "last"):
        assert not torch.equal(run(variants[k]), ref), "the group's %s channel does not reach its logits" % k


# ---- the whole head and the module -----------------------------------------------------------------------------------------
def _head_case(family_name, channels, n):
    case = dict(gi.EMM_CASES[family_name], channels=channels)
    cfg = O.EMMConfig(channels=channels, rz=case["rz"], search_region=case["search_region"], scales=case["scales"],
                      pad_pixels=case["pad_pixels"], min_search_wh=case["min_search_wh"],
                      use_centerness=case["use_centerness"], sigma=case["sigma"], amodal=case["amodal"])
    rs = np.random.RandomState(9000 + channels)
    shapes = gi.feature_shapes(case["image_wh"], channels)
    feats_a = [_dev(rs.standard_normal(s)) for s in shapes]
    feats_b = [_dev(rs.standard_normal(s)) for s in shapes]
    boxes = np.array(case["boxes"][:n], dtype=np.float32)
    params = _dev_params(gi.predictor_params(rs, channels, boxes))
    return case, cfg, feats_a, feats_b, _dev(boxes), params


@pytest.mark.gpu
@pytest.mark.parametrize("family_name,channels,groups,n", [("default", 64, 4, 4), ("default", 128, 8, 4), ("aot", 96, 24, 2)])
def test_one_call_head_equals_the_operator_composition_at_other_group_counts(ops, family_name, channels, groups, n):
    """``emm_track(..., gn_groups=g)`` against pooling + correlation -> ``emm_predictor(gn_groups=g)`` -> ``emm_decode``, bit
    for bit (the form of test_one_call_entry_points_equal_operator_composition).  C = 96 with 24 groups at rx 35 / rz 7 and
    two tracks launches the split form of the blocked towers: the one-call path gets the plane maxima from the pooling +
    correlation kernel, the stand-alone operator makes them itself."""
    case, cfg, feats_a, feats_b, boxes, params = _head_case(family_name, channels, n)
    assert (cfg.rx, cfg.rz) == ((30, 15) if family_name == "default" else (35, 7))
    z, sr = ops.emm_extract_cache(feats_a, boxes, cfg.rz, cfg.scales, cfg.sampling_ratio, cfg.pad_pixels,
                                  cfg.search_expansion, cfg.min_search_wh)
    clip = None if case["amodal"] else case["image_wh"]
    bb, conf, idx = ops.emm_track(feats_b, boxes, sr, z, params, cfg.rx, cfg.rz, cfg.scales, cfg.sampling_ratio,
                                  cfg.pad_pixels, sigma=cfg.sigma, use_centerness=cfg.use_centerness, clip_wh=clip,
                                  gn_groups=groups, return_index=True)
    resp = ops.sr_xcorr_fused(feats_b, boxes, sr, z, cfg.rx, cfg.rz, cfg.scales, cfg.sampling_ratio, cfg.pad_pixels)
    logits = ops.emm_predictor(resp, params, gn_groups=groups)
    bb2, conf2, idx2 = ops.emm_decode(logits, sr, boxes, cfg.rx, cfg.rz, cfg.pad_pixels, sigma=cfg.sigma,
                                      use_centerness=cfg.use_centerness, return_index=True, clip_wh=clip)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bb).all()) and bool(torch.isfinite(conf).all())
    assert torch.equal(idx, idx2) and torch.equal(bb, bb2) and torch.equal(conf, conf2), "cells %s vs %s" % (
        idx.tolist(), idx2.tolist())
    # ... and the group count reaches the towers: the logits are the oracle's for this count, not for the default's
    cpu = {k: v.cpu().double() for k, v in params.items()}
    ref = torch.cat(O.predictor(resp.cpu().double(), cpu, groups, 1e-5), 1)
    scale = ref.abs().amax(dim=(0, 2, 3), keepdim=True)
    assert E.scaled_error(logits.cpu(), ref, scale) < E.TOL64
    if family_name == "default":
        other = torch.cat(O.predictor(resp.cpu().double(), cpu, 32, 1e-5), 1)
        assert E.scaled_error(other, ref, scale) > 100 * E.TOL64


@pytest.mark.gpu
def test_predictor_module_passes_its_group_count_through(ops):
    """``EMMPredictor`` built from a config with MODEL.GROUP_NORM.NUM_GROUPS = 16 computes 16-group towers."""
    from siammot_amd.config import get_default_cfg
    from siammot_amd.emm import EMMPredictor
    cfg = get_default_cfg(channels=64)
    cfg.MODEL.GROUP_NORM.NUM_GROUPS = 16
    pred = EMMPredictor(cfg).to(DEV).eval()
    assert pred.gn_groups == 16 and pred.cls_tower[1].num_groups == 16
    rs = np.random.RandomState(516)
    params = gi.predictor_params(rs, 64, E.BOXES)
    pred.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    resp = (rs.standard_normal((2, 64, 16, 16)) * 15.0).astype(np.float32)
    with torch.no_grad():
        got = torch.cat(pred(_dev(resp)), 1).cpu()
    p64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
    ref = torch.cat(O.predictor(torch.from_numpy(resp).double(), p64, 16, 1e-5), 1)
    scale = ref.abs().amax(dim=(0, 2, 3), keepdim=True)
    assert E.scaled_error(got, ref, scale) < E.TOL64
    assert E.scaled_error(torch.cat(O.predictor(torch.from_numpy(resp).double(), p64, 32, 1e-5), 1), ref, scale) > 100 * E.TOL64


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_predictor_refuses_a_group_its_scalar_kernel_cannot_hold_and_writes_nothing(ops):
    """C = 64 with 2 groups at Ho = 29: cpg = 32 is no matrix-core shape and 32 x 841 floats exceed the scalar kernel's
    64 KiB group buffer.  The binding raises, the C entry point returns an error and leaves the output buffer untouched
    (no plane maxima written ahead of a launch that never comes), and the next call works."""
    rs = np.random.RandomState(6429)
    params = _dev_params(gi.predictor_params(rs, 64, E.BOXES))
    n = 9                                       # (a track count at which C = 64 with an admissible cpg takes the split form)
    assert E.blocked_tiles(n, 64) == 2
    resp = _dev(rs.standard_normal((n, 64, 29, 29)) * 15.0)
    with pytest.raises(RuntimeError, match="GroupNorm group too large"):
        ops.emm_predictor(resp, params, gn_groups=2)
    lib = ops.load_library()
    sentinel = -12345.5
    logits = torch.full((n, 7, 29, 29), sentinel, device=DEV)
    tower_ws = torch.empty((n, 128, 29, 29), device=DEV)
    packed = ops.tower_packed(params)
    assert packed is not None
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                                       # noqa: E731
    rc = lib.smot_emm_predictor_fwd(ptr(resp), n, 64, 29, *[ptr(params[k]) for k in ops.PREDICTOR_KEYS], 2, 1e-5,
                                    ptr(packed), ptr(tower_ws), ptr(logits),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and b"GroupNorm group too large" in lib.smot_last_error()
    assert bool((logits == sentinel).all()), "%d words of the refused call's output buffer were written" % int(
        (logits != sentinel).sum())
    out = ops.emm_predictor(resp, params, gn_groups=4).cpu()
    ref = torch.cat(O.predictor(resp.cpu().double(), {k: v.cpu().double() for k, v in params.items()}, 4, 1e-5), 1)
    assert E.scaled_error(out, ref, ref.abs().amax(dim=(0, 2, 3), keepdim=True)) < E.TOL64
