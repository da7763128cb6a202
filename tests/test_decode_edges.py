"""The decode kernel (csrc/decode.hip, K4) against the CPU oracle where its scores leave [0, 1] and at the edges of its
geometry.  Every other decode test feeds strictly positive regression logits, so no score it has seen exceeds 1; the
reference's formula has no such bound: a ReLU'd regression head leaves exact zeros, bicubic overshoot next to them makes
a size ratio negative and the scale penalty exp(0.1 * (1 - s_w * s_h)) unbounded — scores of 1e30, +inf and NaN.  The
kernel promises the arg-max of the exactly evaluated score map for ALL inputs; here it is held to that.

The inputs, the oracle's answers (computed once per case and shared) and the adjudication rule come from
tests/decode_edge_cases.py.  The rule, for every GPU test of this module (``_judge``): a track passes when the kernel's
cell is the fp32 oracle's arg-max (NaN largest, first index wins), or when the oracle's score of the kernel's cell is
within 2 ulp of the oracle's maximum — the libm allowance between torch-CPU and device expf that
test_decode_near_ties_elect_the_exact_argmax uses; for a +inf / NaN maximum the cell must be +inf / NaN itself or sit on
the overflow border (exponent argument within 2^-22 relative of ln FLT_MAX, in fp64), and a later index than the
oracle's is admitted only when every earlier +inf / NaN cell sits on that border.  Tracks passing by the second clause
are EXCUSED, and at most 1 track in 10 of a case may be.  Where the index is the oracle's, boxes agree within 2e-2 px
and confidences within 1e-5 (non-finite values by class).  The CPU tests assert from the oracle alone what keeps that
cap honest: no accidental 2-ulp ties, and every case in the regime it is named for.

What the kernel does about such bands, and the state of the measurements: csrc/decode.hip (DEC_TOL), DESIGN.md §3 K4."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_edge_cases as E
import golden_inputs as gi
from oracle import emm_oracle as O

DEV = "cuda:0"
BOX_ATOL, CONF_ATOL = 2e-2, 1e-5          # the bounds of test_hip_parity._check_decode


# ---- CPU: the generator's conditions, the rule itself, the oracle's up-sampling at the new sizes -------------------
def _tops(orc):
    return orc["score"][np.arange(orc["score"].shape[0]), orc["idx"]]


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_generated_case_is_in_its_regime_and_free_of_accidental_ties(name):
    """Conditions on the INPUTS of this module, from the oracle alone.  If one fails the generator (its seeds) is to be
    changed, not this test."""
    c, orc = E.cases()[name], E.oracle(name)
    s, top = orc["score"], _tops(orc)
    n = s.shape[0]
    assert n <= 48
    # torch.argmax on CPU is what the rule says it is, and the oracle's own cells pass the rule un-excused
    assert np.array_equal(orc["idx"], orc["idx_torch"])
    assert all(v == ("same", 0.0) for v in E.adjudicate(orc, orc["idx"]))
    # no two FINITE cells within 2 ulp of a maximum: an excused track is then a kernel that missed, not a coin toss
    if not c["tie"]:
        near = [E.near_max_cells(orc, k) for k in range(n)]
        assert max(near) <= 1, "%s: tracks with several cells within %g ulp of the maximum: %s" % (name, E.ULPS, near)
    ho = c["d"]["cls"].shape[-1]
    inf_max, nan_max = int(np.isposinf(top).sum()), int(np.isnan(top).sum())
    inf_cells = np.isposinf(s).sum(1)
    with np.errstate(invalid="ignore"):
        above_one = int((top > 1).sum())
    if c["family"] == "sparse":
        share = float((c["d"]["reg"] == 0).mean())
        assert abs(share - {"sparse_25": 0.25, "sparse_75": 0.75}.get(name, 0.5)) < 0.02
    if name == "sparse_25":
        assert above_one >= 10 and np.isfinite(top).any()
    if name == "sparse_50":
        assert n == 24 and above_one >= 20 and inf_max >= 5
    if name == "sparse_75":
        assert n == 24 and int(inf_cells.min()) >= 2
    if name == "sparse_50_n48":
        assert n * (ho + 1) > 768 and inf_max >= 5 and np.isfinite(top).sum() >= 5          # the product picks SPLIT = 1
    if name == "sparse_50_ho29":
        assert (n, ho, orc["G"]) == (8, 29, 464) and not c["cfg"]["use_centerness"] and above_one + nan_max == n
    if c["family"] == "flat":
        sh = int(name.split("_")[1][2:])
        expect = 0.25 * np.exp(0.1 * (1 + sh)) * (1 - c["cfg"]["sigma"])
        assert np.isfinite(s).all() and np.all(np.abs(top / expect - 1) < 0.05)             # 45, 3e12, 3e29 (x 0.6)
        crowd = [E.near_max_cells(orc, k, 200) for k in range(n)]
        assert min(crowd) >= 10, crowd                              # a ranking off by 200 ulp has 10+ wrong cells to elect
        assert max(E.near_max_cells(orc, k, 6) for k in range(n)) == 1                        # ... and one right one
    if name == "sat_cls_x40":
        assert int(np.isnan(s).any(1).sum()) >= 1 and inf_max >= 1
    if name == "sat_cls_inf_rows":
        assert nan_max == n and np.isinf(c["d"]["cls"]).any()
    if name == "sat_reg_plane_zero":
        assert not c["d"]["reg"][:, (0, 2)].any() and int(inf_cells.min()) >= 2
    if name == "sat_window_only":
        assert c["cfg"]["sigma"] == 1.0 and nan_max == n
    if name == "sat_degenerate_boxes":
        w, h = c["d"]["boxes"][:, 2] - c["d"]["boxes"][:, 0], c["d"]["boxes"][:, 3] - c["d"]["boxes"][:, 1]
        assert (w == 0).any() and (h == 0).any() and (w < 0).any() and (h < 0).any()
    if c["family"] == "geometry":
        assert orc["G"] == 16 * ho and np.isfinite(s).all() and float(np.nanmax(top)) < 2.0      # in regime


def test_geometry_sweep_covers_the_kernel_paths():
    geo = [c for c in E.cases().values() if c["family"] == "geometry"]
    assert sorted(c["d"]["cls"].shape[-1] for c in geo) == [1, 2, 3, 5, 17, 32, 33, 46]
    assert {c["cfg"]["rz"] for c in geo} == {1, 3, 15}
    assert {c["cfg"]["use_centerness"] for c in geo} == {True, False}
    assert {c["cfg"]["sigma"] for c in geo} == {0.0, 0.1, 0.4}
    assert all(c["cfg"]["rx"] - c["cfg"]["rz"] + 1 == c["d"]["cls"].shape[-1] and 2 <= len(c["d"]["boxes"]) <= 4 for c in geo)
    # the largest map the LDS guard admits, and the first it refuses (csrc/decode.hip: 7 Ho^2 floats + DEC_STATIC_LDS)
    assert 7 * 46 * 46 * 4 + 6144 <= 65536 < 7 * 47 * 47 * 4 + 6144
    # clipping: over the clipped cases the oracle's unclipped boxes leave the image on every side
    W, H = E.IMAGE_WH
    out = np.zeros(4, int)
    for name, c in E.cases().items():
        if c["clip_wh"] is not None:
            b = E.oracle(name)["bb_raw"]
            out += [(b[:, 0] < 0).sum(), (b[:, 1] < 0).sum(), (b[:, 2] > W - 1).sum(), (b[:, 3] > H - 1).sum()]
    assert (out > 0).all(), out


def test_adjudication_rule_on_hand_made_maps():
    """The rule itself: what it admits and what it must refuse."""
    one = np.float32(1024.0)
    ulp = np.float32(2.0 ** -13)                                # 1024 * 2^-23, the unit of the rule (two fp32 steps below 1024)
    s = np.array([[one - 2 * ulp, one, one - 3 * ulp, 0.5, -np.inf]], np.float32)   # cell 0: 2 ulp below, cell 2: 3 ulp
    assert s[0, 0] < s[0, 1] and s[0, 2] < s[0, 0]
    orc = dict(score=s, idx=E.first_argmax(s), borderline=np.zeros_like(s, bool))
    assert orc["idx"].tolist() == [1]
    assert [E.adjudicate(orc, [k])[0][0] for k in range(5)] == ["excused", "same", "fail", "fail", "fail"]
    assert E.adjudicate(orc, [7])[0][0] == "fail" and E.adjudicate(orc, [-1])[0][0] == "fail"
    inf = np.float32(np.inf)
    s = np.array([[1e30, inf, 3.0, inf, 3.3e38]], np.float32)  # first +inf wins
    orc = dict(score=s, idx=E.first_argmax(s), borderline=np.zeros_like(s, bool))
    assert orc["idx"].tolist() == [1]
    assert [E.adjudicate(orc, [k])[0][0] for k in range(5)] == ["fail", "same", "fail", "fail", "fail"]
    orc["borderline"][0, 1] = True                              # the oracle's cell may be finite on the device: the next +inf
    assert [E.adjudicate(orc, [k])[0][0] for k in range(5)] == ["fail", "same", "fail", "excused", "fail"]
    orc["borderline"][0, (1, 4)] = False, True                  # a finite cell on the border may be +inf on the device ...
    assert E.adjudicate(orc, [4])[0][0] == "fail"               # ... but not behind an earlier +inf that is not
    s = np.array([[0.5, np.nan, inf, np.nan]], np.float32)      # NaN above +inf, first NaN wins
    orc = dict(score=s, idx=E.first_argmax(s), borderline=np.zeros_like(s, bool))
    assert orc["idx"].tolist() == [1]
    assert [E.adjudicate(orc, [k])[0][0] for k in range(4)] == ["fail", "same", "fail", "fail"]
    assert E.same_class_close([1.0, np.nan, np.inf, -np.inf, np.inf, 1.0, np.nan], [1.01, np.nan, np.inf, -np.inf, -np.inf, 1.03, 1.0],
                              2e-2).tolist() == [True, True, True, True, False, False, False]


def test_bicubic_restatement_equals_torch_interpolate_at_the_new_sizes():
    """The oracle's up-sampling has only been pinned at Ho = 16 and 29 (tests/test_oracle_golden.py)."""
    rs = np.random.RandomState(6)
    for ho in (1, 2, 3, 5, 46):
        x = torch.from_numpy(rs.standard_normal((2, 3, ho, ho))).double()
        ref = F.interpolate(x, scale_factor=16, mode="bicubic")
        assert tuple(ref.shape[-2:]) == (16 * ho, 16 * ho)
        assert (O.bicubic_upsample(x) - ref).abs().max() < 1e-12


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _decode(ops, c):
    d, cfg = c["d"], c["cfg"]
    logits = _dev(np.concatenate((d["cls"], d["center"], d["reg"]), 1))
    return ops.emm_decode(logits, _dev(d["sr"]), _dev(d["boxes"]), cfg["rx"], cfg["rz"], cfg["pad_pixels"],
                          sigma=cfg["sigma"], use_centerness=cfg["use_centerness"], return_index=True, clip_wh=c["clip_wh"])


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _bit_equal(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _judge(what, orc, bb, conf, idx, ms=None):
    """THE adjudication of this module (see the module docstring)."""
    bb, conf, idx = bb.cpu().numpy(), conf.cpu().numpy(), idx.cpu().numpy()
    verdicts = E.adjudicate(orc, idx)
    same = np.array([v[0] == "same" for v in verdicts])
    excused = ["track %d: %s" % (k, v[1]) for k, v in enumerate(verdicts) if v[0] == "excused"]
    failed = ["track %d: %s" % (k, v[1]) for k, v in enumerate(verdicts) if v[0] == "fail"]
    print("decode-edge %-22s identical %d / %d, excused %d, failed %d%s%s" % (
        what, same.sum(), len(same), len(excused), len(failed), "" if ms is None else ", %.2f ms" % ms,
        "".join("\n    excused " + e for e in excused) + "".join("\n    FAILED " + e for e in failed)))
    assert not failed, "%s: %d / %d tracks elect a cell the rule does not admit:\n  %s\nexcused:\n  %s" % (
        what, len(failed), len(same), "\n  ".join(failed), "\n  ".join(excused) or "-")
    assert len(excused) <= len(same) // E.EXCUSED_PER_TRACKS, "%s: %d of %d tracks excused (at most 1 in %d):\n  %s" % (
        what, len(excused), len(same), E.EXCUSED_PER_TRACKS, "\n  ".join(excused))
    ok_b = E.same_class_close(bb[same], orc["bb"][same], BOX_ATOL)
    ok_c = E.same_class_close(conf[same], orc["conf"][same], CONF_ATOL)
    assert ok_b.all(), "%s: boxes of identical cells differ (> %g px or another class):\n%s\nvs oracle\n%s" % (
        what, BOX_ATOL, bb[same][~ok_b.all(1)], orc["bb"][same][~ok_b.all(1)])
    assert ok_c.all(), "%s: confidences differ: %s vs oracle %s" % (what, conf[same][~ok_c], orc["conf"][same][~ok_c])
    return int(same.sum()), len(excused)


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_decode_edge_case_against_the_oracle(ops, name):
    c = E.cases()[name]
    orc = E.oracle(name)
    _decode(ops, c)                                              # (first call of a shape: workspace and window allocation)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bb, conf, idx = _decode(ops, c)
    torch.cuda.synchronize()
    _judge(name, orc, bb, conf, idx, (time.perf_counter() - t0) * 1e3)


@pytest.mark.gpu
def test_decode_refuses_what_its_lds_and_grid_cannot_hold(ops):
    """Ho = 47 (7 Ho^2 floats + the static arrays exceed 64 KiB) and an even rz are refused with a message, before any
    launch: the outputs of the refused call do not exist, the next call works."""
    c = E.cases()["geo_ho2_rz3"]
    d = c["d"]
    with pytest.raises(RuntimeError, match="Ho=47 too large for LDS"):
        ops.emm_decode(torch.zeros((1, 7, 47, 47), device=DEV), _dev(d["sr"][:1]), _dev(d["boxes"][:1]), 49, 3, 512)
    with pytest.raises(RuntimeError, match="odd rz"):
        ops.emm_decode(torch.zeros((1, 7, 16, 16), device=DEV), _dev(d["sr"][:1]), _dev(d["boxes"][:1]), 31, 16, 512)
    with pytest.raises(RuntimeError, match="Ho == rx-rz\\+1"):
        ops.emm_decode(torch.zeros((1, 7, 16, 16), device=DEV), _dev(d["sr"][:1]), _dev(d["boxes"][:1]), 30, 13, 512)
    torch.cuda.synchronize()
    _judge("after refusals", E.oracle("geo_ho2_rz3"), *_decode(ops, c))


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.FORM_CASES)
def test_decode_forms_agree_bit_for_bit(ops, name):
    """One, two and four thread groups per band (the product picks by N and G) elect the same cell and report the same
    bits, three calls in a row reuse the self-resetting tickets, and the band + finalize structure of the measurement
    library reports the same bits wherever it elects the same cell."""
    c = E.cases()[name]
    outs = [_decode(ops, c) for _ in range(3)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert _bit_equal(o, outs[0]), "%s: repeated product calls differ" % name
    for split in (1, 2, 4):
        with ops.debug_library(SMOT_DECODE_SPLIT=split):
            got = _decode(ops, c)
            torch.cuda.synchronize()
        assert _bit_equal(got, outs[0]), "%s: SPLIT = %d differs from the product: cells %s vs %s" % (
            name, split, got[2].tolist(), outs[0][2].tolist())
    with ops.debug_library(SMOT_DECODE_2PASS=1):
        ref = _decode(ops, c)
        torch.cuda.synchronize()
    same = outs[0][2] == ref[2]
    print("decode-edge %-22s two-pass structure elects the same cell on %d / %d tracks" % (name, int(same.sum()), len(same)))
    assert _bit_equal((outs[0][0][same], outs[0][1][same]), (ref[0][same], ref[1][same]))
    _judge(name + " (forms)", E.oracle(name), *outs[0])


@pytest.mark.gpu
def test_decode_through_the_towers_with_a_relu_sparse_regression_head(ops):
    """The one-call path feeds the decode from the tower kernel's partial sums and applies the ReLU itself
    (LogitSrc::combine).  test_one_call_entry_points_equal_operator_composition with a regression head whose bias no
    longer dominates: about half of the reg logits are exact zeros, the scores leave [0, 1]."""
    case = gi.EMM_CASES["default"]
    cfg = O.EMMConfig(channels=case["channels"], rz=case["rz"], search_region=case["search_region"], scales=case["scales"],
                      pad_pixels=case["pad_pixels"], min_search_wh=case["min_search_wh"],
                      use_centerness=case["use_centerness"], sigma=case["sigma"], amodal=case["amodal"])
    inp = gi.emm_case_inputs("default")
    feats_a = [_dev(f) for f in inp["features_a"]]
    feats_b = [_dev(f) for f in inp["features_b"]]
    boxes = _dev(inp["boxes"])
    z, sr = ops.emm_extract_cache(feats_a, boxes, cfg.rz, cfg.scales, cfg.sampling_ratio, cfg.pad_pixels,
                                  cfg.search_expansion, cfg.min_search_wh)
    resp = ops.sr_xcorr_fused(feats_b, boxes, sr, z, cfg.rx, cfg.rz, cfg.scales, cfg.sampling_ratio, cfg.pad_pixels)
    # reg.bias lowered from half a box side to zero, reg.weight scaled so that the surviving logits are box-sized again
    params = dict(inp["params"])
    params["reg.bias"] = np.zeros(4, np.float32)
    spread = float(ops.emm_predictor(resp, {k: _dev(v) for k, v in params.items()})[:, 3:].std().cpu())
    side = float(np.mean(np.abs(inp["boxes"][:, 2:] - inp["boxes"][:, :2])))
    params["reg.weight"] = (params["reg.weight"] * np.float32(0.5 * side / spread)).astype(np.float32)
    params = {k: _dev(v) for k, v in params.items()}
    logits = ops.emm_predictor(resp, params)
    zeros = float((logits[:, 3:] == 0).float().mean().cpu())
    assert 0.3 <= zeros <= 0.7, "share of zero reg logits %.3f" % zeros
    bb, conf, idx = ops.emm_track(feats_b, boxes, sr, z, params, cfg.rx, cfg.rz, cfg.scales, cfg.sampling_ratio,
                                  cfg.pad_pixels, sigma=cfg.sigma, use_centerness=cfg.use_centerness,
                                  clip_wh=case["image_wh"], return_index=True)
    bb2, conf2, idx2 = ops.emm_decode(logits, sr, boxes, cfg.rx, cfg.rz, cfg.pad_pixels, sigma=cfg.sigma,
                                      use_centerness=cfg.use_centerness, return_index=True, clip_wh=case["image_wh"])
    torch.cuda.synchronize()
    assert _bit_equal((bb, conf, idx), (bb2, conf2, idx2)), "one call %s vs composition %s" % (idx.tolist(), idx2.tolist())
    lg = logits.cpu().numpy()
    d = dict(cls=lg[:, :2], center=lg[:, 2:3], reg=lg[:, 3:], boxes=inp["boxes"], sr=sr.cpu().numpy())
    orc = E.oracle_eval(d, dict(rx=cfg.rx, rz=cfg.rz, pad_pixels=cfg.pad_pixels, use_centerness=cfg.use_centerness,
                                sigma=cfg.sigma), case["image_wh"])
    with np.errstate(invalid="ignore"):
        tops = _tops(orc)
        print("decode-edge towers: share of zero reg logits %.3f, oracle maxima %s" % (zeros, tops.tolist()))
        assert int((~(tops <= 1)).sum()) >= 1, "no track of the sparse head leaves [0, 1]: %s" % tops.tolist()
    _judge("through the towers", orc, bb2, conf2, idx2)
