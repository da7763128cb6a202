"""Box-head post-processing of the detections (csrc/box_detect.hip, ``ops.box_detect_post``, ``TrackBoxHead.detect_raw`` /
``forward`` on id-less proposals, ``siammot_amd.detector.DetectionHead``).

CPU: the fp32 restatement (``siammot_amd.box_refine.PostProcessor`` over the numpy NMS) reproduces the reference's own
outputs of tests/golden/box_detect_post.npz bit for bit; ``box_detect_cases.direct`` equals the restatement bit for bit; the
cases meet the conditions that entitle the GPU tests to pin discrete decisions; header, ctypes table and library agree;
proposals with ids keep today's path.
GPU: counts, labels and proposal rows exactly, boxes and scores within the case's bound against fp64; rows beyond the
count, determinism and NaN logits bit for bit; the wiring through ``TrackBoxHead`` and ``DetectionHead`` with one
device-to-host copy."""
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

import box_detect_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
XFORM_CLIP = math.log(1000.0 / 16)
NONEMPTY = tuple(n for n in B.CASE_NAMES if n != "d_m64_c0_k2")


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.GOLDEN_CASES)
def test_restatement_reproduces_the_reference_bitwise(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "box_detect_post.npz"))
    r = B.restated(B.case(name))
    assert r["boxes"].shape == g[name + "/boxes"].shape and len(r["boxes"]) > 0
    assert np.array_equal(bits(r["boxes"]), bits(g[name + "/boxes"]))
    assert np.array_equal(bits(r["scores"]), bits(g[name + "/scores"]))
    assert np.array_equal(r["labels"], g[name + "/labels"])
    assert (r["ids"] == -1).all()


@pytest.mark.parametrize("name", NONEMPTY)
def test_direct_form_equals_the_restatement_bitwise(name):
    c = B.case(name)
    r, d = B.restated(c), B.reference(name)["f32"]
    assert np.array_equal(bits(r["boxes"]), bits(d["boxes"])) and np.array_equal(bits(r["scores"]), bits(d["scores"]))
    assert np.array_equal(r["labels"], d["labels"])
    assert d["counts"][0] == len(d["rows"]) == d["counts"][1:].sum()
    for j in range(1, c["num_classes"]):                               # inside a class: ascending proposal row
        assert (np.diff(d["rows"][d["labels"] == j]) > 0).all()


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_cases_meet_their_conditions(name):
    c, ref = B.case(name), B.reference(name)
    cond = B.conditions(c, ref)
    print(name, cond)
    assert cond["score_margin"] > cond["score_bound"], cond
    assert cond["score_gap"] > 2.0 * cond["score_bound"], cond
    assert cond["iou_clear"] and cond["exact"] and cond["same_decisions"], cond
    if c["family"] == "exact":
        assert cond["score_gap"] > 1e-5
    if c["ordinary"]:
        supp = cond["candidates"] - cond["survivors"]
        assert 5 * supp >= cond["candidates"] and 5 * cond["survivors"] >= cond["candidates"], cond
    assert B.conditions_hold(c, cond)
    if c["family"] == "decode":
        assert c["count"] <= 300 and c["head_out"][:, c["num_classes"]:].any()


def test_case_table_covers_the_aspects():
    cs = {n: B.case(n) for n in B.CASE_NAMES}
    assert {c["count"] for c in cs.values()} >= {0, 1, 63, 64, 65, 300, 2048}
    assert {c["num_classes"] for c in cs.values()} >= {2, 3, 17}
    assert (cs["d_m512_c300_k3"]["M"], cs["d_m512_c300_k3"]["count"]) == (512, 300)
    assert (cs["d_m64_c0_k2"]["M"], cs["d_m64_c0_k2"]["count"]) == (64, 0)
    assert cs["d_agn_m65_k3"]["agnostic"] and cs["d_amodal_m63_k2"]["clip_wh"] is None
    assert cs["d_clip1x1_m65_k2"]["clip_wh"] == (1, 1) and cs["d_w_m65_k3"]["weights"] != B.YAML_WEIGHTS
    assert B.reference("d_m64_c0_k2")["f32"]["counts"].tolist() == [0, 0]
    assert B.reference("d_clip1x1_m65_k2")["f32"]["counts"].tolist() == [1, 1]      # every box is the one pixel


def test_deliberate_edges_are_decided_as_stated():
    c, ref = B.case("edge_k4"), B.reference("edge_k4")
    d, rank = ref["f32"], c["rank_of_row"]
    row = lambda k: int(np.nonzero(rank == k)[0][0])
    kept1 = set(d["rows"][d["labels"] == 1].tolist())
    cand1 = set(np.nonzero(d["prob"][:, 1] > F32(0.05))[0].tolist())
    assert cand1 == {row(k) for k in range(116)}
    a, b = (row(k) for k in B.EDGE_RANKS["half"])
    assert a in kept1 and b in kept1                                   # IoU exactly 0.5: not above the threshold
    a, b = (row(k) for k in B.EDGE_RANKS["above"])
    assert a in kept1 and b not in kept1                               # 67 / 133
    a, b, cc = (row(k) for k in B.EDGE_RANKS["chain"])
    assert a in kept1 and b not in kept1 and cc in kept1               # B is dead, so C lives
    a, b, cc, e = (row(k) for k in B.EDGE_RANKS["tile"])
    assert a in kept1 and b not in kept1 and cc in kept1 and e not in kept1          # ranks 62, 63 | 64, 65
    (ra, rb), = c["identical"]
    assert ra < rb and np.array_equal(c["head_out"][ra], c["head_out"][rb]) and np.array_equal(c["boxes"][ra], c["boxes"][rb])
    assert ra in kept1 and rb not in kept1                             # the lower row wins
    assert d["counts"][2] == 0 and d["counts"][1] == 116 - 5 and d["counts"][3] > 0
    assert (d["prob"][:, 3] > F32(0.05)).all()                         # class 3: every row is a candidate
    t, rt = B.case("edge_thresh_k20"), B.reference("edge_thresh_k20")
    (r7,) = t["at_threshold"]
    assert (rt["f32"]["prob"][r7] == F32(0.05)).all()                  # exactly the threshold in fp32 ...
    assert r7 not in rt["f32"]["rows"].tolist() and len(rt["f32"]["rows"]) > 20      # ... so in no class


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "smot_emm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(smot_[a-z0-9_]+)\s*\(", src))


def test_header_ops_table_and_library_agree_on_the_new_symbols():
    import siammot_amd.ops as ops
    if not os.path.exists(ops.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ops.load_library()
    src = open(os.path.join(ROOT, "include", "smot_emm.h")).read()
    for name in ("smot_box_detect_post_ws_bytes", "smot_box_detect_post_fwd"):
        assert name in _header_symbols() and name in ops.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "Replaces:" in src[src.index("BOX-HEAD POST-PROCESSING OF THE DETECTIONS"):src.index("smot_box_detect_post_ws_bytes(int")]
    assert lib.smot_abi_version() == ops.ABI_VERSION == 14
    M, K = ops.BOX_DETECT_MAX_ROWS, ops.BOX_DETECT_MAX_CLASSES
    assert (M, K) == (2048, 128)
    for m, k in ((0, 2), (M + 1, 2), (300, 1), (300, K + 1), (-1, 2)):
        assert lib.smot_box_detect_post_ws_bytes(m, k) == -1
    assert lib.smot_box_detect_post_ws_bytes(300, 2) >= ops.box_detect_mask_bytes(300, 2) == 300 * 5 * 8
    assert ops.box_detect_mask_bytes(M, K) == 127 * 2048 * 32 * 8 <= lib.smot_box_detect_post_ws_bytes(M, K)
    # refusals come before any pointer is touched
    bad = lambda **kw: lib.smot_box_detect_post_fwd(None, kw.get("ld", 10), kw.get("K", 2), kw.get("KR", 2), None, None,
                                                    kw.get("M", 8), 10.0, 10.0, 5.0, 5.0, XFORM_CLIP, 0.0, 0.0, 0.05,
                                                    kw.get("nms", 0.5), None, None, None, None, None, None, None)
    assert bad() != 0 and b"null pointer" in lib.smot_last_error()
    assert bad(nms=0.0) != 0 and b"nms_thresh" in lib.smot_last_error()
    assert bad(M=M + 1) != 0 and bad(K=K + 1, KR=K + 1, ld=5 * (K + 1)) != 0 and bad(KR=3) != 0 and bad(ld=9) != 0


class _StubPooler(torch.nn.Module):
    def __init__(self, channels, resolution):
        super(_StubPooler, self).__init__()
        self.shape = (channels, resolution, resolution)

    def forward(self, x, boxes):
        n = sum(len(b) for b in boxes)
        return torch.linspace(-1.0, 1.0, n * int(np.prod(self.shape))).reshape((n,) + self.shape)


def _small_cfg(channels=16, classes=3, dim=64):
    from siammot_amd.config import get_default_cfg
    cfg = get_default_cfg(channels=channels)
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = dim
    cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES = classes
    return cfg


def test_cpu_and_id_carrying_proposals_keep_todays_path():
    import siammot_amd.ops as ops
    from oracle import solver_oracle as SO
    from siammot_amd.box_refine import TrackBoxHead
    from siammot_amd.structures import BoxList

    def cpu_nms(boxlist, thresh):
        return boxlist[torch.from_numpy(SO.nms_indices(boxlist.bbox.numpy(), boxlist.get_field("scores").numpy(), thresh))]
    torch.manual_seed(3)
    head = TrackBoxHead(_small_cfg(), 16, pooler=_StubPooler(16, 7), nms_fn=cpu_nms).eval()

    def no_raw(*a, **k):
        raise AssertionError("the device path was taken")
    head.detect_raw = no_raw
    boxes = torch.from_numpy(B.case("d_m63_k3")["boxes"][:12].copy())
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        with_ids = BoxList(boxes, B.IMAGE_WH)
        with_ids.add_field("ids", torch.tensor([-1, 4, -1, -1, 9, -1, -1, -1, 2, -1, -1, -1]))
        x, res, losses = head(None, [with_ids])
        assert losses == {} and x.shape == (12, 64) and sorted(res[0].fields()) == ["ids", "labels", "scores"]
        assert not head.detect_ok(with_ids)
        plain = BoxList(boxes, B.IMAGE_WH)
        assert not head.detect_ok(plain)                               # CPU tensors, injected pooler and NMS
        _, res2, _ = head(None, [plain])
        assert (res2[0].get_field("ids") == -1).all()
    assert dict(ops.FALLBACKS) == before


# ---- the wiring case: a small head whose CPU oracle leaves coarse margins -----------------------------------------------
WIRING = dict(seed=121, channels=16, dim=64, classes=3, rows=40, valid=33, image_wh=(320, 192), score_margin=1e-3, delta=0.05,
              groups=12, cls_scale=50.0, background=2.0)


def _wiring_inputs():
    w = WIRING
    rs = np.random.RandomState(w["seed"])
    W, H = w["image_wh"]
    feats = [rs.standard_normal((1, w["channels"], H // s, W // s)).astype(F32) for s in (4, 8, 16, 32)]
    gxy = rs.uniform(0.0, 1.0, (w["groups"], 2)) * (W - 90.0, H - 70.0)
    gwh = rs.uniform(24.0, 80.0, (w["groups"], 2))
    g = rs.randint(0, w["groups"], w["rows"])
    xy = gxy[g] + rs.uniform(-0.15, 0.15, (w["rows"], 2)) * gwh[g]
    boxes = np.concatenate((xy, xy + gwh[g] * rs.uniform(0.9, 1.1, (w["rows"], 2))), 1).astype(F32)
    boxes[w["valid"]:] = 0.0                                           # what the RPN leaves beyond its count
    torch.manual_seed(w["seed"])
    from siammot_amd.box_refine import TrackBoxHead
    head = TrackBoxHead(_small_cfg(w["channels"], w["classes"], w["dim"]), w["channels"]).eval()
    with torch.no_grad():
        head.predictor.cls_score.weight.mul_(w["cls_scale"])
        head.predictor.cls_score.bias[0] += w["background"]
        head.predictor.bbox_pred.weight.mul_(3.0)
    return feats, boxes, head


def _wiring_case(head_out, boxes):
    w = WIRING
    return B._case("decode", np.asarray(head_out, F32), boxes, w["valid"], w["classes"], clip_wh=w["image_wh"])


def test_wiring_case_leaves_coarse_margins_on_the_cpu_oracle():
    from oracle import box_head_oracle as BO
    from siammot_amd.structures import BoxList
    w = WIRING
    feats, boxes, head = _wiring_inputs()
    fe = head.feature_extractor
    with torch.no_grad():
        x = BO.OraclePooler(7, fe.pooler.scales, 2)([torch.from_numpy(f) for f in feats],
                                                    [BoxList(torch.from_numpy(boxes[:w["valid"]].copy()), w["image_wh"])])
        h = torch.relu(fe.fc7(torch.relu(fe.fc6(x.reshape(x.shape[0], -1)))))
        ho = torch.cat(head.predictor(h), 1).numpy()
    c = _wiring_case(np.concatenate((ho, np.zeros((w["rows"] - w["valid"], ho.shape[1]), F32))), boxes)
    cond = B.conditions(c, score_bound=w["score_margin"], delta=w["delta"])
    print(cond)
    assert cond["score_margin"] > w["score_margin"] and cond["score_gap"] > 2 * w["score_margin"] and cond["iou_clear"], cond
    assert cond["same_decisions"] and 0 < cond["survivors"] < cond["candidates"]
    assert min(B.reference_eval(c)["f32"]["counts"][1:]) > 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _launch(c, head_out=None, boxes=None):
    import siammot_amd.ops as ops
    dev = "cuda:0"
    ho = torch.from_numpy(np.ascontiguousarray(c["head_out"] if head_out is None else head_out)).to(dev)
    bx = torch.from_numpy(np.ascontiguousarray(c["boxes"] if boxes is None else boxes)).to(dev)
    count = torch.tensor([c["count"]], dtype=torch.int32, device=dev)
    out = ops.box_detect_post(ho, c["num_classes"], c["reg_classes"], bx, count, c["weights"], XFORM_CLIP, c["clip_wh"],
                              c["score_thresh"], c["nms_thresh"])
    return [t.cpu().numpy() for t in out]


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def _check_against_reference(out, c, ref):
    boxes, scores, labels, rows, count = out
    d, f64 = ref["f32"], ref["f64"]
    n, cap = int(d["counts"][0]), c["M"] * (c["num_classes"] - 1)
    assert boxes.shape == (cap, 4) and scores.shape == labels.shape == rows.shape == (cap,) and count.shape == (c["num_classes"],)
    assert labels.dtype == np.int64 and rows.dtype == np.int32 and count.dtype == np.int32
    print("counts", count.tolist()[:8], "reference", d["counts"].tolist()[:8])
    assert count.tolist() == d["counts"].tolist()
    assert np.array_equal(labels[:n], d["labels"]) and np.array_equal(rows[:n], d["rows"])
    if n:
        eb = np.abs(boxes[:n].astype(np.float64) - f64["dec"][d["rows"], d["labels"]])
        es = np.abs(scores[:n].astype(np.float64) - f64["prob"][d["rows"], d["labels"]])
        bound = ref["box_bound"][d["rows"], d["labels"]]
        print("box error / bound %.3f, score error %.3e (bound %.3e)" % ((eb / bound).max(), es.max(), ref["score_bound"]))
        assert (eb <= bound).all() and (es <= ref["score_bound"]).all()
    assert not boxes[n:].any() and not scores[n:].any() and not labels[n:].any() and not rows[n:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_one_launch_per_case_against_the_reference(name):
    c = B.case(name)
    _check_against_reference(_launch(c), c, B.reference(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("d_m512_c300_k3", "d_m64_c0_k2"))
def test_rows_beyond_the_count_do_not_exist(name):
    c = B.case(name)
    clean = _launch(c)
    for a, b in ((np.nan, 1e30), (1e30, np.nan)):
        ho, bx = c["head_out"].copy(), c["boxes"].copy()
        ho[c["count"]:], bx[c["count"]:] = a, b
        assert _same_bits(_launch(c, ho, bx), clean)
    _check_against_reference(clean, c, B.reference(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("x_m2048_k2", "d_m300_k3"))
def test_two_runs_give_the_same_bits(name):
    c = B.case(name)
    assert _same_bits(_launch(c), _launch(c))


@pytest.mark.gpu
def test_a_row_with_a_nan_logit_is_in_no_class():
    c, d = B.case("d_m300_k3"), B.reference("d_m300_k3")["f32"]
    victims = [int(d["rows"][0]), int(d["rows"][len(d["rows"]) // 2]), int(d["rows"][-1])]      # three survivors
    dirty, removed = c["head_out"].copy(), c["head_out"].copy()
    dirty[victims[0], 0] = np.nan
    dirty[victims[1], 2] = np.nan
    dirty[victims[2], 1] = np.inf                                       # torch: inf - inf = NaN in the soft-max
    removed[victims, :3] = (60.0, 0.0, 0.0)                             # foreground scores e^-60: below every threshold
    got, want = _launch(c, dirty), _launch(c, removed)
    assert _same_bits(got, want)
    assert not set(victims) & set(got[3][:got[4][0]].tolist())
    ref = B.direct(c, torch.float32, exclude=victims)
    assert got[4].tolist() == ref["counts"].tolist() and np.array_equal(got[3][:got[4][0]], ref["rows"])


def _count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
        syncs = [x for x in w if "synchroniz" in str(x.message).lower()]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, len(syncs)


@pytest.mark.gpu
def test_track_box_head_on_id_less_device_proposals():
    import siammot_amd.ops as ops
    from siammot_amd.structures import BoxList
    w, dev = WIRING, "cuda:0"
    feats, boxes, head = _wiring_inputs()
    head = head.to(dev)
    feats = [torch.from_numpy(f).to(dev) for f in feats]
    bx = torch.from_numpy(boxes).to(dev)
    count = torch.tensor([w["valid"]], dtype=torch.int32, device=dev)
    raw = head.detect_raw(feats, bx, count, w["image_wh"])
    ho = raw[6].cpu().numpy()
    assert raw[5].shape == (w["rows"], w["dim"]) and ho.shape == (w["rows"], w["classes"] * 5)
    # the restated PostProcessor on the head outputs the call itself computed
    c = _wiring_case(ho, boxes)
    ref = B.reference_eval(c)
    cond = B.conditions(c, ref, score_bound=w["score_margin"], delta=w["delta"])
    print(cond)
    assert cond["score_margin"] > w["score_margin"] and cond["score_gap"] > 2 * w["score_margin"] and cond["iou_clear"], cond
    r = B.restated(c)
    assert np.array_equal(bits(r["boxes"]), bits(ref["f32"]["boxes"])) and np.array_equal(r["labels"], ref["f32"]["labels"])
    _check_against_reference([t.cpu().numpy() for t in raw[:5]], c, ref)
    # forward: the same detections from M = 33 rows (the GEMMs' rounding differs from M = 40 by far less than the margins)
    before = ops.FALLBACKS["box_detect_torch"]
    prop = BoxList(bx[:w["valid"]].clone(), w["image_wh"])
    prop.add_field("objectness", torch.rand(w["valid"], device=dev))
    assert head.detect_ok(prop)
    with torch.no_grad():
        (x, res, losses), syncs = _count_syncs(lambda: head(feats, [prop]))
    assert syncs == 1 and losses == {} and ops.FALLBACKS["box_detect_torch"] == before
    out, d = res[0], ref["f32"]
    assert x.shape == (w["valid"], w["dim"]) and out.fields() == ["scores", "ids", "labels"] and out.mode == "xyxy"
    assert tuple(out.size) == w["image_wh"] and len(out) == d["counts"][0]
    assert out.get_field("labels").cpu().numpy().tolist() == d["labels"].tolist()
    assert (out.get_field("ids") == -1).all() and out.get_field("ids").dtype == torch.int64
    assert np.abs(out.bbox.cpu().numpy() - d["boxes"]).max() < w["delta"]
    assert np.abs(out.get_field("scores").cpu().numpy() - d["scores"]).max() < w["score_margin"]
    np.testing.assert_allclose(x.cpu().numpy(), raw[5][:w["valid"]].cpu().numpy(), rtol=1e-4, atol=1e-5)
    # an injected NMS keeps today's path, counted
    head.post_processor.nms_fn = lambda boxlist, thresh: boxlist
    with torch.no_grad():
        _, res2, _ = head(feats, [prop])
    assert ops.FALLBACKS["box_detect_torch"] == before + 1 and len(res2[0]) >= len(out)


@pytest.mark.gpu
def test_detection_head_equals_the_two_modules_composed_with_one_host_copy():
    import bench
    import rpn_proposal_cases as R
    import siammot_amd.ops as ops
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.detector import DetectionHead, build_detection_head
    from siammot_amd.structures import BoxList
    from siammot_amd.track_head import build_tracking_loop
    dev = "cuda"
    cfg = _small_cfg(bench.CHANNELS, 2, 64)
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    image_wh = (bench.NET_HW[1], bench.NET_HW[0])
    torch.manual_seed(0)
    det_head = build_detection_head(cfg, BoxCoder(R.WEIGHTS), bench.CHANNELS).to(dev)
    assert isinstance(det_head, DetectionHead)
    with torch.no_grad():
        det_head.box_head.predictor.bbox_pred.weight.mul_(0.02)
        det_head.box_head.predictor.cls_score.weight.mul_(4.0)
    obj, reg = R.golden_inputs(0, num_images=1)
    obj, reg = [torch.from_numpy(o).to(dev) for o in obj], [torch.from_numpy(r).to(dev) for r in reg]
    anchors = [[BoxList(torch.from_numpy(a).to(dev), image_wh) for a in R.anchors()]]       # a corner of the frame
    feats = bench.synthetic_features(100, dev)
    before = dict(ops.FALLBACKS)
    res, syncs = _count_syncs(lambda: det_head(anchors, obj, reg, feats))
    with torch.no_grad():
        composed, syncs2 = _count_syncs(lambda: det_head.box_head(feats, det_head.rpn_post(anchors, obj, reg))[1])
    assert dict(ops.FALLBACKS) == before
    print("host copies: DetectionHead %d, composition %d; detections %d" % (syncs, syncs2, len(res[0])))
    assert syncs == 1 and syncs2 > syncs
    a, b = res[0], composed[0]
    assert len(a) == len(b) > 0 and a.fields() == ["scores", "ids", "labels"] and sorted(b.fields()) == sorted(a.fields()) and tuple(a.size) == image_wh
    assert a.get_field("labels").tolist() == b.get_field("labels").tolist()
    np.testing.assert_allclose(a.bbox.cpu().numpy(), b.bbox.cpu().numpy(), rtol=0, atol=1e-2)
    np.testing.assert_allclose(a.get_field("scores").cpu().numpy(), b.get_field("scores").cpu().numpy(), rtol=0, atol=1e-4)
    # ... and the detections are what a tracking loop takes
    loop = build_tracking_loop(cfg, dev)
    bench.init_predictor(loop.track.tracker.predictor, a.bbox.cpu())
    loop.track.tracker.to(dev)
    out = loop(feats, a)
    assert out.has_field("ids") and len(out) <= len(a)
