"""RPN proposal selection (siammot_amd.rpn / ops.rpn_proposals / csrc/rpn_proposals.hip).

CPU: the numpy restatement (tests/rpn_proposal_cases.py) and the package's torch composition reproduce the reference's
results of tests/golden/rpn_proposals.npz bit for bit; the fixture meets the conditions its generator searched for.
GPU: every stage of the device path against the restatement — selection, clip / filter / NMS / merge exactly; the decode
against an fp64 evaluation with a bound taken from the fp32 restatement's own error.
"""
import os
import warnings

import numpy as np
import pytest
import torch

import rpn_proposal_cases as R
from oracle.solver_oracle import nms_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
_cache = {}


def fixture():
    if "fx" not in _cache:
        z = np.load(os.path.join(ROOT, "tests", "golden", "rpn_proposals.npz"))
        fx = {k: z[k] for k in z.files}
        L = len(R.LEVELS)
        fx["obj"] = [fx["objectness_%d" % l] for l in range(L)]
        fx["reg"] = [fx["regression_%d" % l].astype(F32) for l in range(L)]
        fx["anc"] = R.anchors()
        _cache["fx"] = fx
    return _cache["fx"]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def numpy_nms_fn(boxes, scores, thresh):
    return torch.from_numpy(nms_indices(boxes.numpy(), scores.numpy(), thresh))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_fixture_meets_the_conditions_of_its_generator():
    fx = fixture()
    obj, reg = R.golden_inputs(int(np.asarray(fx["seed"]).reshape(-1)[0]))
    for l in range(len(R.LEVELS)):
        assert fx["obj"][l].dtype == F32 and fx["regression_%d" % l].dtype == np.float16
        assert np.array_equal(bits(obj[l]), bits(fx["obj"][l])) and np.array_equal(bits(reg[l]), bits(fx["reg"][l]))
    bites = {"post": False, "min_size": False}
    for name, case in R.GOLDEN_CASES.items():
        c = R.conditions(fx["obj"], fx["reg"], fx["anc"], case)
        print(name, c)
        assert c["distinct"], name
        assert c["iou_margin"] >= R.IOU_MARGIN, (name, c)
        assert c["size_margin"] >= R.SIZE_MARGIN, (name, c)
        for img in range(case["N"]):
            for idx, logit, box in R.candidates(fx["obj"], fx["reg"], fx["anc"], img, case["pre"]):
                b, s, _, _ = R.clip_filter(box, logit, R.IMAGE_WH, case["min_size"], case["amodal"])
                bites["min_size"] |= len(b) < len(box)
                bites["post"] |= len(nms_indices(b, s, R.NMS_THRESH)) > case["post"]
    assert bites["post"] and bites["min_size"]            # the truncation and the size filter both act somewhere


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_numpy_restatement_reproduces_the_reference(name):
    fx, case = fixture(), R.GOLDEN_CASES[name]
    res = R.pipeline(fx["obj"], fx["reg"], fx["anc"], case)
    for i, (boxes, objectness) in enumerate(res):
        assert boxes.shape == fx["%s/boxes_%d" % (name, i)].shape
        assert np.array_equal(bits(boxes), bits(fx["%s/boxes_%d" % (name, i)]))
        assert np.array_equal(bits(objectness), bits(fx["%s/objectness_%d" % (name, i)]))


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_torch_composition_on_cpu_reproduces_the_reference(name):
    from siammot_amd.rpn import RPNPostProcessor
    from siammot_amd.structures import BoxList
    fx, case = fixture(), R.GOLDEN_CASES[name]
    N = case["N"]
    post = RPNPostProcessor(case["pre"], case["post"], R.NMS_THRESH, case["min_size"], fpn_post_nms_top_n=case["fpn"],
                            amodal=case["amodal"], nms_fn=numpy_nms_fn).eval()
    anchors = [[BoxList(torch.from_numpy(a.copy()), R.IMAGE_WH) for a in fx["anc"]] for _ in range(N)]
    with torch.no_grad():
        res = post(anchors, [torch.from_numpy(o[:N].copy()) for o in fx["obj"]],
                   [torch.from_numpy(r[:N].copy()) for r in fx["reg"]])
    assert len(res) == N
    for i, bl in enumerate(res):
        assert bl.mode == "xyxy" and tuple(bl.size) == R.IMAGE_WH and bl.fields() == ["objectness"]
        assert np.array_equal(bits(bl.bbox.numpy()), bits(fx["%s/boxes_%d" % (name, i)]))
        assert np.array_equal(bits(bl.get_field("objectness").numpy()), bits(fx["%s/objectness_%d" % (name, i)]))


def test_restatement_exp_is_anchored_outside_torch():
    """``exp32`` / ``sigmoid32`` are torch's CPU kernels (the fixture's own; numpy's fp32 exp differs from them in the last
    bit, see rpn_proposal_cases.exp32 and DESIGN.md).  Anchor them outside torch, to numpy's fp64 evaluation rounded once
    (the correctly rounded value but for double rounding): a 1-ulp exp is within 1 ulp of it; the sigmoid adds two
    roundings of half an ulp each to the exp's one: within 2."""
    x = np.concatenate([np.linspace(-12, R.XFORM_CLIP, 200001), np.random.RandomState(1).standard_normal(200000) * 2]).astype(F32)
    ulps = lambda a, b: int(np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64)).max())
    x64 = x.astype(np.float64)
    assert ulps(R.exp32(x), np.exp(x64).astype(F32)) <= 1
    assert ulps(R.sigmoid32(x), (1.0 / (1.0 + np.exp(-x64))).astype(F32)) <= 2


def test_calls_beyond_the_merge_lds_or_the_mask_budget_take_the_torch_path():
    import siammot_amd.ops as ops
    from siammot_amd.rpn import RPNPostProcessor
    from siammot_amd.structures import BoxList
    one = BoxList(torch.zeros(4, 4), R.IMAGE_WH)
    inside = lambda p, N, L: p._within_capacity([[one] * L] * N, [None] * L)
    assert inside(RPNPostProcessor(2048, 2048, 0.7, 0), 1, 7)
    assert not inside(RPNPostProcessor(2048, 2048, 0.7, 0), 1, 8)          # 8 x 2048 keys + the counters: past 64 KiB of LDS
    assert inside(RPNPostProcessor(2048, 2032, 0.7, 0, fpn_post_nms_top_n=2048), 1, 8)
    assert ops.rpn_mask_bytes(4, 5, 1000) == 4 * 5 * 1000 * 16 * 8 and ops.rpn_mask_bytes(64, 8, 2048) == 268435456
    assert inside(RPNPostProcessor(1000, 300, 0.7, 0), 64, 5)              # 41 MB
    assert not inside(RPNPostProcessor(2048, 300, 0.7, 0), 64, 5)          # 168 MB of bitmask: the torch path
    lib = ops.load_library()
    import ctypes
    three = (ctypes.c_int * 8)(*[3] * 8)
    assert lib.smot_rpn_proposals_ws_bytes(1, 8, ctypes.cast(three, ctypes.c_void_p), ctypes.cast(three, ctypes.c_void_p),
                                           ctypes.cast(three, ctypes.c_void_p), 2048, 2048) > 0


def test_factory_reads_the_config_keys():
    from siammot_amd.config import get_default_cfg
    from siammot_amd.rpn import RPNPostProcessor, make_rpn_postprocessor
    cfg = get_default_cfg()
    assert (cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST) == (1000, 300, 300)
    assert (cfg.MODEL.RPN.NMS_THRESH, cfg.MODEL.RPN.MIN_SIZE, cfg.MODEL.RPN.FPN_POST_NMS_PER_BATCH) == (0.7, 0, True)
    cfg.MODEL.RPN.update(PRE_NMS_TOP_N_TEST=11, POST_NMS_TOP_N_TEST=7, FPN_POST_NMS_TOP_N_TEST=5, NMS_THRESH=0.6, MIN_SIZE=3,
                         FPN_POST_NMS_PER_BATCH=False)
    cfg.INPUT.AMODAL = True
    coder = object()
    p = make_rpn_postprocessor(cfg, coder, is_train=False)
    assert isinstance(p, RPNPostProcessor) and p.box_coder is coder
    assert (p.pre_nms_top_n, p.post_nms_top_n, p.fpn_post_nms_top_n, p.nms_thresh, p.min_size, p.fpn_post_nms_per_batch,
            p._amodal) == (11, 7, 5, 0.6, 3, False, True)
    d = RPNPostProcessor(1000, 300, 0.7, 0)
    assert d.fpn_post_nms_top_n == 300 and d.box_coder.weights == (1.0, 1.0, 1.0, 1.0) and d._amodal is False


def test_training_raises():
    from siammot_amd.rpn import RPNPostProcessor
    post = RPNPostProcessor(256, 32, 0.7, 0)
    with pytest.raises(NotImplementedError):
        post.train()([], [], [])
    with pytest.raises(NotImplementedError):
        post.eval()([], [], [], targets=[None])


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def run_op(obj, reg, anc, case, image_wh=R.IMAGE_WH, dtype=None, per_image_anchors=None, thresh=R.NMS_THRESH):
    """ops.rpn_proposals on numpy inputs (obj / reg: per level [N, ...]; anc: per level [n, 4], shared by the images
    unless ``per_image_anchors``).  -> host copies of (boxes, objectness, count, candidates)."""
    import siammot_amd.ops as ops
    dev = "cuda:0"
    N = case["N"]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a[:N])).to(dev) if dtype is None else torch.from_numpy(np.ascontiguousarray(a[:N])).to(dev).to(dtype)
    o, r = [to(x) for x in obj], [to(x) for x in reg]
    if per_image_anchors is None:
        shared = [torch.from_numpy(a).to(dev) for a in anc]
        anchors = [shared for _ in range(N)]
    else:
        anchors = [[torch.from_numpy(a).to(dev) for a in per] for per in per_image_anchors]
    sizes = image_wh if isinstance(image_wh, list) else [image_wh] * N
    boxes, scores, count, cand = ops.rpn_proposals(o, r, anchors, sizes, case["pre"], case["post"], case["fpn"], thresh,
                                                   case["min_size"], amodal=case["amodal"], return_candidates=True)
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy(), {k: v.cpu().numpy() for k, v in cand.items()}


def zero_reg(obj):
    return [np.zeros((o.shape[0], 4 * o.shape[1]) + o.shape[2:], F32) for o in obj]


def zero_anchors(obj):
    return [np.zeros((o.shape[1] * o.shape[2] * o.shape[3], 4), F32) for o in obj]


def select_cases():
    rng = np.random.RandomState(7)
    fx = fixture()
    c = {"small": (fx["obj"], 256)}
    c["tie_blocks"] = ([(np.floor(rng.rand(2, 3, 24, 40) * 24) / 8 - 1).astype(F32)], 256)       # 24 values: ties across rank k
    c["all_equal"] = ([np.full((2, 3, 24, 40), 0.5, F32), np.full((2, 3, 48, 80), -1.25, F32)], 256)
    z = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], F32), size=(2, 3, 24, 40))
    c["signed_zeros"] = ([z.astype(F32)], 1200)
    c["n_equals_k"] = ([rng.standard_normal((2, 3, 3, 5)).astype(F32)], 45)
    c["n_below_k"] = ([rng.standard_normal((2, 3, 3, 5)).astype(F32), rng.standard_normal((2, 3, 6, 10)).astype(F32)], 2048)
    c["k_1"] = ([rng.standard_normal((2, 3, 24, 40)).astype(F32)], 1)
    c["level0_headline"] = ([rng.standard_normal((1, 3, 176, 320)).astype(F32)], 1000)
    c["level0_headline_ties"] = ([(np.round(rng.standard_normal((1, 3, 176, 320)) * 16) / 16).astype(F32)], 1000)
    # two images of 42 chunks each, different contents, ties across rank k: the per-image chunk bookkeeping of the tie pass
    c["level0_headline_ties_two_images"] = ([(np.round(rng.standard_normal((2, 3, 176, 320)) * 16) / 16).astype(F32),
                                             (np.round(rng.standard_normal((2, 3, 88, 160)) * 8) / 8).astype(F32)], 1000)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "tie_blocks", "all_equal", "signed_zeros", "n_equals_k", "n_below_k", "k_1",
                                  "level0_headline", "level0_headline_ties", "level0_headline_ties_two_images"])
def test_selection_is_the_stable_descending_argsort(name):
    obj, pre = select_cases()[name]
    N = obj[0].shape[0]
    case = dict(N=N, pre=pre, post=8, fpn=8, min_size=0, amodal=True)
    _, _, _, cand = run_op(obj, zero_reg(obj), zero_anchors(obj), case)
    for l, o in enumerate(obj):
        flat = R.flatten_logits(o)
        k = min(pre, flat.shape[1])
        for i in range(N):
            want = R.select(flat[i], k)
            assert cand["count"][i, l] == k
            got = cand["index"][i, l, :k]
            assert np.array_equal(got, want), "%s image %d level %d: first difference at rank %d" % (
                name, i, l, int(np.nonzero(got != want)[0][0]))
            assert np.array_equal(bits(cand["logit"][i, l, :k]), bits(flat[i][want]))


def decode_bound(deltas, anc):
    """(fp64 boxes, the fp32 restatement's largest error against them, one ulp of the largest coordinate)."""
    b64 = R.decode(deltas, anc, dtype=np.float64)
    b32 = R.decode(deltas, anc).astype(np.float64)
    ok = np.isfinite(b64)
    return b64, float(np.abs(b32 - b64)[ok].max()), float(np.spacing(F32(np.abs(b64[ok]).max())))


@pytest.mark.gpu
def test_decode_against_fp64():
    fx = fixture()
    reg = [r.copy() for r in fx["reg"]]
    rng = np.random.RandomState(3)
    for r in reg:                                            # regressions above the clamp (dw, dh) and one NaN delta per level
        C = r.shape[1]
        r[:, 2:C:4][rng.rand(*r[:, 2:C:4].shape) < 0.05] = 5.0
        r[:, 3:C:4][rng.rand(*r[:, 3:C:4].shape) < 0.05] = 7.5
    case = dict(N=2, pre=256, post=32, fpn=100, min_size=0, amodal=False)
    nan_rows = []
    for l, (o, r) in enumerate(zip(fx["obj"], reg)):          # the NaN goes where it is selected: the best logit of image 0
        best = R.select(R.flatten_logits(o)[0], 1)[0]
        hw, a = divmod(int(best), R.NUM_ANCHORS)
        r[0, 4 * a + (l % 4), hw // o.shape[3], hw % o.shape[3]] = np.nan
        nan_rows.append(l % 4)
    _, _, _, cand = run_op(fx["obj"], reg, fx["anc"], case)
    worst, worst_ref, n_clamped = 0.0, 0.0, 0
    for l in range(len(reg)):
        for i in range(2):
            k = cand["count"][i, l]
            idx = cand["index"][i, l, :k]
            deltas, anc = R.flatten_regression(reg[l])[i][idx], fx["anc"][l][idx]
            n_clamped += int((deltas[:, 2:] > R.XFORM_CLIP).sum())
            b64, err_ref, ulp = decode_bound(deltas, anc)
            got = cand["box"][i, l, :k].astype(np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(b64))
            if i == 0:                                       # dx, dw -> x1 and x2; dy, dh -> y1 and y2
                assert np.isnan(got[0]).tolist() == [nan_rows[l] % 2 == 0, nan_rows[l] % 2 == 1] * 2
            ok = ~np.isnan(b64)
            err = float(np.abs(got - b64)[ok].max())
            print("level %d image %d: device error %.3e, fp32 restatement %.3e (ratio %.2f), ulp %.3e" % (
                l, i, err, err_ref, err / err_ref, ulp))
            assert err <= 2 * err_ref + ulp
            worst, worst_ref = max(worst, err), max(worst_ref, err_ref)
    assert n_clamped > 20
    print("decode: largest device error %.3e px, restatement %.3e px, ratio %.2f" % (worst, worst_ref, worst / worst_ref))


def boxes_level(boxes, logits):
    """A level whose decoded boxes ARE ``boxes`` (zero deltas on anchors with exact sides): obj [1,1,1,n], anchors [n,4]."""
    n = len(boxes)
    return np.asarray(logits, F32).reshape(1, 1, 1, n), np.asarray(boxes, F32).reshape(n, 4)


def random_boxes(rng, n, n_big, wh=(600, 400)):
    """``n`` boxes with integer corners, the first ``n_big`` with sides of 20..120 px (they overlap), the rest 2 px."""
    x1, y1 = rng.randint(0, wh[0] - 130, n), rng.randint(0, wh[1] - 130, n)
    w, h = rng.randint(20, 121, n), rng.randint(20, 121, n)
    w[n_big:], h[n_big:] = 2, 2
    b = np.stack([x1, y1, x1 + w - 1, y1 + h - 1], 1).astype(F32)
    p = rng.permutation(n)
    return b[p]


def chain_boxes(n, w=100, h=40, d=12):
    """Every box suppresses the next (IoU 88/112) and not the one after (76/124) at threshold 0.7."""
    return np.array([[i * d, 10, i * d + w - 1, 10 + h - 1] for i in range(n)], F32)


def stage_cases():
    rng = np.random.RandomState(11)
    tiny = lambda n: random_boxes(rng, n, 0)
    lg = lambda n: rng.permutation(n).astype(F32) / 8 - 3                  # distinct logits
    levels = [random_boxes(rng, 90, 63), random_boxes(rng, 90, 64), random_boxes(rng, 90, 65), chain_boxes(70)]
    cases = {}
    # image 1 ends with no proposal: min_size empties every level
    cases["survivors_63_64_65_chain_empty_image"] = dict(
        images=[[(b, lg(len(b))) for b in levels], [(tiny(len(b)), lg(len(b))) for b in levels]],
        case=dict(N=2, pre=128, post=40, fpn=100, min_size=4, amodal=False), wh=(1000, 500))
    # one emptied level; the merge is asked for more rows than there are
    cases["emptied_level_fpn_above_total"] = dict(
        images=[[(levels[0], lg(90)), (tiny(90), lg(90)), (levels[3], lg(70))], [(levels[2], lg(90)), (levels[1], lg(90)), (tiny(70), lg(70))]],
        case=dict(N=2, pre=128, post=300, fpn=2048, min_size=4, amodal=False), wh=(450, 330))       # the clip bites
    cases["single_level_no_merge"] = dict(
        images=[[(np.concatenate([chain_boxes(70), levels[2]]), lg(160))]],
        case=dict(N=1, pre=256, post=50, fpn=20, min_size=4, amodal=False), wh=(1000, 500))
    cases["amodal_min_size_0"] = dict(
        images=[[(levels[1] - F32(50), lg(90)), (levels[3], lg(70))]],
        case=dict(N=1, pre=64, post=300, fpn=60, min_size=0, amodal=True), wh=(700, 500))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["survivors_63_64_65_chain_empty_image", "emptied_level_fpn_above_total",
                                  "single_level_no_merge", "amodal_min_size_0"])
def test_clip_filter_nms_merge_are_exact_on_the_device_candidates(name):
    sc = stage_cases()[name]
    case, images = sc["case"], sc["images"]
    L = len(images[0])
    wh = sc["wh"]
    obj, per_image_anchors = [], []
    for l in range(L):
        obj.append(np.concatenate([boxes_level(*img[l])[0] for img in images], 0))
    for img in images:
        per_image_anchors.append([boxes_level(*lv)[1] for lv in img])
    boxes, scores, count, cand = run_op(obj, zero_reg(obj), None, case, image_wh=wh, per_image_anchors=per_image_anchors)
    cap = case["fpn"] if L > 1 else min(case["post"], case["pre"])
    assert boxes.shape == (case["N"], cap, 4)
    if name.startswith("survivors"):
        surv = [len(R.clip_filter(cand["box"][0, l, :cand["count"][0, l]], cand["logit"][0, l, :cand["count"][0, l]], wh, 4, False)[0])
                for l in range(3)]
        assert surv == [63, 64, 65]
    for i in range(case["N"]):
        ks = [cand["count"][i, l] for l in range(L)]
        for l in range(L):                                   # zero deltas: the decoded boxes are the anchors
            assert np.array_equal(bits(cand["box"][i, l, :ks[l]]), bits(per_image_anchors[i][l][cand["index"][i, l, :ks[l]]]))
        want_b, want_s = R.post_stages([cand["box"][i, l, :ks[l]] for l in range(L)],
                                       [cand["logit"][i, l, :ks[l]] for l in range(L)], wh, case)
        if L == 1:
            want_b = want_b[:cap]
        assert count[i] == len(want_b), (name, i, count[i], len(want_b))
        assert np.array_equal(bits(boxes[i, :count[i]]), bits(want_b))
        assert not boxes[i, count[i]:].any() and not scores[i, count[i]:].any()
    if name.startswith("survivors"):
        assert count[1] == 0 and count[0] > 0
    if name == "single_level_no_merge":
        assert count[0] == 50                                # the level's list as it is, not cut to fpn_post_nms_top_n
    if name == "emptied_level_fpn_above_total":
        assert 0 < count[0] < 2048


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_end_to_end_against_the_reference(name):
    fx, case = fixture(), R.GOLDEN_CASES[name]
    boxes, scores, count, cand = run_op(fx["obj"], fx["reg"], fx["anc"], case)
    for i in range(case["N"]):
        want_b, want_s = fx["%s/boxes_%d" % (name, i)], fx["%s/objectness_%d" % (name, i)]
        assert count[i] == len(want_b)
        bound = 0.0
        for l in range(len(R.LEVELS)):
            idx = cand["index"][i, l, :cand["count"][i, l]]
            _, err_ref, ulp = decode_bound(R.flatten_regression(fx["reg"][l])[i][idx], fx["anc"][l][idx])
            bound = max(bound, 2 * err_ref + ulp)
        err = float(np.abs(boxes[i, :count[i]].astype(np.float64) - want_b).max())
        ulps = np.abs(bits(scores[i, :count[i]]).astype(np.int64) - bits(want_s).astype(np.int64)).max()
        print("%s image %d: %d proposals, box error %.3e px (bound %.3e), objectness within %d ulp" % (name, i, count[i], err, bound, ulps))
        assert err <= bound
        assert ulps <= 2
        assert not boxes[i, count[i]:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_return_the_bits_of_the_float_call(dtype):
    fx, case = fixture(), R.GOLDEN_CASES["n2_clip_post32_min4"]
    rnd = lambda a: torch.from_numpy(a).to(dtype).float().numpy()
    obj, reg = [rnd(o) for o in fx["obj"]], [rnd(r) for r in fx["reg"]]
    half = run_op(obj, reg, fx["anc"], case, dtype=dtype)
    full = run_op(obj, reg, fx["anc"], case)
    assert half[2].min() > 0
    for h, f in zip(half[:3], full[:3]):
        assert np.array_equal(h.view(np.int32), f.view(np.int32))
    n = half[3]["count"]
    assert np.array_equal(n, full[3]["count"])
    for k in ("index", "logit", "box"):
        for i in range(case["N"]):
            for l in range(len(R.LEVELS)):
                assert np.array_equal(half[3][k][i, l, :n[i, l]].view(np.int32), full[3][k][i, l, :n[i, l]].view(np.int32))


def device_module_inputs(case):
    from siammot_amd.structures import BoxList
    fx = fixture()
    dev, N = "cuda:0", case["N"]
    shared = [torch.from_numpy(a).to(dev) for a in fx["anc"]]
    anchors = [[BoxList(a, R.IMAGE_WH) for a in shared] for _ in range(N)]
    return anchors, [torch.from_numpy(o[:N].copy()).to(dev) for o in fx["obj"]], [torch.from_numpy(r[:N].copy()).to(dev) for r in fx["reg"]]


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
        syncs = [x for x in w if "synchroniz" in str(x.message).lower()]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, syncs


@pytest.mark.gpu
def test_module_returns_the_raw_rows_with_one_host_copy():
    import siammot_amd.ops as ops
    from siammot_amd.rpn import RPNPostProcessor
    case = R.GOLDEN_CASES["n2_clip_post32_min4"]
    anchors, obj, reg = device_module_inputs(case)
    post = RPNPostProcessor(case["pre"], case["post"], R.NMS_THRESH, case["min_size"], fpn_post_nms_top_n=case["fpn"],
                            amodal=case["amodal"]).eval()
    raw_args = (obj, reg, [[a.bbox for a in per] for per in anchors], [R.IMAGE_WH] * case["N"], case["pre"], case["post"],
                case["fpn"], R.NMS_THRESH, case["min_size"])
    post(anchors, obj, reg)                                  # (library load, workspace allocation)
    before = ops.FALLBACKS["rpn_torch"]
    res, syncs = count_syncs(lambda: post(anchors, obj, reg))
    assert len(syncs) == 1, "expected ONE device->host copy, saw %d: %s" % (len(syncs), [str(x.message)[:80] for x in syncs])
    (boxes, scores, count), syncs = count_syncs(lambda: ops.rpn_proposals(*raw_args, amodal=case["amodal"]))
    assert len(syncs) == 0, [str(x.message)[:80] for x in syncs]
    assert ops.FALLBACKS["rpn_torch"] == before
    count = count.cpu().tolist()
    assert len(res) == case["N"]
    for i, bl in enumerate(res):
        assert bl.mode == "xyxy" and tuple(bl.size) == R.IMAGE_WH and bl.fields() == ["objectness"] and len(bl) == count[i] > 0
        assert torch.equal(bl.bbox, boxes[i, :count[i]]) and torch.equal(bl.get_field("objectness"), scores[i, :count[i]])


@pytest.mark.gpu
def test_call_above_a_capacity_takes_the_torch_path():
    import siammot_amd.ops as ops
    from siammot_amd.rpn import RPNPostProcessor
    case = R.GOLDEN_CASES["n2_clip_post32_min4"]
    anchors, obj, reg = device_module_inputs(case)
    mk = lambda fpn: RPNPostProcessor(case["pre"], case["post"], R.NMS_THRESH, case["min_size"], fpn_post_nms_top_n=fpn,
                                      amodal=case["amodal"]).eval()
    before = ops.FALLBACKS["rpn_torch"]
    hip = mk(2048)(anchors, obj, reg)                        # both above the total: every kept row, best first
    assert ops.FALLBACKS["rpn_torch"] == before
    tor = mk(3000)(anchors, obj, reg)
    assert ops.FALLBACKS["rpn_torch"] == before + 1
    fx = fixture()
    for i in range(case["N"]):
        assert len(hip[i]) == len(tor[i]) > 100
        bound = 0.0
        for l in range(len(R.LEVELS)):
            idx = R.select(R.flatten_logits(fx["obj"][l])[i], min(case["pre"], fx["anc"][l].shape[0]))
            _, err_ref, ulp = decode_bound(R.flatten_regression(fx["reg"][l])[i][idx], fx["anc"][l][idx])
            bound = max(bound, 2 * err_ref + ulp)
        # both sides are fp32 evaluations whose exp differs: each within the bound of the fp64 values
        assert float((hip[i].bbox - tor[i].bbox).abs().max()) <= 2 * bound
        a, b = hip[i].get_field("objectness").cpu().numpy(), tor[i].get_field("objectness").cpu().numpy()
        assert np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64)).max() <= 4


@pytest.mark.gpu
def test_non_finite_logits_stay_in_range():
    fx = fixture()
    rng = np.random.RandomState(5)
    obj = [o.copy() for o in fx["obj"]]
    for o in obj:
        m = rng.rand(*o.shape)
        o[m < 0.02] = np.nan
        o[(m >= 0.02) & (m < 0.04)] = np.inf
        o[(m >= 0.04) & (m < 0.06)] = -np.inf
        o[(m >= 0.06) & (m < 0.07)] = -np.float32(np.nan)
    case = dict(N=2, pre=256, post=32, fpn=100, min_size=0, amodal=False)
    boxes, scores, count, cand = run_op(obj, fx["reg"], fx["anc"], case)
    assert ((count >= 0) & (count <= case["fpn"])).all()
    for l, a in enumerate(fx["anc"]):
        k = min(case["pre"], len(a))
        assert (cand["count"][:, l] == k).all()
        idx = cand["index"][:, l, :k]
        assert ((idx >= 0) & (idx < len(a))).all()
        for i in range(2):
            assert len(np.unique(idx[i])) == k
