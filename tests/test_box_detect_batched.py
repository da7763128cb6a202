"""The box head over the images of a call: ``ops.box_detect_post_batched`` (csrc/box_detect.hip), ``ops.roi_align_levels_batched``,
``poolers.Pooler`` / ``TrackBoxHead.forward`` / ``detector.DetectionHead`` on several images.

The contract is equality with the single-image path, which tests/test_box_detect.py pins to the reference: every output of
image b of a batched call equals, bit for bit, what the single-image op returns on that image's rows alone.

CPU: header, ctypes table and library agree on the three new symbols; the entry refuses bad row ranges before any launch; the
second wiring image leaves the same coarse margins on the CPU oracle as the first.
GPU: the raw op against the single-image op as bytes (tails and counts included), isolation of the images, determinism, the
pooler on three images in four map forms, ``TrackBoxHead.forward`` and ``DetectionHead`` with ONE device-to-host copy for the
whole call, and the per-image path over capacity."""
import ctypes
import math

import numpy as np
import pytest
import torch

import box_detect_cases as B
import test_box_detect as T

F32 = np.float32
XFORM_CLIP = math.log(1000.0 / 16)
NEW_SYMBOLS = ("smot_roi_align_levels_batched_typed_fwd", "smot_box_detect_post_batched_ws_bytes",
               "smot_box_detect_post_batched_fwd")
# the batches of the raw-op tests: case names, None = an image of zero rows
BATCHES = dict(k2=("d_m300_k2", "d_m64_c0_k2", "x_m2048_k2"),          # a count of zero, the 2048-row capacity: nblk 5 / 1 / 32
               k3=("d_m300_k3", None, "d_m512_c300_k3"),
               edge=("edge_k4", None, "edge_k4"))
WIRING_SEED_2 = 152            # the second image of the wiring tests (chosen on the CPU: the oracle test below)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def _library():
    import siammot_amd.ops as ops
    import os
    if not os.path.exists(ops.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ops, ops.load_library()


def test_header_ops_table_and_library_agree_on_the_batched_symbols():
    ops, lib = _library()
    for name in NEW_SYMBOLS:
        assert name in T._header_symbols() and name in ops.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.smot_abi_version() == ops.ABI_VERSION == 14          # additive: the ABI version stands
    assert ops.box_detect_mask_bytes_batched([300, 0, 2048], 2) == ops.box_detect_mask_bytes(300, 2) + ops.box_detect_mask_bytes(2048, 2)


def test_batched_entry_refuses_bad_row_ranges_before_any_launch():
    ops, lib = _library()
    BAD_ARG = -1

    def call(num_images, row_start, M, K=2):
        rs = (ctypes.c_int * (ops.MAX_IMAGES + 2))(*row_start)
        rc = lib.smot_box_detect_post_batched_fwd(None, 5 * K, K, K, None, None, M, 10.0, 10.0, 5.0, 5.0, XFORM_CLIP, 0.0, 0.0,
                                                  0.05, 0.5, None, None, None, None, None, None, None, num_images,
                                                  ctypes.cast(rs, ctypes.c_void_p))
        return rc, lib.smot_last_error()
    rc, msg = call(0, [0], 0)
    assert rc == BAD_ARG and b"num_images=0" in msg
    rc, msg = call(65, [0] * 66, 0)
    assert rc == BAD_ARG and b"num_images=65" in msg
    rc, msg = call(2, [1, 8, 16], 16)
    assert rc == BAD_ARG and b"row_start[0]=1" in msg
    rc, msg = call(3, [0, 8, 4, 16], 16)
    assert rc == BAD_ARG and b"decreases at image 1" in msg
    rc, msg = call(2, [0, 8, 16], 17)
    assert rc == BAD_ARG and b"expected N=17" in msg
    rc, msg = call(2, [0, 8, 2057], 2057)
    assert rc == BAD_ARG and b"M=2049 not in [1,2048]" in msg           # bd_check_shapes' text
    # a legal split (an image without rows included) reaches the pointer check: the row ranges came first
    rc, msg = call(3, [0, 8, 8, 2056], 2056)
    assert rc != 0 and b"null pointer" in msg

    def ws(num_images, row_start, K=2):
        rs = (ctypes.c_int * (ops.MAX_IMAGES + 2))(*row_start)
        return lib.smot_box_detect_post_batched_ws_bytes(num_images, ctypes.cast(rs, ctypes.c_void_p), K)
    for m in (1, 64, 65, 300, 2048):
        assert ws(1, [0, m]) == lib.smot_box_detect_post_ws_bytes(m, 2) > 0          # one image: the single-image layout
        assert ws(1, [0, m], 17) == lib.smot_box_detect_post_ws_bytes(m, 17)
    assert ws(2, [0, 0, 0]) > 0                                      # no rows at all: the counters of two images
    assert ws(3, [0, 300, 300, 364]) >= ws(1, [0, 300]) + ws(1, [0, 64]) >= ops.box_detect_mask_bytes_batched([300, 0, 64], 2)
    assert ws(0, [0]) == ws(65, [0] * 66) == ws(2, [1, 8, 16]) == ws(2, [0, 8, 4]) == ws(1, [0, 2049]) == ws(1, [0, 8], 1) == -1


def _image_inputs(seed):
    """Maps and proposals of one wiring image from ``seed``: the generator of ``test_box_detect._wiring_inputs`` (same draws in
    the same order — seed 121 gives its maps and boxes) without the head, which stays the first image's."""
    w = T.WIRING
    rs = np.random.RandomState(seed)
    W, H = w["image_wh"]
    feats = [rs.standard_normal((1, w["channels"], H // s, W // s)).astype(F32) for s in (4, 8, 16, 32)]
    gxy = rs.uniform(0.0, 1.0, (w["groups"], 2)) * (W - 90.0, H - 70.0)
    gwh = rs.uniform(24.0, 80.0, (w["groups"], 2))
    g = rs.randint(0, w["groups"], w["rows"])
    xy = gxy[g] + rs.uniform(-0.15, 0.15, (w["rows"], 2)) * gwh[g]
    boxes = np.concatenate((xy, xy + gwh[g] * rs.uniform(0.9, 1.1, (w["rows"], 2))), 1).astype(F32)
    boxes[w["valid"]:] = 0.0
    return feats, boxes


def _second_image_inputs():
    return _image_inputs(WIRING_SEED_2)


def test_second_wiring_image_leaves_coarse_margins_on_the_cpu_oracle():
    from oracle import box_head_oracle as BO
    from siammot_amd.structures import BoxList
    w = T.WIRING
    _, _, head = T._wiring_inputs()
    feats, boxes = _second_image_inputs()
    f0, b0, _ = T._wiring_inputs()                                  # the copied generator is the first image's, draw for draw
    f1, b1 = _image_inputs(w["seed"])
    assert np.array_equal(b0, b1) and all(np.array_equal(x, y) for x, y in zip(f0, f1)) and not np.array_equal(boxes, b0)
    fe = head.feature_extractor
    with torch.no_grad():
        x = BO.OraclePooler(7, fe.pooler.scales, 2)([torch.from_numpy(f) for f in feats],
                                                    [BoxList(torch.from_numpy(boxes[:w["valid"]].copy()), w["image_wh"])])
        h = torch.relu(fe.fc7(torch.relu(fe.fc6(x.reshape(x.shape[0], -1)))))
        ho = torch.cat(head.predictor(h), 1).numpy()
    c = T._wiring_case(np.concatenate((ho, np.zeros((w["rows"] - w["valid"], ho.shape[1]), F32))), boxes)
    cond = B.conditions(c, score_bound=w["score_margin"], delta=w["delta"])
    print(cond)
    assert cond["score_margin"] > w["score_margin"] and cond["score_gap"] > 2 * w["score_margin"] and cond["iou_clear"], cond
    assert cond["same_decisions"] and 0 < cond["survivors"] < cond["candidates"]
    assert min(B.reference_eval(c)["f32"]["counts"][1:]) > 0


# ---- GPU: the raw op ----------------------------------------------------------------------------------------------------
def _batch(key):
    """-> (cases (None: an image of zero rows), head_out [M, ld], boxes [M, 4], rows per image, counts)."""
    cases = [None if n is None else B.case(n) for n in BATCHES[key]]
    first = next(c for c in cases if c is not None)
    for c in cases:
        if c is not None:
            assert all(c[k] == first[k] for k in ("num_classes", "reg_classes", "weights", "clip_wh", "score_thresh", "nms_thresh"))
            assert c["head_out"].shape[1] == first["head_out"].shape[1]
    ho = np.concatenate([c["head_out"] for c in cases if c is not None])
    bx = np.concatenate([c["boxes"] for c in cases if c is not None])
    rows = [0 if c is None else c["M"] for c in cases]
    counts = [0 if c is None else c["count"] for c in cases]
    return cases, ho, bx, rows, counts


def _launch_batched(cases, ho, bx, rows, counts):
    import siammot_amd.ops as ops
    dev = "cuda:0"
    c = next(c for c in cases if c is not None)
    out = ops.box_detect_post_batched(torch.from_numpy(np.ascontiguousarray(ho)).to(dev), c["num_classes"], c["reg_classes"],
                                      torch.from_numpy(np.ascontiguousarray(bx)).to(dev), rows,
                                      torch.tensor(counts, dtype=torch.int32, device=dev), c["weights"], XFORM_CLIP,
                                      c["clip_wh"], c["score_thresh"], c["nms_thresh"])
    return [t.cpu().numpy() for t in out]


def _image(out, rows, b, K):
    """Image b's share of a batched call's outputs, shaped as the single-image op returns them."""
    lo, hi = sum(rows[:b]) * (K - 1), sum(rows[:b + 1]) * (K - 1)
    return [out[0][lo:hi], out[1][lo:hi], out[2][lo:hi], out[3][lo:hi], out[4][b]]


def _single(c, ho, bx, rows, b):
    """The single-image op on image b's rows of the batch's inputs (zero rows: the empty outputs and zero counts)."""
    K = c["num_classes"]
    if rows[b] == 0:
        return [np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(K, np.int32)]
    lo, hi = sum(rows[:b]), sum(rows[:b + 1])
    return T._launch(c, ho[lo:hi], bx[lo:hi])


def _assert_images_equal_singles(out, cases, ho, bx, rows, which=None):
    first = next(c for c in cases if c is not None)
    K = first["num_classes"]
    assert out[4].shape == (len(rows), K) and out[0].shape == (sum(rows) * (K - 1), 4)
    for b, c in enumerate(cases):
        if which is not None and b not in which:
            continue
        got, want = _image(out, rows, b, K), _single(c or first, ho, bx, rows, b)
        print("image %d: counts %s, single-image op %s" % (b, got[4].tolist()[:8], want[4].tolist()[:8]))
        assert [g.dtype for g in got] == [w.dtype for w in want] and [g.shape for g in got] == [w.shape for w in want]
        assert T._same_bits(got, want), "image %d of the batch differs from the single-image op" % b


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(BATCHES))
def test_every_image_equals_the_single_image_op_bit_for_bit(key):
    cases, ho, bx, rows, counts = _batch(key)
    out = _launch_batched(cases, ho, bx, rows, counts)
    _assert_images_equal_singles(out, cases, ho, bx, rows)
    if key == "k3":                                                  # ... and the reference, per image
        for b, name in enumerate(BATCHES[key]):
            if name is not None:
                T._check_against_reference(_image(out, rows, b, 3), cases[b], B.reference(name))
    if key == "edge":                                                # class 2 has no candidate in either image
        assert out[4][:, 2].tolist() == [0, 0, 0] and out[4][1].tolist() == [0, 0, 0, 0] and out[4][0, 1] == 116 - 5


@pytest.mark.gpu
def test_images_are_isolated():
    cases, ho, bx, rows, counts = _batch("k3")
    clean = _launch_batched(cases, ho, bx, rows, counts)
    # rows at and beyond count[2] of the third image do not exist for anybody
    lo = rows[0] + rows[1] + counts[2]
    assert lo < sum(rows)
    for a, b in ((np.nan, 1e30), (1e30, np.nan)):
        h2, b2 = ho.copy(), bx.copy()
        h2[lo:], b2[lo:] = a, b
        assert T._same_bits(_launch_batched(cases, h2, b2, rows, counts), clean)
    # NaN logits in three surviving rows of image 0: image 0 changes as the single-image op does, nobody else changes
    d = B.reference("d_m300_k3")["f32"]
    victims = [int(d["rows"][0]), int(d["rows"][len(d["rows"]) // 2]), int(d["rows"][-1])]
    dirty = ho.copy()
    dirty[victims[0], 0] = np.nan
    dirty[victims[1], 2] = np.nan
    dirty[victims[2], 1] = np.inf
    got = _launch_batched(cases, dirty, bx, rows, counts)
    _assert_images_equal_singles(got, cases, dirty, bx, rows, which=(0,))
    g0 = _image(got, rows, 0, 3)
    assert not set(victims) & set(g0[3][:g0[4][0]].tolist()) and g0[4][0] < _image(clean, rows, 0, 3)[4][0]
    for b in (1, 2):
        assert T._same_bits(_image(got, rows, b, 3), _image(clean, rows, b, 3))


@pytest.mark.gpu
def test_two_runs_of_the_capacity_batch_give_the_same_bits():
    batch = _batch("k2")
    assert max(batch[3]) == 2048
    assert T._same_bits(_launch_batched(*batch), _launch_batched(*batch))


# ---- GPU: the pooler ----------------------------------------------------------------------------------------------------
POOL_SCALES = (0.25, 0.125, 0.0625, 0.03125)


def _pooler_inputs():
    rs = np.random.RandomState(77)
    W, H = T.WIRING["image_wh"]
    feats = [rs.standard_normal((3, 16, H // s, W // s)).astype(F32) for s in (4, 8, 16, 32)]

    def boxes(n):
        side = np.resize(np.array([30.0, 90.0, 150.0, 200.0, 300.0, 500.0, 700.0]), n) * rs.uniform(0.95, 1.05, n)
        wh = np.stack((side * rs.uniform(0.8, 1.25, n), side), 1)
        xy = rs.uniform(-20.0, 1.0, (n, 2)) * (1.0, 1.0) + rs.uniform(0.0, 1.0, (n, 2)) * (W * 0.6, H * 0.6)
        return np.concatenate((xy, xy + wh), 1).astype(F32)
    per_image = [boxes(40), np.zeros((0, 4), F32), boxes(7)]
    for b in (per_image[0], per_image[2]):                           # all four levels: LevelMapper on the box's own area
        s = np.sqrt((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1))
        lvl = np.clip(np.floor(4 + np.log2(s / 224 + 1e-6)), 2, 5)
        assert set(lvl.tolist()) == {2.0, 3.0, 4.0, 5.0}
    return feats, per_image


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("fp32", "fp16", "channels_last", "fp32_out14"))
def test_pooler_on_three_images_equals_the_single_image_calls(form):
    import siammot_amd.ops as ops
    from siammot_amd.poolers import Pooler
    from siammot_amd.structures import BoxList
    dev = "cuda:0"
    feats, per_image = _pooler_inputs()
    x = [torch.from_numpy(f).to(dev) for f in feats]
    if form == "fp16":
        x = [f.half() for f in x]
    if form == "channels_last":
        x = [f.contiguous(memory_format=torch.channels_last) for f in x]
        assert ops._levels_layout(x, 4) == ops.FEAT_CHANNELS_LAST
    size = 14 if form == "fp32_out14" else 7
    pooler = Pooler(size, POOL_SCALES, 2)
    lists = [BoxList(torch.from_numpy(b).to(dev), T.WIRING["image_wh"]) for b in per_image]
    got = pooler(x, lists)
    singles = [pooler([f[b:b + 1] for f in x], [lists[b]]) for b in range(3)]
    assert [tuple(s.shape) for s in singles] == [(40, 16, size, size), (0, 16, size, size), (7, 16, size, size)]
    want = torch.cat(singles, 0)
    assert got.dtype == torch.float32 and got.shape == want.shape == (47, 16, size, size)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert float(got.abs().max()) > 0.1
    if form == "fp32":
        rois = torch.cat([l.bbox for l in lists], 0)
        for rows in ([40, 0, 6], [40, 7], [47, 0, 0, 0], [40, -1, 8]):
            with pytest.raises(RuntimeError):
                ops.roi_align_levels_batched(x, rois, rois, rows, 7, POOL_SCALES, 2)
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.roi_align_levels_batched(x, rois.cpu(), rois.cpu(), [40, 0, 7], 7, POOL_SCALES, 2)


# ---- GPU: the modules ---------------------------------------------------------------------------------------------------
def _wiring_batch(dev):
    """Image 0 = the wiring inputs as they are, image 1 = no proposals (maps of another seed), image 2 = the second seed."""
    w = T.WIRING
    feats0, boxes0, head = T._wiring_inputs()
    feats2, boxes2 = _second_image_inputs()
    rs = np.random.RandomState(9)
    feats1 = [rs.standard_normal(f.shape).astype(F32) for f in feats0]
    feats = [torch.from_numpy(np.concatenate(fs)).to(dev) for fs in zip(feats0, feats1, feats2)]
    return head.to(dev), feats, [boxes0, np.zeros((0, 4), F32), boxes2]


@pytest.mark.gpu
def test_track_box_head_on_two_images_and_an_empty_one():
    import siammot_amd.ops as ops
    from siammot_amd.structures import BoxList
    w, dev = T.WIRING, "cuda:0"
    head, feats, boxes = _wiring_batch(dev)
    rows, valid = [w["rows"], 0, w["rows"]], [w["valid"], 0, w["valid"]]
    bx = torch.from_numpy(np.concatenate(boxes)).to(dev)
    count = torch.tensor(valid, dtype=torch.int32, device=dev)
    raw = head.detect_raw_batched(feats, bx, rows, count, w["image_wh"])
    ho = raw[6].cpu().numpy()
    assert raw[5].shape == (2 * w["rows"], w["dim"]) and ho.shape == (2 * w["rows"], w["classes"] * 5)
    assert raw[4].shape == (3, w["classes"]) and raw[4][1].tolist() == [0] * w["classes"]
    out = [t.cpu().numpy() for t in raw[:5]]
    refs = {}
    for b, lo in ((0, 0), (2, w["rows"])):                           # the restated PostProcessor on the head outputs of the call
        c = T._wiring_case(ho[lo:lo + w["rows"]], boxes[b])
        ref = refs[b] = B.reference_eval(c)
        cond = B.conditions(c, ref, score_bound=w["score_margin"], delta=w["delta"])
        print(b, cond)
        assert cond["score_margin"] > w["score_margin"] and cond["score_gap"] > 2 * w["score_margin"] and cond["iou_clear"], cond
        T._check_against_reference(_image(out, rows, b, w["classes"]), c, ref)
    # forward: one device-to-host copy for the three images
    props = [BoxList(torch.from_numpy(b[:n].copy()).to(dev), w["image_wh"]) for b, n in zip(boxes, valid)]
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        (x, res, losses), syncs = T._count_syncs(lambda: head(feats, props))
        singles = [head([f[b:b + 1] for f in feats], [props[b]]) for b in (0, 2)]
    print("host copies of the three-image call: %d" % syncs)
    assert syncs == 1 and losses == {} and dict(ops.FALLBACKS) == before
    assert len(res) == 3 and x.shape == (2 * w["valid"], w["dim"])
    empty = res[1]
    assert len(empty) == 0 and empty.fields() == ["scores", "ids", "labels"] and tuple(empty.size) == w["image_wh"]
    for (b, lo), (xs, single, _) in zip(((0, 0), (2, w["valid"])), singles):
        a, s, d = res[b], single[0], refs[b]["f32"]
        assert a.fields() == ["scores", "ids", "labels"] and a.mode == "xyxy" and tuple(a.size) == w["image_wh"]
        assert len(a) == len(s) == d["counts"][0] > 0
        assert a.get_field("labels").tolist() == s.get_field("labels").tolist() == d["labels"].tolist()
        assert (a.get_field("ids") == -1).all() and a.get_field("ids").dtype == torch.int64
        assert (a.bbox - s.bbox).abs().max() < w["delta"] and np.abs(a.bbox.cpu().numpy() - d["boxes"]).max() < w["delta"]
        assert (a.get_field("scores") - s.get_field("scores")).abs().max() < w["score_margin"]
        assert np.abs(a.get_field("scores").cpu().numpy() - d["scores"]).max() < w["score_margin"]
        np.testing.assert_allclose(x[lo:lo + w["valid"]].cpu().numpy(), xs.cpu().numpy(), rtol=1e-4, atol=1e-5)
    # an injected NMS: the per-image path, counted once per image
    head.post_processor.nms_fn = lambda boxlist, thresh: boxlist
    count_before = ops.FALLBACKS["box_detect_torch"]
    with torch.no_grad():
        x2, res2, _ = head(feats, props)
    assert ops.FALLBACKS["box_detect_torch"] == count_before + 3
    assert x2.shape == x.shape and [len(r) >= len(a) for r, a in zip(res2, res)] == [True] * 3 and len(res2[1]) == 0


@pytest.mark.gpu
def test_a_call_whose_images_are_all_empty_returns_empty_boxlists():
    import siammot_amd.ops as ops
    from siammot_amd.structures import BoxList
    w, dev = T.WIRING, "cuda:0"
    head, feats, _ = _wiring_batch(dev)
    feats = [f[:2].contiguous() for f in feats]
    props = [BoxList(torch.zeros((0, 4), device=dev), w["image_wh"]) for _ in range(2)]
    assert head.detect_batch_ok(props)
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        (x, res, losses), syncs = T._count_syncs(lambda: head(feats, props))
    assert syncs == 1 and losses == {} and dict(ops.FALLBACKS) == before
    assert x.shape == (0, w["dim"]) and x.dtype == torch.float32 and len(res) == 2
    for r in res:
        assert len(r) == 0 and r.bbox.shape == (0, 4) and r.fields() == ["scores", "ids", "labels"]
        assert tuple(r.size) == w["image_wh"] and r.get_field("ids").dtype == r.get_field("labels").dtype == torch.int64
    raw = head.detect_raw_batched(feats, torch.zeros((0, 4), device=dev), [0, 0], torch.zeros(2, dtype=torch.int32, device=dev),
                                  w["image_wh"])
    assert raw[4].cpu().tolist() == [[0] * w["classes"]] * 2 and raw[0].shape == (0, 4) and raw[6].shape == (0, w["classes"] * 5)
    # the raw op wants exactly one count per image, and [M, 4] boxes, as RuntimeErrors
    bx, ho = torch.zeros((8, 4), device=dev), torch.zeros((8, w["classes"] * 5), device=dev)
    tail = ((10.0, 10.0, 5.0, 5.0), XFORM_CLIP, w["image_wh"], 0.05, 0.5)
    with pytest.raises(RuntimeError, match="count"):
        ops.box_detect_post_batched(ho, 3, 3, bx, [4, 4], torch.zeros(3, dtype=torch.int32, device=dev), *tail)
    with pytest.raises(RuntimeError, match=r"\[M, 4\]"):
        ops.box_detect_post_batched(ho, 3, 3, torch.zeros((), device=dev), [4, 4], torch.zeros(2, dtype=torch.int32, device=dev),
                                    *tail)


@pytest.mark.gpu
def test_over_the_summed_capacity_forward_goes_image_by_image(monkeypatch):
    import siammot_amd.ops as ops
    from siammot_amd.structures import BoxList
    w, dev = T.WIRING, "cuda:0"
    head, feats, boxes = _wiring_batch(dev)
    feats = [f[[0, 2]].contiguous() for f in feats]
    props = [BoxList(torch.from_numpy(boxes[b][:w["valid"]].copy()).to(dev), w["image_wh"]) for b in (0, 2)]
    one = ops.box_detect_mask_bytes(w["valid"], w["classes"])
    assert head.detect_batch_ok(props)
    monkeypatch.setattr(ops, "BOX_DETECT_MAX_MASK_BYTES", one + one // 2)      # each image fits, the two together do not
    assert not head.detect_batch_ok(props) and all(head.detect_ok(p) for p in props)

    def no_batch(*a, **k):
        raise AssertionError("the batched device path was taken")
    monkeypatch.setattr(head, "detect_raw_batched", no_batch)
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        (x, res, _), syncs = T._count_syncs(lambda: head(feats, props))
        singles = [head([f[b:b + 1] for f in feats], [props[b]]) for b in range(2)]
    assert syncs == 2 and dict(ops.FALLBACKS) == before
    assert torch.equal(x, torch.cat([s[0] for s in singles], 0))
    for a, (_, s, _) in zip(res, singles):
        assert len(a) == len(s[0]) > 0 and torch.equal(a.bbox, s[0].bbox)
        for f in ("scores", "ids", "labels"):
            assert torch.equal(a.get_field(f), s[0].get_field(f))


@pytest.mark.gpu
def test_detection_head_on_two_images_with_one_host_copy():
    import bench
    import rpn_proposal_cases as R
    import siammot_amd.ops as ops
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.detector import build_detection_head
    from siammot_amd.emm import EMM
    from siammot_amd.structures import BoxList
    from siammot_amd.track_utils import build_track_utils
    dev = "cuda"
    cfg = T._small_cfg(bench.CHANNELS, 2, 64)
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    image_wh = (bench.NET_HW[1], bench.NET_HW[0])
    torch.manual_seed(0)
    det_head = build_detection_head(cfg, BoxCoder(R.WEIGHTS), bench.CHANNELS).to(dev)
    with torch.no_grad():
        det_head.box_head.predictor.bbox_pred.weight.mul_(0.02)
        det_head.box_head.predictor.cls_score.weight.mul_(4.0)
    obj, reg = R.golden_inputs(0, num_images=2)
    obj, reg = [torch.from_numpy(o).to(dev) for o in obj], [torch.from_numpy(r).to(dev) for r in reg]
    level_anchors = [torch.from_numpy(a).to(dev) for a in R.anchors()]
    anchors = [[BoxList(a, image_wh) for a in level_anchors] for _ in range(2)]
    per_image = [bench.synthetic_features(100 + b, dev) for b in range(2)]
    feats = tuple(torch.cat(fs, 0) for fs in zip(*per_image))
    assert det_head.raw_ok(anchors, obj)
    before = dict(ops.FALLBACKS)
    res, syncs = T._count_syncs(lambda: det_head(anchors, obj, reg, feats))

    def image_by_image():
        return [det_head([anchors[b]], [o[b:b + 1] for o in obj], [r[b:b + 1] for r in reg], per_image[b])[0] for b in range(2)]
    singles, syncs_singles = T._count_syncs(image_by_image)
    assert dict(ops.FALLBACKS) == before
    print("host copies: one call %d, image by image %d; detections %s" % (syncs, syncs_singles, [len(r) for r in res]))
    assert syncs == 1 and syncs_singles == 2 and len(res) == 2
    for a, s in zip(res, singles):
        assert len(a) == len(s) > 0 and a.fields() == ["scores", "ids", "labels"] and tuple(a.size) == image_wh
        assert a.get_field("labels").tolist() == s.get_field("labels").tolist()
        assert (a.get_field("ids") == -1).all()
        np.testing.assert_allclose(a.bbox.cpu().numpy(), s.bbox.cpu().numpy(), rtol=0, atol=1e-2)
        np.testing.assert_allclose(a.get_field("scores").cpu().numpy(), s.get_field("scores").cpu().numpy(), rtol=0, atol=1e-4)
    # ... and the B BoxLists are what the batched EMM extraction takes, as they are
    emm = EMM(cfg, build_track_utils(cfg)).to(dev).eval()
    with torch.no_grad():
        z, srs, dets = emm.extract_cache(feats, res)
    n = sum(len(r) for r in res)
    assert z.shape == (n, bench.CHANNELS, emm.rz, emm.rz) and len(srs) == len(dets) == 2
    assert [len(s) for s in srs] == [len(r) for r in res] and all(s.bbox.shape[1] == 4 for s in srs)
