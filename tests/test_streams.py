"""Streams: every entry of the library launches on the CURRENT torch stream of its tensors' device, scratch is kept per
(device, stream), and an image that a module computes once and keeps (packed weights, anchor grids) is complete for every
stream that reads it (``ops.StreamImage``).  Helpers: tests/stream_cases.py.

(a) every operator family off the default stream, behind a 20 ms busy kernel, returns the default stream's bits: a launch,
    memset or copy that went to the null stream would run 20 ms before its producers and read something else;
(b) a cached image packed on stream A — late: A is busy for 20 ms and the image holds NaN until then — is complete for a
    consumer on stream B that follows at once, with no host synchronisation; the same after a parameter changed in place;
(c) two streams working at once on two data sets, enqueued interleaved from one thread, give the bits of the same calls made
    one after the other on the default stream;
(d) CPU: the helpers import without a device, CPU tensors never reach the ordering code, and the ``ops`` names the wrappers
    of (b) patch are the names the modules call.

Every yardstick is the library's own result on the default stream, compared bit for bit: nothing here depends on a tolerance.
"""
import inspect
import math
import time

import numpy as np
import pytest
import torch

import stream_cases as S

DEV = S.DEV
F32 = np.float32
SCALES = (0.25, 0.125, 0.0625, 0.03125)
SMALL = ((12, 20), (6, 10))                                     # the two map sizes of the module tests
XFORM_CLIP = math.log(1000.0 / 16)
YAML_WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ops():
    import siammot_amd.ops as ops
    ops.load_library()
    return ops


# =========================================================================================================================
# (a) every operator off the default stream returns the default stream's bits
# =========================================================================================================================
def _off_default(op, x1, x2):
    """The procedure of (a): references of X2, then X1, on the default stream (so that a stale intermediate in a reused block
    is X1's); X2 on a fresh side stream behind a spin; X1 on the default stream again."""
    torch.cuda.synchronize()                                     # inputs made on the default stream are complete
    ref2 = op(x2)
    ref1 = op(x1)
    torch.cuda.synchronize()
    (side,) = S.fresh_streams(1, apart_from=[torch.cuda.current_stream()])   # (beside the default stream: see runs_beside)
    with torch.cuda.stream(side):
        S.spin()
        out = op(x2)
    side.synchronize()
    assert not S.bits_equal(ref1, ref2), "the two input sets give one result: the comparison below would prove nothing"
    assert S.bits_equal(out, ref2), "the side stream's result is not the default stream's"
    again = op(x1)
    torch.cuda.synchronize()
    assert S.bits_equal(again, ref1), "the default stream's result changed after the side stream's call"


# ---- the head's operators: C = 32, 3 tracks, four levels from 96 x 160 down ------------------------------------------------
EMM_WH, EMM_C = (640, 384), 32
EMM_BOXES = (np.array([(40.3, 50.7, 71.9, 114.2), (150.5, 60.25, 214.0, 187.5), (250.0, 100.0, 349.5, 299.0)], F32),
             np.array([(300.2, 30.1, 459.7, 349.9), (60.0, 200.0, 130.0, 330.0), (480.5, 90.25, 600.0, 260.0)], F32))


def _emm_maps(seed, B=1):
    import golden_inputs as gi
    rs = np.random.RandomState(seed)
    return tuple(_d(rs.standard_normal((B,) + s[1:]).astype(F32)) for s in gi.feature_shapes(EMM_WH, EMM_C)[:4])


def _emm_params(seed=3):
    import golden_inputs as gi
    return {k: _d(v) for k, v in gi.predictor_params(np.random.RandomState(seed), EMM_C, EMM_BOXES[0]).items()}


def _head_inputs():
    """Two sets (maps A, maps B, boxes) and, made on the default stream, what the later stages of the chain take."""
    ops = _ops()
    params, sets = _emm_params(), []
    for k in (0, 1):
        fa, fb, boxes = _emm_maps(10 + k), _emm_maps(20 + k), _d(EMM_BOXES[k])
        sr = ops.search_region(boxes, 512, 1.0, 0)
        z = ops.roi_align_levels(fa, boxes, boxes, 15, SCALES, 2)
        resp, pooled = ops.sr_xcorr_fused(fb, boxes, sr, z, 30, 15, SCALES, 2, 512, return_pooled=True)
        logits = ops.emm_predictor(resp, params)
        sets.append(dict(fa=fa, fb=fb, boxes=boxes, sr=sr, z=z, resp=resp, pooled=pooled, logits=logits))
    torch.cuda.synchronize()
    return ops, params, sets


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["roi_align_levels", "sr_xcorr_fused", "xcorr_depthwise", "emm_predictor", "emm_decode"])
def test_head_operators_off_the_default_stream(family):
    ops, params, sets = _head_inputs()
    op = {
        "roi_align_levels": lambda x: (ops.roi_align_levels(x["fa"], x["boxes"], x["boxes"], 15, SCALES, 2, return_levels=True),
                                       ops.roi_align_levels(x["fb"], x["sr"], x["boxes"], 30, SCALES, 2, [128, 64, 32, 16])),
        "sr_xcorr_fused": lambda x: (ops.sr_xcorr_fused(x["fb"], x["boxes"], x["sr"], x["z"], 30, 15, SCALES, 2, 512),
                                     ops.sr_xcorr_fused(x["fb"], x["boxes"], x["sr"], x["z"], 30, 15, SCALES, 2, 512,
                                                        return_pooled=True)),
        "xcorr_depthwise": lambda x: ops.xcorr_depthwise(x["pooled"], x["z"]),
        "emm_predictor": lambda x: (ops.emm_predictor(x["resp"], params), ops.emm_predictor(x["resp"], params, winograd=False)),
        "emm_decode": lambda x: ops.emm_decode(x["logits"], x["sr"], x["boxes"], 30, 15, 512, return_index=True, clip_wh=EMM_WH),
    }[family]
    _off_default(op, sets[0], sets[1])


def _emm_module():
    from siammot_amd.config import get_default_cfg
    from siammot_amd.emm import EMM
    from siammot_amd.track_utils import build_track_utils
    cfg = get_default_cfg(channels=EMM_C)
    emm = EMM(cfg, build_track_utils(cfg)).to(DEV).eval()
    emm.predictor.load_state_dict(_emm_params())
    return emm


def _dets(boxes, id0=0):
    from siammot_amd.structures import BoxList
    n = len(boxes)
    d = BoxList(_d(boxes), EMM_WH, mode="xyxy")
    d.add_field("ids", torch.arange(id0, id0 + n, device=DEV))
    d.add_field("labels", torch.ones(n, dtype=torch.int64, device=DEV))
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("images", [1, 2])
def test_emm_module_off_the_default_stream(images):
    """``extract_cache``, then the frame pair with the extraction's order hint (``ops.emm_extract_cache`` / ``emm_track``);
    with two images the batched forms (a list of BoxLists, maps ``[2, C, H, W]``)."""
    emm = _emm_module()
    assert emm.use_order_hint
    sets = []
    for k in (0, 1):
        fa, fb = _emm_maps(30 + k, images), _emm_maps(40 + k, images)
        dets = _dets(EMM_BOXES[k]) if images == 1 else [_dets(EMM_BOXES[k]), _dets(EMM_BOXES[1 - k][:2], 10)]
        sets.append((fa, fb, dets))

    def op(x):
        fa, fb, dets = x
        with torch.no_grad():
            z, sr, d = emm.extract_cache(fa, dets)
            _, res, _ = emm(fb, d, sr, template_features=z)
        return z, sr, d, res
    _off_default(op, sets[0], sets[1])


# ---- NMS, proposals, the box head ---------------------------------------------------------------------------------------------
def _nms_set(seed, n=65):
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 300, (n, 2))
    wh = rs.uniform(30, 120, (n, 2))
    return _d(np.concatenate((xy, xy + wh), 1).astype(F32)), _d(rs.uniform(0, 1, n).astype(F32))


@pytest.mark.gpu
def test_nms_off_the_default_stream():
    ops = _ops()
    _off_default(lambda x: (ops.nms(x[0], x[1], 0.5), ops.nms_keep_mask(x[0], x[1], 0.5)), _nms_set(1), _nms_set(2))


@pytest.mark.gpu
def test_rpn_proposals_off_the_default_stream():
    import rpn_proposal_cases as R
    ops = _ops()
    case = R.GOLDEN_CASES["n2_clip_post32_min4"]
    anchors = [[_d(a) for a in R.anchors()]] * case["N"]
    sets = [tuple([_d(t[:case["N"]]) for t in part] for part in R.golden_inputs(seed, case["N"])) for seed in (5, 6)]

    def op(x):
        boxes, scores, count = ops.rpn_proposals(x[0], x[1], anchors, [R.IMAGE_WH] * case["N"], case["pre"], case["post"],
                                                 case["fpn"], R.NMS_THRESH, case["min_size"], amodal=case["amodal"])
        n = count.cpu().tolist()
        return count, [(boxes[i, :c], scores[i, :c]) for i, c in enumerate(n)]
    _off_default(op, sets[0], sets[1])


def _detect_set(seed):
    import box_detect_cases as B
    c = B.build_case("d_m65_k17", seed)
    return c, _d(c["head_out"]), _d(c["boxes"]), torch.tensor([c["count"]], dtype=torch.int32, device=DEV)


@pytest.mark.gpu
def test_box_detect_post_off_the_default_stream():
    ops = _ops()

    def op(x):
        c, ho, bx, count = x
        boxes, scores, labels, rows, cnt = ops.box_detect_post(ho, c["num_classes"], c["reg_classes"], bx, count, c["weights"],
                                                               XFORM_CLIP, c["clip_wh"], c["score_thresh"], c["nms_thresh"])
        n = int(cnt[0])
        return cnt, boxes[:n], scores[:n], labels[:n], rows[:n]
    _off_default(op, _detect_set(1400), _detect_set(1401))


def _refine_layers(g, C=16, dim6=128, dim7=64, classes=3):
    def lin(o, i):
        return (torch.randn((o, i), generator=g) / i ** 0.5).to(DEV), torch.randn((o,), generator=g).mul(0.1).to(DEV)
    return lin(dim6, C * 49) + lin(dim7, dim6) + lin(classes, dim7) + lin(4 * classes, dim7)


def _refine_set(seed, rows_per_image, C=16, classes=3):
    g = torch.Generator().manual_seed(seed)
    B, n = len(rows_per_image), sum(rows_per_image)
    feats = tuple(torch.randn((B, C, 352 // s_, 640 // s_), generator=g).to(DEV) for s_ in (1, 2, 4, 8))
    xy = torch.rand((n, 2), generator=g) * torch.tensor([1000.0, 500.0])
    wh = 20.0 + torch.rand((n, 2), generator=g) * 200.0
    return (feats, torch.cat((xy, xy + wh), 1).to(DEV), torch.randint(1, classes, (n,), generator=g).to(DEV),
            (torch.randperm(n, generator=g) + 2 ** 33).to(DEV), torch.rand((n,), generator=g).to(DEV))


@pytest.mark.gpu
def test_box_refine_off_the_default_stream():
    ops = _ops()
    layers = _refine_layers(torch.Generator().manual_seed(7))

    def op(x):
        feats, boxes, labels, ids, conf = x
        return ops.box_refine(feats, SCALES, 7, 2, boxes, labels, ids, conf, layers, YAML_WEIGHTS, XFORM_CLIP, (1280, 704), False)
    _off_default(op, _refine_set(1, [9]), _refine_set(2, [9]))


@pytest.mark.gpu
def test_box_refine_batched_off_the_default_stream():
    ops = _ops()
    layers = _refine_layers(torch.Generator().manual_seed(8))
    rows = [5, 7]                                                # two cameras

    def op(x):
        feats, boxes, labels, ids, conf = x
        return ops.box_refine_batched(feats, SCALES, 7, 2, boxes, labels, ids, conf, rows, layers, YAML_WEIGHTS, XFORM_CLIP,
                                      (1280, 704), False)
    _off_default(op, _refine_set(3, rows), _refine_set(4, rows))


@pytest.mark.gpu
def test_linear_rows_off_the_default_stream():
    ops = _ops()
    M, K, N = 33, 100, 130
    g = torch.Generator().manual_seed(11)
    w, b = (torch.randn((N, K), generator=g) / K ** 0.5).to(DEV), torch.randn((N,), generator=g).to(DEV)
    x1, x2 = torch.randn((M, K), generator=g).to(DEV), torch.randn((M, K), generator=g).to(DEV)
    _off_default(lambda x: (ops.linear_rows(x, w, b, relu=True), ops.linear_rows(x, w, None, relu=False)), x1, x2)


# ---- RPN head, FPN, DLA operators ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rpn_head_and_fpn_off_the_default_stream_with_images_already_packed():
    import fpn_cases as P
    import rpn_head_cases as H
    ops = _ops()
    C, A, cin = 32, 3, (32, 64)
    head = ops.rpn_head_pack(*[_d(v) for v in H.params(C, A)])
    prm = P.params(C, cin)
    pyramid = ops.fpn_pack([(_d(iw), _d(ib)) for iw, ib, _, _ in prm], [(_d(lw), _d(lb)) for _, _, lw, lb in prm])
    torch.cuda.synchronize()                                     # the images are complete: the caller's ordering
    sets = [([_d(v) for v in H.maps(C, 1, SMALL, seed)], [_d(v) for v in P.maps(cin, 1, SMALL, seed)]) for seed in (0, 1)]
    _off_default(lambda x: (ops.rpn_head(x[0], head, C, A), ops.fpn(x[1], pyramid, cin, C)), sets[0], sets[1])


@pytest.mark.gpu
def test_dla_operators_off_the_default_stream():
    """``dla_stem``, ``dla_conv3x3`` and ``dla_conv1x1`` at the smallest case each has in tests/test_dla.py."""
    import dla_cases as D
    ops = _ops()

    def cases(seed):
        return (D.stem_case(16, 32, (32, 32), 1, seed=seed), D.conv3x3_case(64, 64, 1, (13, 21), 1, seed=seed),
                D.conv1x1_case([(32, False), (32, False)], 32, (13, 21), 1, seed=seed))

    def dev(c):
        stem, c3, c1 = c
        return ((_d(stem["image"]), [tuple(_d(t) for t in layer) for layer in stem["layers"]]),
                tuple(_d(c3[k]) for k in ("x", "w", "scale", "shift", "residual")),
                ([_d(s) for s in c1["src"]], c1["pooled"], _d(c1["w"]), _d(c1["scale"]), _d(c1["shift"])))

    def op(x):
        (image, layers), (a, w, scale, shift, res), (src, pooled, w1, s1, b1) = x
        return (ops.dla_stem(image, layers), ops.dla_conv3x3(a, w, scale, shift, 1, res, True),
                ops.dla_conv1x1(src, pooled, w1, s1, b1, True))
    _off_default(op, dev(cases(0)), dev(cases(1)))


# ---- pre-processing ------------------------------------------------------------------------------------------------------------
def _frames(seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (90, 160, 3)).astype(np.uint8) for _ in range(2)]


def _preprocessor():
    from siammot_amd.preprocess import FramePreprocessor
    pre = FramePreprocessor(72, 128, 32, device=DEV)             # 90 x 160 frames go to 64 x 128
    assert pre.get_size((160, 90)) == (64, 128)
    return pre


@pytest.mark.gpu
def test_preprocessing_device_frames_off_the_default_stream():
    ops = _ops()
    pre = _preprocessor()
    tables = pre.tables((90, 160), (64, 128))                    # (made by blocking copies: complete when this returns)

    def op(frames):
        return (ops.preprocess_frame(frames[0], tables, (64, 128), pre.pixel_mean, pre.pixel_std, False), pre.batch(frames),
                pre.batch(frames, dtype=torch.float16, channels_last=True))
    _off_default(op, [_d(f) for f in _frames(1)], [_d(f) for f in _frames(2)])


@pytest.mark.gpu
def test_preprocessing_host_frames_off_the_default_stream():
    """Host numpy frames: the pinned staging copy, its event and the device twin of the staging buffer run on the side stream
    too.  A ``FramePreprocessor`` is a one-stream-at-a-time object (its device buffer is reused in stream order): the calls
    here follow one another, each stream synchronised before the next one's call."""
    pre = _preprocessor()

    def op(frames):
        out = pre.batch(frames).clone()                          # (the clone: on the stream of the call)
        one = pre(frames[1]).clone()
        torch.cuda.current_stream().synchronize()
        return out, one
    _off_default(op, _frames(3), _frames(4))


# ---- the track solver: its "current stream" synchronisation on a side stream ----------------------------------------------------
def _solver_set(seed, n=9):
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 400, (n, 2))
    wh = rs.uniform(60, 200, (n, 2))
    boxes = np.concatenate((xy, xy + wh), 1).astype(F32)
    return (_d(boxes), _d(rs.uniform(0.3, 1.0, n).astype(F32)), torch.full((n,), -1, dtype=torch.int64, device=DEV),
            torch.ones(n, dtype=torch.int64, device=DEV))


def _fresh_state(cap):
    state = torch.zeros(8 + 3 * cap, dtype=torch.int32, device=DEV)
    state[0] = -1
    return state


def _solved(ops, fbuf, ibuf, rec, M, state):
    """What a solver launch defines, from its record on the host ``rec`` (a numpy array): header, kept rows, ids, the rows."""
    K, A, na = int(rec[0]), int(rec[1]), int(rec[4])
    buf = ops.FrameBuffers(fbuf, ibuf, M)
    parts = [rec[lo:lo + n].copy() for lo, n in ((0, 3), (4, 4), (8, K), (8 + M, K), (8 + 2 * M, A), (8 + 3 * M, na))]
    return parts, [t.clone() for t in buf.kept(K)], [t.clone() for t in buf.active(A)], state[:5].clone(), state[8:8 + na].clone()


@pytest.mark.gpu
def test_track_solve_with_a_host_record_ring_off_the_default_stream():
    """The record arrives in pinned host memory and ``ring.wait`` is the call's one synchronisation — of the CURRENT stream.
    Behind a spin on a side stream the polling runs out and the event recorded on that stream decides: were it recorded on,
    or the wait made for, the null stream, the record would not be there (``wait_host_record`` raises) or be the last one's.
    The test itself does not synchronise between the launch and reading the record."""
    from siammot_amd.solver import TrackPool
    ops = _ops()
    cap = TrackPool.DEVICE_CAPACITY
    ring = ops.HostRecordRing(torch.device(DEV), cap)

    def op(det):
        state = _fresh_state(cap)
        fbuf, ibuf, rec, M = ops.track_solve(det, None, 1.0, (0.4, 0.6, 0.4), 0.5, 3, state, cap, host_record=ring)
        ring.record_event()
        ring.wait(rec)
        host = ring.view(rec).copy()                             # (no torch.cuda.synchronize() before this read)
        assert host[3] != 0 and int(host[7]) == M == len(det[0]) and 0 < int(host[0]) <= M
        return _solved(ops, fbuf, ibuf, host, M, state)
    _off_default(op, _solver_set(1), _solver_set(2))


@pytest.mark.gpu
def test_track_solve_batched_off_the_default_stream():
    from siammot_amd.solver import TrackPool
    ops = _ops()
    cap = TrackPool.DEVICE_CAPACITY

    def op(cameras):
        states = [_fresh_state(cap) for _ in cameras]
        bufs, rec, offsets = ops.track_solve_batched([(det, None, 1.0, (0.4, 0.6, 0.4), 0.5, 3, st, cap)
                                                      for det, st in zip(cameras, states)])
        recs = ops.track_solve_records(rec, offsets)             # its synchronisation: the current stream's
        out = []
        for b, (det, st) in enumerate(zip(cameras, states)):
            M = len(det[0])
            assert recs[b][3] != 0 and int(recs[b][7]) == M and 0 < int(recs[b][0]) <= M
            out.append(_solved(ops, bufs[b].fbuf, bufs[b].ibuf, recs[b], M, st))
        return out
    _off_default(op, [_solver_set(3), _solver_set(4, 5)], [_solver_set(5), _solver_set(6, 5)])


# =========================================================================================================================
# (b) a cached image computed on one stream is complete for every other stream
# =========================================================================================================================
def _fpn_module(compute_dtype):
    import fpn_cases as P
    from siammot_amd.fpn import FPN, LastLevelMaxPool
    cin, C = (32, 64), 32
    fpn = P.load_fpn(FPN(cin, C, top_blocks=LastLevelMaxPool(), compute_dtype=compute_dtype), P.params(C, cin), DEV)
    return fpn, [_d(v) for v in P.maps(cin, 1, SMALL)], fpn.fpn_layer1.weight


def _rpn_head_module(compute_dtype):
    import rpn_head_cases as H
    from siammot_amd.rpn import RPNHead
    C, A = 32, 3
    head = H.load_head(RPNHead(None, C, A, compute_dtype=compute_dtype), H.params(C, A), DEV)
    return head, [_d(v) for v in H.maps(C, 1, SMALL)], head.conv.weight


def _dla_module(levels, channels, shape, **kw):
    import dla_cases as D
    from siammot_amd.dla import DLA
    model = DLA(levels, channels, **kw)
    model = D.load(model, D.params(model, D.SEED), DEV)
    return model, _d(D.image(shape, D.SEED)), model.level5.root.conv.weight


def _dla34(**kw):
    import dla_cases as D
    levels, channels, shape = D.NET_CASES["A"]
    return _dla_module(levels, channels, shape, **kw)


def _dla_bottleneck():
    import dla_bottleneck_cases as DB
    levels, channels, shape, residual_root = DB.NET_CASES["F"]   # the smallest bottleneck body (200 keys, 64 x 64)
    return _dla_module(levels, channels, shape, block="bottleneck", residual_root=residual_root)


class _Grids(torch.nn.Module):
    """``AnchorGenerator.grid_anchors`` with a consumer: the grids are cached tensors, and what reads them on the stream of
    the call here is a copy."""

    def __init__(self):
        super(_Grids, self).__init__()
        from siammot_amd.rpn import AnchorGenerator
        self.gen = AnchorGenerator((32, 64), (0.5, 1.0, 2.0), (8, 16))

    def forward(self, grid_sizes):
        return [t.clone() for t in self.gen.grid_anchors(grid_sizes)]


def _anchor_module():
    grids = _Grids().to(DEV)
    return grids, SMALL, grids.gen.cell_anchors._buffers["0"]


# cache -> (the module's builder -> (module, input, the tensor the repack changes), the ``ops`` function its image comes from)
CACHES = {
    "fpn_fp32": (lambda: _fpn_module(None), "fpn_pack"),
    "fpn_fp16": (lambda: _fpn_module(torch.float16), "fpn_half_pack"),
    "rpn_head_fp32": (lambda: _rpn_head_module(None), "rpn_head_pack"),
    "rpn_head_fp16": (lambda: _rpn_head_module(torch.float16), "rpn_head_half_pack"),
    "dla34_fp32": (lambda: _dla34(operands="fp32"), "dla_pack"),
    "dla34_bf16": (lambda: _dla34(compute_dtype=torch.bfloat16), "dla_half_pack"),
    "dla_bottleneck": (_dla_bottleneck, "dla_net_pack"),
    "anchor_grids": (_anchor_module, "rpn_anchors"),
}


def _two_streams(module, x, box, ref, what):
    """Steps 3 to 5 of (b): the call under stream A (which packs, late), at once the call under stream B, the precondition
    that A's spin is still running when B's call has returned, and both results against ``ref``."""
    a, b = S.fresh_streams(2)
    calls = box.get("calls", 0)
    with torch.no_grad():
        with torch.cuda.stream(a):
            out_a = module(x)
        with torch.cuda.stream(b):
            out_b = module(x)
    still_spinning = box["spun"][-1].query() is False
    host_ms = (time.perf_counter() - box["host_t0"]) * 1e3
    torch.cuda.synchronize()
    assert box["calls"] == calls + 1, "%s: the image was packed %d times for two calls" % (what, box["calls"] - calls)
    assert still_spinning, ("%s: the spin on stream A had ended when B's call returned, %.2f ms of host time after it was enqueued: "
                            "the delay did not outlast the host's work and the comparison would prove nothing" % (what, host_ms))
    assert S.bits_equal(out_a, ref), "%s: the producing stream's own result is wrong (NaN: %s)" % (what, S.any_nan(out_a))
    assert S.bits_equal(out_b, ref), ("%s: the other stream read the image before it was written (NaN: %s)"
                                      % (what, S.any_nan(out_b)))


@pytest.mark.gpu
@pytest.mark.parametrize("cache", sorted(CACHES))
def test_cached_image_is_complete_for_every_stream(cache, monkeypatch):
    import rpn_head_cases as H
    ops = _ops()
    build, pack_name = CACHES[cache]
    torch.cuda.synchronize()
    S.cycles_per_ms()                                            # (calibrated before anything is timed against it)
    print("spin calibration: _sleep(%d) took %.3f ms -> %.0f cycles per ms, %d cycles for %g ms"
          % (S.PROBE_CYCLES, S.probe_ms(), S.cycles_per_ms(), int(S.SPIN_MS * S.cycles_per_ms()), S.SPIN_MS))

    # 1. the reference on the default stream, and an identical module with nothing packed yet
    first, x, weight = build()
    with torch.no_grad():
        ref = first(x)
        module, _, changed = build()
        module.load_state_dict(first.state_dict())
        weight.add_(1)
        ref_changed = first(x)
        warm, _, _ = build()
        warm(x)                                                  # 6.'s module: packed on the default stream
        torch.empty(8, device=DEV).fill_(float("nan"))            # (the wrapper's fill kernel is loaded before it is timed)
    torch.cuda.synchronize()
    assert not S.any_nan(ref) and not S.any_nan(ref_changed) and not S.bits_equal(ref, ref_changed)

    # 2. the module's image comes late and holds NaN until it comes
    box = {}
    monkeypatch.setattr(ops, pack_name, S.late_pack(getattr(ops, pack_name), box))
    # 3. - 5.
    _two_streams(module, x, box, ref, cache)
    # 7. a weight changes in place on A's side of the program; the repack is late again
    with torch.no_grad():
        changed.add_(1)
    torch.cuda.synchronize()
    _two_streams(module, x, box, ref_changed, cache + ", repacked")
    monkeypatch.undo()
    print("stream probes so far: %(tried)d pairs of streams tried, %(shared)d of them on a shared queue" % S._probes)

    # 6. a warm module on a side stream: the ordering is an event wait on the device, not a host synchronisation
    (side,) = S.fresh_streams(1)

    def on_side():
        with torch.no_grad(), torch.cuda.stream(side):
            return warm(x)
    got, syncs = H.count_syncs(on_side)
    torch.cuda.synchronize()
    assert len(syncs) == 0, [str(w.message)[:80] for w in syncs]
    assert S.bits_equal(got, ref)


# =========================================================================================================================
# (c) two streams at once do not cross
# =========================================================================================================================
CALLS = 6                                                        # per stream, enqueued A, B, A, B, ...


def _interleaved(step, sets):
    """``step(data, i)`` for i in 0 .. CALLS - 1 on each data set: one after the other on the default stream (the yardstick),
    then set 0 on stream A and set 1 on stream B, enqueued alternately from this thread behind a spin at the head of each
    stream, with no synchronisation of this function's in between.  -> (default-stream results, two-stream results)."""
    torch.cuda.synchronize()
    want = [[step(data, i) for i in range(CALLS)] for data in sets]
    torch.cuda.synchronize()
    streams = S.fresh_streams(2)
    for s in streams:
        with torch.cuda.stream(s):
            S.spin()
    got = [[], []]
    for i in range(CALLS):
        for k, s in enumerate(streams):
            with torch.cuda.stream(s):
                got[k].append(step(sets[k], i))
    torch.cuda.synchronize()
    return want, got


@pytest.mark.gpu
def test_two_streams_of_emm_track_do_not_cross():
    """Two scenes (C = 32, 3 and 5 tracks): extraction and head per call, free of host synchronisation, so both queues hold
    all six calls before either stream's spin ends — the (device, stream) workspaces, the order hints and the head's hand-off
    buffers of the two streams are live at the same time."""
    ops = _ops()
    params = _emm_params()
    five = np.concatenate((EMM_BOXES[1], np.array([(20.0, 20.0, 180.0, 340.0), (400.0, 150.0, 460.0, 370.0)], F32)))
    sets = [dict(boxes=_d(b), fa=[_emm_maps(50 + 10 * k + j) for j in range(3)], fb=[_emm_maps(80 + 10 * k + j) for j in range(3)])
            for k, b in enumerate((EMM_BOXES[0], five))]

    def step(data, i):
        fa, fb, boxes = data["fa"][i % 3], data["fb"][(i + i // 3) % 3], data["boxes"]
        z, sr, hint = ops.emm_extract_cache(fa, boxes, 15, SCALES, 2, 512, 1.0, 0, hint=True)
        bb, conf = ops.emm_track(fb, boxes, sr, z, params, 30, 15, SCALES, 2, 512, sigma=0.4, use_centerness=True,
                                 clip_wh=EMM_WH, order_hint=hint)
        return z, sr, bb, conf
    want, got = _interleaved(step, sets)
    for k in (0, 1):
        assert not S.bits_equal(want[k][0], want[k][1])          # (the calls of a stream differ from one another)
        for i in range(CALLS):
            assert S.bits_equal(got[k][i], want[k][i]), "stream %d, call %d" % (k, i)


def _detection_modules():
    """One set of modules for both streams, as one process serving two cameras has it: FPN (32, 64) -> 32 with the top block,
    ``RPNModule`` and a ``DetectionHead`` over three levels of an 80 x 48 image (maps 12 x 20, 6 x 10, 3 x 5)."""
    import fpn_cases as P
    import rpn_head_cases as H
    import rpn_proposal_cases as R
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.config import get_default_cfg
    from siammot_amd.detector import build_detection_head
    from siammot_amd.fpn import FPN, LastLevelMaxPool
    from siammot_amd.rpn import RPNModule
    C, cin = 32, (32, 64)
    cfg = get_default_cfg(channels=C)
    cfg.MODEL.RPN.ANCHOR_SIZES, cfg.MODEL.RPN.ANCHOR_STRIDE = (16, 32, 64), (4, 8, 16)
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    cfg.MODEL.ROI_BOX_HEAD.POOLER_SCALES, cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = (0.25, 0.125, 0.0625), 64
    fpn = P.load_fpn(FPN(cin, C, top_blocks=LastLevelMaxPool()), P.params(C, cin), DEV)
    torch.manual_seed(5)
    rpn = RPNModule(cfg, C)
    H.load_head(rpn.head, H.params(C, 3, seed=2), DEV)
    rpn = rpn.to(DEV).eval()
    det = build_detection_head(cfg, BoxCoder(R.WEIGHTS), C).to(DEV).eval()
    H.load_head(det.rpn_head, H.params(C, 3, seed=1), DEV)
    with torch.no_grad():
        det.box_head.predictor.bbox_pred.weight.mul_(0.02)
        det.box_head.predictor.cls_score.weight.mul_(4.0)
    return fpn, rpn, det, cin


@pytest.mark.gpu
def test_two_streams_of_the_detection_modules_do_not_cross():
    """FPN -> RPN head -> ``RPNModule`` proposals -> box head through ``DetectionHead.forward_features``, the modules shared
    by the two streams (their packed weights and anchor grids with them).  Each call reads its counts back, which
    synchronises its own stream only."""
    import fpn_cases as P
    ops = _ops()
    fpn, rpn, det, cin = _detection_modules()
    size = (80, 48)
    sets = [[[_d(v) for v in P.maps(cin, 1, SMALL, seed=100 * k + j)] for j in range(3)] for k in (0, 1)]

    def step(data, i):
        with torch.no_grad():
            feats = fpn(data[i % 3])
            proposals = rpn([size], feats)
            return feats, proposals, det.forward_features(feats, size)
    before = dict(ops.FALLBACKS)
    want, got = _interleaved(step, sets)
    assert dict(ops.FALLBACKS) == before, "a module left its device path: %s" % (dict(ops.FALLBACKS),)
    assert all(len(w[1][0]) > 0 for per in want for w in per), "no proposals: the box head had nothing to work on"
    for k in (0, 1):
        assert not S.bits_equal(want[k][0], want[k][1])
        for i in range(CALLS):
            assert S.bits_equal(got[k][i], want[k][i]), "stream %d, call %d" % (k, i)


@pytest.mark.gpu
def test_two_tracking_loops_on_two_streams_equal_two_on_the_default_stream():
    """measure/debug/loop_streams_soak.py as a test: 12 frames of two videos, video v on stream v with a spin at the head of
    every frame, against the same two videos on the default stream — boxes, ids and scores of every frame and the pools'
    ``_max_id`` at the end.  Each loop owns its frame plan, record ring and device-resident pool; the workspaces are per
    stream."""
    import golden_inputs as gi
    from fake_tracker import detections
    from siammot_amd.config import get_default_cfg
    from siammot_amd.track_head import build_tracking_loop
    frames = 12
    cfg = get_default_cfg(channels=32)
    cfg.MODEL.TRACK_HEAD.MAX_DORMANT_FRAMES = 3
    cfg.MODEL.TRACK_HEAD.TRACK_THRESH = 0.5
    cfg.MODEL.TRACK_HEAD.RESUME_TRACK_THRESH = 0.5
    torch.manual_seed(5)
    loops = [build_tracking_loop(cfg, device=torch.device(DEV), refine_tracks=False) for _ in range(4)]
    with torch.no_grad():
        for name in ("cls", "center", "reg"):
            getattr(loops[0].track.tracker.predictor, name).weight.mul_(20.0)
    for lp in loops[1:]:
        lp.track.tracker.load_state_dict(loops[0].track.tracker.state_dict())
    shapes = gi.feature_shapes((1280, 704), 32)
    maps = [[tuple(_d(np.random.RandomState(9 + v + 7 * j).standard_normal(s).astype(F32)) for s in shapes) for j in range(3)]
            for v in (0, 1)]
    rs = [np.random.RandomState(5 + (v & 1)) for v in range(4)]   # (every loop gets detections of its own: the same values)
    dets = [[detections(rs[v], f).to(DEV) for f in range(frames)] for v in range(4)]
    torch.cuda.synchronize()
    streams = S.fresh_streams(2)

    def row(out):
        return out.bbox.clone(), out.get_field("ids").clone(), out.get_field("scores").clone()
    got, want = [[], []], [[], []]
    with torch.no_grad():
        for f in range(frames):
            for v in (0, 1):
                with torch.cuda.stream(streams[v]):
                    S.spin()
            for v in (0, 1):                                     # video v on stream v
                with torch.cuda.stream(streams[v]):
                    got[v].append(row(loops[v](maps[v][f % 3], dets[v][f])))
        torch.cuda.synchronize()
        for f in range(frames):                                  # the same videos on the default stream
            for v in (0, 1):
                want[v].append(row(loops[2 + v](maps[v][f % 3], dets[2 + v][f])))
        torch.cuda.synchronize()
    for v in (0, 1):
        for f in range(frames):
            assert S.bits_equal(got[v][f], want[v][f]), "video %d, frame %d" % (v, f)
        assert loops[v].solver.track_pool._max_id == loops[2 + v].solver.track_pool._max_id >= 0
    assert max(len(r[0]) for r in want[0]) > 3 and not S.bits_equal(want[0][-1], want[1][-1])


# =========================================================================================================================
# (d) CPU
# =========================================================================================================================
def test_stream_cases_import_and_compare_bits_without_a_device():
    nan = torch.tensor([float("nan"), 1.0, -0.0])
    assert S.bits_equal(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not S.bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not S.bits_equal(torch.zeros(2), torch.zeros(2, dtype=torch.float64)) and not S.bits_equal(torch.zeros(2), torch.zeros(3))
    assert S.bits_equal((nan, [torch.arange(3), None, 4]), [nan, (torch.arange(3), None, 4)])
    assert not S.bits_equal((nan, 1), (nan,)) and not S.bits_equal([torch.arange(3)], [torch.arange(3) + 1])
    assert S.bits_equal(torch.tensor([1.0], dtype=torch.bfloat16), torch.tensor([1.0], dtype=torch.bfloat16))
    from siammot_amd.structures import BoxList
    a, b = BoxList(torch.zeros(2, 4), (8, 6)), BoxList(torch.zeros(2, 4), (8, 6))
    a.add_field("scores", nan[:2])
    assert not S.bits_equal(a, b)
    b.add_field("scores", nan[:2].clone())
    assert S.bits_equal(a, b) and S.bits_equal([a], [b]) and S.any_nan([a]) and not S.any_nan(torch.arange(3))
    b.add_field("ids", torch.arange(2))
    assert not S.bits_equal(a, b)
    with pytest.raises(ValueError):
        S.spin(S.SPIN_MAX_MS + 1)                                # refused before anything reaches a device
    assert S.SPIN_MS == 20.0 and S.SPIN_MAX_MS == 100.0


def test_cpu_tensors_never_reach_the_ordering_code(monkeypatch):
    import dla_cases as D
    import fpn_cases as P
    import rpn_head_cases as H
    import siammot_amd.ops as ops
    from siammot_amd.dla import DLA
    from siammot_amd.fpn import FPN, LastLevelMaxPool
    from siammot_amd.rpn import AnchorGenerator, RPNHead

    def refuse(*args, **kwargs):
        raise AssertionError("ops.StreamImage reached with CPU tensors")
    monkeypatch.setattr(ops, "StreamImage", refuse)
    with torch.no_grad():
        for ct in (None, torch.float16):
            fpn = P.load_fpn(FPN((32, 64), 32, top_blocks=LastLevelMaxPool(), compute_dtype=ct), P.params(32, (32, 64)), "cpu")
            assert len(fpn([torch.from_numpy(v) for v in P.maps((32, 64), 1, SMALL)])) == 3
            head = H.load_head(RPNHead(None, 32, 3, compute_dtype=ct), H.params(32, 3), "cpu")
            assert len(head([torch.from_numpy(v) for v in H.maps(32, 1, SMALL)])[0]) == 2
        model = DLA(*D.DLA34).eval()
        assert len(model(torch.from_numpy(D.image((32, 32), 1)))) == 4
        gen = AnchorGenerator((32, 64), (0.5, 1.0, 2.0), (8, 16))
        assert [tuple(t.shape) for t in gen.grid_anchors(SMALL)] == [(12 * 20 * 3, 4), (6 * 10 * 3, 4)]


def test_the_patched_names_are_the_names_the_modules_call():
    import siammot_amd.dla as dla
    import siammot_amd.fpn as fpn
    import siammot_amd.ops as ops
    import siammot_amd.rpn as rpn
    callers = {"fpn_pack": fpn.FPN.packed, "fpn_half_pack": fpn.FPN.packed, "rpn_head_pack": rpn.RPNHead.packed,
               "rpn_head_half_pack": rpn.RPNHead.packed, "dla_pack": dla.DLA._pack, "dla_half_pack": dla.DLA._pack,
               "dla_net_pack": dla.DLA._pack, "rpn_anchors": rpn.AnchorGenerator.grid_anchors}
    assert sorted(callers) == sorted(name for _, name in CACHES.values())
    for name, caller in callers.items():
        assert callable(getattr(ops, name)), name
        assert "ops.%s(" % name in inspect.getsource(caller), "%s does not call ops.%s" % (caller.__qualname__, name)
    for cls in (fpn.FPN, rpn.RPNHead, dla.DLA, rpn.AnchorGenerator):
        assert "ops.StreamImage(" in inspect.getsource(cls), cls.__name__
    assert callable(ops.StreamImage) and hasattr(ops.StreamImage, "get")
