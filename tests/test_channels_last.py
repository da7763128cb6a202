"""Channels-last feature maps read in place by the tracker head and its poolers (``SMOT_FEAT_CHANNELS_LAST``).

The contract: a call whose maps are channels-last returns, for every output, exactly the bits the same call returns on
``tuple(f.contiguous() for f in maps)`` — the NCHW path, which is pinned to the oracle and the golden vectors elsewhere.
No tolerance appears below.  Comparison rule: NaN positions identical, every other value bit-identical, hints as int32."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_half_maps import (DEV, FAMILIES, SCALES, Pair, _bits_equal, _boxes, _det, _emm, _hint_equal, _img, _params,
                            _placed_boxes, _same_pair, _typed_calls)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
WH = (512, 256)


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_flag_is_declared_and_versions_stand():
    import siammot_amd.ops as ops
    lib = ops.load_library()
    src = open(os.path.join(ROOT, "include", "smot_emm.h")).read()
    assert re.search(r"#define\s+SMOT_FEAT_CHANNELS_LAST\s+16\b", src)
    assert ops.FEAT_CHANNELS_LAST == 16
    assert ops.FEAT_TYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    assert ops.ABI_VERSION == 14 and lib.smot_abi_version() == 14        # additive: no new symbol, the ABI version stands


def test_empty_calls_take_the_flag_and_other_values_are_refused():
    import siammot_amd.ops as ops
    lib = ops.load_library()
    calls = _typed_calls(lib)
    for name, call in calls.items():
        for ft in (16, 17, 18):
            rc = call(ft)
            assert rc == 0 or (name == "sr_xcorr_gather" and rc == -2), (name, ft, rc, lib.smot_last_error())
    calls["track_frame"] = lambda ft: lib.smot_track_frame_typed_fwd(ctypes.c_void_p(0), ft, ctypes.c_void_p(0))
    for name, call in calls.items():
        for bad in (19, 32, 3, -1):
            assert call(bad) == -1, (name, bad)
            msg = lib.smot_last_error()
            assert b"feat_type=%d" % bad in msg, (name, bad, msg)


def test_layout_rule():
    import siammot_amd.ops as ops
    nchw = torch.zeros((2, 8, 6, 10))
    nhwc = nchw.to(memory_format=CL)
    assert ops.maps_layout(nchw) == 0
    assert ops.maps_layout(nhwc) == 16 and not nhwc.is_contiguous()
    assert ops.maps_layout(torch.zeros((2, 1, 6, 10)).to(memory_format=CL)) == 0          # C == 1: both layouts -> NCHW
    assert ops.maps_layout(torch.zeros((2, 8, 1, 1)).to(memory_format=CL)) == 0           # H == W == 1: both -> NCHW
    assert ops.maps_layout(nhwc[1:2]) == 16                                               # a batch slice of a channels-last batch
    assert ops.maps_layout(nchw.permute(0, 1, 3, 2)) == 0                                 # a strided view that is neither
    assert ops.maps_layout(torch.zeros((8, 6, 10))) == 0                                  # not 4-D
    # the call-level rule: every level channels-last and C % 8 == 0
    assert ops._levels_layout((nhwc, nhwc), 2) == 16
    assert ops._levels_layout((nhwc, nchw), 2) == 0
    c20 = torch.zeros((1, 20, 6, 10)).to(memory_format=CL)
    assert ops.maps_layout(c20) == 16 and ops._levels_layout((c20,), 1) == 0
    # a channels-last view that does not start at a 16-byte boundary goes through the copy, as it always did
    odd = torch.zeros((2 * 8 * 6 * 10 + 4,), dtype=torch.float16)[4:].as_strided((2, 8, 6, 10), (480, 1, 80, 8))
    assert ops.maps_layout(odd) == 16 and odd.data_ptr() % 16 == 8 and ops._levels_layout((odd,), 1) == 0


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


def _cl_maps(C, image_wh, seed, dtype, B=1, widths=None, scale=1.0):
    """Channels-last maps of an image (levels /4 .. /32, or the given level widths) and their NCHW copies."""
    W, H = image_wh
    g = torch.Generator().manual_seed(seed)
    cl = []
    for l, s in enumerate((4, 8, 16, 32)):
        w = W // s if widths is None else widths[l]
        cl.append((torch.randn((B, C, H // s, w), generator=g) * scale).to(dtype).to(DEV).to(memory_format=CL))
    assert all(not f.is_contiguous() and f.is_contiguous(memory_format=CL) for f in cl)
    return tuple(cl), tuple(f.contiguous() for f in cl)


# 4. operators
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [32, 128, 256, 40])
def test_operators_equal_the_call_on_the_nchw_copy(ops, C, dtype):
    rx, rz, pad, exp, msw = FAMILIES["30/15"][:5]
    cl, nc = _cl_maps(C, WH, 1, dtype)
    boxes = _boxes(12, WH, 2, sizes=[(20, 40), (40, 80), (60, 110), (100, 200), (16, 16), (200, 70)])
    sr = ops.search_region(boxes, pad, exp, msw)
    pc = [int(pad / ((2 ** i) * 4)) for i in range(4)]
    for size in (7, 15, 30, 35):          # 7 / 15 / 30: the separable kernel; 35: the generic one
        got, lv = ops.roi_align_levels(cl, sr, boxes, size, SCALES, 2, pc, return_levels=True)
        ref, lr = ops.roi_align_levels(nc, sr, boxes, size, SCALES, 2, pc, return_levels=True)
        _bits_equal(got, ref, "roi_align_levels %d C=%d" % (size, C))
        assert torch.equal(lv, lr)
    # the generic kernel at the other sampling ratios: its staged and its unstaged branch (a roi as large as the image)
    wide = torch.tensor([[0.0, 0.0, 511.0, 200.0], [5.0, 3.0, 500.0, 250.0], [100.0, 100.0, 180.0, 190.0]], device=DEV)
    for g in (1, 3, 4):
        _bits_equal(ops.roi_align_levels(cl[:1], wide, wide, 9, SCALES[:1], g), ops.roi_align_levels(nc[:1], wide, wide, 9, SCALES[:1], g),
                    "generic kernel, sampling ratio %d C=%d" % (g, C))
    # roi_align (rois5) on two images, through layers.ROIAlign / poolers.Pooler too
    from siammot_amd.layers import ROIAlign
    from siammot_amd.poolers import Pooler
    from siammot_amd.structures import BoxList
    cb, nb = _cl_maps(C, WH, 3, dtype, B=2)
    rois5 = torch.cat([torch.tensor([[0.0], [1.0], [1.0], [0.0], [5.0]], device=DEV), _boxes(5, WH, 4)], dim=1)
    for lvl, scale in ((0, 0.25), (2, 0.0625)):
        _bits_equal(ops.roi_align(cb[lvl], rois5, scale, 7, 7, 2), ops.roi_align(nb[lvl], rois5, scale, 7, 7, 2),
                    "roi_align level %d C=%d" % (lvl, C))
        ra = ROIAlign((5, 9), scale, 3)
        _bits_equal(ra(cb[lvl], rois5), ra(nb[lvl], rois5), "layers.ROIAlign level %d C=%d" % (lvl, C))
    pooler = Pooler((7, 7), SCALES, 2)
    bl = [BoxList(boxes, WH, mode="xyxy")]
    _bits_equal(pooler(cl, bl), pooler(nc, bl), "poolers.Pooler C=%d" % C)
    if C == 40:
        return                            # (pooling-only operators at this C)
    z = ops.roi_align_levels(nc, boxes, boxes, rz, SCALES, 2)
    a = ops.sr_xcorr_fused(cl, boxes, sr, z, rx, rz, SCALES, 2, pad, return_pooled=True)
    b = ops.sr_xcorr_fused(nc, boxes, sr, z, rx, rz, SCALES, 2, pad, return_pooled=True)
    _bits_equal(a[0], b[0], "sr_xcorr_fused response C=%d" % C)
    _bits_equal(a[1], b[1], "sr_xcorr_fused pooled planes C=%d" % C)
    _bits_equal(ops.sr_xcorr_fused(cl, boxes, sr, z, rx, rz, SCALES, 2, pad), b[0], "sr_xcorr_fused without x_debug C=%d" % C)


# 5. every window class of the separable kernel
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("geometry", ["704x1280", "odd widths"])
def test_every_window_class_of_the_separable_kernel(ops, geometry, dtype):
    if geometry == "704x1280":
        wh, widths = (1280, 704), None
    else:
        wh, widths = (1284, 704), (321, 161, 81, 41)
    C = 128
    narrow = _placed_boxes(wh, (20, 40, 60), (101.0, 105.0, 110.0, 116.0), 1)
    mid = _placed_boxes(wh, (90, 120, 200), (33.0, 37.0, 42.0, 48.0), 2)
    wide = torch.tensor([[400.0, 300.0, 700.0, 420.0]], device=DEV)      # a 600-pixel search region: 75 cells of level 1
    boxes = torch.cat([narrow, mid, wide, _boxes(5, wh, 3)], dim=0)
    (ca, na), (cb, nb) = _cl_maps(C, wh, 20, dtype, widths=widths), _cl_maps(C, wh, 21, dtype, widths=widths)
    P = Pair(ops, "30/15", C, wh, _params(C, boxes, 5))
    got, oh = P.run(ca, cb, boxes, hint=True)
    ref, of = P.run(na, nb, boxes, hint=True)
    _same_pair(got, ref, geometry)
    _hint_equal(oh, of, "hint")
    seen = set()
    for ymin, ymax, xmin, xmax in oh.view(torch.int32)[:, 8:12].cpu().numpy():   # (the hint's own bounds: words 10, 11 = xmin, xmax)
        if xmax >= xmin:
            ww = xmax - xmin + 1
            seen.add(("<=32" if ww <= 32 else ("33..64" if ww <= 64 else ">64"), int(xmin) & 1))
    for cls in ("<=32", "33..64", ">64"):
        assert any(s[0] == cls for s in seen), (cls, seen)
    assert {s[1] for s in seen} == {0, 1}, seen
    # stand-alone poolers on rois in the zero border, on a strip wider than 64 cells, and on everything above
    pad = 512
    pc = [int(pad / ((2 ** i) * 4)) for i in range(4)]
    border = torch.tensor([[5.0, 5.0, 100.0, 90.0], [wh[0] + 2 * pad - 120.0, 10.0, wh[0] + 2 * pad - 8.0, 100.0],
                           [300.0, 2.0, 460.0, 60.0]], device=DEV)
    strip = torch.tensor([[pad + 2.0, pad + 40.0, pad + wh[0] - 3.0, pad + 70.0], [pad + 7.0, pad + 300.0, pad + 700.0, pad + 330.0]],
                         device=DEV)
    rois = torch.cat([border, strip, ops.search_region(boxes, pad, 1.0, 0)], dim=0)
    lvl_boxes = torch.cat([border, torch.tensor([[0.0, 0.0, 30.0, 30.0], [0.0, 0.0, 40.0, 40.0]], device=DEV), boxes], dim=0)
    for size in (7, 15, 30):
        a = ops.roi_align_levels(ca, rois, lvl_boxes, size, SCALES, 2, pc)
        b = ops.roi_align_levels(na, rois, lvl_boxes, size, SCALES, 2, pc)
        _bits_equal(a, b, "%s pooler %d" % (geometry, size))
        assert float(a[:2].abs().max()) == 0.0                                       # entirely in the zero border: exact zeros
    z = ops.roi_align_levels(na, lvl_boxes, lvl_boxes, 15, SCALES, 2)
    a = ops.sr_xcorr_fused(ca, lvl_boxes, rois, z, 30, 15, SCALES, 2, pad, return_pooled=True)
    b = ops.sr_xcorr_fused(na, lvl_boxes, rois, z, 30, 15, SCALES, 2, pad, return_pooled=True)
    _bits_equal(a[0], b[0], "fused on border / strip rois")
    _bits_equal(a[1], b[1], "fused pooled planes on border / strip rois")


# 6. frame pairs: plain, hinted, masked; hints across the two layouts
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_frame_pairs_equal_the_pairs_on_the_nchw_copy(ops, dtype):
    C = 64
    (ca, na), (cb, nb) = _cl_maps(C, WH, 11, dtype), _cl_maps(C, WH, 12, dtype)
    sizes = [(20, 40), (40, 80), (60, 110), (100, 200), (16, 16), (200, 70)]
    for N in (1, 30, 100, 280):
        boxes = _boxes(N, WH, 13, sizes=sizes)
        P = Pair(ops, "30/15", C, WH, _params(C, boxes, 14))
        for hint in ((False, True) if N <= 256 else (False,)):
            got, oh = P.run(ca, cb, boxes, hint=hint)
            ref, of = P.run(na, nb, boxes, hint=hint)
            _same_pair(got, ref, "N=%d hint=%s" % (N, hint))
            _hint_equal(oh, of, "order hint bytes N=%d" % N)
            if N >= 2 and N <= 256:
                assert oh is not None and ops.order_hint_status(oh) == 0 and ops.order_hint_status(of) == 0
        # the masked extraction: a device count below the capacity
        nv = max(N - 3, 1)
        count = torch.tensor([nv], dtype=torch.int32, device=DEV)
        a = ops.emm_extract_cache(ca, boxes, P.rz, SCALES, 2, P.pad, P.exp, P.msw, n_valid=count)
        b = ops.emm_extract_cache(na, boxes, P.rz, SCALES, 2, P.pad, P.exp, P.msw, n_valid=count)
        _bits_equal(a[0][:nv], b[0][:nv], "masked templates N=%d" % N)
        _bits_equal(a[1][:nv], b[1][:nv], "masked search regions N=%d" % N)
        _bits_equal(a[0][:nv], ref["z"][:nv], "masked vs plain templates N=%d" % N)
        if N == 30:
            # cross-use: a hint written from NCHW maps feeds a channels-last head, and the reverse
            zc, src_, oh_c = P.extract(ca, boxes, hint=True)
            zn, srn, oh_n = P.extract(na, boxes, hint=True)
            plain = P.track(nb, boxes, srn, zn)
            x1 = P.track(cb, boxes, srn, zn, order_hint=oh_n)
            x2 = P.track(nb, boxes, src_, zc, order_hint=oh_c)
            torch.cuda.synchronize()
            assert ops.order_hint_status(oh_c) == 0 and ops.order_hint_status(oh_n) == 0
            for x, what in ((x1, "NCHW hint -> channels-last head"), (x2, "channels-last hint -> NCHW head")):
                for u, v, k in zip(x, plain, ("bb", "conf", "idx")):
                    _bits_equal(u, v, "%s: %s" % (what, k))


# 7. batched calls
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_calls_equal_one_image_calls_and_the_nchw_batch(ops, dtype):
    lib = ops.load_library()
    B, C, rows = 3, 64, [5, 0, 7]
    (ca, na), (cb, nb) = _cl_maps(C, WH, 40, dtype, B=B), _cl_maps(C, WH, 41, dtype, B=B)
    boxes = _boxes(sum(rows), WH, 42, sizes=[(20, 40), (40, 80), (60, 110), (100, 200), (16, 16), (200, 70)])
    P = Pair(ops, "30/15", C, WH, _params(C, boxes, 43))
    got, oh = P.run(ca, cb, boxes, rows, hint=True)
    ref, of = P.run(na, nb, boxes, rows, hint=True)
    _same_pair(got, ref, "B=3 vs the NCHW batch")
    _hint_equal(oh, of, "hint B=3")
    ho, n0 = P.rx - P.rz + 1, 0
    for b, r in enumerate(rows):
        if r > 0:
            sl = _img(ca, b)
            assert all(ops.maps_layout(f) == 16 for f in sl)         # the slice of a channels-last batch is channels-last
            one, _ = P.run(sl, _img(cb, b), boxes[n0:n0 + r])
            if lib.smot_emm_tower_form(r, C, ho) == lib.smot_emm_tower_form(sum(rows), C, ho):
                _same_pair(got, one, "B=3 image %d" % b, rows=(n0, n0 + r))
            else:           # (another tower form for that row count: the pooling's outputs are still the same bits)
                _bits_equal(got["z"][n0:n0 + r], one["z"], "templates, image %d" % b)
                _bits_equal(got["sr"][n0:n0 + r], one["sr"], "search regions, image %d" % b)
        n0 += r
    # the batched extraction at other template sizes: 7 (the separable kernel's 7-bin form), 9 (the generic kernel's batched form)
    for rz in (7, 9):
        a = ops.emm_extract_cache_batched(ca, boxes, rows, rz, SCALES, 2, P.pad, P.exp, P.msw)
        b = ops.emm_extract_cache_batched(na, boxes, rows, rz, SCALES, 2, P.pad, P.exp, P.msw)
        _bits_equal(a[0], b[0], "batched templates, rz=%d" % rz)
        _bits_equal(a[1], b[1], "batched search regions, rz=%d" % rz)


# 8. special values
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_special_values_come_through_exactly(ops, dtype):
    C = 32
    (ca, _), (cb, _) = _cl_maps(C, WH, 31, dtype), _cl_maps(C, WH, 32, dtype)
    box = torch.tensor([[40.0, 40.0, 120.0, 100.0], [200.0, 60.0, 330.0, 200.0]], device=DEV)
    sub = torch.tensor(np.array([0x0001], dtype=np.uint16).view(np.int16)).view(torch.float16).to(dtype).item()   # 2^-24
    vals = [float("nan"), float("inf"), sub, -0.0]
    for m in (ca, cb):
        for l in (0, 1):
            s = 4 * 2 ** l
            for k, v in enumerate(vals):        # cells inside the first box's window (and its search region's), several channels
                y, x = (50 + 10 * k) // s, (60 + 12 * k) // s
                m[l][0, k::5, y, x] = v
                m[l][0, (k + 2)::7, y + 1, x + 1] = v
    assert all(ops.maps_layout(f) == 16 for f in ca + cb)
    na, nb = tuple(f.contiguous() for f in ca), tuple(f.contiguous() for f in cb)
    boxes = torch.cat([box, _boxes(10, WH, 34, sizes=[(40, 60), (80, 50), (24, 24)])], dim=0)
    P = Pair(ops, "30/15", C, WH, _params(C, boxes, 35))
    got, oh = P.run(ca, cb, boxes, hint=True)
    ref, of = P.run(na, nb, boxes, hint=True)
    _same_pair(got, ref, "special values")
    _hint_equal(oh, of, "hint")
    for size in (7, 15, 30, 35):
        _bits_equal(ops.roi_align_levels(ca, boxes, boxes, size, SCALES, 2), ops.roi_align_levels(na, boxes, boxes, size, SCALES, 2),
                    "pooler %d on special values" % size)
    assert bool(torch.isnan(got["z"]).any()) and bool(torch.isinf(got["z"]).any())        # they really reached outputs


# 9. one EMM module, layouts and dtypes alternating
@pytest.mark.gpu
def test_alternating_layouts_and_dtypes_through_one_module(ops):
    C = 64
    init = _boxes(5, WH, 71, sizes=[(20, 40), (40, 80), (60, 110)])
    emm, fresh = _emm(C, init, 72), _emm(C, init, 72)
    order = [(torch.float32, False), (torch.float32, True), (torch.float16, True), (torch.float16, False), (torch.float32, True),
             (torch.float16, True), (torch.float32, False), (torch.float16, True), (torch.float32, True)]
    with torch.no_grad():
        for t, (dt, cl) in enumerate(order):
            size = WH if t not in (5, 6) else (640, 256)
            ca, na = _cl_maps(C, size, 200 + t, dt)
            cb, nb = _cl_maps(C, size, 300 + t, dt)
            det = _det(init, 0, 5, size)
            z, sr, d = emm.extract_cache(ca if cl else na, det)
            _, res, _ = emm(cb if cl else nb, d, sr, template_features=z)
            det2 = _det(init, 0, 5, size)
            z2, sr2, d2 = fresh.extract_cache(na, det2)
            _, res2, _ = fresh(nb, d2, sr2, template_features=z2)
            fresh.__dict__.pop("_plan", None)                 # (the reference module plans every call anew)
            what = "call %d (%s, %s)" % (t, dt, "channels-last" if cl else "NCHW")
            _bits_equal(z, z2, "templates, " + what)
            _bits_equal(sr[0].bbox, sr2[0].bbox, "search regions, " + what)
            _bits_equal(res[0].bbox, res2[0].bbox, "boxes, " + what)
            _bits_equal(res[0].get_field("scores"), res2[0].get_field("scores"), "scores, " + what)
    plans = emm.__dict__["_plan"]
    assert set(plans) == {torch.float32, torch.float16, (torch.float32, 16), (torch.float16, 16)}
    assert all(p.ft == ops.FEAT_TYPES[p.g.dtype] | (16 if isinstance(k, tuple) else 0) for k, p in plans.items())


# 10. the tracking loop
def _detections(rs, frame, n_objects=10):
    """Objects on slow linear paths in a 512x256 image; each is detected with probability 0.85; plus a few false positives."""
    from siammot_amd.structures import BoxList
    base = np.random.RandomState(1234)
    c0 = base.uniform(40, [470, 220], (n_objects, 2))
    vel = base.uniform(-2, 2, (n_objects, 2))
    wh = base.uniform(20, 50, (n_objects, 2))
    c = c0 + vel * frame
    det = rs.rand(n_objects) < 0.85
    boxes = np.concatenate((c - wh / 2, c + wh / 2), 1)[det]
    nfp = int(rs.randint(0, 3))
    fp_c = rs.uniform(30, [480, 230], (nfp, 2))
    boxes = np.concatenate((boxes, np.concatenate((fp_c - 12, fp_c + 12), 1)), 0).astype(np.float32)
    scores = rs.uniform(0.45, 0.99, len(boxes)).astype(np.float32)
    bl = BoxList(torch.from_numpy(boxes), WH, mode="xyxy")
    bl.add_field("ids", torch.full((len(boxes),), -1, dtype=torch.int64))
    bl.add_field("labels", torch.ones(len(boxes), dtype=torch.int64))
    bl.add_field("scores", torch.from_numpy(scores))
    return bl


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("refine", [False, True])
def test_tracking_loop_on_channels_last_maps_equals_the_loop_on_the_nchw_copy(ops, refine, dtype):
    from siammot_amd.box_refine import RefineTracks, TrackBoxHead
    from siammot_amd.config import get_default_cfg
    from siammot_amd.track_head import build_tracking_loop
    dev = torch.device(DEV)
    cfg = get_default_cfg(channels=32)
    cfg.MODEL.TRACK_HEAD.MAX_DORMANT_FRAMES = 3
    cfg.MODEL.TRACK_HEAD.TRACK_THRESH = 0.35
    cfg.MODEL.TRACK_HEAD.RESUME_TRACK_THRESH = 0.5
    loops = []
    for k in range(2):
        rt = False
        if refine:
            torch.manual_seed(7)
            rt = RefineTracks(TrackBoxHead(cfg, 32).to(dev).eval())
        loops.append(build_tracking_loop(cfg, device=dev, refine_tracks=rt))
    with torch.no_grad():
        for name in ("cls", "center", "reg"):
            getattr(loops[0].track.tracker.predictor, name).weight.mul_(20.0)
    loops[1].track.tracker.load_state_dict(loops[0].track.tracker.state_dict())
    g = torch.Generator().manual_seed(9)
    feats = [tuple(torch.randn((1, 32, WH[1] // s, WH[0] // s), generator=g).to(dtype).to(dev).to(memory_format=CL)
                   for s in (4, 8, 16, 32, 64)) for _ in range(4)]
    rs = [np.random.RandomState(5), np.random.RandomState(5)]
    general0 = ops.FALLBACKS["general_frame"]
    plans, ids_seen = [], set()
    with torch.no_grad():
        for f in range(8):
            h = feats[f % 4]
            a = loops[0](h, _detections(rs[0], f).to(dev))
            b = loops[1](tuple(x.contiguous() for x in h), _detections(rs[1], f).to(dev))
            _bits_equal(a.bbox, b.bbox, "boxes, frame %d" % f)
            _bits_equal(a.get_field("scores"), b.get_field("scores"), "scores, frame %d" % f)
            assert torch.equal(a.get_field("ids"), b.get_field("ids")), "ids, frame %d" % f
            pa, pb = loops[0].solver.track_pool, loops[1].solver.track_pool
            assert pa.get_active_ids() == pb.get_active_ids() and pa._dormant_ids == pb._dormant_ids and pa._max_id == pb._max_id
            ids_seen |= set(pa.get_active_ids())
            ma, mb = loops[0].track_memory, loops[1].track_memory
            assert len(ma[2][0]) == len(mb[2][0])
            if len(mb[2][0]):
                _bits_equal(ma[0], mb[0], "memory templates, frame %d" % f)
                _bits_equal(ma[1][0].bbox, mb[1][0].bbox, "memory search regions, frame %d" % f)
                _bits_equal(ma[2][0].bbox, mb[2][0].bbox, "memory boxes, frame %d" % f)
            plans.append(loops[0].__dict__.get("_plan"))
    assert len(ids_seen) >= 5, ids_seen
    # the fast path: the frame plan made on the first frame (a channels-last plan) is refreshed, never rebuilt — a failed
    # ``_geometry_refresh`` makes a new plan object — and no frame took the general path
    assert ops.FALLBACKS["general_frame"] == general0
    plan = plans[1]
    assert plan is not None and all(p is plan for p in plans[2:]) and plans[0] in (None, plan)
    assert plan.ft == ops.FEAT_TYPES[dtype] | 16 and plan.g.ft == plan.ft
    assert ops._geometry_refresh(plan.g, feats[1], dev) and not ops._geometry_refresh(plan.g, tuple(x.contiguous() for x in feats[1]), dev)


# 11. no NCHW copy
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_no_nchw_copy_of_a_map_is_made(ops, dtype):
    C = 128
    init = _boxes(4, WH, 91, sizes=[(20, 40), (40, 80), (60, 110)])
    emm = _emm(C, init, 92)
    (ca, _), (cb, _) = _cl_maps(C, WH, 93, dtype), _cl_maps(C, WH, 94, dtype)
    level0 = ca[0].numel() * ca[0].element_size()
    with torch.no_grad():
        for step in range(2):                  # the first pair warms the grow-only workspaces and the caches
            det = _det(init, 0, 4, WH)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.max_memory_allocated()
            z, sr, d = emm.extract_cache(ca, det)
            _, res, _ = emm(cb, d, sr, template_features=z)
            torch.cuda.synchronize()
            grown = torch.cuda.max_memory_allocated() - before
    print("peak memory growth of a frame pair on channels-last %s maps: %d bytes (level 0: %d)" % (dtype, grown, level0))
    assert grown < level0 // 2, (grown, level0)


# 12. what still goes through the NCHW copy keeps today's results
@pytest.mark.gpu
def test_fallbacks_keep_their_results(ops):
    C = 32
    (ca, na), (cb, nb) = _cl_maps(C, WH, 81, torch.float32), _cl_maps(C, WH, 82, torch.float32)
    boxes = _boxes(6, WH, 83, sizes=[(20, 40), (40, 80), (60, 110)])
    P = Pair(ops, "30/15", C, WH, _params(C, boxes, 84))
    ref, _ = P.run(na, nb, boxes, hint=True)
    # one NCHW and three channels-last levels
    got, _ = P.run((na[0],) + ca[1:], (nb[0],) + cb[1:], boxes, hint=True)
    _same_pair(got, ref, "mixed layouts")
    _bits_equal(ops.roi_align_levels((na[0],) + ca[1:], boxes, boxes, 9, SCALES, 2), ops.roi_align_levels(na, boxes, boxes, 9, SCALES, 2),
                "mixed layouts, generic pooler")
    # a permuted view that is neither layout
    t = tuple(f.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2) for f in na)
    assert all(ops.maps_layout(f) == 0 and not f.is_contiguous() for f in t[:3])
    _bits_equal(ops.roi_align_levels(t, boxes, boxes, 15, SCALES, 2), ref["z"], "strided views")
    # channels-last views that do not start at a 16-byte boundary (fp16, 8 bytes into their storage)
    odd = []
    for f in na:
        h = f.half()
        buf = torch.zeros((h.numel() + 4,), dtype=torch.float16, device=DEV)
        v = buf[4:].as_strided(h.shape, h.to(memory_format=CL).stride())
        v.copy_(h)
        odd.append(v)
    assert all(ops.maps_layout(f) == 16 and f.data_ptr() % 16 == 8 for f in odd) and ops._levels_layout(odd, 4) == 0
    for size in (9, 15):
        _bits_equal(ops.roi_align_levels(odd, boxes, boxes, size, SCALES, 2),
                    ops.roi_align_levels(tuple(f.half() for f in na), boxes, boxes, size, SCALES, 2), "views at an odd offset, pooler %d" % size)
    # C = 20
    (c20a, n20a), (c20b, n20b) = _cl_maps(20, WH, 85, torch.float32), _cl_maps(20, WH, 86, torch.float32)
    P20 = Pair(ops, "30/15", 20, WH, None)                  # (no predictor at this C: extraction and pooling + correlation)
    e1, e2 = P20.extract(c20a, boxes, hint=True), P20.extract(n20a, boxes, hint=True)
    _bits_equal(e1[0], e2[0], "C = 20 templates")
    _bits_equal(e1[1], e2[1], "C = 20 search regions")
    _hint_equal(e1[2], e2[2], "C = 20 hint")
    _bits_equal(ops.sr_xcorr_fused(c20b, boxes, e1[1], e1[0], 30, 15, SCALES, 2, 512),
                ops.sr_xcorr_fused(n20b, boxes, e2[1], e2[0], 30, 15, SCALES, 2, 512), "C = 20 pooling + correlation")
    for size in (7, 9):
        _bits_equal(ops.roi_align_levels(c20a, boxes, boxes, size, SCALES, 2), ops.roi_align_levels(n20a, boxes, boxes, size, SCALES, 2),
                    "C = 20, pooler %d" % size)
    # the 35 / 7 family
    P7 = Pair(ops, "35/7", C, WH, P.params)
    _same_pair(P7.run(ca, cb, boxes)[0], P7.run(na, nb, boxes)[0], "35/7")
    sr7 = ops.search_region(boxes, 256, 4.0, 64)
    z7 = ops.roi_align_levels(na, boxes, boxes, 7, SCALES, 2)
    _bits_equal(ops.sr_xcorr_fused(ca, boxes, sr7, z7, 35, 7, SCALES, 2, 256), ops.sr_xcorr_fused(na, boxes, sr7, z7, 35, 7, SCALES, 2, 256),
                "35/7 gather operator")
