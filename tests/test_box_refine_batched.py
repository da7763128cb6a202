"""The box-head refinement of the propagated tracks for several cameras in one library call:
``ops.box_refine_post_batched`` / ``ops.box_refine_batched``, ``TrackBoxHead.refine_raw_batched``, ``RefineTracks`` on
several BoxLists and ``MultiCameraTrackingLoop``'s one refinement call per step.

The yardstick of the device tests is the single-image code (``ops.box_refine``, ``ops.box_refine_post``,
``ops.linear_rows``): both sides run the same device arithmetic in the same order, so every comparison is ``torch.equal``
(bit patterns where NaN is among the values) and no tolerance is invented.  The one comparison with a tolerance is against
the reference's own ``_refine_tracks`` (tests/golden/refine_tracks.npz), with the bounds tests/test_box_refine.py applies to
the single-image device form against the same file."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import box_refine_edge_cases as E
import golden_inputs as gi

DEV = "cuda:0"
XFORM_CLIP = math.log(1000.0 / 16)
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
SCALES = (0.25, 0.125, 0.0625, 0.03125)
IMAGE_WH = (1280, 704)
NEW_SYMBOLS = ("smot_box_refine_batched_max_rows", "smot_box_refine_batched_ws_floats", "smot_box_refine_post_batched_fwd",
               "smot_box_refine_batched_typed_fwd")


def _library():
    import siammot_amd.ops as ops
    if not os.path.exists(ops.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ops, ops.load_library()


def _same_bits(a, b):
    """``torch.equal`` that also holds for equal NaN patterns."""
    if a.dtype is torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


# ---- 1. the premise: a row of a linear layer does not depend on the rows that share its launch ---------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K,N", [(784, 128), (128, 64), (64, 11), (784, 1024)])
def test_rows_of_a_layer_beyond_128_rows_equal_linear_rows_on_any_chunk_of_them(K, N):
    """M = 273 rows (two row blocks of 128 and one of 17) through the form the batched refinement runs its layers in — the
    library's internal launcher, reached through the measurement library's entry — against ``ops.linear_rows`` of the same
    build on chunks of at most 128 rows: the blocks themselves, a chunk that straddles a block boundary, a single row."""
    import siammot_amd.ops as ops
    M = 273
    g = torch.Generator().manual_seed(K * 10 + N)
    x = torch.randn((M, K), generator=g).to(DEV)
    w = (torch.randn((N, K), generator=g) / K ** 0.5).to(DEV)
    b = torch.randn((N,), generator=g).to(DEV)
    with ops.debug_library():
        for relu in (True, False):
            y = ops.linear_rows_blocks(x, w, b, relu=relu)
            assert y.shape == (M, N)
            for r0, r1 in ((0, 128), (128, 256), (256, 273), (100, 130), (272, 273)):
                want = ops.linear_rows(x[r0:r1].contiguous(), w, b, relu=relu)
                assert torch.equal(y[r0:r1], want), (K, N, relu, r0, r1)
        assert float(y.abs().max()) > 0.0


# ---- inputs of the whole-call tests ------------------------------------------------------------------------------------------
def _head(g, C, dim6, dim7, classes, agnostic):
    def lin(o, i):
        return (torch.randn((o, i), generator=g) / i ** 0.5).to(DEV), torch.randn((o,), generator=g).mul(0.1).to(DEV)
    w6, b6 = lin(dim6, C * 49)
    w7, b7 = lin(dim7, dim6)
    wc, bc = lin(classes, dim7)
    wr, br = lin(4 * (2 if agnostic else classes), dim7)
    return (w6, b6, w7, b7, wc, bc, wr, br)


def _maps(g, B, C=16):
    """Four levels of a 704 x 1280 image with C channels, [B, C, H_l, W_l], different contents per image."""
    return tuple(torch.randn((B, C, 352 // s_, 640 // s_), generator=g).to(DEV) for s_ in (1, 2, 4, 8))


def _rows(g, n, classes, amodal=False):
    xy = torch.rand((n, 2), generator=g) * torch.tensor([1000.0, 500.0])
    if amodal:
        xy = xy + torch.tensor([600.0, 0.0])                 # many boxes reach beyond the right border
    wh = 20.0 + torch.rand((n, 2), generator=g) * 200.0
    boxes = torch.cat((xy, xy + wh), 1).to(DEV)
    labels = torch.randint(1, classes, (n,), generator=g).to(DEV)
    ids = (torch.randperm(n, generator=g) + 2 ** 33).to(DEV)
    conf = torch.rand((n,), generator=g).to(DEV)
    return boxes, labels, ids, conf


def _check_against_per_image_calls(feats, rows_per_image, rows, layers, clip_wh, tracktor):
    import siammot_amd.ops as ops
    boxes, labels, ids, conf = rows
    got = ops.box_refine_batched(feats, SCALES, 7, 2, boxes, labels, ids, conf, rows_per_image, layers, WEIGHTS, XFORM_CLIP,
                                 clip_wh, tracktor)
    assert [t.shape[0] for t in got] == [sum(rows_per_image)] * 4
    n0 = 0
    for b, n in enumerate(rows_per_image):
        n1 = n0 + n
        if n:
            one = ops.box_refine(tuple(f[b:b + 1] for f in feats), SCALES, 7, 2, boxes[n0:n1].contiguous(),
                                 labels[n0:n1].contiguous(), ids[n0:n1].contiguous(), conf[n0:n1].contiguous(), layers, WEIGHTS,
                                 XFORM_CLIP, clip_wh, tracktor)
            for k, (a, w) in enumerate(zip(got, one)):
                assert torch.equal(a[n0:n1], w), (rows_per_image, "image %d" % b, "output %d" % k)
        n0 = n1
    return got


# (rows per image, dim6, dim7, classes, class-agnostic, amodal, TRACKTOR)
_WHOLE_CALLS = {
    # an empty image in the middle; class-agnostic with 56 classes = 64 columns, the last width the single call's post kernel
    # sums itself; amodal (no clip)
    "empty-middle-A56-amodal": ((30, 0, 17), 128, 64, 56, True, True, False),
    # the per-image maximum, one row, segments that straddle the row blocks of 128, an exact 16-row tile; per-class K = 12
    # (60 columns); TRACKTOR scores
    "128-1-128-16-K12-tracktor": ((128, 1, 128, 16), 128, 64, 12, False, False, True),
    # leading empties; class-agnostic with 57 classes = 65 columns (the single call reduces the head in a launch of its own)
    "leading-empties-A57": ((0, 0, 5), 128, 64, 57, True, False, False),
    # the call's cap: eight images of 128 rows
    "8x128-cap": ((128,) * 8, 128, 64, 3, False, False, False),
    # the yaml head (1024-1024, person / background) on four cameras of 30 tracks
    "4x30-yaml-head": ((30,) * 4, 1024, 1024, 2, False, False, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_WHOLE_CALLS))
def test_batched_refinement_equals_the_one_image_call_on_every_image(case):
    """``ops.box_refine_batched`` against ``ops.box_refine`` on ``features[l][b:b+1]`` and image b's rows: every output of
    every image, bit for bit."""
    import siammot_amd.ops as ops
    rows_per_image, dim6, dim7, classes, agnostic, amodal, tracktor = _WHOLE_CALLS[case]
    g = torch.Generator().manual_seed(len(case) * 131 + dim7)
    feats = _maps(g, len(rows_per_image))
    layers = _head(g, 16, dim6, dim7, classes, agnostic)
    rows = _rows(g, sum(rows_per_image), classes, amodal)
    assert sum(rows_per_image) <= ops.box_refine_batched_max_rows() == 1024
    got = _check_against_per_image_calls(feats, list(rows_per_image), rows, layers, None if amodal else IMAGE_WH, tracktor)
    if amodal:
        assert bool((got[0][:, 2] > 1279).any())             # nothing was clipped
    if not tracktor:
        assert float(got[1].min()) > 1.0 and float(got[1].max()) <= 2.0


# ---- 4. ranks, LDS tables and the score pairing are the image's own ------------------------------------------------------------
def _post_images(dirty):
    """Three images with K = 5 per-class heads.  Image 0: the 40 rows of ``nonfinite_case`` — clean and all of label 2, or
    (``dirty``) with its non-finite rows and its own random labels; image 1: 33 rows alternating labels 1 and 2; image 2:
    strictly descending labels."""
    d, clean, at = E.nonfinite_case(40, True)
    c0 = dict(d if dirty else clean)
    if not dirty:
        c0["labels"] = np.full(40, 2, np.int64)              # all rows of one label
    c1 = dict(E._generic("ranks", 2101, 33, 5))
    c1["labels"] = np.where(np.arange(33) % 2 == 0, 1, 2).astype(np.int64)
    c2 = dict(E._generic("ranks", 2102, 4, 5))
    c2["labels"] = np.array([4, 3, 2, 1], np.int64)
    return [c0, c1, c2]


def _post_call(ops, cases_):
    cat = lambda k: torch.from_numpy(np.concatenate([c[k] for c in cases_])).to(DEV)
    return ops.box_refine_post_batched(cat("head_out"), 5, 5, cat("boxes"), cat("labels"), cat("ids"), cat("track_conf"),
                                       [len(c["boxes"]) for c in cases_], WEIGHTS, XFORM_CLIP, IMAGE_WH)


def _post_single(ops, c):
    t = lambda k: torch.from_numpy(c[k]).to(DEV)
    return ops.box_refine_post(t("head_out"), 5, 5, t("boxes"), t("labels"), t("ids"), t("track_conf"), WEIGHTS, XFORM_CLIP,
                               IMAGE_WH)


@pytest.mark.gpu
def test_ranks_and_score_pairing_do_not_leak_between_images():
    """Each image's segment of ``ops.box_refine_post_batched`` equals ``ops.box_refine_post`` on it alone — the grouping by
    label, the ids, and the pairing of the box-head score of output row p with the matching score of INPUT row p of the
    SAME image.  With non-finite rows in image 0 the other two images are bit for bit what they are without them."""
    import siammot_amd.ops as ops
    results = {}
    for dirty in (False, True):
        imgs = _post_images(dirty)
        got = _post_call(ops, imgs)
        n0 = 0
        for b, c in enumerate(imgs):
            n1 = n0 + len(c["boxes"])
            one = _post_single(ops, c)
            for k, (a, w) in enumerate(zip(got, one)):
                assert _same_bits(a[n0:n1], w), (dirty, "image %d" % b, "output %d" % k)
            # the rows are the image's own, regrouped: its ids, in the stable order of its labels
            order = np.argsort(c["labels"], kind="stable")
            assert got[2][n0:n1].cpu().numpy().tolist() == c["ids"][order].tolist()
            assert got[3][n0:n1].cpu().numpy().tolist() == c["labels"][order].tolist()
            n0 = n1
        results[dirty] = got
    assert bool(torch.isnan(results[True][1][:40]).any())                    # the dirty rows did reach the kernel
    for k in range(4):
        assert _same_bits(results[True][k][40:], results[False][k][40:]), k
    # the pairing is by input row of the image: in image 2 (labels descending: the order reverses) a pairing by output row,
    # or by a row of the whole call, gives other scores
    c2 = _post_images(False)[2]
    ref = E.direct(c2, torch.float32)
    wrong = E.direct(c2, torch.float32, pairing="output")
    got2 = results[False][1][73:].cpu().numpy()
    assert np.abs(got2 - ref["scores"]).max() < 1e-5 < np.abs(got2 - wrong["scores"]).max()


# ---- 5. fp16 / bf16 maps, channels-last ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fp16-channels-last", "bf16-nchw"])
def test_batched_refinement_on_half_maps_equals_the_typed_one_image_call(form):
    g = torch.Generator().manual_seed(77)
    feats = _maps(g, 2)
    if form == "fp16-channels-last":
        feats = tuple(f.half().contiguous(memory_format=torch.channels_last) for f in feats)
    else:
        feats = tuple(f.bfloat16() for f in feats)
    layers = _head(g, 16, 128, 64, 3, False)
    rows = _rows(g, 47, 3)
    _check_against_per_image_calls(feats, [30, 17], rows, layers, IMAGE_WH, False)


# ---- 6. against the reference's own _refine_tracks ----------------------------------------------------------------------------
def _golden_head():
    from test_box_refine import _cfg
    from siammot_amd.box_refine import TrackBoxHead
    c, inp = gi.REFINE_CASE, gi.refine_case_inputs()
    head = TrackBoxHead(_cfg(), c["channels"])
    head.load_state_dict({k: torch.from_numpy(v) for k, v in inp["params"].items()}, strict=True)
    return c, inp, head.to(DEV).eval()


def _golden_batch(c, inp):
    """The seven-track golden case as image 1 of three; images 0 and 2 have other maps and other rows."""
    rs = np.random.RandomState(61)
    feats = []
    for f in inp["features"]:
        other = rs.standard_normal((2,) + f.shape[1:]).astype(np.float32)
        feats.append(torch.from_numpy(np.concatenate((other[:1], f, other[1:]))).to(DEV))
    W, H = c["image_wh"]
    def some(n):
        xy = rs.uniform(0, 1, (n, 2)) * (W - 60.0, H - 60.0)
        return (np.concatenate((xy, xy + rs.uniform(12, 120, (n, 2))), 1).astype(np.float32), rs.uniform(0.3, 1.0, n).astype(np.float32),
                (100 + rs.permutation(n)).astype(np.int64), rs.randint(1, c["num_classes"], n).astype(np.int64))
    parts = [some(5), tuple(inp[k] for k in ("track_boxes", "track_scores", "track_ids", "track_labels")), some(9)]
    args = [torch.from_numpy(np.concatenate([p[k] for p in parts])).to(DEV) for k in range(4)]
    return feats, args, [5, 7, 9]


@pytest.mark.gpu
def test_batched_refinement_matches_the_reference_golden_on_its_image():
    from test_box_refine import GOLD
    c, inp, head = _golden_head()
    g = np.load(GOLD)
    feats, args, rows = _golden_batch(c, inp)
    assert head.refine_batch_ok(rows)
    bb, sc, ids, lab = head.refine_raw_batched(feats, *args, rows, c["image_wh"])
    assert ids[5:12].cpu().tolist() == g["refine_ids"].tolist()
    assert lab[5:12].cpu().tolist() == g["refine_labels"].tolist()
    np.testing.assert_allclose(bb[5:12].cpu().numpy(), g["refine_bbox"], rtol=0, atol=2e-3)
    np.testing.assert_allclose(sc[5:12].cpu().numpy(), g["refine_scores"], rtol=0, atol=2e-5)
    assert sorted(ids[:5].cpu().tolist()) == list(range(100, 105)) and sorted(ids[12:].cpu().tolist()) == list(range(100, 109))


# ---- 7. no synchronisation ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refine_raw_batched_enqueues_without_a_host_synchronisation():
    from siammot_amd.box_refine import RefineTracks
    c, inp, head = _golden_head()
    feats, args, rows = _golden_batch(c, inp)
    refine = RefineTracks(head)
    assert refine.offers_batched() and refine.refine_batch_ok(rows)
    first = refine.refine_raw_batched(feats, *args, rows, c["image_wh"])           # warm-up: workspace, library handle
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                        # any host synchronisation inside raises
    try:
        again = refine.refine_raw_batched(feats, *args, rows, c["image_wh"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(first, again))


# ---- 8. the loop ----------------------------------------------------------------------------------------------------------------
class _CountedRefinement(object):
    """Beside ``test_multi_camera_gpu._Counted`` (solver entries, stream synchronisations): the calls of the two refinement
    entries of the library and of the ``RefineTracks`` object itself."""

    def __init__(self, refine):
        self.refine = refine

    def __enter__(self):
        from test_multi_camera_gpu import _Counted
        import siammot_amd.ops as ops
        self.base = _Counted().__enter__()
        self.lib = ops.load_library()
        self.real = (self.lib.smot_box_refine_batched_typed_fwd, self.lib.smot_box_refine_typed_fwd)
        self.batched = self.single = 0

        def batched(*a):
            self.batched += 1
            return self.real[0](*a)

        def single(*a):
            self.single += 1
            return self.real[1](*a)
        self.lib.smot_box_refine_batched_typed_fwd, self.lib.smot_box_refine_typed_fwd = batched, single
        return self

    def __exit__(self, *exc):
        self.lib.smot_box_refine_batched_typed_fwd, self.lib.smot_box_refine_typed_fwd = self.real
        self.base.__exit__(*exc)


def _refining_loops(B):
    """(multi-camera loop, B default ``TrackingLoop``s, the refinement) on one set of weights: the product's own
    ``RefineTracks`` over a small ``TrackBoxHead``."""
    import siammot_amd.ops as ops
    from test_multi_camera_gpu import _cfg
    from siammot_amd.box_refine import RefineTracks, TrackBoxHead, build_refine_tracks
    from siammot_amd.multi_camera import build_multi_camera_tracking_loop
    from siammot_amd.track_head import build_tracking_loop
    cfg = _cfg()
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    head = TrackBoxHead(cfg, 32).to(DEV).eval()
    with torch.no_grad():
        head.predictor.bbox_pred.weight.mul_(0.05)                 # small regressions: tracks stay near their objects
        head.predictor.cls_score.bias.copy_(torch.tensor([-2.0, 2.0]))

    class Counting(RefineTracks):
        calls = 0

        def __call__(self, features, tracks):
            Counting.calls += 1
            return RefineTracks.__call__(self, features, tracks)
    built = build_refine_tracks(cfg, 32, box_head=head)
    refine = Counting(built.box, built.tracktor)
    multi = build_multi_camera_tracking_loop(cfg, B, device=DEV, refine_tracks=refine)
    with torch.no_grad():
        for name in ("cls", "center", "reg"):
            getattr(multi.emm.predictor, name).weight.mul_(20.0)
    ops.tower_packed(multi.emm.predictor.param_dict())
    singles = [build_tracking_loop(cfg, device=DEV, refine_tracks=refine) for _ in range(B)]
    for lp in singles:
        lp.track.tracker.load_state_dict(multi.emm.state_dict())
    return multi, singles, refine, Counting


@pytest.mark.gpu
def test_multi_camera_loop_refines_all_cameras_in_one_call_and_equals_default_loops():
    """B = 3, camera 1 starved, 12 frames: outputs, pool state and track memory of every camera equal those of a default
    ``TrackingLoop`` of its own (which refines through the one-image one-call entry) in every frame; a step makes one
    synchronisation, one solver entry, ONE call of the refinement callable and one batched library entry; nothing falls back.
    With ``batched_refinement = False`` the callable is called once per camera that propagated boxes again."""
    import siammot_amd.ops as ops
    from test_multi_camera_gpu import _same_camera, _traffic
    B, FRAMES = 3, 12
    rs = np.random.RandomState(9)
    shapes = gi.feature_shapes((1280, 704), 32)
    maps = [tuple(torch.from_numpy(rs.standard_normal((B,) + tuple(s[1:])).astype(np.float32)).to(DEV) for s in shapes)
            for _ in range(2)]
    multi, singles, refine, Counting = _refining_loops(B)
    dets_of = _traffic((5, 6, 7), FRAMES)
    fallbacks = {k: ops.FALLBACKS[k] for k in ("refine_per_camera", "multi_camera_per_camera")}
    refined_steps = 0
    with _CountedRefinement(refine) as n:
        for f in range(FRAMES):
            feats = maps[f % 2]
            live = [b for b in range(B) if multi.track_memory[b] is not None and len(multi.track_memory[b][2][0]) > 0]
            before = (n.base.entry, n.base.syncs, n.batched, n.single, Counting.calls)
            outs = multi(feats, [dets_of(b, f).to(DEV) for b in range(B)])
            after = (n.base.entry, n.base.syncs, n.batched, n.single, Counting.calls)
            step = tuple(a - b for a, b in zip(after, before))
            assert step == (1, 1, 1 if live else 0, 0, 1 if live else 0), (f, live, step)
            refined_steps += bool(live)
            for b in range(B):
                want = singles[b](tuple(x[b:b + 1] for x in feats), dets_of(b, f).to(DEV))
                _same_camera(multi, b, outs[b], singles[b], want, "camera %d, frame %d" % (b, f))
        assert refined_steps >= 8
        assert ops.FALLBACKS["refine_per_camera"] == fallbacks["refine_per_camera"]
        assert ops.FALLBACKS["multi_camera_per_camera"] == fallbacks["multi_camera_per_camera"]
        # camera by camera on request: one call of the callable per camera with propagated boxes, no batched entry
        multi.batched_refinement = False
        live = [b for b in range(B) if multi.track_memory[b] is not None and len(multi.track_memory[b][2][0]) > 0]
        assert len(live) >= 2
        before = (n.batched, Counting.calls, ops.FALLBACKS["refine_per_camera"])
        multi(maps[0], [dets_of(b, FRAMES - 1).to(DEV) for b in range(B)])
        assert (n.batched, Counting.calls, ops.FALLBACKS["refine_per_camera"]) == (before[0], before[1] + len(live), before[2])


def test_refine_batch_ok_sends_an_image_over_128_rows_and_a_call_over_the_cap_camera_by_camera(monkeypatch):
    """The fallback's decision on the host: ``TrackBoxHead.refine_batch_ok`` by row counts (weights and library stubbed: no
    device here), and the loop's counter when the callable offers the batched form and refuses the step's counts."""
    import siammot_amd.ops as ops
    from test_box_refine import _cfg
    from siammot_amd.box_refine import RefineTracks, TrackBoxHead
    from siammot_amd.multi_camera import MultiCameraTrackingLoop
    c = gi.REFINE_CASE
    head = TrackBoxHead(_cfg(), c["channels"]).eval()
    monkeypatch.setattr(head, "raw_ok", lambda n: 0 < n <= 512)                      # (the device check of the weights aside)
    monkeypatch.setattr(ops, "linear_rows_max_rows", lambda: 128)
    monkeypatch.setattr(ops, "box_refine_batched_max_rows", lambda: 1024)
    assert head.refine_batch_ok([30, 0, 17]) and head.refine_batch_ok([128] * 8) and head.refine_batch_ok([0, 0, 5])
    assert not head.refine_batch_ok([129, 5])                  # an image that alone would not take the one-call path
    assert not head.refine_batch_ok([128] * 8 + [1])           # the call's cap
    assert not head.refine_batch_ok([0, 0]) and not head.refine_batch_ok([]) and not head.refine_batch_ok([1] * 65)
    assert not head.refine_batch_offered()                     # CPU weights: the loop does not even ask
    # the loop: a callable that offers the batched form and refuses these counts is called camera by camera, counted once
    from siammot_amd.structures import BoxList
    seen = []

    class Refusing(RefineTracks):
        def offers_batched(self):
            return True

        def batch_ok(self, tracks):
            seen.append([len(t) for t in tracks])
            return False

        def __call__(self, features, tracks):
            assert len(tracks) == 1 and features[0].shape[0] == 1
            return tracks
    loop = MultiCameraTrackingLoop(None, [None] * 3, [None] * 3, Refusing(None))
    t = BoxList(torch.zeros((2, 4)), (64, 64))
    before = ops.FALLBACKS["refine_per_camera"]
    assert loop._refine_batched((torch.zeros(3, 1, 2, 2),), [t, None, t]) is False
    assert seen == [[2, 0, 2]] and ops.FALLBACKS["refine_per_camera"] == before + 1
    loop.batched_refinement = False
    assert loop._refine_batched((torch.zeros(3, 1, 2, 2),), [t, None, t]) is False
    assert ops.FALLBACKS["refine_per_camera"] == before + 1 and len(seen) == 1


# ---- 9. RefineTracks.__call__ on several lists (host) --------------------------------------------------------------------------
def test_refine_tracks_on_several_lists_refines_every_image():
    """Three BoxLists on CPU tensors and a CPU ``TrackBoxHead`` (the oracle's pooler): three lists come back, each equal to
    the one-image call on ``f[b:b+1]``, the empty one untouched."""
    from oracle import box_head_oracle as BO
    from test_box_refine import _cfg, _cpu_nms, _proposals
    from siammot_amd.box_refine import RefineTracks, TrackBoxHead
    c, inp = gi.REFINE_CASE, gi.refine_case_inputs()
    head = TrackBoxHead(_cfg(), c["channels"], pooler=BO.OraclePooler(c["resolution"], c["scales"], c["sampling_ratio"]),
                        nms_fn=_cpu_nms)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in inp["params"].items()}, strict=True)
    head = head.eval()
    rs = np.random.RandomState(3)
    feats = [torch.from_numpy(np.concatenate((f, rs.standard_normal((2,) + f.shape[1:]).astype(np.float32)))) for f in inp["features"]]
    full = _proposals(inp["track_boxes"], inp["track_ids"], "cpu", inp["track_labels"], inp["track_scores"])
    empty = full[:0]
    part = _proposals(inp["track_boxes"][2:6], inp["track_ids"][2:6], "cpu", inp["track_labels"][2:6], inp["track_scores"][2:6])
    refine = RefineTracks(head)
    assert not refine.offers_batched()
    with torch.no_grad():
        out = refine(feats, [full, empty, part])
        want = [refine([f[b:b + 1] for f in feats], [t])[0] for b, t in ((0, full), (2, part))]
    assert len(out) == 3 and out[1] is empty
    for got, w in zip((out[0], out[2]), want):
        assert torch.equal(got.bbox, w.bbox) and sorted(got.fields()) == ["ids", "labels", "scores"]
        for k in got.fields():
            assert torch.equal(got.get_field(k), w.get_field(k)), k
    assert not torch.equal(out[2].bbox, refine([f[0:1] for f in feats], [part])[0].bbox)      # image 2's own maps were read
    np.testing.assert_allclose(out[0].bbox.numpy(), np.load(os.path.join(os.path.dirname(__file__), "golden",
                                                                         "refine_tracks.npz"))["refine_bbox"], rtol=0, atol=2e-4)


# ---- 10. symbols and argument validation (host: before any launch) --------------------------------------------------------------
def test_header_ops_table_and_library_agree_on_the_batched_refinement_symbols():
    from test_host import _header_symbols
    ops, lib = _library()
    for name in NEW_SYMBOLS:
        assert name in _header_symbols() and name in ops.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.smot_abi_version() == ops.ABI_VERSION == 14          # additive: the ABI version stands
    assert lib.smot_box_refine_batched_max_rows() == 1024 and lib.smot_linear_rows_max_rows() == 128
    assert "refine_per_camera" in ops.FALLBACKS
    # the workspace: rows of the four buffers + the largest layer's K-slice sums; refused calls answer 0
    ws = lib.smot_box_refine_batched_ws_floats
    assert ws(0, 16, 7, 128, 64, 3, 3) == ws(1025, 16, 7, 128, 64, 3, 3) == 0
    assert ws(30, 16, 7, 128, 64, 3, 3) >= 30 * (784 + 128 + 64 + 15)
    assert ws(256, 16, 7, 128, 64, 3, 3) > ws(128, 16, 7, 128, 64, 3, 3) > 0


def test_batched_refinement_entries_validate_before_any_launch():
    ops, lib = _library()
    BAD_ARG, UNSUPPORTED = -1, -2
    P = ctypes.c_void_p

    def table(row_start):
        return ctypes.cast((ctypes.c_int * (ops.MAX_IMAGES + 2))(*row_start), P)

    def whole(num_images, row_start, N, ptr=None, ws=None, pooled=7, dim6=128, table_=True):
        """``ptr``: what every data pointer holds (never dereferenced: every call here ends before its first launch)."""
        p = P(ptr)
        lv = ctypes.cast((P * 4)(*[ptr] * 4), P)
        hw = ctypes.cast((ctypes.c_int * 4)(8, 8, 8, 8), P)
        sc = ctypes.cast((ctypes.c_float * 4)(*SCALES), P)
        rc = lib.smot_box_refine_batched_typed_fwd(lv, 0, hw, hw, sc, 4, 16, pooled, 2, p, p, p, p, N, p, p, dim6, p, p, 64, p, p, 3,
                                                   p, p, 3, 10.0, 10.0, 5.0, 5.0, XFORM_CLIP, 1280.0, 704.0, 0, P(ws if ws else ptr),
                                                   p, p, p, p, None, num_images, table(row_start) if table_ else None)
        return rc, lib.smot_last_error()

    def post(num_images, row_start, N, ptr=None, table_=True):
        p = P(ptr)
        rc = lib.smot_box_refine_post_batched_fwd(p, 15, 3, 3, p, p, p, p, N, 10.0, 10.0, 5.0, 5.0, XFORM_CLIP, 1280.0, 704.0, 0,
                                                  p, p, p, p, None, num_images, table(row_start) if table_ else None)
        return rc, lib.smot_last_error()
    for call in (whole, post):
        rc, msg = call(0, [0], 0)
        assert rc == BAD_ARG and b"num_images=0" in msg, (call.__name__, rc, msg)
        rc, msg = call(65, [0] * 66, 0)
        assert rc == BAD_ARG and b"num_images=65" in msg
        rc, msg = call(2, [0, 4, 8], 8, table_=False)
        assert rc == BAD_ARG and b"null row_start" in msg
        rc, msg = call(2, [1, 8, 16], 16)
        assert rc == BAD_ARG and b"row_start[0]=1" in msg
        rc, msg = call(3, [0, 8, 4, 16], 16)
        assert rc == BAD_ARG and b"decreases at image 1" in msg
        rc, msg = call(2, [0, 8, 16], 17)
        assert rc == BAD_ARG and b"expected N=17" in msg
        # a legal table (an image without rows in it) reaches the pointer check: the row ranges came first
        rc, msg = call(3, [0, 8, 8, 16], 16)
        assert rc == BAD_ARG and b"null pointer" in msg
        # no image has rows: nothing is launched, whatever the pointers are
        assert call(3, [0, 0, 0, 0], 0)[0] == 0 and call(64, [0] * 65, 0)[0] == 0
    # the whole call: an image over 128 rows (named), the cap, the one-call path's own conditions — all before any pointer
    rc, msg = whole(3, [0, 8, 137, 140], 140)
    assert rc == UNSUPPORTED and b"image 1 has 129 rows" in msg
    rc, msg = whole(9, [128 * b for b in range(9)] + [1025], 1025)
    assert rc == UNSUPPORTED and b"1025 rows" in msg
    rc, msg = whole(2, [0, 8, 16], 16, pooled=14)
    assert rc == UNSUPPORTED and b"pooler 14x14" in msg
    rc, msg = whole(2, [0, 8, 16], 16, dim6=130)
    assert rc == UNSUPPORTED and b"layer widths" in msg
    rc, msg = whole(2, [0, 8, 16], 16, ptr=4096, ws=4096 + 8)
    assert rc == BAD_ARG and b"16-byte aligned" in msg
    # the post-processing alone: an image beyond the kernel's 512 rows, named
    rc, msg = post(2, [0, 8, 521], 521)
    assert rc == BAD_ARG and b"image 1 has 513 rows" in msg


# ---- 11. a callable without the batched form is still called camera by camera (host) ------------------------------------------
def test_the_loop_calls_a_plain_refinement_callable_camera_by_camera_on_cpu():
    import types
    from fake_tracker import SEQ, FakeTracker, detections
    from test_multi_camera import BatchedFakeTracker, _numpy_mask, _same_boxlist
    from siammot_amd.multi_camera import MultiCameraTrackingLoop
    from siammot_amd.solver import TrackPool, TrackSolver
    from siammot_amd.structures import BoxList
    from siammot_amd.track_head import TrackHead, TrackingLoop
    import siammot_amd.ops as ops
    B, FRAMES = 3, 6
    tu = types.SimpleNamespace(pad_pixels=SEQ["pad"])
    calls = []

    def refine(features, tracks):
        assert len(tracks) == 1 and features[0].shape[0] == 1
        calls.append(len(tracks[0]))
        t = tracks[0]
        out = BoxList(t.bbox + 1.0, t.size, mode=t.mode)
        out.add_field("ids", t.get_field("ids"))
        out.add_field("labels", t.get_field("labels"))
        out.add_field("scores", 1.0 + 0.5 * t.get_field("scores"))
        return [out]

    def parts(tracker):
        pool = TrackPool(max_dormant_frames=2)
        return TrackHead(tracker, tu, pool).eval(), TrackSolver(pool, *SEQ["thresholds"], nms_mask_fn=_numpy_mask)
    singles = [TrackingLoop(*parts(FakeTracker(SEQ["pad"])), refine_tracks=refine).eval() for _ in range(B)]
    shared = BatchedFakeTracker(SEQ["pad"])
    heads, solvers = zip(*[parts(shared) for _ in range(B)])
    multi = MultiCameraTrackingLoop(shared, list(heads), list(solvers), refine_tracks=refine).eval()
    assert multi.batched_refinement is True
    rs = [[np.random.RandomState(11 + b) for b in range(B)] for _ in range(2)]
    feats = (torch.zeros(B),)
    before = ops.FALLBACKS["refine_per_camera"]
    for f in range(FRAMES):
        dets = [[detections(r, f) for r in side] for side in rs]
        live = sum(1 for m in multi.track_memory if m is not None and len(m[2][0]) > 0)
        n_calls = len(calls)
        outs = multi(feats, dets[0])
        assert len(calls) == n_calls + live, f                                   # once per camera that propagated boxes
        for b in range(B):
            _same_boxlist(outs[b], singles[b](tuple(x[b:b + 1] for x in feats), dets[1][b]), "camera %d, frame %d" % (b, f))
    assert len(calls) >= 2 * B * (FRAMES - 1)                                    # (the single loops' calls included)
    assert ops.FALLBACKS["refine_per_camera"] == before                          # nothing wanted the batched form
