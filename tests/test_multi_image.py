"""Several images (video streams) per call of the EMM head: smot_emm_track_batched_fwd / smot_emm_extract_cache_batched_fwd,
ops.emm_track_batched / ops.emm_extract_cache_batched and EMM.forward / EMM.extract_cache over lists of B BoxLists.

The contract: the rows of image b of a batched call get exactly — bit for bit — what a one-image call on that image's maps
gives them (boxes, scores, arg-max index, templates, search regions)."""
import ctypes

import numpy as np
import pytest
import torch

import golden_inputs as gi

DEV = "cuda:0"
SCALES = (0.25, 0.125, 0.0625, 0.03125)
# (rx, rz, pad_pixels, search_expansion, min_search_wh, sigma, use_centerness) of the two yaml families
FAMILIES = {"30/15": (30, 15, 512, 1.0, 0, 0.4, True), "35/7": (35, 7, 256, 4.0, 64, 0.1, False)}


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_batched_symbols_are_exported():
    import siammot_amd.ops as ops
    lib = ops.load_library()
    for name in ("smot_emm_track_batched_fwd", "smot_emm_extract_cache_batched_fwd"):
        assert name in ops.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert ops.ABI_VERSION == 14 and lib.smot_abi_version() == 14
    assert callable(ops.emm_track_batched) and callable(ops.emm_extract_cache_batched)


def _track_rc(lib, N, num_images, starts):
    null = ctypes.c_void_p(0)
    rs = (ctypes.c_int * len(starts))(*starts) if starts is not None else None
    return lib.smot_emm_track_batched_fwd(null, null, null, null, null, 4, 128, null, null, null, N, 30, 15, 2, null, 32,
                                          1e-5, null, 16, 512.0, 0.6, 0.4, 1, 0.0, 0.0, null, null, null, null, null, null,
                                          num_images, rs)


def _extract_rc(lib, N, num_images, starts):
    null = ctypes.c_void_p(0)
    rs = (ctypes.c_int * len(starts))(*starts) if starts is not None else None
    return lib.smot_emm_extract_cache_batched_fwd(null, null, null, null, 4, 128, null, N, 15, 2, 512.0, 1.0, 0.0, null,
                                                  null, null, null, num_images, rs)


@pytest.mark.parametrize("call", [_track_rc, _extract_rc])
def test_batched_argument_errors_are_reported_without_a_device(call):
    """Row-range validation happens before any launch (and before any pointer is looked at)."""
    import siammot_amd.ops as ops
    lib = ops.load_library()
    cases = [
        (3, 0, [0], b"num_images=0"),
        (3, 65, [0] * 65 + [3], b"num_images=65"),
        (3, 2, [1, 2, 3], b"row_start[0]=1"),
        (3, 3, [0, 2, 1, 3], b"decreases"),
        (3, 2, [0, 1, 2], b"expected N=3"),
        (3, 1, None, b"null row_start"),
    ]
    for N, b, starts, msg in cases:
        assert call(lib, N, b, starts) == -1, (N, b, starts)
        assert msg in lib.smot_last_error(), (lib.smot_last_error(), msg)
    # legal: images without rows, and no rows at all (nothing is launched)
    assert call(lib, 0, 3, [0, 0, 0, 0]) == 0
    assert call(lib, 0, 64, [0] * 65) == 0


def test_emm_forward_rejects_a_feature_batch_that_does_not_match_the_boxes():
    from siammot_amd.config import get_default_cfg
    from siammot_amd.emm import EMM
    from siammot_amd.structures import BoxList
    from siammot_amd.track_utils import build_track_utils
    cfg = get_default_cfg(channels=32)
    emm = EMM(cfg, build_track_utils(cfg)).eval()
    feats = tuple(torch.zeros((3, 32, 96 // s, 128 // s)) for s in (4, 8, 16, 32))
    boxes = [BoxList(torch.tensor([[1.0, 2.0, 30.0, 40.0]]), (128, 96), mode="xyxy") for _ in range(2)]
    with pytest.raises(RuntimeError, match="feature batch"):
        emm(feats, boxes, boxes, template_features=torch.zeros((2, 32, 15, 15)))
    with pytest.raises(RuntimeError, match="feature batch"):
        emm.extract_cache(feats, boxes)
    feats2 = tuple(f[:2] for f in feats)
    other = [boxes[0], BoxList(torch.tensor([[1.0, 2.0, 30.0, 40.0]]), (256, 96), mode="xyxy")]
    with pytest.raises(RuntimeError, match="differ in size"):
        emm(feats2, other, other, template_features=torch.zeros((2, 32, 15, 15)))
    with pytest.raises(RuntimeError, match="template_features"):
        emm(feats2, boxes, boxes, template_features=torch.zeros((3, 32, 15, 15)))


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


def _maps(B, C, image_wh, seed, copies_of_one=False):
    W, H = image_wh
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in (4, 8, 16, 32):
        shape = (1 if copies_of_one else B, C, H // s, W // s)
        f = torch.randn(shape, generator=g)
        out.append((f.expand(B, -1, -1, -1) if copies_of_one else f).contiguous().to(DEV))
    return tuple(out)


def _boxes(n, image_wh, seed):
    rs = np.random.RandomState(seed)
    sizes = [(32, 64), (64, 128), (100, 200), (160, 320), (24, 24), (300, 120)]
    out = []
    for i in range(n):
        w, h = sizes[i % len(sizes)]
        w, h = min(w, image_wh[0] - 2), min(h, image_wh[1] - 2)
        x1 = rs.uniform(-0.2 * w, image_wh[0] - 0.8 * w)
        y1 = rs.uniform(-0.2 * h, image_wh[1] - 0.8 * h)
        out.append([x1, y1, x1 + w, y1 + h])
    return torch.tensor(np.array(out, dtype=np.float32)).to(DEV)


def _params(C, boxes, seed):
    p = gi.predictor_params(np.random.RandomState(seed), C, boxes.cpu().numpy())
    return {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}


def _img(feats, b):
    return tuple(f[b:b + 1] for f in feats)


class Pair(object):
    """One frame pair (extraction on maps A, head on maps B) through the batched or the single-image entry points."""

    def __init__(self, ops, fam, C, image_wh, params):
        self.ops, self.C, self.image_wh, self.params = ops, C, image_wh, params
        self.rx, self.rz, self.pad, self.exp, self.msw, self.sigma, self.cent = FAMILIES[fam]

    def extract(self, fa, boxes, rows=None, hint=False):
        o = self.ops
        if rows is None:
            return o.emm_extract_cache(fa, boxes, self.rz, SCALES, 2, self.pad, self.exp, self.msw, hint=hint)
        return o.emm_extract_cache_batched(fa, boxes, rows, self.rz, SCALES, 2, self.pad, self.exp, self.msw, hint=hint)

    def track(self, fb, boxes, sr, z, rows=None, order_hint=None):
        o = self.ops
        kw = dict(sigma=self.sigma, use_centerness=self.cent, clip_wh=self.image_wh, return_index=True, order_hint=order_hint)
        if rows is None:
            return o.emm_track(fb, boxes, sr, z, self.params, self.rx, self.rz, SCALES, 2, self.pad, **kw)
        return o.emm_track_batched(fb, boxes, sr, z, rows, self.params, self.rx, self.rz, SCALES, 2, self.pad, **kw)

    def run(self, fa, fb, boxes, rows=None, hint=False):
        z, sr, oh = self.extract(fa, boxes, rows, hint=True)
        bb, conf, idx = self.track(fb, boxes, sr, z, rows, order_hint=oh if hint else None)
        torch.cuda.synchronize()
        return dict(bb=bb, conf=conf, idx=idx, z=z, sr=sr), oh


def _bitwise(a, b, what, rows=None):
    for k in ("bb", "conf", "idx", "z", "sr"):
        x, y = a[k], b[k]
        if rows is not None:
            x = x[rows[0]:rows[1]]
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        assert torch.equal(x, y), "%s: %s differs (max |d| %s)" % (what, k, (x.double() - y.double()).abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("hint", [False, True])
@pytest.mark.parametrize("fam", ["30/15", "35/7"])
def test_batch_of_copies_equals_one_call_with_all_rows(ops, fam, hint):
    C, wh, B = 128, (1280, 704), 4
    fa, fb = _maps(B, C, wh, 1, copies_of_one=True), _maps(B, C, wh, 2, copies_of_one=True)
    boxes = _boxes(30, wh, 3)
    P = Pair(ops, fam, C, wh, _params(C, boxes, 4))
    rows = [8, 7, 0, 15]
    got, oh = P.run(fa, fb, boxes, rows, hint=hint)
    ref, _ = P.run(_img(fa, 0), _img(fb, 0), boxes, None, hint=hint)
    if hint and fam == "30/15":
        assert oh is not None and ops.order_hint_status(oh) == 0
    _bitwise(got, ref, "%s hint=%s" % (fam, hint))


def _per_image_check(ops, P, fa, fb, boxes, rows, got, fam):
    """The rows of every image equal a one-image call on that image (bitwise; the oracle's tolerances where the tower form
    of the image's own track count is not the batch's)."""
    lib = ops.load_library()
    ho = P.rx - P.rz + 1
    n0 = 0
    for b, r in enumerate(rows):
        if r > 0:
            ref, _ = P.run(_img(fa, b), _img(fb, b), boxes[n0:n0 + r])
            if lib.smot_emm_tower_form(r, P.C, ho) == lib.smot_emm_tower_form(sum(rows), P.C, ho):
                _bitwise(got, ref, "%s image %d" % (fam, b), rows=(n0, n0 + r))
            else:
                _against_oracle(P, fa, fb, b, boxes[n0:n0 + r], {k: v[n0:n0 + r] for k, v in got.items()}, ref)
        n0 += r


def _against_oracle(P, fa, fb, b, boxes, got, ref):
    from oracle import emm_oracle as O
    cfg = O.EMMConfig(channels=P.C, rz=P.rz, search_region=P.rx / P.rz, scales=SCALES, pad_pixels=P.pad,
                      min_search_wh=P.msw, use_centerness=P.cent, sigma=P.sigma, amodal=False)
    cpu = lambda t: t.detach().cpu()
    z_ref, sr_ref = O.extract_cache(cfg, [cpu(f[b:b + 1]) for f in fa], cpu(boxes))
    bb, conf, _ = O.emm_forward(cfg, {k: cpu(v) for k, v in P.params.items()}, [cpu(f[b:b + 1]) for f in fb], cpu(boxes),
                                sr_ref, z_ref, P.image_wh)
    assert torch.equal(got["idx"], ref["idx"])
    assert (cpu(got["bb"]) - bb).abs().max() < 5e-2 and (cpu(got["conf"]) - conf).abs().max() < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["30/15", "35/7"])
def test_distinct_images_equal_one_image_calls_and_permute(ops, fam):
    C, wh, B = 128, (1280, 704), 3
    fa, fb = _maps(B, C, wh, 11), _maps(B, C, wh, 12)
    rows = [9, 5, 12]
    boxes = _boxes(sum(rows), wh, 13)
    P = Pair(ops, fam, C, wh, _params(C, boxes, 14))
    got, _ = P.run(fa, fb, boxes, rows, hint=True)
    _per_image_check(ops, P, fa, fb, boxes, rows, got, fam)
    # images (and their rows) in another order: the outputs in that order
    perm = [2, 0, 1]
    starts = np.cumsum([0] + rows)
    ridx = torch.tensor(np.concatenate([np.arange(starts[b], starts[b + 1]) for b in perm]), device=DEV)
    pf = lambda fs: tuple(f[perm].contiguous() for f in fs)
    got_p, _ = P.run(pf(fa), pf(fb), boxes[ridx], [rows[b] for b in perm], hint=True)
    _bitwise({k: v[ridx] for k, v in got.items()}, got_p, "%s permuted" % fam)


@pytest.mark.gpu
def test_edges_empty_images_single_image_many_rows_and_max_images(ops):
    C, wh = 64, (512, 384)
    fa, fb = _maps(5, C, wh, 21), _maps(5, C, wh, 22)
    boxes = _boxes(12, wh, 23)
    P = Pair(ops, "30/15", C, wh, _params(C, boxes, 24))
    for rows in ([0, 0, 4, 3, 5], [4, 0, 0, 8, 0], [6, 0, 0, 0, 6], [0, 12, 0, 0, 0]):
        got, _ = P.run(fa, fb, boxes, rows, hint=True)
        _per_image_check(ops, P, fa, fb, boxes, rows, got, "rows %s" % rows)
    # all images empty
    z, sr = P.extract(fa, boxes[:0], [0] * 5)
    bb, conf, idx = P.track(fb, boxes[:0], sr, z, [0] * 5)
    assert bb.shape == (0, 4) and conf.shape == (0,) and z.shape == (0, C, 15, 15)
    # one image through the batched entry == the existing entry
    got, _ = P.run(_img(fa, 3), _img(fb, 3), boxes, [12], hint=True)
    ref, _ = P.run(_img(fa, 3), _img(fb, 3), boxes, None, hint=True)
    _bitwise(got, ref, "B=1")
    # more than 256 rows: no hint is written, the head ranks / runs unhinted
    big = _boxes(280, wh, 25)
    rows = [100, 0, 90, 40, 50]
    got, oh = P.run(fa, fb, big, rows, hint=True)
    assert oh is None
    _per_image_check(ops, P, fa, fb, big, rows, got, "280 rows")
    # SMOT_MAX_IMAGES images on small maps, one or two rows each (some none)
    B, wh2 = ops.MAX_IMAGES, (256, 192)
    fa2, fb2 = _maps(B, 32, wh2, 26), _maps(B, 32, wh2, 27)
    rows = [(b % 3) for b in range(B)]
    small = _boxes(sum(rows), wh2, 28)
    P2 = Pair(ops, "30/15", 32, wh2, _params(32, small, 29))
    got, _ = P2.run(fa2, fb2, small, rows, hint=True)
    _per_image_check(ops, P2, fa2, fb2, small, rows, got, "64 images")


@pytest.mark.gpu
def test_images_past_4_gib(ops):
    """C = 256 maps of a 1056x1920 input: level 0 of one image is 130 MB, so image 34 starts past 2^32 bytes."""
    C, wh, B = 256, (1920, 1056), 35
    W, H = wh
    last = B - 1
    fa, fb = [], []
    g = torch.Generator().manual_seed(31)
    for s in (4, 8, 16, 32):
        for lst in (fa, fb):
            f = torch.zeros((B, C, H // s, W // s), device=DEV)
            f[last].copy_(torch.randn((C, H // s, W // s), generator=g))
            f[0].copy_(torch.randn((C, H // s, W // s), generator=g))
            lst.append(f)
    assert fa[0][last].data_ptr() - fa[0].data_ptr() >= 2 ** 32
    rows = [2] + [0] * (B - 2) + [6]
    boxes = _boxes(8, wh, 32)
    P = Pair(ops, "30/15", C, wh, _params(C, boxes, 33))
    got, _ = P.run(fa, fb, boxes, rows, hint=True)
    ref, _ = P.run(_img(fa, last), _img(fb, last), boxes[2:], None, hint=True)
    _bitwise(got, ref, "image %d" % last, rows=(2, 8))
    ref0, _ = P.run(_img(fa, 0), _img(fb, 0), boxes[:2], None, hint=True)
    _bitwise(got, ref0, "image 0", rows=(0, 2))
    del fa, fb
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_order_hint_of_a_batched_extraction(ops):
    C, wh = 128, (1280, 704)
    fa, fb = _maps(4, C, wh, 41), _maps(4, C, wh, 42)
    rows = [10, 6, 0, 14]
    boxes = _boxes(30, wh, 43)
    P = Pair(ops, "30/15", C, wh, _params(C, boxes, 44))
    hinted, oh = P.run(fa, fb, boxes, rows, hint=True)
    plain, _ = P.run(fa, fb, boxes, rows, hint=False)
    assert oh is not None and ops.order_hint_status(oh) == 0
    _bitwise(hinted, plain, "hint vs none")
    # a hint made under another row split: identical results, or NaN rows with the status word raised — never other numbers
    other = [5, 5, 10, 10]
    z, sr, oh2 = P.extract(fa, boxes, other, hint=True)
    bb, conf, idx = P.track(fb, boxes, plain["sr"], plain["z"], rows, order_hint=oh2)
    torch.cuda.synchronize()
    if ops.order_hint_status(oh2) == 0:
        assert torch.equal(bb, plain["bb"]) and torch.equal(conf, plain["conf"]) and torch.equal(idx, plain["idx"])
    else:
        assert torch.isnan(bb).all() and torch.isnan(conf).all()


@pytest.mark.gpu
def test_module_loop_of_four_streams_equals_four_single_stream_loops(ops):
    from siammot_amd.config import get_default_cfg
    from siammot_amd.emm import EMM
    from siammot_amd.structures import BoxList
    from siammot_amd.track_utils import build_track_utils
    C, wh, B, T = 64, (512, 384), 4, 20
    cfg = get_default_cfg(channels=C)
    emm = EMM(cfg, build_track_utils(cfg)).to(DEV).eval()
    counts = [4, 1, 3, 6]
    init = _boxes(sum(counts), wh, 51)
    emm.predictor.load_state_dict(_params(C, init, 52))
    frames = [_maps(B, C, wh, 100 + t) for t in range(T + 1)]

    def det_of(b):
        n0 = sum(counts[:b])
        d = BoxList(init[n0:n0 + counts[b]].clone(), wh, mode="xyxy")
        d.add_field("ids", torch.arange(n0, n0 + counts[b], device=DEV))
        d.add_field("labels", torch.ones(counts[b], dtype=torch.int64, device=DEV))
        return d

    singles = []
    with torch.no_grad():
        for b in range(B):
            det, outs = det_of(b), []
            for t in range(T):
                z, sr, d = emm.extract_cache(_img(frames[t], b), det)
                _, res, _ = emm(_img(frames[t + 1], b), d, sr, template_features=z)
                det = res[0]
                outs.append((z, sr[0].bbox, det.bbox, det.get_field("scores")))
            singles.append(outs)
        dets = [det_of(b) for b in range(B)]
        for t in range(T):
            z, srs, ds = emm.extract_cache(frames[t], dets)
            assert len(srs) == B and len(ds) == B
            _, res, _ = emm(frames[t + 1], ds, srs, template_features=z)
            assert len(res) == B
            n0 = 0
            for b in range(B):
                zs, srb, bb, sc = singles[b][t]
                assert torch.equal(z[n0:n0 + counts[b]], zs), (t, b)
                assert torch.equal(srs[b].bbox, srb), (t, b)
                assert torch.equal(res[b].bbox, bb) and torch.equal(res[b].get_field("scores"), sc), (t, b)
                assert torch.equal(res[b].get_field("ids"), dets[b].get_field("ids"))
                n0 += counts[b]
            dets = res


# ---- the generic poolers of a batch (pooled sizes / sampling ratios that neither separable kernel takes) -----------------
GENERIC_WH, GENERIC_ROWS = (256, 128), [2, 0, 3]          # four levels, 64 x 32 down to 8 x 4; the second image has no rows
FAMILIES["20/9"] = (20, 9, 512, 1.0, 0, 0.4, True)        # (20, 10) is refused by the decode kernel's check (odd rz only)


def _generic_maps(seed, dtype, layout):
    f = tuple(m.to(dtype) for m in _maps(len(GENERIC_ROWS), 32, GENERIC_WH, seed))
    return tuple(m.to(memory_format=torch.channels_last) for m in f) if layout == "channels-last" else f


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("layout", ["NCHW", "channels-last"])
def test_generic_poolers_of_a_batch_equal_one_image_calls(ops, layout, dtype):
    """rz = 9 at sampling ratios 1..4: the generic ROIAlign kernel's batched forms (and, for the search regions, the
    stand-alone kernel) against the single-image forms on each image's maps, bit for bit."""
    fa = _generic_maps(61, dtype, layout)
    boxes = _boxes(sum(GENERIC_ROWS), GENERIC_WH, 62)
    for ratio in (1, 2, 3, 4):
        z, sr = ops.emm_extract_cache_batched(fa, boxes, GENERIC_ROWS, 9, SCALES, ratio, 512, 1.0, 0)
        assert z.shape == (sum(GENERIC_ROWS), 32, 9, 9) and sr.shape == (sum(GENERIC_ROWS), 4)
        n0 = 0
        for b, r in enumerate(GENERIC_ROWS):
            z1, sr1 = ops.emm_extract_cache(_img(fa, b), boxes[n0:n0 + r], 9, SCALES, ratio, 512, 1.0, 0)
            assert z1.shape == (r, 32, 9, 9) and sr1.shape == (r, 4)
            assert torch.equal(z[n0:n0 + r], z1), "templates: ratio %d, image %d" % (ratio, b)
            assert torch.equal(sr[n0:n0 + r], sr1), "search regions: ratio %d, image %d" % (ratio, b)
            n0 += r


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_generic_head_of_a_batch_equals_one_image_calls(ops, dtype):
    """(rx, rz) = (20, 9) takes neither fused kernel: generic pooler + smot_xcorr_dw_fwd, batched against image by image."""
    fa, fb = _generic_maps(71, dtype, "NCHW"), _generic_maps(72, dtype, "NCHW")
    boxes = _boxes(sum(GENERIC_ROWS), GENERIC_WH, 73)
    P = Pair(ops, "20/9", 32, GENERIC_WH, _params(32, boxes, 74))
    got, _ = P.run(fa, fb, boxes, GENERIC_ROWS)
    assert got["bb"].shape == (sum(GENERIC_ROWS), 4) and torch.isfinite(got["bb"]).all() and torch.isfinite(got["conf"]).all()
    _per_image_check(ops, P, fa, fb, boxes, GENERIC_ROWS, got, "20/9")
