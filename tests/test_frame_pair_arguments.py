"""The frame pair's four kernels take their first-used arguments as leading pointers and scalars (kernel-argument preload,
siam-mot_amd/build.py).  A pointer that lands in the wrong slot goes wrong silently, so every launch path of the three
families is crossed here at the smallest shapes that reach it: C = 128, a 128 x 160 net input, N = 1 and N = 9 tracks (9
crosses the towers' 8-track grid padding).

No arithmetic changed, so paths that launch the same kernels are compared bit for bit; the one-call head against the
operators called one by one (stand-alone fp32 correlation instead of the matrix-pipe one) keeps the tolerances
tests/test_hip_parity.py::test_one_call_entry_points_equal_operator_composition applies between those two paths."""
import numpy as np
import pytest
import torch

from test_half_maps import DEV, FAMILIES, SCALES, Pair, _bits_equal, _boxes, _maps, _params, _same_pair

pytestmark = pytest.mark.gpu

C = 128
WH = (160, 128)                           # net input: 128 rows x 160 columns
SIZES = [(20, 30), (40, 60), (64, 40), (16, 16), (100, 80), (30, 90)]
CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


@pytest.fixture(scope="module")
def scene():
    """Maps of the two frames (fp16 values, held as fp32 and as fp16), boxes and one set of predictor weights — computed
    once, read by every test."""
    (ha, fa), (hb, fb) = _maps(C, WH, 101, torch.float16), _maps(C, WH, 102, torch.float16)
    boxes = _boxes(9, WH, 103, sizes=SIZES)
    return dict(ha=ha, fa=fa, hb=hb, fb=fb, boxes=boxes, params=_params(C, boxes, 104))


def _close(got, ref, atol, what):
    err = (got.double() - ref.double()).abs().max().item() if got.numel() else 0.0
    assert err <= atol, "%s: max |d| %.3e > %.1e" % (what, err, atol)


def _chain(ops, fam, fa, fb, boxes, params):
    """EMM.extract_cache and the head as the operators called one by one."""
    rx, rz, pad, exp, msw, sigma, cent = FAMILIES[fam]
    z = ops.roi_align_levels(fa, boxes, boxes, rz, SCALES, 2)
    sr = ops.search_region(boxes, pad, exp, msw)
    pc = [int(pad * s) for s in SCALES]
    x = ops.roi_align_levels(fb, sr, boxes, rx, SCALES, 2, pc)
    logits = ops.emm_predictor(ops.xcorr_depthwise(x, z), params)
    bb, conf, idx = ops.emm_decode(logits, sr, boxes, rx, rz, pad, sigma=sigma, use_centerness=cent, return_index=True,
                                   clip_wh=WH)
    return dict(bb=bb, conf=conf, idx=idx, z=z, sr=sr)


@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("fam", ["30/15", "35/7"])
def test_one_call_head_and_extraction_equal_the_operators_one_by_one(ops, scene, fam, n):
    """smot_roi_align -> smot_xcorr_dw -> smot_emm_predictor -> smot_emm_decode against the one-call entries; the 35 / 7
    family goes through the blocked 29 x 29 tower form and the decode kernel's logits source."""
    boxes = scene["boxes"][:n].contiguous()
    one, _ = Pair(ops, fam, C, WH, scene["params"]).run(scene["fa"], scene["fb"], boxes)
    ref = _chain(ops, fam, scene["fa"], scene["fb"], boxes, scene["params"])
    assert torch.equal(one["z"], ref["z"]) and torch.equal(one["sr"], ref["sr"])
    assert torch.equal(one["idx"], ref["idx"])
    _close(one["bb"], ref["bb"], 1e-3, "one call vs operators: boxes (%s, N=%d)" % (fam, n))
    _close(one["conf"], ref["conf"], 1e-5, "one call vs operators: conf (%s, N=%d)" % (fam, n))


@pytest.mark.parametrize("n", [1, 9])
def test_track_fwd_is_bit_identical_across_its_launch_paths(ops, scene, n):
    boxes = scene["boxes"][:n].contiguous()
    fa, fb, ha, hb = scene["fa"], scene["fb"], scene["ha"], scene["hb"]
    pair = Pair(ops, "30/15", C, WH, scene["params"])
    base, oh = pair.run(fa, fb, boxes)                                        # smot_emm_track_fwd, no hint
    assert (oh is not None) == (n >= 2)
    if oh is not None:                                                        # with the extraction's order hint
        hinted, _ = pair.run(fa, fb, boxes, hint=True)
        _same_pair(hinted, base, "hinted vs unhinted")
        assert ops.order_hint_status(oh) == 0
    batched, ohb = pair.run(fa, fb, boxes, rows=[n])                          # batched kernels, a batch of one image
    _same_pair(batched, base, "batched (one image) vs single image")
    if ohb is not None:
        _same_pair(pair.run(fa, fb, boxes, rows=[n], hint=True)[0], base, "batched with hint vs single image")
    # the typed entry on fp32 maps: feat_type 0, one image, rows [0, N]
    lib = ops.load_library()
    g = ops._geometry(fb, SCALES, pair.pad, boxes.device)
    assert g.ft == 0
    work = torch.empty((lib.smot_emm_track_ws_floats(n, C, pair.rx, pair.rz),), device=DEV)
    bb, conf = torch.empty((n, 4), device=DEV), torch.empty((n,), device=DEV)
    idx = torch.empty((n,), dtype=torch.int64, device=DEV)
    rc = ops._head_call(lib, g, batched=True)(
        boxes.data_ptr(), base["sr"].data_ptr(), base["z"].data_ptr(), n, pair.rx, pair.rz, 2,
        ops._param_block(scene["params"]).a_pp, 32, 1e-5, ops.hann_window(16 * ops.UP_SCALE, boxes.device).data_ptr(),
        pair.pad, pair.sigma, pair.cent, float(WH[0]), float(WH[1]), work.data_ptr(), bb.data_ptr(), conf.data_ptr(),
        idx.data_ptr(), None, ops._stream(boxes.device))
    assert rc == 0, lib.smot_last_error()
    torch.cuda.synchronize()
    for k, v in (("bb", bb), ("conf", conf), ("idx", idx)):
        _bits_equal(v, base[k], "typed entry on fp32 maps: %s" % k)
    # fp16 maps against their exact fp32 upcast (the *_half_* kernels)
    half, _ = pair.run(ha, hb, boxes, hint=oh is not None)
    _same_pair(half, base, "fp16 maps vs their fp32 upcast")
    # channels-last maps against NCHW, fp32 and fp16 (the *_nhwc_* kernels)
    for what, a, b in (("fp32", fa, fb), ("fp16", ha, hb)):
        ca, cb = tuple(f.to(memory_format=CL) for f in a), tuple(f.to(memory_format=CL) for f in b)
        assert ops._levels_layout(cb, 4) == ops.FEAT_CHANNELS_LAST
        _same_pair(pair.run(ca, cb, boxes, hint=oh is not None)[0], base, "channels-last %s vs NCHW" % what)


def test_masked_extraction_leaves_rows_past_n_valid_untouched(ops, scene):
    cap, nv = 9, 5
    boxes, fa = scene["boxes"], scene["fa"]
    rx, rz, pad, exp, msw = FAMILIES["30/15"][:5]
    z_ref, sr_ref = ops.emm_extract_cache(fa, boxes, rz, SCALES, 2, pad, exp, msw)
    lib = ops.load_library()
    g = ops._geometry(fa, SCALES, 0, boxes.device)
    sentinel = -12345.5
    z = torch.full((cap, C, rz, rz), sentinel, device=DEV)
    both = torch.full((cap * (ops.HINT_FLOATS + 4),), sentinel, device=DEV)
    sr, hint = both[cap * ops.HINT_FLOATS:].view(cap, 4), both[:cap * ops.HINT_FLOATS].view(cap, ops.HINT_FLOATS)
    n_valid = torch.tensor([nv], dtype=torch.int32, device=DEV)
    for with_hint in (False, True):
        z.fill_(sentinel)
        both.fill_(sentinel)
        rc = ops._extract_call(lib, g, masked=True)(boxes.data_ptr(), cap, rz, 2, pad, exp, msw, z.data_ptr(), sr.data_ptr(),
                                                    hint.data_ptr() if with_hint else None, ops._stream(boxes.device),
                                                    n_valid.data_ptr())
        assert rc == 0, lib.smot_last_error()
        torch.cuda.synchronize()
        _bits_equal(z[:nv], z_ref[:nv], "masked extraction: valid templates")
        _bits_equal(sr[:nv], sr_ref[:nv], "masked extraction: valid search regions")
        assert bool((z[nv:] == sentinel).all()) and bool((sr[nv:] == sentinel).all())
        assert bool((hint[nv:] == sentinel).all())                 # entries and by-roi records of rows that do not exist
        assert bool((hint[:nv] != sentinel).any()) == with_hint
    # the public masked call returns the same valid rows
    z2, sr2 = ops.emm_extract_cache(fa, boxes, rz, SCALES, 2, pad, exp, msw, n_valid=n_valid)
    _bits_equal(z2[:nv], z_ref[:nv], "emm_extract_cache(n_valid): templates")
    _bits_equal(sr2[:nv], sr_ref[:nv], "emm_extract_cache(n_valid): search regions")


def test_a_hint_of_other_boxes_still_poisons_every_row(ops, scene):
    pair = Pair(ops, "30/15", C, WH, scene["params"])
    boxes = scene["boxes"]
    z, sr, oh = pair.extract(scene["fa"], boxes, hint=True)
    other = _boxes(9, WH, 777, sizes=SIZES[::-1])
    z2, sr2, oh2 = pair.extract(scene["fa"], other, hint=True)
    assert oh is not None and ops.order_hint_status(oh) == 0
    bb, conf, _ = pair.track(scene["fb"], other, sr2, z2, order_hint=oh)      # the hint of `boxes` with the rois of `other`
    torch.cuda.synchronize()
    assert ops.order_hint_status(oh) != 0
    assert bool(torch.isnan(bb).all()) and bool(torch.isnan(conf).all())
    good, _, _ = pair.track(scene["fb"], other, sr2, z2, order_hint=oh2)      # its own hint: clean
    assert ops.order_hint_status(oh2) == 0 and not bool(torch.isnan(good).any())


@pytest.mark.parametrize("n", [1, 9])
def test_the_35_7_family_is_bit_identical_single_image_and_batched(ops, scene, n):
    boxes = scene["boxes"][:n].contiguous()
    pair = Pair(ops, "35/7", C, WH, scene["params"])
    base, _ = pair.run(scene["fa"], scene["fb"], boxes)
    _same_pair(pair.run(scene["fa"], scene["fb"], boxes, rows=[n])[0], base, "35/7 batched (one image) vs single image")
    _same_pair(pair.run(scene["ha"], scene["hb"], boxes)[0], base, "35/7 fp16 maps vs their fp32 upcast")
    assert not bool(torch.isnan(base["bb"]).any()) and np.isfinite(base["conf"].cpu().numpy()).all()
