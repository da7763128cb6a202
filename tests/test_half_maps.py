"""fp16 / bf16 feature maps through the tracker head and its poolers (the ``smot_*_typed_fwd`` entry points).

The contract: for T in {fp16, bf16}, a call on maps of element type T returns BIT FOR BIT what the same call returns on
``maps.float()`` — the conversion T -> fp32 is exact and the kernels convert in registers right behind each load.  No
tolerance appears below except in the one anchor against the oracle's pooler (the fp32 pooler's own bound).  Comparison
rule: NaN positions identical, every other value bit-identical (NaN payloads are not compared)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import golden_inputs as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SCALES = (0.25, 0.125, 0.0625, 0.03125)
# (rx, rz, pad_pixels, search_expansion, min_search_wh, sigma, use_centerness) of the two yaml families
FAMILIES = {"30/15": (30, 15, 512, 1.0, 0, 0.4, True), "35/7": (35, 7, 256, 4.0, 64, 0.1, False)}
HALF = [torch.float16, torch.bfloat16]
TYPED = ("smot_roi_align_levels_typed_fwd", "smot_roi_align_typed_fwd", "smot_sr_xcorr_fused_typed_fwd",
         "smot_sr_xcorr_gather_typed_fwd", "smot_emm_track_typed_fwd", "smot_emm_extract_cache_typed_fwd",
         "smot_box_refine_typed_fwd", "smot_track_frame_typed_fwd")


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_typed_symbols_are_declared_bound_and_exported():
    import siammot_amd.ops as ops
    lib = ops.load_library()
    src = open(os.path.join(ROOT, "include", "smot_emm.h")).read()
    for name in TYPED:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in ops.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name, val in (("SMOT_FEAT_F32", 0), ("SMOT_FEAT_F16", 1), ("SMOT_FEAT_BF16", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src), name
    assert ops.FEAT_TYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    assert ops.ABI_VERSION == 14 and lib.smot_abi_version() == 14        # additive: the ABI version stands


def _typed_calls(lib):
    """Each typed entry point on null pointers and N = 0 rows, as a function of feat_type."""
    null = ctypes.c_void_p(0)
    rs = (ctypes.c_int * 2)(0, 0)
    return {
        "roi_align_levels": lambda ft: lib.smot_roi_align_levels_typed_fwd(null, ft, null, null, null, null, 4, 128, null, null, 0,
                                                                           15, 15, 2, null, null, null),
        "roi_align": lambda ft: lib.smot_roi_align_typed_fwd(null, ft, 1, 128, 8, 8, 0, null, 0, 0.25, 7, 7, 2, null, null),
        "sr_xcorr_fused": lambda ft: lib.smot_sr_xcorr_fused_typed_fwd(null, ft, null, null, null, null, 4, 128, null, null, null,
                                                                       0, 30, 15, 2, null, null, null),
        "sr_xcorr_gather": lambda ft: lib.smot_sr_xcorr_gather_typed_fwd(null, ft, null, null, null, null, 4, 128, null, null, null,
                                                                         0, 35, 7, 2, null, null),
        "emm_track": lambda ft: lib.smot_emm_track_typed_fwd(null, ft, null, null, null, null, 4, 128, null, null, null, 0, 30, 15,
                                                             2, null, 32, 1e-5, null, 16, 512.0, 0.6, 0.4, 1, 0.0, 0.0, null, null,
                                                             null, null, null, null, 1, rs),
        "emm_extract_cache": lambda ft: lib.smot_emm_extract_cache_typed_fwd(null, ft, null, null, null, 4, 128, null, 0, 15, 2,
                                                                             512.0, 1.0, 0.0, null, null, null, null, 1, rs, null),
        "box_refine": lambda ft: lib.smot_box_refine_typed_fwd(null, ft, null, null, null, 4, 128, 7, 2, null, null, null, null, 0,
                                                               null, null, 1024, null, null, 1024, null, null, 2, null, null, 2,
                                                               10.0, 10.0, 5.0, 5.0, 4.135, 0.0, 0.0, 0, null, null, null, null,
                                                               null, null),
    }


def test_unknown_feat_type_is_refused_before_anything_is_looked_at():
    import siammot_amd.ops as ops
    lib = ops.load_library()
    calls = _typed_calls(lib)
    calls["track_frame"] = lambda ft: lib.smot_track_frame_typed_fwd(ctypes.c_void_p(0), ft, ctypes.c_void_p(0))
    for name, call in calls.items():
        for bad in (3, -1):
            assert call(bad) == -1, (name, bad)
            msg = lib.smot_last_error()
            assert b"feat_type=%d" % bad in msg, (name, bad, msg)
    # the legal empty call (no rows: nothing is launched, no pointer is read) for all three types
    del calls["track_frame"]                 # (its argument block cannot be null)
    for name, call in calls.items():
        for ft in (0, 1, 2):
            assert call(ft) == 0, (name, ft, lib.smot_last_error())
    # the masked extraction through the typed entry point is a one-image form
    null = ctypes.c_void_p(0)
    rs = (ctypes.c_int * 3)(0, 0, 0)
    assert lib.smot_emm_extract_cache_typed_fwd(null, 1, null, null, null, 4, 128, null, 0, 15, 2, 512.0, 1.0, 0.0, null, null,
                                                null, null, 2, rs, ctypes.c_void_p(8)) == -1
    assert b"num_images == 1" in lib.smot_last_error()


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


def _bits_equal(a, b, what):
    """NaN positions identical, every non-NaN value bit-identical."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.numel() == 0:
        return
    if a.dtype.is_floating_point:
        na, nb = torch.isnan(a), torch.isnan(b)
        assert torch.equal(na, nb), "%s: NaN positions differ (%d vs %d NaNs)" % (what, int(na.sum()), int(nb.sum()))
        ia, ib = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
        same = (ia == ib) | na
        assert bool(same.all()), "%s: %d of %d values differ in bits (max |d| %s)" % (
            what, int((~same).sum()), a.numel(), (a.double() - b.double())[~na].abs().max().item())
    else:
        assert torch.equal(a, b), what


def _hint_equal(a, b, what):
    """Order hints are compared as bytes (they hold geometry, never map data)."""
    assert (a is None) == (b is None), what
    if a is not None:
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def _maps(C, image_wh, seed, dtype, B=1, widths=None, scale=1.0):
    """Half maps of an image (levels /4 .. /32, or the given level widths) and their exact fp32 upcast."""
    W, H = image_wh
    g = torch.Generator().manual_seed(seed)
    half = []
    for l, s in enumerate((4, 8, 16, 32)):
        w = W // s if widths is None else widths[l]
        half.append((torch.randn((B, C, H // s, w), generator=g) * scale).to(dtype).to(DEV))
    return tuple(half), tuple(f.float() for f in half)


def _boxes(n, image_wh, seed, sizes=None):
    rs = np.random.RandomState(seed)
    sizes = sizes or [(32, 64), (64, 128), (100, 200), (160, 320), (24, 24), (300, 120)]
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
    """One frame pair (extraction on maps A, head on maps B) through the public one-image or batched operators."""

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


def _same_pair(a, b, what, rows=None):
    for k in ("bb", "conf", "idx", "z", "sr"):
        x = a[k] if rows is None else a[k][rows[0]:rows[1]]
        _bits_equal(x, b[k], "%s: %s" % (what, k))


# 3. the poolers and the two pooling + correlation operators
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
def test_poolers_and_correlation_operators_equal_the_upcast_call(ops, dtype):
    C, wh = 128, (1280, 704)
    h, f = _maps(C, wh, 1, dtype)
    boxes = _boxes(30, wh, 2)
    for fam in FAMILIES:
        rx, rz, pad, exp, msw = FAMILIES[fam][:5]
        sr = ops.search_region(boxes, pad, exp, msw)
        pc = [int(pad / ((2 ** i) * 4)) for i in range(4)]
        for size in (7, 15, 30, 35):          # 7 / 15 / 30: the separable kernel; 35: the generic one
            got, lv = ops.roi_align_levels(h, sr, boxes, size, SCALES, 2, pc, return_levels=True)
            ref, lr = ops.roi_align_levels(f, sr, boxes, size, SCALES, 2, pc, return_levels=True)
            assert got.dtype is torch.float32
            _bits_equal(got, ref, "roi_align_levels %d (%s)" % (size, fam))
            assert torch.equal(lv, lr)
        z = ops.roi_align_levels(f, boxes, boxes, rz, SCALES, 2)
        _bits_equal(ops.sr_xcorr_fused(h, boxes, sr, z, rx, rz, SCALES, 2, pad),
                    ops.sr_xcorr_fused(f, boxes, sr, z, rx, rz, SCALES, 2, pad), "sr_xcorr_fused %s" % fam)
        if fam == "30/15":
            a = ops.sr_xcorr_fused(h, boxes, sr, z, rx, rz, SCALES, 2, pad, return_pooled=True)
            b = ops.sr_xcorr_fused(f, boxes, sr, z, rx, rz, SCALES, 2, pad, return_pooled=True)
            _bits_equal(a[1], b[1], "pooled planes of the fused kernel")
    # generic kernel at other sampling ratios (its staged and its direct-gather branch: a roi as large as the image)
    wide = torch.tensor([[0.0, 0.0, 1279.0, 40.0], [5.0, 3.0, 1270.0, 700.0], [100.0, 100.0, 180.0, 190.0]], device=DEV)
    for g in (1, 3, 4):
        _bits_equal(ops.roi_align_levels(h[:1], wide, wide, 9, SCALES[:1], g), ops.roi_align_levels(f[:1], wide, wide, 9, SCALES[:1], g),
                    "generic kernel, sampling ratio %d" % g)
    # layers.ROIAlign / poolers.Pooler: half in, fp32 out (upstream's float_function)
    from siammot_amd.layers import ROIAlign
    from siammot_amd.poolers import Pooler
    from siammot_amd.structures import BoxList
    hb, fb = _maps(64, (512, 384), 3, dtype, B=3)
    rois5 = torch.cat([torch.tensor([[0.0], [2.0], [1.0], [2.0], [5.0]], device=DEV), _boxes(5, (512, 384), 4)], dim=1)
    for lvl, scale in ((0, 0.25), (2, 0.0625)):
        ra = ROIAlign((7, 7), scale, 2)
        got, ref = ra(hb[lvl], rois5), ra(fb[lvl], rois5)
        assert got.dtype is torch.float32
        _bits_equal(got, ref, "layers.ROIAlign level %d" % lvl)
    pooler = Pooler((7, 7), SCALES, 2)
    bl = [BoxList(boxes, wh, mode="xyxy")]
    _bits_equal(pooler(h, bl), pooler(f, bl), "poolers.Pooler")


# 4. the two halves of a frame pair, both yaml families, with and without hint, and hints across the two types
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("fam", ["30/15", "35/7"])
def test_extract_cache_and_track_equal_the_upcast_call(ops, fam, dtype):
    C, wh = 128, (1280, 704)
    (ha, fa), (hb, fb) = _maps(C, wh, 11, dtype), _maps(C, wh, 12, dtype)
    boxes = _boxes(30, wh, 13)
    P = Pair(ops, fam, C, wh, _params(C, boxes, 14))
    # extraction, plain and with hint
    zh, srh = P.extract(ha, boxes)
    zf, srf = P.extract(fa, boxes)
    _bits_equal(zh, zf, "templates")
    _bits_equal(srh, srf, "search regions")
    assert zh.dtype is torch.float32
    for hint in (False, True):
        got, oh_h = P.run(ha, hb, boxes, hint=hint)
        ref, oh_f = P.run(fa, fb, boxes, hint=hint)
        _same_pair(got, ref, "%s hint=%s" % (fam, hint))
        _hint_equal(oh_h, oh_f, "order hint bytes")
        if fam == "30/15":
            assert oh_h is not None and ops.order_hint_status(oh_h) == 0 and ops.order_hint_status(oh_f) == 0
    if fam == "30/15":
        # cross-use: the half extraction's hint feeds the fp32 head on the upcast maps, and the reverse
        zh, srh, oh_h = P.extract(ha, boxes, hint=True)
        zf, srf, oh_f = P.extract(fa, boxes, hint=True)
        plain = P.track(fb, boxes, srf, zf)
        x1 = P.track(fb, boxes, srh, zh, order_hint=oh_h)
        x2 = P.track(hb, boxes, srf, zf, order_hint=oh_f)
        torch.cuda.synchronize()
        assert ops.order_hint_status(oh_h) == 0 and ops.order_hint_status(oh_f) == 0
        for x, what in ((x1, "half hint -> fp32 head"), (x2, "fp32 hint -> half head")):
            for a, b, k in zip(x, plain, ("bb", "conf", "idx")):
                _bits_equal(a, b, "%s: %s" % (what, k))


# 5. every load form of the separable kernel: window widths, odd / even xmin, odd map widths, zero border, C, N
def _placed_boxes(image_wh, widths_px, x_starts, seed):
    """Boxes of the given widths (pixels) whose left edges sit at the given pixel offsets (-> odd and even first cells)."""
    rs = np.random.RandomState(seed)
    out = []
    for w in widths_px:
        for x0 in x_starts:
            h = min(max(w // 2, 12), image_wh[1] // 2)
            y0 = rs.uniform(0, image_wh[1] - h)
            out.append([x0, y0, x0 + w, y0 + h])
    return torch.tensor(np.array(out, dtype=np.float32)).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("geometry", ["704x1280", "odd widths"])
def test_every_load_form_of_the_separable_kernel(ops, geometry, dtype):
    if geometry == "704x1280":
        wh, widths = (1280, 704), None
    else:
        wh, widths = (1284, 704), (321, 161, 81, 41)          # rows start at 2-byte, not 4-byte, alignment
    # search windows of <= 32 columns, 33..64 and > 64 (a roi across the whole level 0); left edges 4 px apart walk through
    # odd and even first cells on every level; plus rois entirely inside the virtual zero border
    narrow = _placed_boxes(wh, (20, 40, 60), (101.0, 105.0, 110.0, 116.0), 1)
    mid = _placed_boxes(wh, (90, 120, 200), (33.0, 37.0, 42.0, 48.0), 2)
    seen = set()
    for C in (32, 128, 256):
        (ha, fa), (hb, fb) = _maps(C, wh, 20 + C, dtype, widths=widths), _maps(C, wh, 21 + C, dtype, widths=widths)
        # (a 300x120 box well inside the image: its 600-pixel search region is 75 cells of level 1, none clipped away)
        wide = torch.tensor([[400.0, 300.0, 700.0, 420.0]], device=DEV)
        base = torch.cat([narrow, mid, wide, _boxes(5, wh, 3)], dim=0)
        for N in ((1, 30, 100, 280) if C == 128 else (30,)):
            boxes = base[:N] if N <= base.shape[0] else torch.cat([base, _boxes(N - base.shape[0], wh, 4)], dim=0)
            P = Pair(ops, "30/15", C, wh, _params(C, boxes, 5))
            got, oh = P.run(ha, hb, boxes, hint=(N <= 256))
            ref, of = P.run(fa, fb, boxes, hint=(N <= 256))
            _same_pair(got, ref, "%s C=%d N=%d" % (geometry, C, N))
            _hint_equal(oh, of, "hint C=%d N=%d" % (C, N))
            if C == 128 and N == 30:
                # the window classes and the parity of xmin really occur (from the hint's own bounds: words 10, 11 = xmin, xmax)
                ent = oh.view(torch.int32)[:, 8:12].cpu().numpy()
                for ymin, ymax, xmin, xmax in ent:
                    if xmax >= xmin:
                        ww = xmax - xmin + 1
                        seen.add(("<=32" if ww <= 32 else ("33..64" if ww <= 64 else ">64"), int(xmin) & 1))
        # stand-alone poolers on rois in the zero border, on a degenerate strip wider than 64 cells, and on everything above
        pad = 512
        pc = [int(pad / ((2 ** i) * 4)) for i in range(4)]
        border = torch.tensor([[5.0, 5.0, 100.0, 90.0], [wh[0] + 2 * pad - 120.0, 10.0, wh[0] + 2 * pad - 8.0, 100.0],
                               [300.0, 2.0, 460.0, 60.0]], device=DEV)
        strip = torch.tensor([[pad + 2.0, pad + 40.0, pad + wh[0] - 3.0, pad + 70.0], [pad + 7.0, pad + 300.0, pad + 700.0, pad + 330.0]],
                             device=DEV)
        rois = torch.cat([border, strip, ops.search_region(base, pad, 1.0, 0)], dim=0)
        lvl_boxes = torch.cat([border, torch.tensor([[0.0, 0.0, 30.0, 30.0], [0.0, 0.0, 40.0, 40.0]], device=DEV), base], dim=0)
        for size in (7, 15, 30):
            got = ops.roi_align_levels(ha, rois, lvl_boxes, size, SCALES, 2, pc)
            ref = ops.roi_align_levels(fa, rois, lvl_boxes, size, SCALES, 2, pc)
            _bits_equal(got, ref, "%s C=%d pooler %d" % (geometry, C, size))
            assert float(got[:2].abs().max()) == 0.0                                   # entirely in the zero border
        z = ops.roi_align_levels(fa, lvl_boxes, lvl_boxes, 15, SCALES, 2)
        _bits_equal(ops.sr_xcorr_fused(ha, lvl_boxes, rois, z, 30, 15, SCALES, 2, pad),
                    ops.sr_xcorr_fused(fa, lvl_boxes, rois, z, 30, 15, SCALES, 2, pad), "fused on border / strip rois C=%d" % C)
        # the 35 / 7 gathers on the same geometry (8-byte pieces at 2-byte alignment, pieces that reach a plane's end)
        last = torch.tensor([[wh[0] - 60.0 + 256, wh[1] - 50.0 + 256, wh[0] + 256 + 30.0, wh[1] + 256 + 20.0]], device=DEV)
        rois7 = torch.cat([ops.search_region(base, 256, 4.0, 64), last], dim=0)
        lb7 = torch.cat([base, torch.tensor([[0.0, 0.0, 20.0, 20.0]], device=DEV)], dim=0)
        z7 = ops.roi_align_levels(fa, lb7, lb7, 7, SCALES, 2)
        _bits_equal(ops.sr_xcorr_fused(ha, lb7, rois7, z7, 35, 7, SCALES, 2, 256),
                    ops.sr_xcorr_fused(fa, lb7, rois7, z7, 35, 7, SCALES, 2, 256), "gather kernel C=%d" % C)
    for cls in ("<=32", "33..64", ">64"):
        assert any(s[0] == cls for s in seen), (cls, seen)
    assert {s[1] for s in seen} == {0, 1}, seen
    assert ("33..64", 1) in seen and ("33..64", 0) in seen, seen        # the two-columns-per-lane form at both alignments


# 6. special values
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
def test_special_values_come_through_exactly(ops, dtype):
    C, wh = 32, (512, 384)
    (ha, _), (hb, _) = _maps(C, wh, 31, dtype, scale=1e-3), _maps(C, wh, 32, dtype)
    if dtype is torch.float16:
        bits = [0x0001, 0x03FF, 0x8001, 0x83FF, 0x7BFF, 0xFBFF, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x0400]
        # 2^-24, 2^-14 - 2^-24 (subnormals, both signs), largest finite, -0.0, +inf, -inf, NaN, smallest normal
    else:
        bits = [0x0001, 0x007F, 0x8001, 0x7F7F, 0xFF7F, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0080]
    special = torch.tensor(np.array(bits, dtype=np.uint16).view(np.int16)).to(DEV).view(dtype)
    # subnormals: a whole region of level 0 / 1 (so that pooled values are sums of subnormals only) and scattered cells
    sub = special[:4 if dtype is torch.float16 else 3]
    g = torch.Generator().manual_seed(33)
    for m in (ha, hb):
        for l in (0, 1):
            H, W = m[l].shape[2:]
            pick = torch.randint(0, sub.numel(), (C, H // 2, W // 2), generator=g).to(DEV)
            m[l][0, :, :H // 2, :W // 2] = sub[pick]
            idx = torch.randint(0, H * W, (C, 40), generator=g).to(DEV)
            val = special[torch.randint(0, special.numel(), (C, 40), generator=g).to(DEV)]
            m[l][0].view(C, -1).scatter_(1, idx, val)
    fa, fb = tuple(f.float() for f in ha), tuple(f.float() for f in hb)
    assert bool((sub.float() != 0).all())            # the upcast keeps the subnormals (else the reference itself is flushed)
    boxes = torch.cat([_boxes(20, wh, 34, sizes=[(40, 60), (80, 50), (24, 24)]),
                       torch.tensor([[4.0, 4.0, 120.0, 90.0], [10.0, 20.0, 60.0, 80.0]], device=DEV)], dim=0)
    P = Pair(ops, "30/15", C, wh, _params(C, boxes, 35))
    got, oh = P.run(ha, hb, boxes, hint=True)
    ref, of = P.run(fa, fb, boxes, hint=True)
    _same_pair(got, ref, "special values")
    _hint_equal(oh, of, "hint")
    for size in (7, 15, 30, 35):
        a = ops.roi_align_levels(ha, boxes, boxes, size, SCALES, 2)
        b = ops.roi_align_levels(fa, boxes, boxes, size, SCALES, 2)
        _bits_equal(a, b, "pooler %d on special values" % size)
    # the subnormal region really produced non-zero pooled values below the normal range, and NaN / inf really reached outputs
    t = ops.roi_align_levels(ha, boxes[-2:], boxes[-2:], 15, SCALES, 2)
    finite = t[torch.isfinite(t)]
    if dtype is torch.float16:            # (bf16 subnormals are fp32 subnormals: what the fp32 arithmetic does with them is not this test's)
        assert bool(((finite != 0) & (finite.abs() < 2.0 ** -14)).any())
    assert bool(torch.isnan(got["z"]).any()) and bool(torch.isinf(got["z"]).any())
    P7 = Pair(ops, "35/7", C, wh, P.params)
    _same_pair(P7.run(ha, hb, boxes)[0], P7.run(fa, fb, boxes)[0], "special values, 35/7")


# 7. batched calls
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("fam", ["30/15", "35/7"])
def test_batched_calls_equal_one_image_calls_and_the_upcast_batch(ops, fam, dtype):
    lib = ops.load_library()
    for B, C, wh, rows in ((1, 64, (512, 384), [12]), (4, 128, (1280, 704), [9, 0, 5, 16]),
                           (64, 32, (256, 192), [(b % 3) for b in range(64)])):
        (ha, fa), (hb, fb) = _maps(C, wh, 40 + B, dtype, B=B), _maps(C, wh, 41 + B, dtype, B=B)
        boxes = _boxes(sum(rows), wh, 42)
        P = Pair(ops, fam, C, wh, _params(C, boxes, 43))
        got, oh = P.run(ha, hb, boxes, rows, hint=True)
        ref, of = P.run(fa, fb, boxes, rows, hint=True)
        _same_pair(got, ref, "%s B=%d vs the upcast batch" % (fam, B))
        _hint_equal(oh, of, "hint B=%d" % B)
        ho, n0 = P.rx - P.rz + 1, 0
        for b, r in enumerate(rows):
            if r > 0:
                one, _ = P.run(_img(ha, b), _img(hb, b), boxes[n0:n0 + r])
                if lib.smot_emm_tower_form(r, C, ho) == lib.smot_emm_tower_form(sum(rows), C, ho):
                    _same_pair(got, one, "%s B=%d image %d" % (fam, B, b), rows=(n0, n0 + r))
                else:           # (another tower form for that row count: the pooling's outputs are still the same bits)
                    _bits_equal(got["z"][n0:n0 + r], one["z"], "templates, image %d" % b)
                    _bits_equal(got["sr"][n0:n0 + r], one["sr"], "search regions, image %d" % b)
            n0 += r


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
def test_half_images_past_4_gib(ops, dtype):
    """C = 256 maps of a 2112x1920 input: level 0 of one half image is 130 MB, so image 34 starts past 2^32 bytes."""
    C, wh, B = 256, (1920, 2112), 35
    W, H = wh
    last = B - 1
    fa, fb = [], []
    g = torch.Generator().manual_seed(51)
    for s in (4, 8, 16, 32):
        for lst in (fa, fb):
            f = torch.zeros((B, C, H // s, W // s), dtype=dtype, device=DEV)
            f[last].copy_(torch.randn((C, H // s, W // s), generator=g).to(dtype))
            f[0].copy_(torch.randn((C, H // s, W // s), generator=g).to(dtype))
            lst.append(f)
    assert fa[0][last].data_ptr() - fa[0].data_ptr() >= 2 ** 32
    rows = [2] + [0] * (B - 2) + [6]
    boxes = _boxes(8, wh, 52)
    P = Pair(ops, "30/15", C, wh, _params(C, boxes, 53))
    got, _ = P.run(fa, fb, boxes, rows, hint=True)
    ref, _ = P.run(_img(fa, last), _img(fb, last), boxes[2:], None, hint=True)
    _same_pair(got, ref, "image %d" % last, rows=(2, 8))
    ref0, _ = P.run(_img(fa, 0), _img(fb, 0), boxes[:2], None, hint=True)
    _same_pair(got, ref0, "image 0", rows=(0, 2))
    del fa, fb, f
    torch.cuda.empty_cache()


# 8. / 10. the EMM module
def _emm(C, init, seed):
    from siammot_amd.config import get_default_cfg
    from siammot_amd.emm import EMM
    from siammot_amd.track_utils import build_track_utils
    cfg = get_default_cfg(channels=C)
    emm = EMM(cfg, build_track_utils(cfg)).to(DEV).eval()
    emm.predictor.load_state_dict(_params(C, init, seed))
    return emm


def _det(init, n0, n, wh):
    from siammot_amd.structures import BoxList
    d = BoxList(init[n0:n0 + n].clone(), wh, mode="xyxy")
    d.add_field("ids", torch.arange(n0, n0 + n, device=DEV))
    d.add_field("labels", torch.ones(n, dtype=torch.int64, device=DEV))
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
def test_module_loops_on_half_maps_equal_the_loops_on_upcast_maps(ops, dtype):
    C, wh, B, T = 64, (512, 384), 4, 20
    counts = [4, 1, 3, 6]
    init = _boxes(sum(counts), wh, 61)
    emm = _emm(C, init, 62)
    frames = [_maps(C, wh, 100 + t, dtype, B=B) for t in range(T + 1)]
    with torch.no_grad():
        # one stream (image 2), hints in use
        hints = 0
        dh, df = _det(init, 5, 3, wh), _det(init, 5, 3, wh)
        for t in range(T):
            zh, srh, d1 = emm.extract_cache(_img(frames[t][0], 2), dh)
            zf, srf, d2 = emm.extract_cache(_img(frames[t][1], 2), df)
            _bits_equal(zh, zf, "templates, frame %d" % t)
            _bits_equal(srh[0].bbox, srf[0].bbox, "search regions, frame %d" % t)
            oh = srh[0].__dict__.get("order_hint")
            hints += oh is not None
            if oh is not None:
                _hint_equal(oh.data, srf[0].order_hint.data, "hint, frame %d" % t)
            _, rh, _ = emm(_img(frames[t + 1][0], 2), d1, srh, template_features=zh)
            _, rf, _ = emm(_img(frames[t + 1][1], 2), d2, srf, template_features=zf)
            _bits_equal(rh[0].bbox, rf[0].bbox, "boxes, frame %d" % t)
            _bits_equal(rh[0].get_field("scores"), rf[0].get_field("scores"), "scores, frame %d" % t)
            dh, df = rh[0], rf[0]
        assert hints == T
        # a list of four streams
        dh = [_det(init, sum(counts[:b]), counts[b], wh) for b in range(B)]
        df = [_det(init, sum(counts[:b]), counts[b], wh) for b in range(B)]
        for t in range(T):
            zh, srh, d1 = emm.extract_cache(frames[t][0], dh)
            zf, srf, d2 = emm.extract_cache(frames[t][1], df)
            _bits_equal(zh, zf, "batched templates, frame %d" % t)
            _, rh, _ = emm(frames[t + 1][0], d1, srh, template_features=zh)
            _, rf, _ = emm(frames[t + 1][1], d2, srf, template_features=zf)
            for b in range(B):
                _bits_equal(srh[b].bbox, srf[b].bbox, "search regions, frame %d stream %d" % (t, b))
                _bits_equal(rh[b].bbox, rf[b].bbox, "boxes, frame %d stream %d" % (t, b))
                _bits_equal(rh[b].get_field("scores"), rf[b].get_field("scores"), "scores, frame %d stream %d" % (t, b))
            dh, df = rh, rf


@pytest.mark.gpu
def test_alternating_dtypes_through_one_module(ops):
    """fp32, fp16 and bf16 maps frame by frame through ONE EMM instance (its cached plans / geometries), and a change of
    map size on the way: every call equals a fresh module's call on the upcast maps."""
    C, wh = 64, (512, 384)
    init = _boxes(5, wh, 71)
    emm, fresh = _emm(C, init, 72), _emm(C, init, 72)
    order = [torch.float32, torch.float16, torch.bfloat16, torch.float16, torch.float32, torch.bfloat16, torch.bfloat16,
             torch.float16, torch.float32, torch.float32, torch.float16]
    with torch.no_grad():
        for t, dt in enumerate(order):
            size = wh if t not in (5, 6) else (640, 384)
            ma, _ = _maps(C, size, 200 + t, dt if dt is not torch.float32 else torch.float16)
            mb, _ = _maps(C, size, 300 + t, dt if dt is not torch.float32 else torch.float16)
            if dt is torch.float32:
                ma, mb = tuple(f.float() for f in ma), tuple(f.float() for f in mb)
            det = _det(init, 0, 5, size)
            z, sr, d = emm.extract_cache(ma, det)
            _, res, _ = emm(mb, d, sr, template_features=z)
            det2 = _det(init, 0, 5, size)
            z2, sr2, d2 = fresh.extract_cache(tuple(f.float() for f in ma), det2)
            _, res2, _ = fresh(tuple(f.float() for f in mb), d2, sr2, template_features=z2)
            fresh.__dict__.pop("_plan", None)                 # (the reference module plans every call anew)
            _bits_equal(z, z2, "templates, call %d (%s)" % (t, dt))
            _bits_equal(sr[0].bbox, sr2[0].bbox, "search regions, call %d (%s)" % (t, dt))
            _bits_equal(res[0].bbox, res2[0].bbox, "boxes, call %d (%s)" % (t, dt))
            _bits_equal(res[0].get_field("scores"), res2[0].get_field("scores"), "scores, call %d (%s)" % (t, dt))
    plans = emm.__dict__["_plan"]
    assert set(plans) == {torch.float32, torch.float16, torch.bfloat16}
    assert all(p.g.dtype is dt and p.ft == ops.FEAT_TYPES[dt] for dt, p in plans.items())


# 9. the tracking loop
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("refine", [False, True])
def test_tracking_loop_on_half_maps_equals_the_loop_on_upcast_maps(ops, refine, dtype):
    from fake_tracker import detections
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
    shapes = gi.feature_shapes((1280, 704), 32)
    rs_f = np.random.RandomState(9)
    feats = [tuple(torch.from_numpy(rs_f.standard_normal(s).astype(np.float32)).to(dtype).to(dev) for s in shapes)
             for _ in range(6)]
    rs = [np.random.RandomState(5), np.random.RandomState(5)]
    dormant_seen, ids_seen = 0, set()
    frames = 30
    with torch.no_grad():
        for f in range(frames):
            h = feats[f % 6]
            a = loops[0](h, detections(rs[0], f % 40).to(dev))
            b = loops[1](tuple(x.float() for x in h), detections(rs[1], f % 40).to(dev))
            _bits_equal(a.bbox, b.bbox, "boxes, frame %d" % f)
            _bits_equal(a.get_field("scores"), b.get_field("scores"), "scores, frame %d" % f)
            assert torch.equal(a.get_field("ids"), b.get_field("ids")), "ids, frame %d" % f
            pa, pb = loops[0].solver.track_pool, loops[1].solver.track_pool
            assert pa.get_active_ids() == pb.get_active_ids() and pa._dormant_ids == pb._dormant_ids and pa._max_id == pb._max_id
            dormant_seen += len(pa._dormant_ids) > 0
            ids_seen |= set(pa.get_active_ids())
            ma, mb = loops[0].track_memory, loops[1].track_memory
            assert len(ma[2][0]) == len(mb[2][0])
            if len(mb[2][0]):
                _bits_equal(ma[0], mb[0], "memory templates, frame %d" % f)
                _bits_equal(ma[1][0].bbox, mb[1][0].bbox, "memory search regions, frame %d" % f)
                _bits_equal(ma[2][0].bbox, mb[2][0].bbox, "memory boxes, frame %d" % f)
                assert torch.equal(ma[2][0].get_field("ids"), mb[2][0].get_field("ids")), "memory order, frame %d" % f
    assert dormant_seen >= 3 and len(ids_seen) >= 5, (dormant_seen, ids_seen)        # tracks started, were suspended, resumed


# 11. what is refused
@pytest.mark.gpu
def test_mixed_and_unsupported_dtypes_raise(ops):
    C, wh = 32, (256, 192)
    h16, f32 = _maps(C, wh, 81, torch.float16)
    b16, _ = _maps(C, wh, 81, torch.bfloat16)
    boxes = _boxes(4, wh, 82)
    P = Pair(ops, "30/15", C, wh, _params(C, boxes, 83))
    z, sr = P.extract(f32, boxes)
    mixed = (h16[0], b16[1], h16[2], h16[3])
    mixed32 = (f32[0], f32[1], f32[2], h16[3])
    for m, names in ((mixed, ("float16", "bfloat16")), (mixed32, ("float32", "float16"))):
        for call in (lambda: P.extract(m, boxes), lambda: P.track(m, boxes, sr, z),
                     lambda: ops.roi_align_levels(m, boxes, boxes, 15, SCALES, 2),
                     lambda: ops.sr_xcorr_fused(m, boxes, sr, z, 30, 15, SCALES, 2, 512),
                     lambda: P.extract(tuple(x.expand(2, -1, -1, -1).contiguous() for x in m), boxes, [2, 2])):
            with pytest.raises(RuntimeError) as e:
                call()
            assert names[0] in str(e.value) and names[1] in str(e.value), str(e.value)
    for bad in (tuple(f.double() for f in f32), tuple(f.to(torch.int32) for f in f32)):
        for call in (lambda: P.extract(bad, boxes), lambda: P.track(bad, boxes, sr, z),
                     lambda: ops.roi_align_levels(bad, boxes, boxes, 15, SCALES, 2)):
            with pytest.raises(RuntimeError, match="must be float32"):
                call()
    # only the maps have a type: half boxes / templates are refused as before
    with pytest.raises(RuntimeError, match="must be float32"):
        P.track(h16, boxes, sr, z.half())
    with pytest.raises(RuntimeError, match="must be float32"):
        P.extract(h16, boxes.half())


# 12. no hidden cast
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
def test_no_fp32_copy_of_a_map_is_made(ops, dtype):
    C, wh = 128, (1280, 704)
    init = _boxes(4, wh, 91)
    emm = _emm(C, init, 92)
    (ha, _), (hb, _) = _maps(C, wh, 93, dtype), _maps(C, wh, 94, dtype)
    level0_fp32 = ha[0].numel() * 4
    assert level0_fp32 == 128 * 176 * 320 * 4
    with torch.no_grad():
        for step in range(2):                  # the first pair warms the grow-only workspaces and the caches
            det = _det(init, 0, 4, wh)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.max_memory_allocated()
            z, sr, d = emm.extract_cache(ha, det)
            _, res, _ = emm(hb, d, sr, template_features=z)
            torch.cuda.synchronize()
            grown = torch.cuda.max_memory_allocated() - before
    print("peak memory growth of a frame pair on %s maps: %d bytes (level 0 as fp32: %d)" % (dtype, grown, level0_fp32))
    assert grown < level0_fp32 // 2, (grown, level0_fp32)


# 13. one anchor outside the fp32 HIP path
@pytest.mark.gpu
def test_fp16_pooler_against_the_oracle():
    import siammot_amd.ops as ops
    from oracle import emm_oracle as O
    C, wh = 32, (128, 96)
    h, f = _maps(C, wh, 95, torch.float16)
    boxes = _boxes(12, wh, 96, sizes=[(20, 30), (40, 24), (60, 50), (12, 12)])
    pad = 64
    sr = ops.search_region(boxes, pad, 1.0, 0)
    pc = [int(pad / ((2 ** i) * 4)) for i in range(4)]
    cpu = [x.cpu() for x in f]
    for size, rois, cells in ((15, boxes, [0] * 4), (30, sr, pc)):
        got = ops.roi_align_levels(h, rois, boxes, size, SCALES, 2, cells).cpu().double()
        padded = [torch.nn.functional.pad(x, (c, c, c, c)) for x, c in zip(cpu, cells)]
        ref = O.sr_pool(padded, boxes.cpu(), rois.cpu(), size, SCALES, 2).double()
        err = (got - ref).abs()
        print("fp16 maps, %dx%d pooler vs the oracle: max |d| = %.3g" % (size, size, err.max().item()))
        assert bool((err <= 1e-5 + 1e-5 * ref.abs()).all()), (size, err.max().item())       # test_hip_parity's bound
