"""Deterministic inputs and reference answers for tests/test_box_refine_edges.py: the box head's post-processing of the
propagated tracks (csrc/box_refine.hip, ``box_refine_post_kernel``) at the edges every other test leaves out:

  * ranks     row order, ids, labels and the score pairing at wave and workgroup boundaries (N = 1 .. 512, K = 2 .. 40,
              five label patterns, 41-bit ids, matching scores with an exact 0.0 and 1.0);
  * agnostic  class-agnostic regression (``reg_classes = 2``: the LAST four delta columns) with poison in the first four
              and in the padding columns of a wider row;
  * xform     ``dw`` / ``dh`` one fp32 ulp below, at and above log(1000/16), +-1e4, +-inf;
  * clip      boxes decoded past every border, wholly outside, exactly on W - 1 / H - 1, a 1x1 image, amodal (no
              clipping) with the same inputs and with proposals around +-1e6;
  * softmax   equal logits, a label 180 below / above the maximum (scores exactly 1.0 / 2.0), a common offset of 1e4,
              logits at +-88;
  * degenerate proposals of width 1, 0, negative and sub-pixel; three sets of regression weights; TRACKTOR scores.

The reference answer of a case is computed once and cached: ``reference(name)["f32"]`` is the restated
``PostProcessor`` + ``RefineTracks`` (siammot_amd.box_refine, on CPU: the reference's arithmetic, pinned to the
reference's own code by tests/golden/refine_post_edges.npz), ``["f64"]`` the same operation written out directly
(``direct``) in double precision; ``direct`` in fp32 must equal the restatement bit for bit (asserted by the CPU tests),
which is what entitles its fp64 form to be called the same operation.  ``direct`` also takes the three ways a kernel
can be subtly wrong that the CPU tests need (other delta columns, output-order score pairing, another grouping) and
keeps rows with non-finite values, which the reference drops.  Nothing here touches a device."""
import functools
import math

import numpy as np
import torch

F32 = np.float32
IMAGE_WH = (1280, 704)
XFORM_CLIP = math.log(1000.0 / 16)                   # what the product hands the kernel (rounded to fp32 on the way)
XFORM_CLIP32 = F32(XFORM_CLIP)                       # ... and what torch.clamp(fp32 tensor, max=XFORM_CLIP) compares with
ID_BASE = 2 ** 40
MARGIN = 2.0 ** -22                                  # two fp32 ulp: device expf against libm (decode_edge_cases.ULPS)
GOLDEN_CASES = ("ranks_n65_k3_random", "agn_k5_n300", "amodal_n512_k16", "clip_1280", "xform_w5_clip", "softmax_tracktor")


# ---- input recipes ------------------------------------------------------------------------------------------------
def _boxes(rs, n):
    xy = rs.uniform(0.0, 1.0, (n, 2)) * (1000.0, 500.0)
    wh = rs.uniform(20.0, 220.0, (n, 2))
    return np.concatenate((xy, xy + wh), 1).astype(F32)


def _labels(rs, n, K, pattern):
    if pattern == "one":
        lab = np.full(n, K - 1)
    elif pattern == "desc":                          # strictly descending: the rank reverses the input
        assert n <= K - 1
        lab = np.arange(K - 1, K - 1 - n, -1)
    elif pattern == "blockdesc":                     # non-increasing, most rows on the last label
        lab = np.sort(np.where(rs.uniform(size=n) < 0.6, K - 1, rs.randint(1, K, n)))[::-1]
    elif pattern == "alt":
        lab = np.where(np.arange(n) % 2 == 0, K - 1, 1)
    elif pattern == "two":
        lab = np.where(rs.uniform(size=n) < 0.5, 11, 3)
    elif pattern == "low1":                          # label 1 on a quarter of the rows, the others above it
        lab = np.where(rs.uniform(size=n) < 0.25, 1, rs.randint(2, max(K, 3), n)) if K > 2 else np.ones(n)
    else:
        lab = rs.randint(1, K, n)
    return np.ascontiguousarray(lab, np.int64)


def _conf(rs, n):
    conf = rs.uniform(0.0, 1.0, n).astype(F32)
    if n >= 2:
        a, b = rs.choice(n, 2, replace=False)
        conf[a], conf[b] = 0.0, 1.0
    return conf


def _poison(n, cols):
    """Distinct values around 1e3: as deltas they move a box by a hundred widths and stretch it to the clip."""
    return (900.0 + 3.5 * np.arange(cols)[None, :] + 0.125 * (np.arange(n)[:, None] % 64)).astype(F32)


def _head(rs, n, K, agnostic, weights, pad=0, spread=1.0):
    KR = 2 if agnostic else K
    ld = K + 4 * KR + pad
    ho = np.empty((n, ld), F32)
    ho[:, :K] = rs.standard_normal((n, K)) * 2.0
    ho[:, K:] = _poison(n, ld - K)
    w = np.asarray(weights, np.float64)
    deltas = lambda m: (rs.standard_normal((n, m, 4)) * (0.5, 0.5, 0.3, 0.3) * w * spread).reshape(n, 4 * m)
    if agnostic:
        ho[:, K + 4:K + 8] = deltas(1)
    else:
        ho[:, K:K + 4 * K] = deltas(K)
    return ho


def _case(family, head_out, boxes, labels, ids, conf, K, agnostic=False, weights=(10.0, 10.0, 5.0, 5.0),
          clip_wh=IMAGE_WH, tracktor=False, rows=None):
    n = len(boxes)
    assert head_out.shape[0] == n and len(labels) == len(ids) == len(conf) == n and n <= 512
    return dict(family=family, head_out=np.ascontiguousarray(head_out, F32), boxes=np.ascontiguousarray(boxes, F32),
                labels=np.ascontiguousarray(labels, np.int64), ids=np.ascontiguousarray(ids, np.int64),
                track_conf=np.ascontiguousarray(conf, F32), weights=tuple(float(w) for w in weights), clip_wh=clip_wh,
                num_classes=K, reg_classes=2 if agnostic else K, agnostic=agnostic, tracktor=tracktor, rows=rows or {})


def _generic(family, seed, n, K, pattern="random", agnostic=False, pad=0, **kw):
    rs = np.random.RandomState(seed)
    weights = kw.get("weights", (10.0, 10.0, 5.0, 5.0))
    ho = _head(rs, n, K, agnostic, weights, pad)
    return _case(family, ho, _boxes(rs, n), _labels(rs, n, K, pattern), ID_BASE + rs.permutation(n), _conf(rs, n), K,
                 agnostic, **kw)


def delta_columns(c, i):
    """Where row i's four deltas live in its row of ``head_out``."""
    K = c["num_classes"]
    return K + (4 if c["agnostic"] else 4 * int(c["labels"][i]))


def _set_deltas(c, i, d):
    k = delta_columns(c, i)
    c["head_out"][i, k:k + 4] = np.asarray(d, F32)


def quotient_preimage(target, w):
    """An fp32 delta whose fp32 quotient by the weight ``w`` is exactly ``target``."""
    target, w = F32(target), F32(w)
    lo = hi = F32(target * w)
    for _ in range(64):
        for cand in (lo, hi):
            if F32(cand / w) == target:
                return cand
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
    raise AssertionError("no fp32 delta with quotient %r by %r" % (target, w))


XFORM_ROWS = ("below", "at", "above", "+1e4", "-1e4", "+inf", "-inf")


def xform_targets():
    return {"below": np.nextafter(XFORM_CLIP32, F32(0)), "at": XFORM_CLIP32, "above": np.nextafter(XFORM_CLIP32, F32(np.inf))}


def _xform(seed, weights, clip_wh):
    """Rows 0..6: dw as in XFORM_ROWS, rows 7..13: dh; rows 14, 15 ordinary.  Small boxes in the middle of the image:
    62.5 times their size stays inside it."""
    rs = np.random.RandomState(seed)
    n, K = 16, 3
    ctr = np.array([640.0, 352.0]) + rs.uniform(-40.0, 40.0, (n, 2))
    wh = rs.uniform(4.0, 10.0, (n, 2))
    boxes = np.concatenate((ctr - 0.5 * wh, ctr + 0.5 * wh), 1)
    c = _case("xform", _head(rs, n, K, False, weights, spread=0.2), boxes, _labels(rs, n, K, "random"),
              ID_BASE + rs.permutation(n), _conf(rs, n), K, weights=weights, clip_wh=clip_wh)
    t = xform_targets()
    for axis in (0, 1):
        for r, kind in enumerate(XFORM_ROWS):
            i, w = 7 * axis + r, weights[2 + axis]
            if kind in t:
                v = quotient_preimage(t[kind], w)
            else:
                v = F32({"+1e4": 1e4, "-1e4": -1e4, "+inf": np.inf, "-inf": -np.inf}[kind]) * F32(w)
            c["head_out"][i, delta_columns(c, i) + 2 + axis] = v
            c["rows"]["d%s %s" % ("wh"[axis], kind)] = i
    return c


def _clip(clip_wh):
    """Rows 0..3 straddle the left, right, top, bottom border; 4..7 lie wholly beyond it; 8, 9 have corners exactly on
    W - 1 / H - 1 (and 0); 10..23 are thrown about by deltas of three box sizes."""
    rs = np.random.RandomState(601)
    n, K = 24, 3
    W, H = IMAGE_WH
    weights = (10.0, 10.0, 5.0, 5.0)
    boxes = _boxes(rs, n)
    boxes[:8] = (600.0, 300.0, 699.0, 379.0)                      # w = 100, h = 80, centre (650, 340)
    boxes[8] = (100.0, 50.0, W - 1.0, H - 1.0)
    boxes[9] = (0.0, 0.0, W - 1.0, H - 1.0)
    c = _case("clip", _head(rs, n, K, False, weights, spread=6.0), boxes, _labels(rs, n, K, "random"),
              ID_BASE + rs.permutation(n), _conf(rs, n), K, weights=weights, clip_wh=clip_wh)
    targets = ((20.0, None), (1270.0, None), (None, 10.0), (None, 695.0), (-300.0, None), (1700.0, None), (None, -300.0),
               (None, 1100.0))
    for i, (tx, ty) in enumerate(targets):
        dx = 0.0 if tx is None else (tx - 650.0) / 100.0 * weights[0]
        dy = 0.0 if ty is None else (ty - 340.0) / 80.0 * weights[1]
        _set_deltas(c, i, (dx, dy, 0.1, -0.1))
    _set_deltas(c, 8, (0.0, 0.0, 0.0, 0.0))
    _set_deltas(c, 9, (0.0, 0.0, 0.0, 0.0))
    c["rows"] = dict(straddle=(0, 1, 2, 3), outside=(4, 5, 6, 7), exact=(8, 9))
    return c


def _softmax(tracktor):
    rs = np.random.RandomState(701)
    n, K = 12, 5
    c = _case("softmax", _head(rs, n, K, False, (10.0, 10.0, 5.0, 5.0)), _boxes(rs, n), _labels(rs, n, K, "random"),
              ID_BASE + rs.permutation(n), _conf(rs, n), K, tracktor=tracktor)
    rows = (("equal", 2, (3.0, 3.0, 3.0, 3.0, 3.0)),
            ("below180", 1, (0.0, -180.0, -1.0, -2.0, -3.0)),
            ("above180", 1, (0.0, 180.0, -1.0, -2.0, -3.0)),
            ("offset1e4", 3, tuple(1e4 + rs.standard_normal(K) * 2.0)),
            ("pm88", 3, (88.0, -88.0, 0.0, 87.5, -87.5)),
            ("pm88_under", 1, (88.0, -88.0, 0.0, 87.5, -87.5)),
            ("all_m88", 2, (-88.0, -88.5, -87.0, -89.0, -88.0)),
            ("all_p88", 4, (88.0, 88.5, 87.0, 89.0, 88.0)))
    for i, (name, lab, logits) in enumerate(rows):
        c["labels"][i] = lab                                 # (per-class head: every class's columns hold deltas)
        c["head_out"][i, :K] = np.asarray(logits, F32)
        c["rows"][name] = i
    return c


def _degenerate():
    rs = np.random.RandomState(801)
    n, K = 16, 3
    weights = (3.0, 7.0, 0.5, 2.0)
    boxes = _boxes(rs, n)
    boxes[:10] = ((300, 200, 300, 260), (300, 200, 299, 260), (300, 200, 295, 260),             # width 1, 0, -4
                  (500, 100, 560, 100), (500, 100, 560, 99), (500, 100, 560, 90),               # height 1, 0, -9
                  (700, 300, 700, 300), (700, 300, 699, 299),                                   # both 1, both 0
                  (300.25, 200.5, 300.5, 200.75), (900.125, 400.0, 900.25, 460.0))              # sub-pixel
    return _case("degenerate", _head(rs, n, K, False, weights), boxes, _labels(rs, n, K, "random"),
                 ID_BASE + rs.permutation(n), _conf(rs, n), K, weights=weights)


def _amodal_far():
    c = _generic("clip", 611, 40, 3, clip_wh=None)
    rs = np.random.RandomState(612)
    xy = rs.choice((-1e6, 1e6), (40, 2)) + rs.uniform(-500.0, 500.0, (40, 2))
    c["boxes"] = np.concatenate((xy, xy + rs.uniform(20.0, 220.0, (40, 2))), 1).astype(F32)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # 1. ranks: (N, K, label pattern); K = 17 / 40 also serve as "per-class regression with many classes"
    c["ranks_n1_k2_one"] = _generic("ranks", 101, 1, 2, "one")
    c["ranks_n63_k3_alt"] = _generic("ranks", 102, 63, 3, "alt", pad=3)
    c["ranks_n64_k16_two"] = _generic("ranks", 103, 64, 16, "two")
    c["ranks_n65_k3_random"] = _generic("ranks", 104, 65, 3)
    c["ranks_n39_k40_desc"] = _generic("ranks", 105, 39, 40, "desc")
    c["ranks_n128_k16_random"] = _generic("ranks", 106, 128, 16, weights=(3.0, 7.0, 0.5, 2.0))
    c["ranks_n129_k17_blockdesc"] = _generic("ranks", 107, 129, 17, "blockdesc")
    c["ranks_n511_k40_random"] = _generic("ranks", 108, 511, 40)
    c["ranks_n512_k2_one"] = _generic("ranks", 109, 512, 2, "one")
    # 2. class-agnostic regression: ld = K + 8 and a padded K + 11
    c["agn_k2_ld10"] = _generic("agnostic", 201, 20, 2, "one", agnostic=True)
    c["agn_k3_ld11"] = _generic("agnostic", 202, 30, 3, "low1", agnostic=True)
    c["agn_k3_ld14"] = _generic("agnostic", 203, 65, 3, "low1", agnostic=True, pad=3)
    c["agn_k5_n300"] = _generic("agnostic", 204, 300, 5, "low1", agnostic=True)
    c["agn_k16_ld27"] = _generic("agnostic", 205, 70, 16, "low1", agnostic=True, pad=3, clip_wh=None)
    # 3. the clamp of dw / dh
    c["xform_w1_amodal"] = _xform(301, (1.0, 1.0, 1.0, 1.0), None)
    c["xform_w5_clip"] = _xform(302, (10.0, 10.0, 5.0, 5.0), IMAGE_WH)
    # 4. clipping and its absence
    c["clip_1280"] = _clip(IMAGE_WH)
    c["clip_1x1"] = _clip((1, 1))
    c["clip_none"] = _clip(None)
    c["amodal_far"] = _amodal_far()
    c["amodal_n512_k16"] = _generic("ranks", 613, 512, 16, clip_wh=None)
    # 5. soft-max, 6. degenerate proposals, 7. TRACKTOR
    c["softmax_tracktor"] = _softmax(True)
    c["softmax_average"] = _softmax(False)
    c["degenerate"] = _degenerate()
    c["tracktor_n70_k5"] = _generic("tracktor", 901, 70, 5, tracktor=True)
    return c


CASE_NAMES = ("ranks_n1_k2_one", "ranks_n63_k3_alt", "ranks_n64_k16_two", "ranks_n65_k3_random", "ranks_n39_k40_desc",
              "ranks_n128_k16_random", "ranks_n129_k17_blockdesc", "ranks_n511_k40_random", "ranks_n512_k2_one",
              "agn_k2_ld10", "agn_k3_ld11", "agn_k3_ld14", "agn_k5_n300", "agn_k16_ld27",
              "xform_w1_amodal", "xform_w5_clip", "clip_1280", "clip_1x1", "clip_none", "amodal_far", "amodal_n512_k16",
              "softmax_tracktor", "softmax_average", "degenerate", "tracktor_n70_k5")


# ---- the reference ------------------------------------------------------------------------------------------------
def _no_nms(boxlist, thresh):
    raise AssertionError("every row is a track: the NMS has nothing to see")


def restated(c):
    """The reference's arithmetic: ``siammot_amd.box_refine.PostProcessor`` + ``RefineTracks`` on CPU in fp32, fed the
    logits / deltas split out of ``head_out`` by a stub box head.  Finite inputs only (a row with a NaN score is dropped
    there, as in the reference)."""
    from siammot_amd.box_refine import BoxCoder, PostProcessor, RefineTracks      # (the case builders above import nothing
    from siammot_amd.structures import BoxList                                    # of the package: the golden generator uses them)
    K, KR = c["num_classes"], c["reg_classes"]
    ho = torch.from_numpy(c["head_out"])
    logits, reg = ho[:, :K].contiguous(), ho[:, K:K + 4 * KR].contiguous()
    post = PostProcessor(0.05, 0.5, BoxCoder(c["weights"]), c["agnostic"], c["clip_wh"] is None, nms_fn=_no_nms)

    def box(features, tracks):
        return None, post((logits, reg), tracks), {}
    t = BoxList(torch.from_numpy(c["boxes"].copy()), c["clip_wh"] or IMAGE_WH, mode="xyxy")
    t.add_field("ids", torch.from_numpy(c["ids"].copy()))
    t.add_field("labels", torch.from_numpy(c["labels"].copy()))
    t.add_field("scores", torch.from_numpy(c["track_conf"].copy()))
    with torch.no_grad():
        r = RefineTracks(box, c["tracktor"])(None, [t])[0]
    return dict(boxes=r.bbox.numpy(), scores=r.get_field("scores").numpy(), ids=r.get_field("ids").numpy(),
                labels=r.get_field("labels").numpy())


def direct(c, dtype=torch.float64, columns="right", pairing="input", grouping="stable", clip=True):
    """The same operation written out: soft-max, the label's probability + 1, ``BoxCoder.decode`` of the row's four
    deltas followed by ``torch.clamp``, a stable grouping by label, the score average with the matching scores in INPUT
    order.  Rows with non-finite values stay.

    What a subtly wrong kernel would do instead: ``columns`` = "label" (the label's columns of a class-agnostic head, or
    those of ``min(label, 15)``: read from the flat buffer as the device would), "last4" (the padded row's last four),
    "first4"; ``pairing`` = "output"; ``grouping`` = "descending" / "reversed" (input order reversed inside a label)."""
    from siammot_amd.box_refine import BoxCoder
    K, n = c["num_classes"], len(c["boxes"])
    ho = torch.from_numpy(c["head_out"]).to(dtype)
    ld = ho.shape[1]
    lab = torch.from_numpy(c["labels"])
    rows = torch.arange(n)
    det = torch.softmax(ho[:, :K].contiguous(), -1)[rows, lab] + 1.0
    if columns == "right":
        col = torch.full((n,), K + 4, dtype=torch.int64) if c["agnostic"] else K + 4 * lab
    elif columns == "label":
        col = K + 4 * (lab if c["agnostic"] else lab.clamp(max=15))
    elif columns == "last4":
        col = torch.full((n,), ld - 4, dtype=torch.int64)
    else:
        col = torch.full((n,), K, dtype=torch.int64)
    flat = torch.cat((ho.reshape(-1), torch.zeros(4 * K + 8, dtype=dtype)))
    deltas = flat[(rows * ld + col)[:, None] + torch.arange(4)[None, :]]
    raw = BoxCoder(c["weights"], float(XFORM_CLIP32)).decode(deltas, torch.from_numpy(c["boxes"]).to(dtype))
    bb = raw.clone()
    if clip and c["clip_wh"] is not None:
        for k, hi in enumerate((c["clip_wh"][0] - 1, c["clip_wh"][1] - 1) * 2):
            bb[:, k] = torch.clamp(bb[:, k], min=0, max=hi)
    if grouping == "stable":
        order = torch.sort(lab, stable=True)[1]
    elif grouping == "descending":
        order = torch.sort(lab, stable=True, descending=True)[1]
    else:
        order = torch.sort(lab.flip(0), stable=True)[1]
        order = (n - 1 - order)
    det_out = det[order]
    conf = torch.from_numpy(c["track_conf"]).to(dtype)
    if pairing == "output":
        conf = conf[order]
    scores = det_out if c["tracktor"] else (det_out + (conf + 1.0)) / 2.0
    return dict(boxes=bb[order].numpy(), scores=scores.numpy(), ids=c["ids"][order.numpy()], labels=c["labels"][order.numpy()],
                raw=raw[order].numpy(), order=order.numpy())


def operand_scale(c):
    """``|pred_ctr| + 0.5 * pred_size + 1`` per output coordinate, in fp64 and in output order: what the last
    subtraction of the decode rounds at."""
    n = len(c["boxes"])
    ho = torch.from_numpy(c["head_out"]).double()
    b = torch.from_numpy(c["boxes"]).double()
    col = torch.tensor([delta_columns(c, i) for i in range(n)], dtype=torch.int64)
    d = ho[torch.arange(n)[:, None], col[:, None] + torch.arange(4)[None, :]]
    wx, wy, ww, wh = c["weights"]
    w, h = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
    pcx, pcy = d[:, 0] / wx * w + b[:, 0] + 0.5 * w, d[:, 1] / wy * h + b[:, 1] + 0.5 * h
    pw = torch.exp(torch.clamp(d[:, 2] / ww, max=float(XFORM_CLIP32))) * w
    ph = torch.exp(torch.clamp(d[:, 3] / wh, max=float(XFORM_CLIP32))) * h
    sx, sy = pcx.abs() + 0.5 * pw.abs() + 1, pcy.abs() + 0.5 * ph.abs() + 1
    order = torch.sort(torch.from_numpy(c["labels"]), stable=True)[1]
    return torch.stack((sx, sy, sx, sy), 1)[order].numpy()


def _rel_err(a, ref, scale):
    """Largest |a - ref| / scale over the elements finite in both (0 where there is none)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(a) & np.isfinite(ref) & np.isfinite(scale)
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        return float((np.abs(a - ref)[fin] / np.broadcast_to(scale, a.shape)[fin]).max())


def reference_eval(c, f32=None):
    f32 = direct(c, torch.float32) if f32 is None else f32
    f64 = direct(c, torch.float64)
    s = operand_scale(c)
    return dict(f32=f32, f64=f64, scale=s, e32_box=_rel_err(f32["boxes"], f64["boxes"], s),
                e32_score=_rel_err(f32["scores"], f64["scores"], 2.0))


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp32 = the restatement of the reference's code, fp64 = ``direct``; ``e32_*`` = the fp32 reference's own largest
    error against fp64, in units of the operand scale (boxes) and of 2 (scores)."""
    c = cases()[name]
    return reference_eval(c, restated(c))


def bounds(ref):
    """The GPU tests' bound, from the reference alone: ``(2 e32 + 2^-22) * s`` element-wise (s = 2 for scores).  The
    kernel promises the reference's op order, separately rounded, so its distance to the fp32 reference is what device
    expf differs from libm by (MARGIN) and what a sequential soft-max sum differs from torch's (of the size of e32)."""
    return (2.0 * ref["e32_box"] + MARGIN) * ref["scale"], (2.0 * ref["e32_score"] + MARGIN) * 2.0


def same_class_within(got, ref, bound):
    """Element-wise: finite reference values within ``bound``, non-finite ones of the same class (NaN, +inf, -inf)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        close = np.isfinite(got) & (np.abs(got - ref) <= bound)
    same = (np.isnan(got) & np.isnan(ref)) | (np.isposinf(got) & np.isposinf(ref)) | (np.isneginf(got) & np.isneginf(ref))
    return np.where(np.isfinite(ref), close, same)


# ---- non-finite rows ------------------------------------------------------------------------------------------------
def nonfinite_case(n, clip):
    """(dirty case, clean case, {kind: row}): K = 5, per-class regression; the dirty rows sit in the first wave and, at
    N = 130, in the last one (rows 128, 129)."""
    clean = _generic("nonfinite", 1000 + n, n, 5, clip_wh=IMAGE_WH if clip else None)
    dirty = dict(clean, head_out=clean["head_out"].copy())
    ho, K = dirty["head_out"], 5
    lab = dirty["labels"]
    kinds = ("logit_nan", "logit_pinf", "logits_all_ninf", "dx_nan", "dy_nan", "dw_nan", "dh_nan", "dx_pinf", "logit_ninf",
             "dw_pinf")
    at = dict(zip(kinds, range(10))) if n < 64 else dict(logit_nan=0, dx_nan=1, dw_nan=2, logit_pinf=3, dh_nan=40,
                                                         logit_ninf=63, dy_nan=128, logit_nan_dw_nan=129)
    for kind, i in at.items():
        other = (int(lab[i]) + 1) % K                       # a class that is not the row's label
        d0 = delta_columns(dirty, i)
        if "logit_nan" in kind:
            ho[i, other] = np.nan
        if kind == "logit_pinf":
            ho[i, other] = np.inf
        if kind == "logit_ninf":
            ho[i, other] = -np.inf
        if kind == "logits_all_ninf":
            ho[i, :K] = -np.inf
        for k, ax in enumerate(("dx", "dy", "dw", "dh")):
            if ax + "_nan" in kind:
                ho[i, d0 + k] = np.nan
            if kind == ax + "_pinf":
                ho[i, d0 + k] = np.inf
    return dirty, clean, at
