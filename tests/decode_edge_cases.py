"""Deterministic inputs for tests/test_decode_edges.py: logits built to take csrc/decode.hip (K4: bicubic x16 up-sampling
+ location grid + penalised arg-max) out of the regime every other decode test feeds it, where scores stay inside [0, 1]:

  * ReLU-sparse regression maps.  The head's ReLU leaves exact zeros in ``reg``; bicubic overshoot next to them makes a
    size ratio negative, ``-s_w * s_h`` positive and the penalty ``exp(0.1 * (1 - s_w * s_h))`` unbounded: scores of
    1e30, +inf, and NaN (0 * inf) where the class probability underflows;
  * near-flat maps at a large score (dozens of cells within 200 ulp of a maximum of 45 .. 3e29);
  * saturation: +-inf class logits, all-zero regression planes (1 / 0), a window-only score over inf penalties,
    template boxes of zero and negative width or height;
  * the kernel's geometry with ordinary logits: Ho from 1 to 46 (one, two and three output columns per lane, the
    largest map its LDS guard admits), rz in {1, 3, 15}, both ``use_centerness`` values, three window weights, clipping;

with the answer of the CPU oracle (oracle/emm_oracle.py, fp32 = the reference's arithmetic; the overflow test of a
cell's exponent in fp64) computed ONCE per case and shared by the CPU and the GPU tests, and the one adjudication rule
all of them use.  Nothing here touches a device."""
import functools
import math

import numpy as np
import torch

import golden_inputs as gi
from oracle import emm_oracle as O

F32 = np.float32
DEFAULT = dict(rx=30, rz=15, pad_pixels=512, use_centerness=True, sigma=0.4)       # Ho = 16
AOT = dict(rx=35, rz=7, pad_pixels=256, use_centerness=False, sigma=0.1)           # Ho = 29
IMAGE_WH = (1280, 704)
# standard-normal quantiles: reg = max(N(0,1) * 0.5 * side - q * 0.5 * side, 0) is zero with probability `share`
QUANTILE = {0.0: -np.inf, 0.25: -0.6744897501960817, 0.5: 0.0, 0.75: 0.6744897501960817}
LN_FLT_MAX = math.log(float(np.finfo(np.float32).max))      # 88.7228...: expf overflows above it
ULPS = 2.0                                                  # libm allowance between torch-CPU and device expf
EXCUSED_PER_TRACKS = 10                                     # at most 1 track in 10 of a case may be excused


# ---- input recipes ------------------------------------------------------------------------------------------------
def _boxes(rs, n, lo=20.0, hi=300.0):
    wh = rs.uniform(lo, hi, (n, 2))
    xy = rs.uniform(0.0, 900.0, (n, 2))
    return np.concatenate((xy, xy + wh), 1).astype(F32), wh


def _side(wh):
    return np.stack((wh[:, 0], wh[:, 1], wh[:, 0], wh[:, 1]), 1)[:, :, None, None]


def _inputs(boxes, cls, center, reg, cfg, expansion=1.0):
    return dict(cls=cls.astype(F32), center=center.astype(F32), reg=reg.astype(F32), boxes=boxes.astype(F32),
                sr=gi.np_search_region(boxes.astype(F32), cfg["pad_pixels"], expansion))


def in_regime(seed, n, ho, cfg, boxes=None):
    """The recipe of the existing decode tests at any Ho: cls, center ~ N(0, 2); reg ~ |N(0, 1)| * 0.5 * box side
    (strictly positive: scores stay inside [0, 1])."""
    rs = np.random.RandomState(seed)
    b, wh = _boxes(rs, n)
    if boxes is not None:
        b = np.asarray(boxes, F32)
        wh = np.stack((b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), 1).astype(np.float64)
    cls = rs.standard_normal((n, 2, ho, ho)) * 2.0
    center = rs.standard_normal((n, 1, ho, ho)) * 2.0
    reg = np.abs(rs.standard_normal((n, 4, ho, ho))) * 0.5 * _side(np.where(wh == 0, 50.0, np.abs(wh)))
    return _inputs(b, cls, center, reg, cfg)


def relu_sparse(seed, n, ho, share, cfg, cls_scale=2.0, expansion=1.0):
    """cls, center ~ N(0, cls_scale); reg = max(N(0, 1) * 0.5 * side - q, 0) with q the `share` quantile: what a ReLU
    on a regression head whose bias does not dominate produces."""
    rs = np.random.RandomState(seed)
    b, wh = _boxes(rs, n)
    cls = rs.standard_normal((n, 2, ho, ho)) * cls_scale
    center = rs.standard_normal((n, 1, ho, ho)) * 2.0
    reg = np.maximum((rs.standard_normal((n, 4, ho, ho)) - QUANTILE[share]) * 0.5 * _side(wh), 0.0)
    return _inputs(b, cls, center, reg, cfg, expansion)


def near_flat(seed, n, sh, cfg):
    """Constant regression planes l = r = -box_w / 4, t = b = sh * box_h: s_w = -0.5, s_h = 2 sh, exponent argument
    0.1 * (1 + sh); cls, center ~ N(0, 2e-4): a nearly flat map at exp(0.1 * (1 + sh)) / 4."""
    rs = np.random.RandomState(seed)
    b, wh = _boxes(rs, n, 20.0, 60.0)        # (small boxes: one ulp of t = 691 * box_h stays below the 2e-2 px bound)
    bw = (b[:, 2] - b[:, 0]).astype(np.float64)[:, None, None]
    bh = (b[:, 3] - b[:, 1]).astype(np.float64)[:, None, None]
    one = np.ones((n, 16, 16))
    reg = np.stack((-0.25 * bw * one, sh * bh * one, -0.25 * bw * one, sh * bh * one), 1)
    cls = rs.standard_normal((n, 2, 16, 16)) * 2e-4
    center = rs.standard_normal((n, 1, 16, 16)) * 2e-4
    return _inputs(b, cls, center, reg, cfg)


def _case(family, d, cfg, clip_wh=None, tie=False):
    return dict(family=family, d=d, cfg=dict(cfg), clip_wh=clip_wh, tie=tie)


def _geometry(ho, rz, use_centerness, sigma, n, seed, clip):
    cfg = dict(rx=ho + rz - 1, rz=rz, pad_pixels=512, use_centerness=use_centerness, sigma=sigma)
    boxes = None
    if clip:
        # template boxes on and beyond every side of the image: the decoded boxes leave it on each of them
        boxes = np.array([(-60, 200, 30, 330), (1240, 300, 1340, 420), (500, -50, 640, 40), (600, 660, 700, 760)], F32)[:n]
    return _case("geometry", in_regime(seed, n, ho, cfg, boxes), cfg, IMAGE_WH if clip else None)


def _saturation_cases():
    c = {}
    c["sat_cls_x40"] = _case("saturation", relu_sparse(301, 24, 16, 0.5, DEFAULT, cls_scale=80.0), DEFAULT)
    d = relu_sparse(302, 4, 16, 0.25, DEFAULT)
    d["cls"][0, 0, 3, :] = np.inf
    d["cls"][1, 1, 12, :] = -np.inf
    d["cls"][2, 0, 0, :] = -np.inf
    d["cls"][2, 1, 15, :] = np.inf
    d["cls"][3, 1, 7, :] = np.inf
    c["sat_cls_inf_rows"] = _case("saturation", d, DEFAULT)
    d = relu_sparse(304, 4, 16, 0.5, DEFAULT)            # tracks 2, 3: t, b ReLU-sparse (negative heights: +inf scores)
    wh = (d["boxes"][:2, 2:] - d["boxes"][:2, :2]).astype(np.float64)
    d["reg"][:2] = np.abs(np.random.RandomState(303).standard_normal((2, 4, 16, 16))) * 0.5 * _side(wh)   # 0, 1: t, b > 0
    d["reg"][:, 0] = 0.0                     # l and r all zero: size ratio +0, 1 / 0 = inf
    d["reg"][:, 2] = 0.0
    d["reg"][1, 1] = 0.0                     # track 1: t as well
    c["sat_reg_plane_zero"] = _case("saturation", d, DEFAULT)
    c["sat_window_only"] = _case("saturation", relu_sparse(305, 8, 16, 0.75, DEFAULT), dict(DEFAULT, sigma=1.0))
    b = np.array([(100, 100, 100, 180), (300, 200, 380, 200), (500, 300, 500, 300), (640, 100, 600, 190),
                  (200, 500, 290, 440), (800, 400, 750, 330)], F32)            # zero / negative width, height, both
    c["sat_degenerate_boxes"] = _case("saturation", in_regime(306, 6, 16, DEFAULT, b), DEFAULT)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(family, d = inputs as in golden_inputs.decode_case_inputs, cfg, clip_wh, tie)."""
    c = {}
    # 1. ReLU-sparse regression maps
    c["sparse_25"] = _case("sparse", relu_sparse(101, 24, 16, 0.25, DEFAULT), DEFAULT)
    c["sparse_50"] = _case("sparse", relu_sparse(102, 24, 16, 0.5, DEFAULT), DEFAULT)
    c["sparse_75"] = _case("sparse", relu_sparse(103, 24, 16, 0.75, DEFAULT), DEFAULT)
    c["sparse_50_n48"] = _case("sparse", relu_sparse(104, 48, 16, 0.5, DEFAULT), DEFAULT)    # N (Ho + 1) > 768: SPLIT = 1
    c["sparse_50_ho29"] = _case("sparse", relu_sparse(105, 8, 29, 0.5, AOT, expansion=4.0), AOT)
    # 2. near-flat maps at a large score
    # (seeds chosen so that no track has a second cell within 6 ulp of its maximum — the kernel must elect THE cell — while
    # 10 .. 65 cells lie within 200 ulp: tests/test_decode_edges.py asserts both from the oracle)
    for (sh, sigma), seed in (((51, 0.0), 771), ((51, 0.4), 455), ((301, 0.0), 511), ((301, 0.4), 515), ((691, 0.0), 891),
                              ((691, 0.4), 1025)):
        c["flat_sh%d_sigma%g" % (sh, sigma)] = _case("flat", near_flat(seed, 6, sh, DEFAULT), dict(DEFAULT, sigma=sigma))
    # 3. saturation and NaN
    c.update(_saturation_cases())
    # 4. geometry sweep with in-regime logits: (Ho, rz, use_centerness, sigma, N, clip)
    for k, (ho, rz, uc, sigma, n, clip) in enumerate(((1, 1, True, 0.4, 3, False), (2, 3, False, 0.1, 4, False),
                                                      (3, 15, True, 0.4, 4, True), (5, 1, False, 0.1, 4, False),
                                                      (17, 3, True, 0.0, 3, True), (32, 15, False, 0.4, 2, False),
                                                      (33, 1, True, 0.0, 2, True), (46, 3, False, 0.1, 2, False))):
        c["geo_ho%d_rz%d" % (ho, rz)] = _geometry(ho, rz, uc, sigma, n, 400 + k, clip)
    return c


CASE_NAMES = ("sparse_25", "sparse_50", "sparse_75", "sparse_50_n48", "sparse_50_ho29",
              "flat_sh51_sigma0", "flat_sh51_sigma0.4", "flat_sh301_sigma0", "flat_sh301_sigma0.4", "flat_sh691_sigma0",
              "flat_sh691_sigma0.4",
              "sat_cls_x40", "sat_cls_inf_rows", "sat_reg_plane_zero", "sat_window_only", "sat_degenerate_boxes",
              "geo_ho1_rz1", "geo_ho2_rz3", "geo_ho3_rz15", "geo_ho5_rz1", "geo_ho17_rz3", "geo_ho32_rz15", "geo_ho33_rz1",
              "geo_ho46_rz3")
FORM_CASES = ("sparse_50", "flat_sh301_sigma0.4", "geo_ho17_rz3", "geo_ho33_rz1")


# ---- the oracle's answer ------------------------------------------------------------------------------------------
def first_argmax(score):
    """``torch.argmax(score, 1)`` on CPU, spelled out: NaN is the largest value, the first index wins."""
    score = np.asarray(score)
    nan = np.isnan(score)
    top = np.where(nan, -np.inf, score).argmax(1)                # (numpy: first occurrence)
    return np.where(nan.any(1), nan.argmax(1), top).astype(np.int64)


def oracle_eval(d, cfg, clip_wh=None):
    """The fp32 oracle on one call's inputs: score map, arg-max (``first_argmax``), box and confidence of that cell
    (clipped with ``O.clip_boxes`` when asked) — and, per cell, whether its penalty sits on the overflow border: the
    exponent argument 0.1 * (1 - s_w * s_h), evaluated in fp64 from the fp32 up-sampled values, within 2^-22 relative of
    ln(FLT_MAX).  There the oracle's expf and the device's may fall on different sides of inf."""
    t = lambda k, dt=torch.float32: torch.from_numpy(np.asarray(d[k])).to(dt)
    boxes = t("boxes")
    up = [O.bicubic_upsample(t(k)) for k in ("cls", "center", "reg")]
    xs, ys = O.grid_axes(t("sr"), cfg["rx"], cfg["rz"], cfg["pad_pixels"])
    bb, conf, idx_torch = O.decode(up[0], up[1], up[2], xs, ys, boxes, cfg["use_centerness"], cfg["sigma"])
    score, _ = O.score_map(up[0], up[1], up[2], boxes, cfg["use_centerness"], cfg["sigma"])
    if clip_wh is not None:
        bb_raw = bb
        bb, conf, _ = O.clip_boxes(bb, conf, clip_wh)
    else:
        bb_raw = bb
    n = boxes.shape[0]
    tlbr = up[2].reshape(n, 4, -1).double()
    s_w = (tlbr[:, 2] + tlbr[:, 0]) / (boxes[:, 2] - boxes[:, 0]).double()[:, None]
    s_h = (tlbr[:, 3] + tlbr[:, 1]) / (boxes[:, 3] - boxes[:, 1]).double()[:, None]
    s_w = torch.max(s_w, 1 / s_w)
    s_h = torch.max(s_h, 1 / s_h)
    arg = (-s_w * s_h + 1) * 0.1
    borderline = ((arg - LN_FLT_MAX).abs() <= 2.0 ** -22 * LN_FLT_MAX).numpy()
    score = score.numpy()
    return dict(score=score, idx=first_argmax(score), idx_torch=idx_torch.numpy(), bb=bb.numpy(), bb_raw=bb_raw.numpy(),
                conf=conf.numpy(), borderline=borderline, G=int(up[0].shape[-1]))


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = cases()[name]
    return oracle_eval(c["d"], c["cfg"], c["clip_wh"])


# ---- the adjudication rule ----------------------------------------------------------------------------------------
def ulps_below_max(orc, n, k):
    """How far the oracle's score of cell k lies below the track's maximum, in ulps of the maximum (finite maxima)."""
    top = float(orc["score"][n, orc["idx"][n]])
    return (top - float(orc["score"][n, k])) / (max(abs(top), 1e-30) * 2.0 ** -23)


def adjudicate(orc, idx):
    """One verdict per track for the cells ``idx`` a decode elected: ("same", 0) — the oracle's arg-max; ("excused",
    why) — another cell the rule admits; ("fail", why).

    Admitted: a cell whose fp32 oracle score is within ULPS ulp of a finite maximum.  For a +inf (or NaN) maximum: a
    cell that is itself +inf (NaN) in the oracle or sits on the overflow border, and only if every +inf (NaN) cell
    with a lower index — which index order would have elected — sits on that border."""
    out = []
    for n, k in enumerate(np.asarray(idx).tolist()):
        s, o, bl = orc["score"][n], int(orc["idx"][n]), orc["borderline"][n]
        if k == o:
            out.append(("same", 0.0))
            continue
        if not 0 <= k < s.shape[0]:
            out.append(("fail", "index %d outside the map" % k))
            continue
        top = s[o]
        if np.isnan(top) or np.isposinf(top):
            peers = np.isnan(s) if np.isnan(top) else np.isposinf(s)
            earlier = np.flatnonzero(peers[:k])
            ok = bool(peers[k] or bl[k]) and bool(bl[earlier].all())
            why = "max %s at %d, cell %d is %s%s, %d earlier peers (%d on the overflow border)" % (
                top, o, k, s[k], " (border)" if bl[k] else "", earlier.size, int(bl[earlier].sum()))
        else:
            u = ulps_below_max(orc, n, k)
            ok = u <= ULPS                                         # (NaN never passes)
            why = "cell %d is %.1f ulp below the max %.9g at %d" % (k, u, top, o)
        out.append(("excused" if ok else "fail", why))
    return out


def same_class_close(got, ref, atol):
    """Element-wise: finite values within ``atol``, non-finite ones of the same class (NaN, +inf, -inf)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        close = np.abs(got - ref) <= atol
    same = (np.isnan(got) & np.isnan(ref)) | (np.isposinf(got) & np.isposinf(ref)) | (np.isneginf(got) & np.isneginf(ref))
    return np.where(fin, np.isfinite(got) & close, same)


def near_max_cells(orc, n, ulps=ULPS):
    """Number of FINITE cells of track n within ``ulps`` of its maximum, the maximum included (0: non-finite maximum)."""
    s = orc["score"][n]
    top = float(s[orc["idx"][n]])
    if not np.isfinite(top):
        return 0
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(np.isfinite(s) & (top - s.astype(np.float64) <= ulps * max(abs(top), 1e-30) * 2.0 ** -23)))
