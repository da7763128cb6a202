"""Seeded inputs and reference answers for tests/test_box_detect.py: the box head's post-processing of proposals that are
all DETECTIONS (csrc/box_detect.hip, ``ops.box_detect_post``) — TEST INFRASTRUCTURE, nothing here touches a device.

Three families of inputs:

  * decode   random logits and deltas on clustered proposals, at most 300 rows that exist: soft-max, per-class decode, clip,
             threshold and NMS coupled as in production.  A discrete decision (candidate or not, suppressed or not) is only
             pinned where no correct fp32 implementation can take it differently, so the inputs meet ``conditions``: every
             score further from the threshold than the score bound, same-class candidate scores further apart than twice
             that bound, and for every same-class candidate pair the fp64 IoU, widened to an interval by moving every decoded
             coordinate by +-delta (the case's box bound in pixels; 0 for a coordinate the clip pins), does not contain the
             NMS threshold.
  * exact    integer proposals inside the image with zero deltas (2048 rows): the decode returns the proposal exactly in
             fp32, every area is an integer below 2^24 and the NMS threshold is 0.5, so IoU > 0.5 is decided by integers
             and every correct implementation takes the same decisions without a margin; logit differences sit on a grid.
  * edge     the exact family with deliberate structure (``edge_k4``): a pair at IoU exactly 0.5 (kept), a pair one
             integer above (suppressed), a chain A > B > C (B dies, so C lives), a chain of four across the 64-candidate
             tile boundary, two rows identical in every input (the lower row wins), a class without a candidate between
             two classes with some, a class where every row is a candidate; ``edge_thresh_k20``: a row of equal logits at
             K = 20, whose scores are exactly the threshold 0.05 and therefore no candidates.

``restated(c)`` is ``siammot_amd.box_refine.PostProcessor`` on CPU in fp32 over ``oracle.solver_oracle.nms_indices`` — the
reference's arithmetic, pinned to the reference's own code by tests/golden/box_detect_post.npz.  ``direct(c, dtype)`` is the
same operation written out; in fp32 it equals the restatement bit for bit (asserted by the CPU tests) and also names the
proposal row of every detection; its fp64 evaluation gives the error bounds: ``(2 e32 + 2^-22) * s`` with s = 2 for scores
and the decode's operand scale for boxes (tests/box_refine_edge_cases.py)."""
import functools
import math

import numpy as np
import torch

from oracle.solver_oracle import nms_indices

F32 = np.float32
IMAGE_WH = (1280, 704)
MARGIN = 2.0 ** -22
YAML_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
GOLDEN_CASES = ("d_m65_k17", "d_m300_k2", "d_m512_c300_k3", "d_agn_m65_k3", "d_amodal_m63_k2", "edge_k4")


def _case(family, head_out, boxes, count, K, agnostic=False, weights=YAML_WEIGHTS, clip_wh=IMAGE_WH, score_thresh=0.05,
          nms_thresh=0.5, ordinary=True, **extra):
    M = len(boxes)
    assert head_out.shape[0] == M and 0 <= count <= M <= 2048
    c = dict(family=family, head_out=np.ascontiguousarray(head_out, F32), boxes=np.ascontiguousarray(boxes, F32),
             count=int(count), M=M, num_classes=K, reg_classes=2 if agnostic else K, agnostic=agnostic,
             weights=tuple(float(w) for w in weights), clip_wh=clip_wh, score_thresh=score_thresh, nms_thresh=nms_thresh,
             ordinary=ordinary, identical=(), at_threshold=())
    c.update(extra)
    return c


# ---- decode family ------------------------------------------------------------------------------------------------------
def _decode_case(seed, M, K, count=None, agnostic=False, weights=YAML_WEIGHTS, clip_wh=IMAGE_WH, score_thresh=0.05,
                 nms_thresh=0.5, pad=0, ordinary=True):
    rs = np.random.RandomState(seed)
    n = M if count is None else count
    KR = 2 if agnostic else K
    groups = max(1, n // 3)
    gxy = rs.uniform(0.0, 1.0, (groups, 2)) * (1000.0, 480.0)
    gwh = rs.uniform(40.0, 200.0, (groups, 2))
    g = rs.randint(0, groups, M)
    xy = gxy[g] + rs.uniform(-0.12, 0.12, (M, 2)) * gwh[g]
    wh = gwh[g] * rs.uniform(0.85, 1.15, (M, 2))
    boxes = np.concatenate((xy, xy + wh), 1)
    ho = np.empty((M, K + 4 * KR + pad), np.float64)
    ho[:, :K] = rs.standard_normal((M, K)) * 2.0
    ho[:, K:] = 900.0 + 3.5 * np.arange(ho.shape[1] - K)[None, :]        # poison wherever no delta belongs
    w = np.asarray(weights, np.float64)
    m = 1 if agnostic else K
    d = (rs.standard_normal((M, m, 4)) * (0.1, 0.1, 0.06, 0.06) * w).reshape(M, 4 * m)
    if agnostic:
        ho[:, K + 4:K + 8] = d
    else:
        ho[:, K:K + 4 * K] = d
    return _case("decode", ho, boxes, n, K, agnostic, weights, clip_wh, score_thresh, nms_thresh, ordinary)


# ---- exact family -------------------------------------------------------------------------------------------------------
def _grid_logits(rs, M, K, lo, hi):
    """Class logits whose differences to class 0 sit on a grid of M distinct points per class (a permutation each)."""
    lg = np.zeros((M, K))
    step = (hi - lo) / M
    for j in range(1, K):
        lg[:, j] = lo + step * (rs.permutation(M) + 0.5)
    return lg


def _exact_case(seed, M, K, size=(30, 160), lo=-3.5, hi=3.0):
    rs = np.random.RandomState(seed)
    W, H = IMAGE_WH
    wh = rs.randint(size[0], size[1], (M, 2))
    xy = np.stack((rs.randint(0, W - size[1], M), rs.randint(0, H - size[1], M)), 1)
    boxes = np.concatenate((xy, xy + wh - 1), 1).astype(np.float64)
    ho = np.zeros((M, K + 4 * K))
    ho[:, :K] = _grid_logits(rs, M, K, lo, hi)
    return _case("exact", ho, boxes, M, K)


def _thin(x, y, n):
    """A box one pixel wide and n pixels tall: IoUs of two on one column are ratios of small integers."""
    return (x, y, x, y + n - 1)


EDGE_RANKS = dict(half=(2, 3), above=(5, 6), chain=(8, 9, 10), identical=(20, 21), tile=(62, 63, 64, 65))


def _edge_case():
    """K = 4, 130 rows, zero deltas.  Class 1: candidates are the rows of rank < 116 in its score order (rank k has the
    logit 1.5 - 0.03 k); class 2 has no candidate; class 3 (score order reversed) has all 130 rows."""
    rs = np.random.RandomState(4101)
    M, K = 130, 4
    rank_of_row = rs.permutation(M)
    ia, ib = EDGE_RANKS["identical"]
    ra, rb = sorted((int(np.nonzero(rank_of_row == ia)[0][0]), int(np.nonzero(rank_of_row == ib)[0][0])))
    rank_of_row[ra], rank_of_row[rb] = ia, ib                       # the lower row comes first among equals
    l1 = 1.5 - 0.03 * rank_of_row
    l1[rb] = l1[ra]
    boxes = np.array([_thin(8 * k + 2, 10, 100) for k in rank_of_row], np.float64)

    def put(ranks, x, specs):
        for k, (dy, n) in zip(ranks, specs):
            boxes[int(np.nonzero(rank_of_row == k)[0][0])] = _thin(x, 10 + dy, n)
    put(EDGE_RANKS["half"], 1100, ((0, 99), (33, 99)))              # intersection 66, union 132: IoU exactly 0.5
    put(EDGE_RANKS["above"], 1110, ((0, 100), (33, 100)))           # 67 / 133: 2 * 67 = 133 + 1
    put(EDGE_RANKS["chain"], 1120, ((0, 100), (30, 100), (60, 100)))                # 70/130, 40/160, 70/130
    put(EDGE_RANKS["tile"], 1130, ((0, 100), (30, 100), (60, 100), (90, 100)))
    put(EDGE_RANKS["identical"], 1140, ((0, 100), (0, 100)))
    ho = np.zeros((M, K + 4 * K))
    ho[:, 1] = l1
    ho[:, 2] = -8.0
    ho[:, 3] = 0.5
    return _case("edge", ho, boxes, M, K, ordinary=False, identical=((ra, rb),), rank_of_row=rank_of_row)


def _edge_thresh_case():
    """K = 20, 65 rows of the exact family; row 7 has equal logits: twenty scores of exactly 1/20 in fp32."""
    rs = np.random.RandomState(4201)
    c = _exact_case(4202, 65, 20, size=(30, 200), lo=-2.0, hi=2.0)
    g = rs.randint(0, 10, 65)                                         # ten clusters: something to suppress
    xy = np.stack((100 * g + rs.randint(0, 12, 65), 40 * (g % 3) + rs.randint(0, 12, 65)), 1)
    wh = rs.randint(60, 90, (65, 2))
    c["boxes"] = np.concatenate((xy, xy + wh - 1), 1).astype(F32)
    c["head_out"][7, :20] = 3.0
    c.update(family="edge", ordinary=False, at_threshold=(7,))
    return c


# seeds found by tools/gen_golden_box_detect.py --search (the first of six per shape that meets ``conditions``)
SEEDS = dict(d_m1_k2=1100, d_m63_k3=1200, d_m64_k2=1300, d_m65_k17=1400, d_m300_k2=1500, d_m300_k3=1600,
             d_m512_c300_k3=1701, d_m64_c0_k2=1800, d_agn_m65_k3=1900, d_amodal_m63_k2=2000, d_clip1x1_m65_k2=2100,
             d_w_m65_k3=2200, x_m2048_k2=3000)


def build_case(name, seed=None):
    s = SEEDS.get(name) if seed is None else seed
    if name == "d_m1_k2":
        c = _decode_case(s, 1, 2, ordinary=False)
        c["head_out"][0, :2] = (0.0, 1.0)                             # (one row: a candidate whatever the seed)
        return c
    if name == "d_m63_k3":
        return _decode_case(s, 63, 3, pad=3)
    if name == "d_m64_k2":
        return _decode_case(s, 64, 2)
    if name == "d_m65_k17":
        return _decode_case(s, 65, 17, ordinary=False)                # (few candidates per class: no fractions asked)
    if name == "d_m300_k2":
        return _decode_case(s, 300, 2)
    if name == "d_m300_k3":
        return _decode_case(s, 300, 3)
    if name == "d_m512_c300_k3":
        return _decode_case(s, 512, 3, count=300)
    if name == "d_m64_c0_k2":
        return _decode_case(s, 64, 2, count=0, ordinary=False)
    if name == "d_agn_m65_k3":
        return _decode_case(s, 65, 3, agnostic=True)
    if name == "d_amodal_m63_k2":
        return _decode_case(s, 63, 2, clip_wh=None)
    if name == "d_clip1x1_m65_k2":
        return _decode_case(s, 65, 2, clip_wh=(1, 1), ordinary=False)
    if name == "d_w_m65_k3":
        return _decode_case(s, 65, 3, weights=(3.0, 7.0, 0.5, 2.0), score_thresh=0.3, nms_thresh=0.4)
    if name == "x_m2048_k2":
        return _exact_case(s, 2048, 2)
    if name == "edge_k4":
        return _edge_case()
    if name == "edge_thresh_k20":
        return _edge_thresh_case()
    raise KeyError(name)


CASE_NAMES = ("d_m1_k2", "d_m63_k3", "d_m64_k2", "d_m65_k17", "d_m300_k2", "d_m300_k3", "d_m512_c300_k3", "d_m64_c0_k2",
              "d_agn_m65_k3", "d_amodal_m63_k2", "d_clip1x1_m65_k2", "d_w_m65_k3", "x_m2048_k2", "edge_k4",
              "edge_thresh_k20")


@functools.lru_cache(maxsize=None)
def case(name):
    return build_case(name)


# ---- the reference ------------------------------------------------------------------------------------------------------
def _oracle_nms(boxlist, thresh):
    keep = nms_indices(boxlist.bbox.numpy(), boxlist.get_field("scores").numpy(), thresh)
    return boxlist[torch.from_numpy(keep)]


def restated(c):
    """``siammot_amd.box_refine.PostProcessor`` on CPU in fp32 on the rows that exist, as an id-less BoxList."""
    from siammot_amd.box_refine import BoxCoder, PostProcessor
    from siammot_amd.structures import BoxList
    K, KR, n = c["num_classes"], c["reg_classes"], c["count"]
    assert n > 0, "the reference cannot reshape zero rows (inference.py:69-71)"
    ho = torch.from_numpy(c["head_out"][:n])
    logits, reg = ho[:, :K].contiguous(), ho[:, K:K + 4 * KR].contiguous()
    post = PostProcessor(c["score_thresh"], c["nms_thresh"], BoxCoder(c["weights"]), c["agnostic"], c["clip_wh"] is None,
                         nms_fn=_oracle_nms)
    prop = BoxList(torch.from_numpy(c["boxes"][:n].copy()), c["clip_wh"] or IMAGE_WH, mode="xyxy")
    with torch.no_grad():
        r = post((logits, reg), [prop])[0]
    return dict(boxes=r.bbox.numpy(), scores=r.get_field("scores").numpy(), labels=r.get_field("labels").numpy(),
                ids=r.get_field("ids").numpy())


def _nms64(boxes, scores, thresh):
    order = np.argsort(-scores, kind="stable")
    b = boxes[order]
    area = (b[:, 2] - b[:, 0] + 1.0) * (b[:, 3] - b[:, 1] + 1.0)
    dead = np.zeros(len(b), bool)
    for i in range(len(b)):
        if dead[i]:
            continue
        w = np.maximum(np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]) + 1.0, 0)
        h = np.maximum(np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]) + 1.0, 0)
        inter = w * h
        dead[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > thresh
    return np.sort(order[~dead])


def direct(c, dtype=torch.float32, exclude=()):
    """The operation written out in ``dtype``: soft-max, ``BoxCoder.decode`` of every class's deltas (or the agnostic
    ones), clip, per class the rows with p > thresh, greedy NMS, survivors by ascending row.  ``exclude``: rows taken out
    of candidacy.  -> boxes, scores, labels, rows, counts [K] (word 0: total) and the dense ``prob`` [n, K], ``dec``
    [n, K, 4] (clipped) and ``raw`` (unclipped)."""
    from siammot_amd.box_refine import BoxCoder
    K, KR, n = c["num_classes"], c["reg_classes"], c["count"]
    f32 = dtype is torch.float32
    if n == 0:                                                         # (the reference cannot reshape zero rows: defined here)
        np_dt = F32 if f32 else np.float64
        return dict(boxes=np.zeros((0, 4), np_dt), scores=np.zeros(0, np_dt), labels=np.zeros(0, np.int64),
                    rows=np.zeros(0, np.int32), counts=np.zeros(K, np.int32), prob=np.zeros((0, K), np_dt),
                    dec=np.zeros((0, K, 4), np_dt), raw=np.zeros((0, K, 4), np_dt))
    ho = torch.from_numpy(c["head_out"][:n]).to(dtype)
    prob = torch.softmax(ho[:, :K].contiguous(), -1)
    reg = ho[:, K:K + 4 * KR].contiguous()
    if c["agnostic"]:
        reg = reg[:, -4:]
    raw = BoxCoder(c["weights"]).decode(reg.reshape(n, -1), torch.from_numpy(c["boxes"][:n]).to(dtype))
    if c["agnostic"]:
        raw = raw.repeat(1, K)
    raw = raw.reshape(n, K, 4)
    dec = raw.clone()
    if c["clip_wh"] is not None:
        for k, hi in enumerate((c["clip_wh"][0] - 1, c["clip_wh"][1] - 1) * 2):
            dec[:, :, k] = torch.clamp(dec[:, :, k], min=0, max=hi)
    prob_n, dec_n = prob.numpy(), dec.numpy()
    thresh = F32(c["score_thresh"]) if f32 else c["score_thresh"]
    out_b, out_s, out_l, out_r, counts = [], [], [], [], [0] * K
    for j in range(1, K):
        with np.errstate(invalid="ignore"):
            cand = np.nonzero(prob_n[:, j] > thresh)[0]
        cand = cand[~np.isin(cand, exclude)]
        if f32:
            keep = nms_indices(dec_n[cand, j], prob_n[cand, j], c["nms_thresh"]) if len(cand) else np.zeros(0, np.int64)
        else:
            keep = _nms64(dec_n[cand, j], prob_n[cand, j], c["nms_thresh"])
        rows = cand[keep]
        counts[j] = len(rows)
        out_b.append(dec_n[rows, j])
        out_s.append(prob_n[rows, j])
        out_l.append(np.full(len(rows), j, np.int64))
        out_r.append(rows.astype(np.int32))
    counts[0] = sum(counts[1:])
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dt)
    return dict(boxes=cat(out_b, (0, 4), prob_n.dtype), scores=cat(out_s, (0,), prob_n.dtype), labels=cat(out_l, (0,), np.int64),
                rows=cat(out_r, (0,), np.int32), counts=np.asarray(counts, np.int32), prob=prob_n, dec=dec_n,
                raw=raw.numpy())


def operand_scale(c):
    """``|pred_ctr| + 0.5 * pred_size + 1`` per (row, class, coordinate) in fp64: what the decode's last subtraction rounds
    at (tests/box_refine_edge_cases.py)."""
    K, KR, n = c["num_classes"], c["reg_classes"], c["count"]
    ho = torch.from_numpy(c["head_out"][:n]).double()
    b = torch.from_numpy(c["boxes"][:n]).double()
    reg = ho[:, K:K + 4 * KR]
    d = reg[:, -4:].repeat(1, K).reshape(n, K, 4) if c["agnostic"] else reg.reshape(n, K, 4)
    wx, wy, ww, wh = c["weights"]
    w, h = (b[:, 2] - b[:, 0] + 1)[:, None], (b[:, 3] - b[:, 1] + 1)[:, None]
    pcx, pcy = d[:, :, 0] / wx * w + b[:, 0:1] + 0.5 * w, d[:, :, 1] / wy * h + b[:, 1:2] + 0.5 * h
    clip = math.log(1000.0 / 16)
    pw, ph = torch.exp(torch.clamp(d[:, :, 2] / ww, max=clip)) * w, torch.exp(torch.clamp(d[:, :, 3] / wh, max=clip)) * h
    sx, sy = pcx.abs() + 0.5 * pw.abs() + 1, pcy.abs() + 0.5 * ph.abs() + 1
    return torch.stack((sx, sy, sx, sy), 2).numpy()


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_eval(case(name))


def reference_eval(c):
    """fp32 and fp64 ``direct``, the dense bounds ``score_bound`` (a number) and ``box_bound`` [n, K, 4], and ``delta``: the
    largest box bound over the candidates, in pixels."""
    f32, f64 = direct(c, torch.float32), direct(c, torch.float64)
    n, K = c["count"], c["num_classes"]
    if n == 0:
        return dict(f32=f32, f64=f64, score_bound=MARGIN * 2.0, box_bound=np.zeros((0, K, 4)), delta=0.0)
    scale = operand_scale(c)
    fg = slice(1, K)
    e_score = float(np.abs(f32["prob"][:, fg].astype(np.float64) - f64["prob"][:, fg]).max() / 2.0)
    e_box = float((np.abs(f32["raw"][:, fg].astype(np.float64) - f64["raw"][:, fg]) / scale[:, fg]).max())
    box_bound = (2.0 * e_box + MARGIN) * scale
    cand = f64["prob"][:, fg] > c["score_thresh"]
    delta = float(box_bound[:, fg][cand].max()) if cand.any() else 0.0
    return dict(f32=f32, f64=f64, score_bound=(2.0 * e_score + MARGIN) * 2.0, box_bound=box_bound, delta=delta)


# ---- conditions on the inputs -------------------------------------------------------------------------------------------
def _iou_interval(b, slack):
    """All pairs of the boxes ``b`` [m, 4] (fp64) whose coordinates are known to +-``slack`` [m, 4]: (lowest, highest) IoU."""
    lo, hi = b - slack, b + slack
    def inter(x1, y1, x2, y2):
        w = np.maximum(np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :]) + 1.0, 0.0)
        h = np.maximum(np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :]) + 1.0, 0.0)
        return w * h
    area = lambda x1, y1, x2, y2: np.maximum(x2 - x1 + 1.0, 0.0) * np.maximum(y2 - y1 + 1.0, 0.0)
    i_lo = inter(hi[:, 0], hi[:, 1], lo[:, 2], lo[:, 3])              # every box as small as it can be
    i_hi = inter(lo[:, 0], lo[:, 1], hi[:, 2], hi[:, 3])
    a_lo, a_hi = area(hi[:, 0], hi[:, 1], lo[:, 2], lo[:, 3]), area(lo[:, 0], lo[:, 1], hi[:, 2], hi[:, 3])
    u_hi = a_hi[:, None] + a_hi[None, :] - i_lo
    u_lo = np.maximum(a_lo[:, None] + a_lo[None, :] - i_hi, i_hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(u_hi > 0, i_lo / u_hi, 0.0), np.where(u_lo > 0, np.minimum(i_hi / u_lo, 1.0), 1.0)


def conditions(c, ref=None, score_bound=None, delta=None):
    """What the inputs of a case promise, from the reference alone -> dict of measured margins and verdicts.
    ``score_bound`` / ``delta``: coarser bounds than the case's own (the wiring test's, which must also cover the rounding
    of the GEMMs in front)."""
    ref = reference_eval(c) if ref is None else ref
    ref = dict(ref, score_bound=ref["score_bound"] if score_bound is None else score_bound,
               delta=ref["delta"] if delta is None else delta)
    K, n = c["num_classes"], c["count"]
    f64, thresh, bound = ref["f64"], c["score_thresh"], ref["score_bound"]
    out = dict(score_bound=bound, delta=ref["delta"], score_margin=np.inf, score_gap=np.inf, iou_clear=True,
               candidates=0, survivors=int(ref["f32"]["counts"][0]), exact=True, same_decisions=True)
    if n == 0:
        return out
    rows = np.ones(n, bool)
    rows[list(c["at_threshold"])] = False
    out["score_margin"] = float(np.abs(f64["prob"][rows, 1:] - thresh).min()) if rows.any() else np.inf
    twin = {b for _, b in c["identical"]}
    for j in range(1, K):
        cand = np.nonzero(f64["prob"][:, j] > thresh)[0]
        out["candidates"] += len(cand)
        s = np.sort(f64["prob"][[r for r in cand if r not in twin], j])
        if len(s) > 1:
            out["score_gap"] = min(out["score_gap"], float(np.diff(s).min()))
        if c["family"] == "decode" and len(cand) > 1:
            b = f64["dec"][cand, j]
            slack = np.full(b.shape, ref["delta"])
            if c["clip_wh"] is not None:                               # a coordinate the clip pins is exact
                raw = f64["raw"][cand, j]
                for k, hi in enumerate((c["clip_wh"][0] - 1, c["clip_wh"][1] - 1) * 2):
                    slack[(raw[:, k] < -ref["delta"]) | (raw[:, k] > hi + ref["delta"]), k] = 0.0
            lo, hi = _iou_interval(b, slack)
            off = ~np.eye(len(cand), dtype=bool)
            out["iou_clear"] &= bool(((lo[off] > c["nms_thresh"]) | (hi[off] < c["nms_thresh"])).all())
    if c["family"] != "decode":
        b = c["boxes"][:n].astype(np.float64)
        W, H = c["clip_wh"]
        area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
        out["exact"] = bool((b == np.round(b)).all() and (b[:, :2] >= 0).all() and (b[:, 2] <= W - 1).all()
                            and (b[:, 3] <= H - 1).all() and 2 * area.max() < 2 ** 24 and c["nms_thresh"] == 0.5
                            and not c["head_out"][:n, K:].any() and (b[:, 2] >= b[:, 0]).all() and (b[:, 3] >= b[:, 1]).all())
    out["same_decisions"] = bool(np.array_equal(ref["f32"]["rows"], f64["rows"]) and np.array_equal(ref["f32"]["labels"], f64["labels"]))
    return out


def conditions_hold(c, cond):
    ok = (cond["score_margin"] > cond["score_bound"] and cond["score_gap"] > 2.0 * cond["score_bound"] and cond["iou_clear"]
          and cond["exact"] and cond["same_decisions"])
    if c["family"] == "exact":
        ok = ok and cond["score_gap"] > 1e-5
    if c["ordinary"]:
        supp = cond["candidates"] - cond["survivors"]
        ok = ok and 5 * supp >= cond["candidates"] and 5 * cond["survivors"] >= cond["candidates"] and cond["candidates"] > 0
    return bool(ok)
