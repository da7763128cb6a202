"""Cases of the RPN proposal selection and a literal numpy fp32 restatement of the pipeline — TEST INFRASTRUCTURE.

The restatement follows the reference (operator_patch/rpn_patch.py:15-60 on upstream's ``RPNPostProcessor.forward`` /
``select_over_all_levels``) stage by stage on numpy float32 arrays, every operation separately rounded; its NMS is
``oracle.solver_oracle.nms_indices``.  Ranking is on the logit (ties: lower index), which is the reference's ranking on
the sigmoid wherever the selected sigmoid values are distinct — a condition the golden cases assert (``conditions``).

``tools/gen_golden_rpn.py`` runs the reference's unmodified operator on ``golden_inputs(seed)`` and stores inputs and
results in tests/golden/rpn_proposals.npz.
"""
import math

import numpy as np

from oracle.solver_oracle import nms_indices

F32 = np.float32
IMAGE_WH = (320, 192)
STRIDES = (4, 8, 16, 32, 64)
NUM_ANCHORS = 3
LEVELS = tuple((IMAGE_WH[1] // s, IMAGE_WH[0] // s) for s in STRIDES)          # (H, W): 48x80 ... 3x5
XFORM_CLIP = math.log(1000.0 / 16)
WEIGHTS = (1.0, 1.0, 1.0, 1.0)
NMS_THRESH = 0.7
IOU_MARGIN = 5e-4
SIZE_MARGIN = 1e-2

# pre 256: the two top levels have fewer anchors (180, 45) than k
GOLDEN_CASES = {
    "n1_clip_post32_min4": dict(N=1, pre=256, post=32, fpn=100, min_size=4, amodal=False),
    "n2_amodal_post300_min0": dict(N=2, pre=256, post=300, fpn=100, min_size=0, amodal=True),
    "n2_clip_post32_min4": dict(N=2, pre=256, post=32, fpn=100, min_size=4, amodal=False),
    "n1_amodal_post300_min0": dict(N=1, pre=256, post=300, fpn=100, min_size=0, amodal=True),
}


def level_anchors(H, W, stride):
    """``[H*W*A, 4]`` fp32 xyxy anchors in the reference's flattened order (h*W + w)*A + a: three shapes of area
    ~(4*stride)^2 around every cell centre; every coordinate is exact in fp32."""
    size = 4.0 * stride
    shapes = np.array([(1.5, 0.75), (1.0, 1.0), (0.75, 1.5)]) * size               # (w, h)
    cy, cx = np.meshgrid(np.arange(H) * stride + stride / 2.0 - 0.5, np.arange(W) * stride + stride / 2.0 - 0.5, indexing="ij")
    cx, cy = cx[:, :, None], cy[:, :, None]
    hw, hh = (shapes[:, 0] - 1) / 2.0, (shapes[:, 1] - 1) / 2.0
    out = np.stack([cx - hw, cy - hh, cx + hw, cy + hh], axis=-1)
    return np.ascontiguousarray(out.reshape(-1, 4).astype(F32))


def anchors(levels=LEVELS, strides=STRIDES):
    return [level_anchors(h, w, s) for (h, w), s in zip(levels, strides)]


def golden_inputs(seed, num_images=2, levels=LEVELS, A=NUM_ANCHORS):
    """Logits (fp32) and regression values (on the fp16 grid) of ``num_images`` images with different contents."""
    rng = np.random.RandomState(seed)
    obj, reg = [], []
    for (h, w) in levels:
        obj.append((rng.standard_normal((num_images, A, h, w)) * 1.5 - 2.0).astype(F32))
        reg.append((rng.standard_normal((num_images, 4 * A, h, w)) * 0.5).astype(np.float16).astype(F32))
    return obj, reg


# ---- the pipeline, stage by stage ---------------------------------------------------------------------------------------
def exp32(x):
    """fp32 exp as the reference's CPU run evaluates it.  The one operation here that is not numpy's: ``np.exp`` on float32
    differs from torch's CPU ``exp`` in the last bit for about a third of the arguments (and the correctly rounded value
    for about 1 %), and the fixture was written by torch; every other operation of the restatement is numpy fp32."""
    import torch
    return torch.exp(torch.from_numpy(np.ascontiguousarray(x, dtype=F32))).numpy()


def sigmoid32(x):
    """... and its sigmoid, for the same reason (1 / (1 + exp32(-x)) differs from it in the last bit for 4 %)."""
    import torch
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x, dtype=F32))).numpy()


def flatten_logits(o):
    """permute_and_flatten of one level: [N, A, H, W] -> [N, H*W*A]."""
    return np.ascontiguousarray(o.transpose(0, 2, 3, 1).reshape(o.shape[0], -1))


def flatten_regression(r):
    """[N, 4A, H, W] -> [N, H*W*A, 4]."""
    N, C, H, W = r.shape
    return np.ascontiguousarray(r.reshape(N, C // 4, 4, H, W).transpose(0, 3, 4, 1, 2).reshape(N, -1, 4))


def select(logits_flat, k):
    """Indices of the k best logits in descending order, ties to the lower index (-0 ranks as +0)."""
    return np.argsort(-(logits_flat.astype(F32) + F32(0)), kind="stable")[:k]


def decode(deltas, anc, weights=WEIGHTS, clip=XFORM_CLIP, dtype=F32):
    """[UPSTREAM] BoxCoder.decode in ``dtype`` (float32: the restatement; float64: the yardstick of the decode test)."""
    d, a = deltas.astype(dtype), anc.astype(dtype)
    one, half = dtype(1), dtype(0.5)
    w = a[:, 2] - a[:, 0] + one
    h = a[:, 3] - a[:, 1] + one
    cx = a[:, 0] + half * w
    cy = a[:, 1] + half * h
    dx, dy = d[:, 0] / dtype(weights[0]), d[:, 1] / dtype(weights[1])
    dw = np.minimum(d[:, 2] / dtype(weights[2]), dtype(clip))
    dh = np.minimum(d[:, 3] / dtype(weights[3]), dtype(clip))
    pcx, pcy = dx * w + cx, dy * h + cy
    ew, eh = (exp32(dw), exp32(dh)) if dtype is F32 else (np.exp(dw), np.exp(dh))
    pw, ph = ew * w, eh * h
    return np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw - one, pcy + half * ph - one], axis=1).astype(dtype)


def clip_filter(boxes, logits, image_wh, min_size, amodal):
    """clip_to_image(remove_empty=False) unless amodal, then remove_small_boxes.  -> (boxes, logits, widths, heights of
    ALL rows after the clip)."""
    b = boxes.astype(F32).copy()
    if not amodal:
        for col, hi in ((0, image_wh[0] - 1), (1, image_wh[1] - 1), (2, image_wh[0] - 1), (3, image_wh[1] - 1)):
            b[:, col] = np.minimum(np.maximum(b[:, col], F32(0)), F32(hi))
    ws = b[:, 2] - b[:, 0] + F32(1)
    hs = b[:, 3] - b[:, 1] + F32(1)
    keep = (ws >= F32(min_size)) & (hs >= F32(min_size))
    return b[keep], logits[keep], ws, hs


def level_nms(boxes, logits, thresh, post):
    keep = nms_indices(boxes, logits, thresh)[:post] if len(boxes) else np.zeros(0, np.int64)
    return boxes[keep], logits[keep]


def merge(level_boxes, level_logits, fpn_post):
    """One image: concatenation in level order; with several levels the min(fpn_post, total) best, ties to the lower
    concatenated position."""
    boxes, logits = np.concatenate(level_boxes, 0), np.concatenate(level_logits, 0)
    if len(level_boxes) > 1:
        order = np.argsort(-(logits + F32(0)), kind="stable")[:min(fpn_post, len(logits))]
        boxes, logits = boxes[order], logits[order]
    return boxes, logits


def post_stages(cand_boxes, cand_logits, image_wh, case, thresh=NMS_THRESH):
    """Clip, filter, NMS and merge of ONE image from its per-level candidates (decoded boxes before the clip and their
    logits, best first).  -> (boxes, logits)."""
    lb, ll = [], []
    for b, s in zip(cand_boxes, cand_logits):
        b, s, _, _ = clip_filter(b, s, image_wh, case["min_size"], case["amodal"])
        b, s = level_nms(b, s, thresh, case["post"])
        lb.append(b)
        ll.append(s)
    return merge(lb, ll, case["fpn"])


def candidates(obj, reg, anc, img, pre):
    """Select + decode of one image: per level (flat indices, logits, decoded boxes)."""
    out = []
    for o, r, a in zip(obj, reg, anc):
        flat = flatten_logits(o[img:img + 1])[0]
        idx = select(flat, min(pre, len(flat)))
        out.append((idx, flat[idx], decode(flatten_regression(r[img:img + 1])[0][idx], a[idx])))
    return out


def pipeline(obj, reg, anc, case, image_wh=IMAGE_WH, thresh=NMS_THRESH):
    """The whole operator.  -> per image (boxes [n,4], objectness [n])."""
    res = []
    for img in range(case["N"]):
        cand = candidates(obj, reg, anc, img, case["pre"])
        boxes, logits = post_stages([c[2] for c in cand], [c[1] for c in cand], image_wh, case, thresh)
        res.append((boxes, sigmoid32(logits)))
    return res


# ---- conditions on the golden inputs (not tolerances: see tools/gen_golden_rpn.py) --------------------------------------
def _chain_iou_margin(boxes, thresh, post):
    """Smallest |IoU - thresh| over the IoUs the greedy chain evaluates between a kept box and a live later box (the chain
    stops at ``post`` kept boxes)."""
    b = boxes.astype(np.float64)
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    dead = np.zeros(len(b), bool)
    margin, kept = np.inf, 0
    for i in range(len(b)):
        if dead[i]:
            continue
        kept += 1
        if kept > post:
            break
        live = np.nonzero(~dead[i + 1:])[0] + i + 1
        if len(live):
            w = np.maximum(np.minimum(b[i, 2], b[live, 2]) - np.maximum(b[i, 0], b[live, 0]) + 1, 0)
            h = np.maximum(np.minimum(b[i, 3], b[live, 3]) - np.maximum(b[i, 1], b[live, 1]) + 1, 0)
            iou = w * h / (area[i] + area[live] - w * h)
            margin = min(margin, float(np.abs(iou - thresh).min()))
            dead[live[iou > thresh]] = True
    return margin


def conditions(obj, reg, anc, case, image_wh=IMAGE_WH, thresh=NMS_THRESH):
    """-> dict(distinct=bool, iou_margin=float, size_margin=float) of one case."""
    distinct, iou_m, size_m = True, np.inf, np.inf
    for img in range(case["N"]):
        lb, ll = [], []
        for idx, logit, box in candidates(obj, reg, anc, img, case["pre"]):
            s = sigmoid32(logit)
            distinct &= len(np.unique(s)) == len(s)
            b, lg, ws, hs = clip_filter(box, logit, image_wh, case["min_size"], case["amodal"])
            size_m = min(size_m, float(np.abs(ws.astype(np.float64) - case["min_size"]).min()),
                         float(np.abs(hs.astype(np.float64) - case["min_size"]).min()))
            iou_m = min(iou_m, _chain_iou_margin(b, thresh, case["post"]))
            b, lg = level_nms(b, lg, thresh, case["post"])
            lb.append(b)
            ll.append(lg)
        s = sigmoid32(np.concatenate(ll))
        distinct &= len(np.unique(s)) == len(s)
    return dict(distinct=bool(distinct), iou_margin=iou_m, size_margin=size_m)


def conditions_hold(c):
    return c["distinct"] and c["iou_margin"] >= IOU_MARGIN and c["size_margin"] >= SIZE_MARGIN
