"""RPN proposal selection: the reference's ``RPNPostProcessor`` (siammot/operator_patch/rpn_patch.py:9-60 on
[UPSTREAM] maskrcnn_benchmark/modeling/rpn/inference.py) for inference.

Two forms of the same operator live here:

* ``RPNPostProcessor.forward`` on device tensors within the capacities of ``ops.rpn_proposals``: every image and level
  in one set of HIP launches, ONE device-to-host copy per call (the N proposal counts) and no other synchronisation;
* ``rpn_proposals_torch``: the same operator as a plain torch composition on this package's ``BoxList``, ``BoxCoder``
  and ``structures.boxlist_nms``, with an injectable NMS.  It is the path for CPU tensors, the fallback beyond the
  capacities (counted in ``ops.FALLBACKS["rpn_torch"]``) and the baseline of tools/rpn_proposals_bench.py.

The reference installs its operator by assignment (rpn_patch.py:90); the same line binds this one:

    rpn_inference.make_rpn_postprocessor = siammot_amd.rpn.make_rpn_postprocessor

The RPN head's convolutions and the anchor generator stay PyTorch modules.
"""
import torch

from . import ops
from .box_refine import BoxCoder
from .structures import TO_REMOVE, BoxList, boxlist_nms, cat_boxlist


def _level_candidates(logits, deltas, anchor_boxes, top_n):
    """One FPN level, all images at once: the ``min(top_n, A*H*W)`` anchors of every image with the highest sigmoid score,
    best first.  logits ``[N, A, H, W]``, deltas ``[N, 4A, H, W]`` (channel 4a + c), anchor_boxes: per image ``[A*H*W, 4]``
    in the order (h*W + w)*A + a.  -> scores ``[N, k]``, deltas ``[N, k, 4]``, anchors ``[N, k, 4]``."""
    N, A, H, W = logits.shape
    cells = H * W * A
    scores = logits.permute(0, 2, 3, 1).reshape(N, cells).sigmoid()
    k = min(top_n, cells)
    scores, order = scores.topk(k, dim=1)                       # sorted: descending
    rows = order.unsqueeze(-1).expand(N, k, 4)
    deltas = deltas.view(N, A, 4, H, W).permute(0, 3, 4, 1, 2).reshape(N, cells, 4).take_along_dim(rows, dim=1)
    anchors = torch.stack(list(anchor_boxes), dim=0).take_along_dim(rows, dim=1)
    return scores, deltas, anchors


def _drop_small(boxlist, min_size):
    """Rows whose two sides (x2 - x1 + 1, y2 - y1 + 1) are both >= min_size."""
    box = boxlist.bbox
    sides = box[:, 2:] - box[:, :2] + TO_REMOVE
    return boxlist[(sides >= min_size).all(dim=1)]


def _suppress(boxlist, nms_thresh, limit, nms_fn):
    """Greedy NMS on the ``objectness`` field, first ``limit`` kept rows.  ``nms_fn(boxes_xyxy, scores, thresh)`` -> kept
    indices in ascending order (upstream's ``_C.nms`` contract); None: ``structures.boxlist_nms`` (the HIP kernel)."""
    if nms_fn is None:
        return boxlist_nms(boxlist, nms_thresh, max_proposals=limit, score_field="objectness")
    if nms_thresh <= 0:
        return boxlist
    kept = nms_fn(boxlist.bbox, boxlist.get_field("objectness"), nms_thresh)
    return boxlist[kept[:limit] if limit > 0 else kept]


def rpn_proposals_torch(anchors, objectness, box_regression, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size,
                        box_coder, fpn_post_nms_top_n, amodal=False, nms_fn=None):
    """The operator as torch operators on any device (``nms_fn`` None: the HIP NMS kernel, device tensors only): what the
    reference computes (rpn_patch.py:15-60, then upstream's selection over all levels), composed from this package's
    ``BoxList``, ``BoxCoder`` and ``boxlist_nms``.  anchors: per image a list of per-level BoxLists.  Returns one BoxList
    per image; ``tests/golden/rpn_proposals.npz`` pins it to the reference's output bit for bit."""
    num_images, num_levels = len(anchors), len(objectness)
    per_image = [[] for _ in range(num_images)]
    for level in range(num_levels):
        scores, deltas, picked = _level_candidates(objectness[level], box_regression[level],
                                                   [anchors[i][level].bbox for i in range(num_images)], pre_nms_top_n)
        boxes = box_coder.decode(deltas.reshape(-1, 4), picked.reshape(-1, 4)).view(num_images, -1, 4)
        for i in range(num_images):
            found = BoxList(boxes[i], anchors[i][level].size, mode="xyxy")
            found.add_field("objectness", scores[i])
            if not amodal:
                found.clip_to_image(remove_empty=False)          # in place
            per_image[i].append(_suppress(_drop_small(found, min_size), nms_thresh, post_nms_top_n, nms_fn))
    results = []
    for levels in per_image:
        merged = cat_boxlist(levels)
        if num_levels > 1:                                       # (upstream makes no selection with one level)
            scores = merged.get_field("objectness")
            best = scores.topk(min(fpn_post_nms_top_n, len(merged)), dim=0).indices
            merged = merged[best]
        results.append(merged)
    return results


class RPNPostProcessor(torch.nn.Module):
    """Drop-in for the reference's ``RPNPostProcessor`` at inference: ``forward(anchors, objectness, box_regression)``
    -> one ``BoxList`` per image (mode xyxy, the image's size, field ``objectness``).  ``nms_fn``: see
    ``rpn_proposals_torch`` (used by the torch path only)."""

    def __init__(self, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, box_coder=None, fpn_post_nms_top_n=None,
                 fpn_post_nms_per_batch=True, amodal=False, nms_fn=None):
        super(RPNPostProcessor, self).__init__()
        self.pre_nms_top_n = pre_nms_top_n
        self.post_nms_top_n = post_nms_top_n
        self.nms_thresh = nms_thresh
        self.min_size = min_size
        if box_coder is None:
            box_coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
        self.box_coder = box_coder
        if fpn_post_nms_top_n is None:
            fpn_post_nms_top_n = post_nms_top_n
        self.fpn_post_nms_top_n = fpn_post_nms_top_n
        self.fpn_post_nms_per_batch = fpn_post_nms_per_batch     # (training only, as upstream)
        self._amodal = amodal
        self.nms_fn = nms_fn

    def _within_capacity(self, anchors, objectness):
        L, N = len(objectness), len(anchors)
        if not (1 <= N <= ops.RPN_MAX_IMAGES and 1 <= L <= ops.RPN_MAX_LEVELS):
            return False
        if not (1 <= self.pre_nms_top_n <= ops.RPN_MAX_TOP_N and self.post_nms_top_n >= 1 and self.nms_thresh > 0):
            return False
        cap = self.fpn_post_nms_top_n if L > 1 else min(self.post_nms_top_n, self.pre_nms_top_n)
        if not 1 <= cap <= ops.RPN_MAX_TOP_N:
            return False
        if L * min(self.post_nms_top_n, self.pre_nms_top_n) * 4 + 64 > ops.RPN_MERGE_LDS_BYTES:
            return False                                       # (8 levels x 2048 rows: the merge's keys do not fit its LDS)
        if ops.rpn_mask_bytes(N, L, self.pre_nms_top_n) > ops.RPN_MAX_MASK_BYTES:
            return False                                       # (the grow-only workspace would keep hundreds of MB)
        if len({a.bbox.data_ptr() for per_image in anchors for a in per_image}) > ops.RPN_MAX_ANCHOR_TENSORS:
            return False
        return all(a.mode == "xyxy" for per_image in anchors for a in per_image)

    def forward(self, anchors, objectness, box_regression, targets=None):
        if self.training or targets is not None:
            raise NotImplementedError("siammot_amd.rpn.RPNPostProcessor is inference-only (no add_gt_proposals)")
        on_device = all(t.is_cuda for t in objectness)
        if not (on_device and self._within_capacity(anchors, objectness)):
            if on_device:
                ops.FALLBACKS["rpn_torch"] += 1
            return rpn_proposals_torch(anchors, objectness, box_regression, self.pre_nms_top_n, self.post_nms_top_n,
                                       self.nms_thresh, self.min_size, self.box_coder, self.fpn_post_nms_top_n,
                                       self._amodal, self.nms_fn)
        sizes = [per_image[0].size for per_image in anchors]
        boxes, scores, count = ops.rpn_proposals(
            objectness, box_regression, [[a.bbox for a in per_image] for per_image in anchors], sizes, self.pre_nms_top_n,
            self.post_nms_top_n, self.fpn_post_nms_top_n, self.nms_thresh, self.min_size, amodal=self._amodal,
            weights=self.box_coder.weights, xform_clip=self.box_coder.bbox_xform_clip)
        counts = count.cpu().tolist()                          # the call's one device-to-host copy
        return [BoxList._wrap(boxes[i, :c], sizes[i], "xyxy", {"objectness": scores[i, :c]}) for i, c in enumerate(counts)]


def make_rpn_postprocessor(config, rpn_box_coder, is_train):
    """The reference's factory (rpn_patch.py:63-86): same signature, same config keys (the ``_TRAIN`` counts when
    ``is_train``, the ``_TEST`` counts otherwise)."""
    rpn = config.MODEL.RPN
    phase = "TRAIN" if is_train else "TEST"
    return RPNPostProcessor(getattr(rpn, "PRE_NMS_TOP_N_" + phase), getattr(rpn, "POST_NMS_TOP_N_" + phase), rpn.NMS_THRESH,
                            rpn.MIN_SIZE, box_coder=rpn_box_coder,
                            fpn_post_nms_top_n=getattr(rpn, "FPN_POST_NMS_TOP_N_" + phase),
                            fpn_post_nms_per_batch=rpn.FPN_POST_NMS_PER_BATCH, amodal=config.INPUT.AMODAL)
