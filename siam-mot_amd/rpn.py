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

The RPN's other two parts are here as well, under upstream's names and ``state_dict`` keys, so that FPN maps go to
proposals without maskrcnn_benchmark's RPN:

* ``RPNHead``: conv3x3 + ReLU and the two 1x1 heads of all images and levels in ONE launch (``ops.rpn_head``, fp32
  matrix cores); CPU tensors, training mode and shapes beyond the kernel's capacities run the ``F.conv2d`` composition
  (``ops.FALLBACKS["rpn_head_torch"]`` counts those calls on device tensors);
* ``AnchorGenerator``: upstream's cell anchors (``generate_anchors``, numpy's half-to-even rounding) as buffers
  ``cell_anchors.{l}``, the grid of all levels in one launch (``ops.rpn_anchors``), cached per map sizes and device: ONE
  tensor per level shared by the images of a call.  The ``visibility`` field is NOT produced (inference never reads it);
* ``RPNModule``: ``anchor_generator``, ``head`` and ``box_selector_test`` under upstream's attribute names, inference only.
"""
import numpy as np
import torch
import torch.nn.functional as F

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


# ---- cell anchors: [UPSTREAM] modeling/rpn/anchor_generator.py generate_anchors, in numpy float64 as there ----------------
def _whctrs(anchor):
    w = anchor[2] - anchor[0] + 1
    h = anchor[3] - anchor[1] + 1
    return w, h, anchor[0] + 0.5 * (w - 1), anchor[1] + 0.5 * (h - 1)


def _mkanchors(ws, hs, x_ctr, y_ctr):
    ws, hs = ws[:, np.newaxis], hs[:, np.newaxis]
    return np.hstack((x_ctr - 0.5 * (ws - 1), y_ctr - 0.5 * (hs - 1), x_ctr + 0.5 * (ws - 1), y_ctr + 0.5 * (hs - 1)))


def generate_anchors(stride=16, sizes=(32, 64, 128, 256, 512), aspect_ratios=(0.5, 1, 2)):
    """``[len(aspect_ratios) * len(sizes), 4]`` float64 xyxy anchors around the cell (0, 0, stride - 1, stride - 1), ratio-major:
    per ratio ``ws = np.round(sqrt(stride^2 / ratio))``, ``hs = np.round(ws * ratio)`` (``np.round``: half to even —
    22.5 -> 22), then scaled by ``size / stride`` about the cell's centre."""
    scales = np.array(sizes, dtype=np.float64) / stride
    ratios = np.array(aspect_ratios, dtype=np.float64)
    w, h, x_ctr, y_ctr = _whctrs(np.array([1, 1, stride, stride], dtype=np.float64) - 1)
    ws = np.round(np.sqrt(w * h / ratios))
    hs = np.round(ws * ratios)
    per_ratio = _mkanchors(ws, hs, x_ctr, y_ctr)
    rows = []
    for i in range(per_ratio.shape[0]):
        w, h, x_ctr, y_ctr = _whctrs(per_ratio[i, :])
        rows.append(_mkanchors(w * scales, h * scales, x_ctr, y_ctr))
    return torch.from_numpy(np.vstack(rows))


def grid_anchors_torch(cell_anchors, strides, grid_sizes):
    """Upstream's ``grid_anchors``: per level ``(shifts.view(-1, 1, 4) + cell.view(1, -1, 4)).reshape(-1, 4)`` in fp32, rows in
    the order (h*W + w)*A + a."""
    out = []
    for (gh, gw), stride, base in zip(grid_sizes, strides, cell_anchors):
        sx = torch.arange(0, gw * stride, step=stride, dtype=torch.float32, device=base.device)
        sy = torch.arange(0, gh * stride, step=stride, dtype=torch.float32, device=base.device)
        sy, sx = torch.meshgrid(sy, sx, indexing="ij")
        sx, sy = sx.reshape(-1), sy.reshape(-1)
        shifts = torch.stack((sx, sy, sx, sy), dim=1)
        out.append((shifts.view(-1, 1, 4) + base.view(1, -1, 4)).reshape(-1, 4))
    return out


class BufferList(torch.nn.Module):
    """Upstream's ``BufferList``: tensors registered as buffers ``"0"``, ``"1"``, ... (keys ``cell_anchors.{l}``)."""

    def __init__(self, buffers=()):
        super(BufferList, self).__init__()
        for i, b in enumerate(buffers):
            self.register_buffer(str(i), b)

    def __len__(self):
        return len(self._buffers)

    def __iter__(self):
        return iter(self._buffers.values())


class AnchorGenerator(torch.nn.Module):
    """Upstream's ``AnchorGenerator`` at inference.  ``forward(image_sizes, feature_maps)`` -> per image a list of per-level
    ``BoxList``s (mode xyxy, no ``visibility`` field: ``straddle_thresh`` is kept for the signature only).  image_sizes: an
    upstream ``ImageList`` (its ``image_sizes`` are (height, width)) or a sequence of this package's ``BoxList.size`` pairs
    (width, height).  On the device the grids of all levels are one launch and are cached per (map sizes, device): every image of
    every later call with these sizes gets the SAME tensor per level."""
    _CACHE_ENTRIES = 8

    def __init__(self, sizes=(128, 256, 512), aspect_ratios=(0.5, 1.0, 2.0), anchor_strides=(8, 16, 32), straddle_thresh=0):
        super(AnchorGenerator, self).__init__()
        if len(anchor_strides) == 1:
            cells = [generate_anchors(anchor_strides[0], sizes, aspect_ratios).float()]
        else:
            if len(anchor_strides) != len(sizes):
                raise RuntimeError("FPN should have #anchor_strides == #sizes")
            cells = [generate_anchors(stride, size if isinstance(size, (tuple, list)) else (size,), aspect_ratios).float()
                     for stride, size in zip(anchor_strides, sizes)]
        self.strides = tuple(int(s) for s in anchor_strides)
        self.cell_anchors = BufferList(cells)
        self.straddle_thresh = straddle_thresh
        self._grids = {}

    def num_anchors_per_location(self):
        return [len(c) for c in self.cell_anchors]

    def grid_anchors(self, grid_sizes):
        """One ``[H_l*W_l*A_l, 4]`` fp32 tensor per level, on the cell anchors' device."""
        cells = list(self.cell_anchors)
        if len(grid_sizes) != len(cells):
            raise RuntimeError("AnchorGenerator: %d feature maps for %d anchor levels" % (len(grid_sizes), len(cells)))
        if not cells[0].is_cuda:
            return grid_anchors_torch(cells, self.strides, grid_sizes)
        key = (tuple(grid_sizes), cells[0].device, tuple((c.data_ptr(), c._version) for c in cells))
        hit = self._grids.get(key)
        if hit is None:
            if len(self._grids) >= self._CACHE_ENTRIES:
                self._grids.clear()
            # (computed on the current stream, ordered for every other one: an event wait on the device, no host synchronisation)
            hit = self._grids[key] = ops.StreamImage(lambda: ops.rpn_anchors(cells, self.strides, grid_sizes), cells[0].device)
        return hit.get()

    def forward(self, image_sizes, feature_maps):
        grid_sizes = [(int(f.shape[-2]), int(f.shape[-1])) for f in feature_maps]
        levels = self.grid_anchors(grid_sizes)
        if hasattr(image_sizes, "image_sizes"):
            image_sizes = [(w, h) for (h, w) in image_sizes.image_sizes]
        return [[BoxList._wrap(a, tuple(size), "xyxy", {}) for a in levels] for size in image_sizes]


def make_anchor_generator(config):
    """Upstream's factory: ``MODEL.RPN.ANCHOR_SIZES`` / ``ASPECT_RATIOS`` / ``ANCHOR_STRIDE`` / ``STRADDLE_THRESH``."""
    rpn = config.MODEL.RPN
    return AnchorGenerator(tuple(rpn.ANCHOR_SIZES), tuple(rpn.ASPECT_RATIOS), tuple(rpn.ANCHOR_STRIDE), rpn.STRADDLE_THRESH)


def rpn_head_torch(features, conv_w, conv_b, cls_w, cls_b, bbox_w, bbox_b):
    """The head as torch operators on any device (half maps are upcast first, as the kernel converts on load)."""
    objectness, regression = [], []
    for x in features:
        t = F.relu(F.conv2d(x.to(conv_w.dtype), conv_w, conv_b, stride=1, padding=1))
        objectness.append(F.conv2d(t, cls_w, cls_b))
        regression.append(F.conv2d(t, bbox_w, bbox_b))
    return objectness, regression


class RPNHead(torch.nn.Module):
    """Upstream's ``RPNHead`` (``@registry.RPN_HEADS.register("SingleConvRPNHead")``): parameters ``conv`` (3x3, C -> C),
    ``cls_logits`` (1x1, C -> A), ``bbox_pred`` (1x1, C -> 4A), normal(std 0.01) weights, zero biases.
    ``forward(features) -> (objectness list, regression list)``.  In eval mode on device maps within ``ops.rpn_head``'s
    capacities: one launch for all images and levels; the packed weights are rebuilt when a parameter's ``_version``, storage
    or device changes.  ``compute_dtype`` (keyword-only): None (the default: nothing changes), ``torch.float16`` or
    ``torch.bfloat16``: the half compute mode (``ops.rpn_head_half``) — the 3x3 convolution multiplies
    the maps and ``conv.weight`` rounded to that type with fp32 accumulation; the two 1x1 heads stay fp32.  CPU tensors and
    every fallback give the bits of the fp32 mode; the ``state_dict`` is the same."""

    def __init__(self, cfg, in_channels, num_anchors, *, compute_dtype=None):
        super(RPNHead, self).__init__()
        if compute_dtype is not None and compute_dtype not in ops.DLA_COMPUTE_TYPES:
            raise ValueError("RPNHead: compute_dtype must be None, torch.float16 or torch.bfloat16, got %r" % (compute_dtype,))
        self.compute_dtype = compute_dtype
        self.conv = torch.nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)
        self.cls_logits = torch.nn.Conv2d(in_channels, num_anchors, kernel_size=1, stride=1)
        self.bbox_pred = torch.nn.Conv2d(in_channels, num_anchors * 4, kernel_size=1, stride=1)
        for layer in (self.conv, self.cls_logits, self.bbox_pred):
            torch.nn.init.normal_(layer.weight, std=0.01)
            torch.nn.init.constant_(layer.bias, 0)
        self.in_channels, self.num_anchors = int(in_channels), int(num_anchors)
        self._packed_key, self._packed = None, None

    def _params(self):
        return (self.conv.weight, self.conv.bias, self.cls_logits.weight, self.cls_logits.bias, self.bbox_pred.weight,
                self.bbox_pred.bias)

    def kernel_ok(self, features):
        """This call takes ``ops.rpn_head``."""
        if self.training or not (1 <= len(features) <= ops.RPN_MAX_LEVELS):
            return False
        dev, dt = features[0].device, features[0].dtype
        if not all(isinstance(f, torch.Tensor) and f.is_cuda and f.dim() == 4 and f.device == dev and f.dtype is dt
                   for f in features):
            return False
        if dt not in ops.FEAT_TYPES or not all(p.dtype is torch.float32 and p.device == dev for p in self._params()):
            return False
        N = features[0].shape[0]
        if not (1 <= N <= ops.RPN_MAX_IMAGES and all(f.shape[0] == N and f.shape[1] == self.in_channels and f.numel() > 0
                                                     for f in features)):
            return False
        return ops.rpn_head_shapes_ok(self.in_channels, self.num_anchors)

    def packed(self):
        """The packed weights for a launch on the current stream: packed on the stream of the first call after a change and
        ordered for every other stream by ``ops.StreamImage`` (an event wait on the device, no host synchronisation)."""
        params = self._params()
        key = (self.compute_dtype,) + tuple((p.data_ptr(), p._version, p.device) for p in params)
        if key != self._packed_key:
            tensors = [p.detach() for p in params]
            if self.compute_dtype is not None:
                self._packed = ops.StreamImage(lambda: ops.rpn_head_half_pack(*tensors, self.compute_dtype), params[0].device)
            else:
                self._packed = ops.StreamImage(lambda: ops.rpn_head_pack(*tensors), params[0].device)
            self._packed_key = key
        return self._packed.get()

    def forward(self, features):
        features = list(features)
        if self.kernel_ok(features):
            if self.compute_dtype is not None:
                return ops.rpn_head_half(features, self.packed(), self.in_channels, self.num_anchors, self.compute_dtype)
            return ops.rpn_head(features, self.packed(), self.in_channels, self.num_anchors)
        if any(isinstance(f, torch.Tensor) and f.is_cuda for f in features):
            ops.FALLBACKS["rpn_head_torch"] += 1
        return rpn_head_torch(features, *self._params())


class RPNModule(torch.nn.Module):
    """Upstream's ``RPNModule`` at inference: FPN maps -> proposals.  ``forward(images_or_sizes, features)`` -> one ``BoxList``
    per image (field ``objectness``); images_or_sizes as ``AnchorGenerator.forward`` takes them.  ``state_dict`` keys are those
    of ``rpn.*`` in a reference checkpoint (``anchor_generator.cell_anchors.{l}``, ``head.conv.*``, ``head.cls_logits.*``,
    ``head.bbox_pred.*``).  ``compute_dtype`` (keyword-only): the head's half compute mode (``RPNHead``)."""

    def __init__(self, cfg, in_channels, *, compute_dtype=None):
        super(RPNModule, self).__init__()
        self.anchor_generator = make_anchor_generator(cfg)
        self.head = RPNHead(cfg, in_channels, self.anchor_generator.num_anchors_per_location()[0], compute_dtype=compute_dtype)
        self.box_selector_test = make_rpn_postprocessor(cfg, BoxCoder(weights=(1.0, 1.0, 1.0, 1.0)), is_train=False)

    def forward(self, images_or_sizes, features, targets=None):
        if self.training or targets is not None:
            raise NotImplementedError("siammot_amd.rpn.RPNModule is an inference path")
        with torch.no_grad():
            objectness, regression = self.head(features)
            anchors = self.anchor_generator(images_or_sizes, features)
            return self.box_selector_test(anchors, objectness, regression)
