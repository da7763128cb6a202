"""Anchors to detections with one device-to-host copy: the RPN's proposal selection and the box head behind one call.

``RPNPostProcessor.forward`` (rpn.py) and ``TrackBoxHead.forward`` (box_refine.py) each read one count back: the number of
proposals, then the number of detections.  ``DetectionHead`` hands the RPN's padded proposals and their device-resident
count straight to the box head (``ops.rpn_proposals`` in raw form -> ``TrackBoxHead.detect_raw``), so only the detection
count crosses to the host — and the result is the BoxList ``TrackingLoop.forward(features, detections)`` takes.

Several images of one size per call (``features[l]`` = ``[N, C, H_l, W_l]``) take the same launches: the RPN's ``boxes [N,
cap, 4]`` and ``count [N]`` go to ``TrackBoxHead.detect_raw_batched`` as they are and the N detection counts are the call's
one copy.  When either half is over its capacity or not on the device, or the images differ in size, the two modules'
``forward``s are composed as they are today.

``forward_features(features, image_size)`` starts one step earlier, at the FPN maps: the RPN head's convolutions
(``rpn.RPNHead``: one launch for all images and levels), the cached anchor grid (``rpn.AnchorGenerator``: no launch once the
map sizes have been seen) and then ``forward`` — still the one copy.

``forward_stages(stages, image_size)`` starts at the backbone's stage maps: the pyramid (``fpn.FPN``: L + 1 launches, no
synchronisation) and then ``forward_features``; the FPN maps are handed back with the detections for the tracker.

``forward_images(images, image_size)`` starts at the pre-processed frames: the backbone body (``dla.DLA``: 37 launches for
DLA-34, no synchronisation) and then ``forward_stages`` — frames to detections on this package's kernels, still the one copy.
"""
import torch

from . import ops
from .box_refine import TrackBoxHead
from .backbone import build_backbone
from .fpn import build_fpn
from .rpn import RPNHead, make_anchor_generator, make_rpn_postprocessor


class DetectionHead(torch.nn.Module):
    """``forward(anchors, objectness, box_regression, features) -> [BoxList]`` per image (fields ``scores``, ``ids`` = -1,
    ``labels``): ``rpn_post`` is an ``rpn.RPNPostProcessor``, ``box_head`` a ``TrackBoxHead``.  With an ``rpn.RPNHead`` and an
    ``rpn.AnchorGenerator`` as well: ``forward_features(features, image_size)``, the same from the FPN maps; with an
    ``fpn.FPN`` too: ``forward_stages(stages, image_size)``, the same from the backbone's stage maps; with a ``backbone``
    (``backbone.build_backbone``: ``body`` and ``fpn``) instead of the ``fpn``: ``forward_images(images, image_size)``."""

    def __init__(self, rpn_post, box_head, rpn_head=None, anchor_generator=None, fpn=None, backbone=None):
        super(DetectionHead, self).__init__()
        self.rpn_post = rpn_post
        self.box_head = box_head
        self.rpn_head = rpn_head
        self.anchor_generator = anchor_generator
        self.fpn = fpn
        self.backbone = backbone

    def _pyramid(self):
        return self.fpn if self.fpn is not None else getattr(self.backbone, "fpn", None)

    def raw_ok(self, anchors, objectness):
        """Both halves take their device paths for this call."""
        rpn, box = self.rpn_post, self.box_head
        N = len(anchors)
        if N < 1 or not all(t.is_cuda for t in objectness):
            return False
        if not (hasattr(rpn, "_within_capacity") and rpn._within_capacity(anchors, objectness)):
            return False
        cap = rpn.fpn_post_nms_top_n if len(objectness) > 1 else min(rpn.post_nms_top_n, rpn.pre_nms_top_n)
        if N == 1:
            return hasattr(box, "detect_shapes_ok") and box.detect_shapes_ok(cap)
        size = tuple(anchors[0][0].size)                       # (one clip for the box head's batched launches)
        return (all(tuple(per_image[0].size) == size for per_image in anchors)
                and hasattr(box, "detect_shapes_ok_batched") and box.detect_shapes_ok_batched([cap] * N))

    @torch.no_grad()
    def forward(self, anchors, objectness, box_regression, features):
        if self.training:
            raise NotImplementedError("siammot_amd.detector.DetectionHead is an inference path")
        rpn, box = self.rpn_post, self.box_head
        if not self.raw_ok(anchors, objectness):
            proposals = rpn(anchors, objectness, box_regression)
            return box(features, proposals)[1]
        size, N = anchors[0][0].size, len(anchors)
        boxes, _, count = ops.rpn_proposals(
            objectness, box_regression, [[a.bbox for a in per_image] for per_image in anchors], [size] * N,
            rpn.pre_nms_top_n, rpn.post_nms_top_n, rpn.fpn_post_nms_top_n, rpn.nms_thresh, rpn.min_size, amodal=rpn._amodal,
            weights=rpn.box_coder.weights, xform_clip=rpn.box_coder.bbox_xform_clip)
        if N == 1:
            det_boxes, scores, labels, _, out_count, _, _ = box.detect_raw(features, boxes[0], count[0:1], size)
            return [box.wrap_detections(det_boxes, scores, labels, out_count, size)]   # the call's one device-to-host copy
        rows = [boxes.shape[1]] * N
        det_boxes, scores, labels, _, out_count, _, _ = box.detect_raw_batched(features, boxes.view(-1, 4), rows, count, size)
        return box.wrap_detections_batched(det_boxes, scores, labels, out_count, rows, size)   # the one copy: N counts

    @torch.no_grad()
    def forward_features(self, features, image_size):
        """FPN maps ``features[l]`` = ``[N, C, H_l, W_l]`` of N images of one size ``image_size`` = (width, height) ->
        what ``forward(anchor_generator(...), *rpn_head(features), features)`` returns, bit for bit."""
        if self.rpn_head is None or self.anchor_generator is None:
            raise RuntimeError("siammot_amd.detector.DetectionHead: forward_features needs an RPN head and an anchor generator "
                               "(build_detection_head(..., rpn_head=True))")
        if self.training:
            raise NotImplementedError("siammot_amd.detector.DetectionHead is an inference path")
        objectness, box_regression = self.rpn_head(features)
        anchors = self.anchor_generator([tuple(image_size)] * int(features[0].shape[0]), features)
        return self.forward(anchors, objectness, box_regression, features)

    @torch.no_grad()
    def forward_stages(self, stages, image_size):
        """Backbone stage maps ``stages[l]`` = ``[N, Cin_l, H_l, W_l]`` of N images of one size -> ``(features, detections)``:
        ``features = fpn(stages)`` and ``forward_features(features, image_size)``, bit for bit."""
        fpn = self._pyramid()
        if fpn is None:
            raise RuntimeError("siammot_amd.detector.DetectionHead: forward_stages needs an FPN "
                               "(build_detection_head(..., fpn=True))")
        if self.training:
            raise NotImplementedError("siammot_amd.detector.DetectionHead is an inference path")
        features = fpn(stages)
        return features, self.forward_features(features, image_size)

    @torch.no_grad()
    def forward_images(self, images, image_size):
        """Pre-processed frames ``images`` = ``[N, 3, H, W]`` (``FramePreprocessor.batch``; H and W multiples of 32) of N
        images of one size -> ``(features, detections)``: ``forward_stages(backbone.body(images), image_size)``, bit for bit."""
        if self.backbone is None:
            raise RuntimeError("siammot_amd.detector.DetectionHead: forward_images needs a backbone "
                               "(build_detection_head(..., backbone=True))")
        if self.training:
            raise NotImplementedError("siammot_amd.detector.DetectionHead is an inference path")
        return self.forward_stages(self.backbone.body(images), image_size)


def build_detection_head(cfg, rpn_box_coder, in_channels, box_head=None, rpn_head=True, fpn=False, backbone=False,
                         compute_dtype=None, half_storage=False):
    """``DetectionHead`` from a config: the reference's RPN factory keys (``MODEL.RPN.*_TEST``) and the given box head or a
    fresh ``TrackBoxHead``.  ``rpn_head``: True for a fresh ``rpn.RPNHead`` and the config's anchor generator
    (``MODEL.RPN.ANCHOR_*``, ``ASPECT_RATIOS``), an ``RPNHead`` to use that one, False / None for a head that starts at the
    anchors (``forward`` only).  ``fpn``: True for the config's pyramid (``fpn.build_fpn``), an ``fpn.FPN`` to use that one,
    False / None for a head that starts at the FPN maps.  ``backbone``: True for the config's body and pyramid
    (``backbone.build_backbone``; it brings the pyramid, so ``fpn`` is not passed with it), a module with ``body`` and ``fpn``
    to use that one.  ``compute_dtype``: None, ``torch.float16`` or ``torch.bfloat16``: the half compute mode of whatever
    this builder creates itself — the fresh ``RPNHead``, ``build_fpn``'s pyramid, ``build_backbone``'s body and pyramid
    (INTEGRATION.md §3q); modules passed in are left as they are.  ``half_storage``: handed to the ``build_backbone`` this
    builder creates itself (the body's maps between layers in ``compute_dtype``)."""
    if box_head is None:
        box_head = TrackBoxHead(cfg, in_channels).eval()
    head, generator = None, None
    if rpn_head:
        generator = make_anchor_generator(cfg)
        head = (RPNHead(cfg, in_channels, generator.num_anchors_per_location()[0], compute_dtype=compute_dtype)
                if rpn_head is True else rpn_head)
    if backbone and fpn:
        raise ValueError("build_detection_head: a backbone brings its pyramid; pass `backbone` or `fpn`, not both")
    pyramid = (build_fpn(cfg, compute_dtype=compute_dtype) if fpn is True else fpn) if fpn else None
    trunk = ((build_backbone(cfg, compute_dtype=compute_dtype, fpn_compute_dtype=compute_dtype, half_storage=half_storage)
              if backbone is True else backbone) if backbone else None)
    return DetectionHead(make_rpn_postprocessor(cfg, rpn_box_coder, is_train=False).eval(), box_head, head, generator,
                         pyramid, trunk).eval()
