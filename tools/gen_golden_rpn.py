#!/usr/bin/env python
"""Generate ``tests/golden/rpn_proposals.npz`` with the REFERENCE's own RPN post-processor on the CPU.

Imported UNMODIFIED from the reference checkout ($SIAMMOT_REFERENCE):
    siammot/operator_patch/rpn_patch.py    RPNPostProcessor.forward_for_single_feature_map, make_rpn_postprocessor
Its ``maskrcnn_benchmark`` imports are satisfied by stubs in ``sys.modules``: the oracle's BoxList / cat_boxlist
(oracle/ref_structures.py), the oracle's BoxCoder (oracle/box_head_oracle.py), the numpy NMS (oracle/solver_oracle.py) and
restatements, below, of upstream's ``permute_and_flatten``, ``remove_small_boxes``, ``boxlist_nms`` and of the base class's
``__init__``, ``forward`` and ``select_over_all_levels`` (modeling/rpn/inference.py).

The inputs are ``tests/rpn_proposal_cases.py::golden_inputs(seed)``; seeds are searched upwards from 0 until every case
meets the conditions of ``rpn_proposal_cases.conditions`` (all selected sigmoid values distinct; every IoU of the greedy
chain at least 5e-4 from the threshold; every side at least 1e-2 px from min_size) — conditions on the inputs, asserted here
and again by tests/test_rpn_proposals.py.  Stored: the seed, the inputs (logits fp32, regression values as fp16) and, per
case and image, the reference's boxes and objectness.

Usage:  python tools/gen_golden_rpn.py
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("SIAMMOT_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rpn_proposal_cases as R                                # noqa: E402
from oracle import solver_oracle as SO                        # noqa: E402
from oracle.box_head_oracle import BoxCoder                   # noqa: E402
from oracle.ref_structures import BoxList, cat_boxlist        # noqa: E402


def permute_and_flatten(layer, N, A, C, H, W):
    """[UPSTREAM] modeling/rpn/utils.py."""
    layer = layer.view(N, -1, C, H, W)
    layer = layer.permute(0, 3, 4, 1, 2)
    return layer.reshape(N, -1, C)


def remove_small_boxes(boxlist, min_size):
    """[UPSTREAM] structures/boxlist_ops.py."""
    xywh_boxes = boxlist.convert("xywh").bbox
    _, _, ws, hs = xywh_boxes.unbind(dim=1)
    keep = ((ws >= min_size) & (hs >= min_size)).nonzero().squeeze(1)
    return boxlist[keep]


def boxlist_nms(boxlist, nms_thresh, max_proposals=-1, score_field="scores"):
    """[UPSTREAM] structures/boxlist_ops.py over the numpy NMS."""
    if nms_thresh <= 0:
        return boxlist
    mode = boxlist.mode
    boxlist = boxlist.convert("xyxy")
    keep = SO.nms_indices(boxlist.bbox.numpy(), boxlist.get_field(score_field).numpy(), nms_thresh)
    if max_proposals > 0:
        keep = keep[:max_proposals]
    return boxlist[torch.from_numpy(keep)].convert(mode)


class UpstreamRPNPostProcessor(torch.nn.Module):
    """[UPSTREAM] modeling/rpn/inference.py ``RPNPostProcessor``: what the reference's subclass inherits (inference)."""

    def __init__(self, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, box_coder=None, fpn_post_nms_top_n=None,
                 fpn_post_nms_per_batch=True):
        super(UpstreamRPNPostProcessor, self).__init__()
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
        self.fpn_post_nms_per_batch = fpn_post_nms_per_batch

    def forward(self, anchors, objectness, box_regression, targets=None):
        sampled_boxes = []
        num_levels = len(objectness)
        anchors = list(zip(*anchors))
        for a, o, b in zip(anchors, objectness, box_regression):
            sampled_boxes.append(self.forward_for_single_feature_map(a, o, b))
        boxlists = list(zip(*sampled_boxes))
        boxlists = [cat_boxlist(list(boxlist)) for boxlist in boxlists]
        if num_levels > 1:
            boxlists = self.select_over_all_levels(boxlists)
        assert not (self.training and targets is not None)
        return boxlists

    def select_over_all_levels(self, boxlists):
        num_images = len(boxlists)
        assert not self.training
        for i in range(num_images):
            objectness = boxlists[i].get_field("objectness")
            post_nms_top_n = min(self.fpn_post_nms_top_n, len(objectness))
            _, inds_sorted = torch.topk(objectness, post_nms_top_n, dim=0, sorted=True)
            boxlists[i] = boxlists[i][inds_sorted]
        return boxlists


def install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod("maskrcnn_benchmark")
    mod("maskrcnn_benchmark.structures")
    mod("maskrcnn_benchmark.structures.bounding_box", BoxList=BoxList)
    mod("maskrcnn_benchmark.structures.boxlist_ops", boxlist_nms=boxlist_nms, remove_small_boxes=remove_small_boxes,
        cat_boxlist=cat_boxlist)
    mod("maskrcnn_benchmark.modeling")
    mod("maskrcnn_benchmark.modeling.box_coder", BoxCoder=BoxCoder)
    rpn = mod("maskrcnn_benchmark.modeling.rpn")
    rpn.inference = mod("maskrcnn_benchmark.modeling.rpn.inference", RPNPostProcessor=UpstreamRPNPostProcessor)
    rpn.utils = mod("maskrcnn_benchmark.modeling.rpn.utils", permute_and_flatten=permute_and_flatten)
    sys.path.insert(0, REFERENCE)


def save_npz_stable(path, arrays):
    """``np.savez_compressed`` with the members' timestamps fixed: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def find_seed(anc, limit=2000):
    for seed in range(limit):
        obj, reg = R.golden_inputs(seed)
        cs = {name: R.conditions(obj, reg, anc, case) for name, case in R.GOLDEN_CASES.items()}
        if all(R.conditions_hold(c) for c in cs.values()):
            return seed, obj, reg, cs
    raise SystemExit("no seed below %d meets the conditions: shrink k on the upper levels, not the margins" % limit)


def main():
    install_stubs()
    from siammot.operator_patch import rpn_patch
    torch.set_grad_enabled(False)
    ns = types.SimpleNamespace
    anc = R.anchors()
    seed, obj, reg, cs = find_seed(anc)
    for name, c in cs.items():
        assert R.conditions_hold(c), (name, c)
        print("seed %d, %s: distinct %s, IoU margin %.2e, size margin %.2e" % (seed, name, c["distinct"], c["iou_margin"],
                                                                                c["size_margin"]))
    out = {"seed": np.int64(seed)}
    for l in range(len(obj)):
        out["objectness_%d" % l] = obj[l]
        out["regression_%d" % l] = reg[l].astype(np.float16)
        assert np.array_equal(out["regression_%d" % l].astype(np.float32), reg[l])
    for name, case in R.GOLDEN_CASES.items():
        cfg = ns(INPUT=ns(AMODAL=case["amodal"]),
                 MODEL=ns(RPN=ns(FPN_POST_NMS_TOP_N_TRAIN=2000, FPN_POST_NMS_TOP_N_TEST=case["fpn"], PRE_NMS_TOP_N_TRAIN=2000,
                                 POST_NMS_TOP_N_TRAIN=2000, PRE_NMS_TOP_N_TEST=case["pre"], POST_NMS_TOP_N_TEST=case["post"],
                                 FPN_POST_NMS_PER_BATCH=True, NMS_THRESH=R.NMS_THRESH, MIN_SIZE=case["min_size"])))
        post = rpn_patch.make_rpn_postprocessor(cfg, BoxCoder(weights=R.WEIGHTS), is_train=False).eval()
        N = case["N"]
        boxlists = [[BoxList(torch.from_numpy(a.copy()), R.IMAGE_WH, mode="xyxy") for a in anc] for _ in range(N)]
        res = post(boxlists, [torch.from_numpy(o[:N].copy()) for o in obj], [torch.from_numpy(r[:N].copy()) for r in reg])
        assert len(res) == N
        for i, bl in enumerate(res):
            assert bl.mode == "xyxy" and tuple(bl.size) == tuple(R.IMAGE_WH)
            out["%s/boxes_%d" % (name, i)] = bl.bbox.numpy()
            out["%s/objectness_%d" % (name, i)] = bl.get_field("objectness").numpy()
            print("%s image %d: %d proposals, objectness %.6f..%.6f" % (name, i, len(bl), out["%s/objectness_%d" % (name, i)].min(),
                                                                       out["%s/objectness_%d" % (name, i)].max()))
    path = os.path.join(ROOT, "tests", "golden", "rpn_proposals.npz")
    save_npz_stable(path, out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
