"""Box head on the RPN's proposals: the torch composition a user paid until now against the device path.

    python tools/box_detect_bench.py [--steps K] [--warmup W] [--out profiles/box_detect_bench.json] [--no-launch-count]

Inputs: the headline maps (704 x 1280 input, C = 128, strides 4..32 for the pooler, five RPN levels, A = 3, 1000 / 300 /
300, RPN threshold 0.7), the yaml's box head (7 x 7 pooler, 1024-1024 MLP) with K = 2 and K = 3 classes, the 300 proposals
the RPN module selects.  Forms, timed in ONE process and interleaved (A B C D A B C D ...) so that clock drift favours none:

    A  the box head as the parent commit runs it on id-less proposals: pooler, ``nn.Linear`` layers and
       ``PostProcessor.filter_results`` as torch operators (a nonzero, gathers, an argsort and an NMS launch per class);
    B  ``TrackBoxHead.forward`` on the same proposals: pooler, library GEMMs, ``ops.box_detect_post`` (four launches), one
       device-to-host copy;
    C  ``RPNPostProcessor.forward`` followed by ``TrackBoxHead.forward`` (two device-to-host copies); ``C_parent``: followed
       by form A;
    D  ``DetectionHead.forward``: the same chain with one device-to-host copy.

Timed with device events around a loop (every form synchronises inside a step); the steps of a form are split over
``REPEATS`` interleaved repeats and ``*_spread_us`` is the spread (max - min) of a form's per-call time over them.
Synchronisations per call are counted with torch's sync debug mode (as tests/test_video_results.py counts them), device
work per call as the torch operators the dispatcher runs plus the library entries called (``count_launches``).  The tool
reports; it exits non-zero only if B is slower than A, or D slower than C_parent, by more than the baseline's spread.
"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from multi_image_bench import time_loop  # noqa: E402
from rpn_proposals_bench import NET_HW, STRIDES, make_case  # noqa: E402

REPEATS = 4
CHANNELS = 128


def make_heads(K, dev):
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.config import get_default_cfg
    from siammot_amd.detector import build_detection_head
    cfg = get_default_cfg(channels=CHANNELS)
    cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES = K
    torch.manual_seed(K)
    det = build_detection_head(cfg, BoxCoder((1.0, 1.0, 1.0, 1.0)), CHANNELS).to(dev).eval()
    with torch.no_grad():
        det.box_head.predictor.cls_score.weight.mul_(6.0)       # scores spread over (0, 1): the threshold and the NMS both act
        det.box_head.predictor.bbox_pred.weight.mul_(0.1)
    return det


def parent_forward(head, features, proposals):
    """``TrackBoxHead.forward`` as it was before the device path: the reference's torch composition."""
    x = head.feature_extractor(features, proposals)
    return x, head.post_processor(head.predictor(x), proposals), {}


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
        return len([x for x in w if "synchroniz" in str(x.message).lower()])
    finally:
        torch.cuda.set_sync_debug_mode("default")


def count_launches(fn):
    """(torch operators that enqueue device work, {library entry: calls}) of one call.  A torch operator is counted when
    the dispatcher runs it and it is no view / metadata operator — each is at least one kernel launch or copy; the
    library's entries enqueue a fixed number each (box_detect_post 4, rpn_proposals 9 + a memset, nms 2, roi_align_levels
    1, linear_rows 2)."""
    from torch.utils._python_dispatch import TorchDispatchMode
    import siammot_amd.ops as ops
    views = ("view", "reshape", "expand", "slice", "select", "transpose", "permute", "squeeze", "unsqueeze", "alias",
             "detach", "as_strided", "t.default", "unbind", "split", "_unsafe_view", "size", "stride", "is_", "sym_",
             "_local_scalar_dense", "unfold", "lift_fresh", "_to_copy.default_cpu")
    n = [0]

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func).replace("aten.", "")
            if not any(name.startswith(v) for v in views):
                n[0] += 1
            return func(*args, **(kwargs or {}))
    lib = ops.load_library()
    calls, saved = {}, {}
    for name in ops.EXPORTED_SYMBOLS:
        if not name.endswith("_fwd"):
            continue
        f = getattr(lib, name)
        saved[name] = f

        def wrapped(*a, _f=f, _n=name):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a)
        setattr(lib, name, wrapped)
    try:
        with Count():
            fn()
    finally:
        for name, f in saved.items():
            setattr(lib, name, f)
    torch.cuda.synchronize()
    return n[0], calls


def run_case(K, steps, warmup, dev, launch_count):
    det = make_heads(K, dev)
    head, rpn = det.box_head, det.rpn_post
    anchors, sets = make_case(1, dev)
    g = torch.Generator().manual_seed(5)
    feats = [tuple(torch.randn((1, CHANNELS, NET_HW[0] // s, NET_HW[1] // s), generator=g).to(dev) for s in STRIDES)
             for _ in range(2)]
    with torch.no_grad():
        props = [rpn(anchors, *sets[k]) for k in range(2)]
    forms = {
        "A_torch_box_head": lambda k: parent_forward(head, feats[k & 1], props[k & 1]),
        "B_device_box_head": lambda k: head(feats[k & 1], props[k & 1]),
        "C_rpn_then_box_head": lambda k: head(feats[k & 1], rpn(anchors, *sets[k & 1])),
        "C_parent_rpn_then_torch_box_head": lambda k: parent_forward(head, feats[k & 1], rpn(anchors, *sets[k & 1])),
        "D_detection_head": lambda k: det(anchors, sets[k & 1][0], sets[k & 1][1], feats[k & 1]),
    }
    out = {"num_classes": K, "net_hw": list(NET_HW), "channels": CHANNELS, "proposals": [len(p[0]) for p in props],
           "steps": steps}
    per = {f: [] for f in forms}
    host = {f: 0.0 for f in forms}
    part = max(steps // REPEATS, 1)
    for _ in range(REPEATS):
        for f, step in forms.items():
            gpu_s, host_s = time_loop(step, part, warmup)
            per[f].append(gpu_s / part * 1e6)
            host[f] += host_s
    for f in forms:
        out[f] = {"us_per_call": sum(per[f]) / REPEATS, "us_per_call_repeats": per[f], "spread_us": max(per[f]) - min(per[f]),
                  "host_enqueue_us_per_call": host[f] / (REPEATS * part) * 1e6}
        with torch.no_grad():
            out[f]["synchronisations_per_call"] = count_syncs(lambda: forms[f](0))
            if launch_count:
                n_ops, calls = count_launches(lambda: forms[f](0))
                out[f]["torch_operators_per_call"], out[f]["library_calls_per_call"] = n_ops, calls
    us = lambda f: out[f]["us_per_call"]
    out["A_over_B_time"] = us("A_torch_box_head") / us("B_device_box_head")
    out["C_parent_over_D_time"] = us("C_parent_rpn_then_torch_box_head") / us("D_detection_head")
    out["C_over_D_time"] = us("C_rpn_then_box_head") / us("D_detection_head")
    out["B_not_slower_than_A"] = bool(us("B_device_box_head") <= us("A_torch_box_head") + out["A_torch_box_head"]["spread_us"])
    out["D_not_slower_than_C_parent"] = bool(us("D_detection_head") <= us("C_parent_rpn_then_torch_box_head")
                                             + out["C_parent_rpn_then_torch_box_head"]["spread_us"])
    with torch.no_grad():
        a, b, d = forms["A_torch_box_head"](0)[1][0], forms["B_device_box_head"](0)[1][0], forms["D_detection_head"](0)[0]
    out["detections"] = {"A": len(a), "B": len(b), "D": len(d)}
    if len(a) == len(b) and len(a):
        out["A_B_same_labels"] = bool((a.get_field("labels") == b.get_field("labels")).all())
        out["A_B_max_box_difference_px"] = float((a.bbox - b.bbox).abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--no-launch-count", action="store_true", help="skip the launch count")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    results = []
    for K in (2, 3):
        r = run_case(K, args.steps, args.warmup, dev, not args.no_launch_count)
        results.append(r)
        print(json.dumps(r), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    slower = [r["num_classes"] for r in results if not (r["B_not_slower_than_A"] and r["D_not_slower_than_C_parent"])]
    if slower:
        print("SLOWER: the device path is slower than the torch path at K = %s" % (slower,), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
