"""Anchors to detections for B cameras: ``DetectionHead`` called image by image against one batched call.

    python tools/detection_batch_bench.py [--steps K] [--warmup W] [--out profiles/detection_batch_bench.json]

Inputs: those of tools/box_detect_bench.py — the headline maps (704 x 1280 input, C = 128, strides 4..32 for the pooler, five
RPN levels, A = 3, 1000 / 300 / 300, RPN threshold 0.7), the yaml's box head (7 x 7 pooler, 1024-1024 MLP) with K = 2 — for
B = 1, 2 and 4 images with different contents.  Forms, timed in ONE process and interleaved (A B A B ...):

    A  ``DetectionHead.forward`` on each image in turn (what a caller with B cameras had to do before the box head took
       several images): B calls, B device-to-host copies, B serial NMS scans;
    B  one ``DetectionHead.forward`` on the B images: the same number of launches as one image, one device-to-host copy.

At B = 1 the two forms are the same code path and measure the spread.  Timed with device events around a loop (every form
synchronises inside a step); the steps of a form are split over ``REPEATS`` interleaved repeats and ``spread_us`` is the
spread (max - min) of its per-call time over them.  Host copies per call are counted with torch's sync debug mode, the
library's entries per call by wrapping them (box_detect_bench.count_launches).  The tool reports; it sets no ratio.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from box_detect_bench import CHANNELS, count_launches, count_syncs, make_heads  # noqa: E402
from multi_image_bench import time_loop  # noqa: E402
from rpn_proposals_bench import NET_HW, STRIDES, make_case  # noqa: E402

REPEATS = 4
NUM_CLASSES = 2


def run_case(B, steps, warmup, dev, launch_count):
    det = make_heads(NUM_CLASSES, dev)
    anchors, sets = make_case(B, dev)
    g = torch.Generator().manual_seed(5)
    feats = [tuple(torch.randn((B, CHANNELS, NET_HW[0] // s, NET_HW[1] // s), generator=g).to(dev) for s in STRIDES)
             for _ in range(2)]
    # the views of one image, made once: slicing is no part of either form
    one = [[([anchors[b]], [o[b:b + 1] for o in sets[k][0]], [r[b:b + 1] for r in sets[k][1]], tuple(f[b:b + 1] for f in feats[k]))
            for b in range(B)] for k in range(2)]

    def image_by_image(k):
        return [det(*one[k & 1][b])[0] for b in range(B)]

    def batched(k):
        return det(anchors, sets[k & 1][0], sets[k & 1][1], feats[k & 1])
    forms = {"A_image_by_image": image_by_image, "B_one_batched_call": batched}
    out = {"images": B, "num_classes": NUM_CLASSES, "net_hw": list(NET_HW), "channels": CHANNELS, "steps": steps}
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
                  "us_per_image": sum(per[f]) / REPEATS / B,
                  "host_enqueue_us_per_call": host[f] / (REPEATS * part) * 1e6}
        with torch.no_grad():
            out[f]["host_copies_per_call"] = count_syncs(lambda: forms[f](0))
            if launch_count:
                n_ops, calls = count_launches(lambda: forms[f](0))
                out[f]["torch_operators_per_call"], out[f]["library_calls_per_call"] = n_ops, calls
    out["A_over_B_time"] = out["A_image_by_image"]["us_per_call"] / out["B_one_batched_call"]["us_per_call"]
    with torch.no_grad():
        a, b = image_by_image(0), batched(0)
    out["detections"] = {"A": [len(x) for x in a], "B": [len(x) for x in b]}
    same = [len(x) == len(y) and bool((x.get_field("labels") == y.get_field("labels")).all()) for x, y in zip(a, b)]
    out["A_B_same_labels"] = all(same)
    if all(same):
        out["A_B_max_box_difference_px"] = max([float((x.bbox - y.bbox).abs().max()) for x, y in zip(a, b) if len(x)] or [0.0])
        out["A_B_max_score_difference"] = max([float((x.get_field("scores") - y.get_field("scores")).abs().max())
                                               for x, y in zip(a, b) if len(x)] or [0.0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--images", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--no-launch-count", action="store_true", help="skip the launch count")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    results = []
    for B in args.images:
        r = run_case(B, args.steps, args.warmup, dev, not args.no_launch_count)
        results.append(r)
        print(json.dumps(r), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
