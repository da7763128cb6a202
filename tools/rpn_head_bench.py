"""RPN head: the ``F.conv2d`` composition on the device against the fused HIP kernel, and FPN maps to detections with and
without ``DetectionHead.forward_features``.

    python tools/rpn_head_bench.py [--steps K] [--warmup W] [--out profiles/rpn_head_bench.json] [--quick] [--forms AB]

Head cases: the headline maps (704 x 1280 input, five levels of strides 4..64, C = 128, A = 3) with 1 and with 4 images,
fp32 and fp16 maps.  One step = the head on all images and levels.  Forms, timed in ONE process, interleaved (A B A B ...)
so that clock drift favours neither:

    A  ``siammot_amd.rpn.rpn_head_torch``: conv3x3 + ReLU + two conv1x1 per level as torch operators (MIOpen / rocBLAS),
       half maps upcast first — the arithmetic of B;
    H  (fp16 maps only) the same composition with the weights cast to fp16: what an all-half pipeline would run, other
       arithmetic (fp16 products and outputs);
    B  ``siammot_amd.rpn.RPNHead.forward``: one launch (csrc/rpn_head.hip).

Detection cases (one image and four, fp32 maps): maps -> detections,

    A  the head's torch composition, upstream's anchor grid rebuilt by torch operators, then ``DetectionHead.forward``;
    B  ``DetectionHead.forward_features``.

Timed with device events around a loop; the K steps of a form are split over ``REPEATS`` interleaved repeats and
``A_spread_us`` is the spread (max - min) of A's per-call time over them.  Nothing is promised: the tool reports A, B and the
spread as measured and whether B is below A by more than the spread.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script (``--quick --forms B``; profiles/rpn_head_kernel_stats.md).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from multi_image_bench import time_loop  # noqa: E402

REPEATS = 4
NET_HW = (704, 1280)
STRIDES = (4, 8, 16, 32, 64)
CHANNELS = 128
LABELS = {"A": "A_torch_composition", "H": "H_torch_half_weights", "B": "B_hip_kernel", "C": "C_hip_split16"}


def make_maps(N, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = NET_HW
    return [torch.randn((N, CHANNELS, H // s, W // s), generator=g).to(dev).to(dtype) for s in STRIDES]


def interleave(steppers, steps, warmup):
    """{form: {us_per_call, host_enqueue_us_per_call, us_per_call_repeats}} and A's spread over the repeats."""
    acc = {f: [0.0, 0.0] for f in steppers}
    per = {f: [] for f in steppers}
    part = max(steps // REPEATS, 1)
    for _ in range(REPEATS):
        for f, step in steppers.items():
            gpu_s, host_s = time_loop(step, part, warmup)
            acc[f][0] += gpu_s
            acc[f][1] += host_s
            per[f].append(gpu_s / part * 1e6)
    done = REPEATS * part
    out = {}
    for f, (gpu_s, host_s) in acc.items():
        out[LABELS[f]] = {"us_per_call": gpu_s / done * 1e6, "host_enqueue_us_per_call": host_s / done * 1e6,
                          "us_per_call_repeats": per[f]}
    if "A" in per:
        out["A_spread_us"] = max(per["A"]) - min(per["A"])
    if "A" in acc and "B" in acc:
        a_us, b_us = acc["A"][0] / done * 1e6, acc["B"][0] / done * 1e6
        out["A_minus_B_us"] = a_us - b_us
        out["A_over_B_time"] = a_us / b_us
        out["B_below_A_by_more_than_A_spread"] = bool(a_us - b_us > out["A_spread_us"])
    return out


def run_head_case(N, dtype, steps, warmup, dev, forms):
    from siammot_amd.rpn import RPNHead, rpn_head_torch
    torch.manual_seed(3)
    head = RPNHead(None, CHANNELS, 3).to(dev).eval()
    with torch.no_grad():
        for p in head._params():
            p.normal_(0.0, 0.05)
    sets = [make_maps(N, dtype, dev, 11 + k) for k in range(2)]       # alternated: no step reads what the last one cached
    params = [p.detach() for p in head._params()]
    half = [p.half() for p in params]
    steppers = {}
    if "A" in forms:
        steppers["A"] = lambda k: rpn_head_torch(sets[k & 1], *params)
    if "H" in forms and dtype is torch.float16:
        steppers["H"] = lambda k: rpn_head_torch(sets[k & 1], *half)
    if "B" in forms:
        steppers["B"] = lambda k: head(sets[k & 1])
    out = {"case": "head", "images": N, "maps": str(dtype).replace("torch.", ""), "net_hw": list(NET_HW), "channels": CHANNELS,
           "anchors_per_cell": 3, "steps": steps}
    out.update(interleave(steppers, steps, warmup))
    if "A" in steppers and "B" in steppers:
        with torch.no_grad():
            (oa, ra), (ob, rb) = steppers["A"](0), steppers["B"](0)
        out["max_abs_difference_A_B"] = max(float((x - y).abs().max()) for x, y in zip(oa + ra, ob + rb))
    return out


def run_detection_case(N, steps, warmup, dev, forms):
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.config import get_default_cfg
    from siammot_amd.detector import build_detection_head
    from siammot_amd.rpn import grid_anchors_torch, rpn_head_torch
    from siammot_amd.structures import BoxList
    cfg = get_default_cfg(channels=CHANNELS)
    torch.manual_seed(4)
    det = build_detection_head(cfg, BoxCoder((1.0, 1.0, 1.0, 1.0)), CHANNELS).to(dev).eval()
    with torch.no_grad():
        for p in det.rpn_head._params():
            p.normal_(0.0, 0.05)
    sets = [make_maps(N, torch.float32, dev, 21 + k) for k in range(2)]
    size = (NET_HW[1], NET_HW[0])
    params = [p.detach() for p in det.rpn_head._params()]
    cells, strides = list(det.anchor_generator.cell_anchors), det.anchor_generator.strides

    def step_a(k):
        feats = sets[k & 1]
        objectness, regression = rpn_head_torch(feats, *params)
        levels = grid_anchors_torch(cells, strides, [tuple(f.shape[-2:]) for f in feats])
        anchors = [[BoxList._wrap(a, size, "xyxy", {}) for a in levels] for _ in range(N)]
        return det(anchors, objectness, regression, feats)

    steppers = {}
    if "A" in forms:
        steppers["A"] = step_a
    if "B" in forms:
        steppers["B"] = lambda k: det.forward_features(sets[k & 1], size)
    out = {"case": "maps_to_detections", "images": N, "maps": "float32", "net_hw": list(NET_HW), "channels": CHANNELS,
           "steps": steps}
    out.update(interleave(steppers, steps, warmup))
    if "B" in steppers:
        out["detections_per_image"] = [len(x) for x in steppers["B"](0)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="one image, fp32 maps, head only (for the kernel-trace runs)")
    ap.add_argument("--forms", default="AHB", help="which of the forms A, H, B to run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    results = []
    head_cases = [(1, torch.float32)] if args.quick else [(1, torch.float32), (4, torch.float32), (1, torch.float16),
                                                          (4, torch.float16)]
    for N, dtype in head_cases:
        results.append(run_head_case(N, dtype, args.steps, args.warmup, dev, args.forms))
        print(json.dumps(results[-1]), flush=True)
    for N in (() if args.quick else (1, 4)):
        results.append(run_detection_case(N, args.steps, args.warmup, dev, args.forms))
        print(json.dumps(results[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
