"""RPN proposal selection: the torch composition a user pays today against the HIP path.

    python tools/rpn_proposals_bench.py [--steps K] [--warmup W] [--out profiles/rpn_proposals_bench.json] [--quick] [--forms AB]

One step = one ``forward(anchors, objectness, box_regression)`` over all images and levels, at the headline maps: a
704 x 1280 input, five levels (strides 4..64), A = 3, pre / post / fpn-post 1000 / 300 / 300, NMS threshold 0.7; with 1
and with 4 images.  Two forms are timed in ONE process, interleaved (A B A B ...) so that clock drift favours neither:

    A  ``siammot_amd.rpn.rpn_proposals_torch`` on the device: the reference's form as torch operators (its NMS is this
       package's HIP kernel behind ``structures.boxlist_nms``);
    B  ``siammot_amd.rpn.RPNPostProcessor.forward``: one set of HIP launches and one device-to-host copy.

Timed with device events around a loop (both forms synchronise inside a step); the K steps of a form are split over
``REPEATS`` interleaved repeats and ``A_spread_us`` is the spread (max - min) of A's per-call time over them — the yardstick:
B must be below A by more than that spread in every case, or the tool exits non-zero.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script (``--quick --forms B``; profiles/rpn_proposals_kernel_stats.md).
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
SIZES = (32, 64, 128, 256, 512)
RATIOS = (0.5, 1.0, 2.0)
PRE, POST, FPN_POST, NMS_THRESH, MIN_SIZE = 1000, 300, 300, 0.7, 0


def level_anchors(H, W, stride, size):
    """[H*W*A, 4] anchors in the flattened order (h*W + w)*A + a: ``size``^2 area at three aspect ratios per cell."""
    ws = torch.tensor([size / r ** 0.5 for r in RATIOS])
    hs = torch.tensor([size * r ** 0.5 for r in RATIOS])
    cy, cx = torch.meshgrid(torch.arange(H) * stride + stride / 2.0, torch.arange(W) * stride + stride / 2.0, indexing="ij")
    cx, cy = cx[:, :, None], cy[:, :, None]
    return torch.stack([cx - ws / 2, cy - hs / 2, cx + ws / 2 - 1, cy + hs / 2 - 1], dim=-1).reshape(-1, 4).float().contiguous()


def make_case(N, dev):
    from siammot_amd.structures import BoxList
    H, W = NET_HW
    g = torch.Generator().manual_seed(11)
    A = len(RATIOS)
    shared = [level_anchors(H // s, W // s, s, z).to(dev) for s, z in zip(STRIDES, SIZES)]
    anchors = [[BoxList(a, (W, H)) for a in shared] for _ in range(N)]
    # two input sets, alternated: no step reads what the step before left in a cache
    sets = []
    for _ in range(2):
        obj = [(torch.randn((N, A, H // s, W // s), generator=g) * 1.5 - 2.0).to(dev) for s in STRIDES]
        reg = [(torch.randn((N, 4 * A, H // s, W // s), generator=g) * 0.3).to(dev) for s in STRIDES]
        sets.append((obj, reg))
    return anchors, sets


def run_case(N, steps, warmup, dev, forms="AB"):
    from siammot_amd.rpn import RPNPostProcessor, rpn_proposals_torch
    anchors, sets = make_case(N, dev)
    post = RPNPostProcessor(PRE, POST, NMS_THRESH, MIN_SIZE, fpn_post_nms_top_n=FPN_POST).eval()

    def step_a(k):
        obj, reg = sets[k & 1]
        return rpn_proposals_torch(anchors, obj, reg, PRE, POST, NMS_THRESH, MIN_SIZE, post.box_coder, FPN_POST)

    def step_b(k):
        obj, reg = sets[k & 1]
        return post(anchors, obj, reg)

    steppers = {"A": step_a, "B": step_b}
    out = {"images": N, "net_hw": list(NET_HW), "levels": len(STRIDES), "anchors_per_cell": len(RATIOS),
           "pre_post_fpn": [PRE, POST, FPN_POST], "nms_thresh": NMS_THRESH, "steps": steps}
    acc = {f: [0.0, 0.0] for f in forms}
    per = {f: [] for f in forms}
    part = max(steps // REPEATS, 1)
    for _ in range(REPEATS):
        for f in forms:
            gpu_s, host_s = time_loop(steppers[f], part, warmup)
            acc[f][0] += gpu_s
            acc[f][1] += host_s
            per[f].append(gpu_s / part * 1e6)
    done = REPEATS * part
    labels = {"A": "A_torch_composition", "B": "B_hip_path"}
    for f, (gpu_s, host_s) in acc.items():
        out[labels[f]] = {"us_per_call": gpu_s / done * 1e6, "host_enqueue_us_per_call": host_s / done * 1e6,
                          "us_per_call_repeats": per[f]}
    if "A" in per:
        out["A_spread_us"] = max(per["A"]) - min(per["A"])
    if "A" in acc and "B" in acc:
        a_us, b_us = acc["A"][0] / done * 1e6, acc["B"][0] / done * 1e6
        out["A_minus_B_us"] = a_us - b_us
        out["A_over_B_time"] = a_us / b_us
        out["B_below_A_by_more_than_A_spread"] = bool(a_us - b_us > out["A_spread_us"])
        # the two forms select the same proposals (their exp differs in the last bits)
        with torch.no_grad():
            ra, rb = step_a(0), step_b(0)
        out["proposals_per_image"] = [len(x) for x in rb]
        out["same_count"] = [len(x) for x in ra] == [len(x) for x in rb]
        if out["same_count"]:
            out["max_box_difference_px"] = max(float((x.bbox - y.bbox).abs().max()) for x, y in zip(ra, rb) if len(x))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="one image only (for the kernel-trace runs)")
    ap.add_argument("--forms", default="AB", help="which of the forms A, B to run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    results = []
    for N in ((1,) if args.quick else (1, 4)):
        r = run_case(N, args.steps, args.warmup, dev, args.forms)
        results.append(r)
        print(json.dumps(r), flush=True)
    failed = [r["images"] for r in results if r.get("B_below_A_by_more_than_A_spread") is False]
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    if failed:
        print("FAILED: B is not below A by more than the spread of A with %s image(s)" % (failed,), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
