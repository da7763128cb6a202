"""DLA-34 body: the torch composition on the device against the HIP path — the body alone, frames to FPN maps and frames to
detections.

    python tools/dla_bench.py [--steps K] [--warmup W] [--out profiles/dla_bench.json] [--quick] [--forms AHB]
    python tools/dla_bench.py --forms AHBC --out profiles/dla_split_bench.json

Cases: the headline 704 x 1280 frame with 1 and with 4 images, fp32 and fp16 images; the recipe's parameters
(tests/dla_cases.py: activations of the size a trained network has, about half of them zero).  One step = all images.  Forms,
timed in ONE process, interleaved (A B A B ...) so that clock drift favours neither:

    A  ``siammot_amd.dla.dla_torch`` on the device: 36 convolutions, 36 frozen-BN affines, ReLUs, cats and max-pools as torch
       operators (MIOpen), fp32 arithmetic on the upcast image — the arithmetic of B;
    H  (fp16 images only) the same composition with fp16 parameters: what an all-half pipeline would run, other arithmetic;
    B  ``siammot_amd.dla.DLA.forward``: 37 launches of csrc/dla.hip;
    C  the same module with ``operands="split16"`` (the trees' 3x3 convolutions on three-part bf16 operands); with C the
       result also carries ``B_spread_us``, ``B_minus_C_us`` and whether C is below B by more than B's spread.

``frames_to_fpn``: A = the torch body and ``fpn_torch``, B = ``backbone(images)``.  ``frames_to_detections``: A = the torch body,
then ``DetectionHead.forward_stages``; B = ``DetectionHead.forward_images``.  C = B with a split-mode body of the same parameters.

Timed with device events around a loop; the K steps of a form are split over four interleaved repeats and ``A_spread_us`` is
the spread (max - min) of A's per-call time over them.  Nothing is promised: the tool reports A, B and the spread as measured
and whether B is below A by more than the spread.  Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run
of this script (``--quick --forms B``; profiles/dla_kernel_stats.md).
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import dla_cases as D  # noqa: E402
from rpn_head_bench import interleave  # noqa: E402

NET_HW = (704, 1280)
CHANNELS = 128


def make_images(N, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, 3) + NET_HW, generator=g).to(dev).to(dtype)


def make_body(dev, operands="fp32"):
    from siammot_amd.dla import dla_34
    body = dla_34(operands=operands)
    return D.load(body, D.params(body, D.SEED), dev)


def against_b(out):
    """B's spread over the repeats and where C stands against B, as ``interleave`` does for B against A."""
    b, c = out.get("B_hip_kernel"), out.get("C_hip_split16")
    if b and c:
        out["B_spread_us"] = max(b["us_per_call_repeats"]) - min(b["us_per_call_repeats"])
        out["B_minus_C_us"] = b["us_per_call"] - c["us_per_call"]
        out["B_over_C_time"] = b["us_per_call"] / c["us_per_call"]
        out["C_below_B_by_more_than_B_spread"] = bool(out["B_minus_C_us"] > out["B_spread_us"])
    return out


def run_body_case(N, dtype, steps, warmup, dev, forms):
    from siammot_amd.dla import dla_torch
    body = make_body(dev)
    sets = [make_images(N, dtype, dev, 11 + k) for k in range(2)]     # alternated: no step reads what the last one cached
    steppers = {}
    if "A" in forms:
        steppers["A"] = lambda k: dla_torch(body, sets[k & 1])
    if "H" in forms and dtype is torch.float16:
        half = copy.deepcopy(body).half()
        steppers["H"] = lambda k: dla_torch(half, sets[k & 1])
    if "B" in forms:
        steppers["B"] = lambda k: body(sets[k & 1])
    if "C" in forms:
        split = make_body(dev, "split16")
        steppers["C"] = lambda k: split(sets[k & 1])
    out = {"case": "body", "images": N, "image_dtype": str(dtype).replace("torch.", ""), "net_hw": list(NET_HW), "steps": steps}
    out.update(against_b(interleave(steppers, steps, warmup)))
    if "B" in steppers and "C" in steppers:
        with torch.no_grad():
            b, c = steppers["B"](0), steppers["C"](0)
        out["max_difference_B_C_of_stage_max"] = [float((x - y).abs().max() / x.abs().max()) for x, y in zip(b, c)]
    if "A" in steppers and "B" in steppers:
        with torch.no_grad():
            a, b = steppers["A"](0), steppers["B"](0)
        out["max_difference_A_B_of_stage_max"] = [float((x - y).abs().max() / x.abs().max()) for x, y in zip(a, b)]
    return out


def run_pipeline_case(N, steps, warmup, dev, forms):
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.config import get_default_cfg
    from siammot_amd.detector import build_detection_head
    from siammot_amd.dla import dla_torch
    from siammot_amd.fpn import fpn_torch
    cfg = get_default_cfg(channels=CHANNELS)
    torch.manual_seed(4)
    det = build_detection_head(cfg, BoxCoder((1.0, 1.0, 1.0, 1.0)), CHANNELS, backbone=True).to(dev).eval()
    body, fpn = det.backbone.body, det.backbone.fpn
    D.load(body, D.params(body, D.SEED), dev)
    with torch.no_grad():
        for p in det.rpn_head._params():
            p.normal_(0.0, 0.05)
    det_c = None
    if "C" in forms:                                                  # the same detector over a split-mode body
        from siammot_amd.backbone import build_backbone
        torch.manual_seed(4)
        det_c = build_detection_head(cfg, BoxCoder((1.0, 1.0, 1.0, 1.0)), CHANNELS,
                                     backbone=build_backbone(cfg, operands="split16")).to(dev).eval()
        det_c.load_state_dict(det.state_dict())
    sets = [make_images(N, torch.float32, dev, 21 + k) for k in range(2)]
    size = (NET_HW[1], NET_HW[0])
    inner, layer = fpn._blocks()
    results = []
    for case, a, b, c in (("frames_to_fpn", lambda k: fpn_torch(dla_torch(body, sets[k & 1]), inner, layer, fpn.top_blocks),
                           lambda k: det.backbone(sets[k & 1]), lambda k: det_c.backbone(sets[k & 1])),
                          ("frames_to_detections", lambda k: det.forward_stages(dla_torch(body, sets[k & 1]), size)[1],
                           lambda k: det.forward_images(sets[k & 1], size)[1], lambda k: det_c.forward_images(sets[k & 1], size)[1])):
        steppers = {}
        if "A" in forms:
            steppers["A"] = a
        if "B" in forms:
            steppers["B"] = b
        if det_c is not None:
            steppers["C"] = c
        out = {"case": case, "images": N, "image_dtype": "float32", "net_hw": list(NET_HW), "channels": CHANNELS, "steps": steps}
        out.update(against_b(interleave(steppers, steps, warmup)))
        results.append(out)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="one fp32 image, the body only (for the kernel-trace runs)")
    ap.add_argument("--forms", default="AHB", help="which of the forms A, H, B, C to run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    results = []
    cases = [(1, torch.float32)] if args.quick else [(1, torch.float32), (4, torch.float32), (1, torch.float16), (4, torch.float16)]
    for N, dtype in cases:
        results.append(run_body_case(N, dtype, args.steps, args.warmup, dev, args.forms))
        print(json.dumps(results[-1]), flush=True)
    for N in (() if args.quick else (1, 4)):
        for r in run_pipeline_case(N, args.steps, args.warmup, dev, args.forms):
            results.append(r)
            print(json.dumps(r), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
