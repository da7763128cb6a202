"""FPN: the torch composition on the device against the HIP path, and backbone stage maps to detections with and without
``DetectionHead.forward_stages``.

    python tools/fpn_bench.py [--steps K] [--warmup W] [--out profiles/fpn_bench.json] [--quick] [--forms AHB]

FPN cases: the headline stage maps (704 x 1280 input, DLA-34 stages of strides 4..32: 176 x 320 ... 22 x 40 with 64, 128,
256, 512 channels, C = 128, ``LastLevelMaxPool``) with 1 and with 4 images, outputs in fp32 and in fp16.  One step = the
pyramid of all images.  Forms, timed in ONE process, interleaved (A B A B ...) so that clock drift favours neither:

    A  ``siammot_amd.fpn.fpn_torch`` on fp32 stage maps: conv1x1 + bilinear resize + add + conv3x3 per level as torch operators
       (MIOpen / rocBLAS), followed by ``.to(float16)`` per map in the fp16-output cases — the arithmetic of B;
    H  (fp16 outputs only) the same composition with fp16 stage maps and weights: what an all-half pipeline would run, other
       arithmetic (fp16 products and outputs);
    B  ``siammot_amd.fpn.FPN.forward`` on fp32 stage maps: L + 1 launches (csrc/fpn.hip), the output type stored directly.

Detection cases (one image and four, fp32): stage maps -> detections,

    A  the torch FPN, then ``DetectionHead.forward_features``;
    B  ``DetectionHead.forward_stages``.

Timed with device events around a loop; the K steps of a form are split over ``REPEATS`` interleaved repeats and
``A_spread_us`` is the spread (max - min) of A's per-call time over them.  Nothing is promised: the tool reports A, B and the
spread as measured and whether B is below A by more than the spread.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script (``--quick --forms B``; profiles/fpn_kernel_stats.md).
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from rpn_head_bench import interleave  # noqa: E402

NET_HW = (704, 1280)
STRIDES = (4, 8, 16, 32)
STAGE_CHANNELS = (64, 128, 256, 512)
CHANNELS = 128


def make_stages(N, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = NET_HW
    return [torch.randn((N, c, H // s, W // s), generator=g).to(dev).to(dtype) for c, s in zip(STAGE_CHANNELS, STRIDES)]


def make_fpn(dev, out_dtype=torch.float32):
    from siammot_amd.fpn import FPN, LastLevelMaxPool
    torch.manual_seed(3)
    return FPN(STAGE_CHANNELS, CHANNELS, top_blocks=LastLevelMaxPool(), out_dtype=out_dtype).to(dev).eval()


def run_fpn_case(N, out_dtype, steps, warmup, dev, forms):
    from siammot_amd.fpn import fpn_torch
    fpn = make_fpn(dev, out_dtype)
    inner, layer = fpn._blocks()
    sets = [make_stages(N, torch.float32, dev, 11 + k) for k in range(2)]       # alternated: no step reads what the last one cached
    half_out = out_dtype is not torch.float32

    def step_a(k):
        out = fpn_torch(sets[k & 1], inner, layer, fpn.top_blocks)
        return [o.to(out_dtype) for o in out] if half_out else out

    steppers = {}
    if "A" in forms:
        steppers["A"] = step_a
    if "H" in forms and half_out:
        half = copy.deepcopy(fpn).to(out_dtype)
        hi, hl = half._blocks()
        half_sets = [[t.to(out_dtype) for t in s] for s in sets]
        steppers["H"] = lambda k: fpn_torch(half_sets[k & 1], hi, hl, half.top_blocks)
    if "B" in forms:
        steppers["B"] = lambda k: fpn(sets[k & 1])
    out = {"case": "fpn", "images": N, "stage_maps": "float32", "outputs": str(out_dtype).replace("torch.", ""),
           "net_hw": list(NET_HW), "stage_channels": list(STAGE_CHANNELS), "channels": CHANNELS, "steps": steps}
    out.update(interleave(steppers, steps, warmup))
    if "A" in steppers and "B" in steppers:
        with torch.no_grad():
            a, b = steppers["A"](0), steppers["B"](0)
        out["max_abs_difference_A_B"] = max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b))
    return out


def run_detection_case(N, steps, warmup, dev, forms):
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.config import get_default_cfg
    from siammot_amd.detector import build_detection_head
    from siammot_amd.fpn import fpn_torch
    cfg = get_default_cfg(channels=CHANNELS)
    torch.manual_seed(4)
    det = build_detection_head(cfg, BoxCoder((1.0, 1.0, 1.0, 1.0)), CHANNELS, fpn=True).to(dev).eval()
    with torch.no_grad():
        for p in det.rpn_head._params():
            p.normal_(0.0, 0.05)
    sets = [make_stages(N, torch.float32, dev, 21 + k) for k in range(2)]
    size = (NET_HW[1], NET_HW[0])
    inner, layer = det.fpn._blocks()
    steppers = {}
    if "A" in forms:
        steppers["A"] = lambda k: det.forward_features(fpn_torch(sets[k & 1], inner, layer, det.fpn.top_blocks), size)
    if "B" in forms:
        steppers["B"] = lambda k: det.forward_stages(sets[k & 1], size)[1]
    out = {"case": "stages_to_detections", "images": N, "stage_maps": "float32", "net_hw": list(NET_HW), "channels": CHANNELS,
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
    ap.add_argument("--quick", action="store_true", help="one image, fp32 outputs, FPN only (for the kernel-trace runs)")
    ap.add_argument("--forms", default="AHB", help="which of the forms A, H, B to run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    results = []
    fpn_cases = [(1, torch.float32)] if args.quick else [(1, torch.float32), (4, torch.float32), (1, torch.float16),
                                                         (4, torch.float16)]
    for N, out_dtype in fpn_cases:
        results.append(run_fpn_case(N, out_dtype, args.steps, args.warmup, dev, args.forms))
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
