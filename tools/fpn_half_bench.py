"""FPN in half compute mode against fp32 mode and the all-fp16 torch composition, and frames -> detections with everything in
half mode against a half body alone.

    python tools/fpn_half_bench.py [--steps K] [--warmup W] [--out profiles/fpn_half_bench.json]
    python tools/fpn_half_bench.py --quick --forms A,B,C --steps 24 --warmup 2     (for the kernel-trace runs)

FPN cases: the headline stage maps (704 x 1280 input, DLA-34 stages: 176 x 320 ... 22 x 40 with 64, 128, 256, 512 channels, C =
128, ``LastLevelMaxPool``), fp32 stage maps and fp32 outputs, with 1 and with 4 images.  One step = the pyramid of all images.
Forms, timed in ONE process and interleaved (``REPEATS`` repeats, each with its own warm-up; every form's spread over the
repeats is reported):

    A  ``FPN.forward`` in fp32 mode: the path of tools/fpn_bench.py's form B, which this mode leaves as it was — the yardstick;
    B  the same with ``compute_dtype=torch.float16``;
    C  the same with ``compute_dtype=torch.bfloat16``;
    D  ``siammot_amd.fpn.fpn_torch`` with fp16 stage maps and weights: what an all-half torch pipeline would run (fp16 outputs).

Detection cases (frames -> detections, DLA-34, one image and four):

    A  ``build_detection_head(..., backbone=build_backbone(cfg, compute_dtype=torch.float16))``: the body alone in half mode;
    B  ``build_detection_head(..., backbone=True, compute_dtype=torch.float16)``: body, pyramid and RPN head in half mode.

What counts: B and C against A, judged by A's spread over the repeats; and B against D.  Nothing is promised: the tool reports
what it measured, and how far B's and C's maps are from A's.  Kernel times come from a separate ``rocprofv3 --kernel-trace
--stats`` run of this script (profiles/fpn_half_kernel_stats.md).
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

from fpn_bench import CHANNELS, NET_HW, make_stages  # noqa: E402
from multi_image_bench import time_loop  # noqa: E402

REPEATS = 4
LABELS = {"A": "A_hip_fp32", "B": "B_hip_fp16_compute", "C": "C_hip_bf16_compute", "D": "D_torch_fp16"}
DET_LABELS = {"A": "A_half_body_only", "B": "B_half_body_pyramid_head"}


def interleave(steppers, steps, warmup, labels=LABELS):
    """{label: {us_per_call, host_enqueue_us_per_call, us_per_call_repeats, spread_us}}: REPEATS passes over all forms."""
    part = max(steps // REPEATS, 1)
    acc = {f: [0.0, 0.0] for f in steppers}
    per = {f: [] for f in steppers}
    for _ in range(REPEATS):
        for f, step in steppers.items():
            gpu_s, host_s = time_loop(step, part, warmup)
            acc[f][0] += gpu_s
            acc[f][1] += host_s
            per[f].append(gpu_s / part * 1e6)
    done = REPEATS * part
    return {labels[f]: {"us_per_call": acc[f][0] / done * 1e6, "host_enqueue_us_per_call": acc[f][1] / done * 1e6,
                        "us_per_call_repeats": per[f], "spread_us": max(per[f]) - min(per[f])} for f in steppers}


def compare(out, labels=LABELS):
    """B and C against the yardstick A (by A's spread), and against D where it ran."""
    a, d = out.get(labels["A"]), out.get(labels.get("D"))
    for f in ("B", "C"):
        m = out.get(labels.get(f))
        if a and m:
            out["A_minus_%s_us" % f] = a["us_per_call"] - m["us_per_call"]
            out["A_over_%s_time" % f] = a["us_per_call"] / m["us_per_call"]
            out["%s_below_A_by_more_than_A_spread" % f] = bool(out["A_minus_%s_us" % f] > a["spread_us"])
        if a and m and d:
            out["D_minus_%s_us" % f] = d["us_per_call"] - m["us_per_call"]
            out["%s_below_D_by_more_than_A_spread" % f] = bool(out["D_minus_%s_us" % f] > a["spread_us"])
    return out


def make_fpn(dev, **kw):
    from siammot_amd.fpn import FPN, LastLevelMaxPool
    from fpn_bench import STAGE_CHANNELS
    torch.manual_seed(3)
    return FPN(STAGE_CHANNELS, CHANNELS, top_blocks=LastLevelMaxPool(), **kw).to(dev).eval()


def run_fpn_case(N, steps, warmup, dev, forms):
    from siammot_amd import ops
    from siammot_amd.fpn import fpn_torch
    fpn = make_fpn(dev)
    sets = [make_stages(N, torch.float32, dev, 11 + k) for k in range(2)]       # alternated: no step reads what the last one cached
    steppers, modes = {}, {}
    if "A" in forms:
        steppers["A"] = lambda k: fpn(sets[k & 1])
    for f, ct in (("B", torch.float16), ("C", torch.bfloat16)):
        if f in forms:
            modes[f] = make_fpn(dev, compute_dtype=ct)                          # (the same seed: the same parameters)
            steppers[f] = (lambda m: lambda k: m(sets[k & 1]))(modes[f])
    if "D" in forms:
        half = copy.deepcopy(fpn).half()
        hi, hl = half._blocks()
        half_sets = [[t.half() for t in s] for s in sets]
        steppers["D"] = lambda k: fpn_torch(half_sets[k & 1], hi, hl, half.top_blocks)
    out = {"case": "fpn", "images": N, "stage_maps": "float32", "outputs": "float32 (D: float16)", "net_hw": list(NET_HW),
           "channels": CHANNELS, "steps": steps, "repeats": REPEATS}
    before = ops.FALLBACKS["fpn_torch"]
    out.update(interleave(steppers, steps, warmup))
    assert ops.FALLBACKS["fpn_torch"] == before, "a device form took the torch composition"
    compare(out)
    if "A" in steppers:
        with torch.no_grad():
            x = steppers["A"](0)
            for f in modes:
                y = steppers[f](0)
                out["max_difference_A_%s_of_level_max" % f] = [float((p - q).abs().max() / p.abs().max()) for p, q in zip(x, y)]
    return out


def run_detection_case(N, steps, warmup, dev, forms):
    from siammot_amd import ops
    from siammot_amd.backbone import build_backbone
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.config import get_default_cfg
    from siammot_amd.detector import build_detection_head
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dla_cases as D
    from dla_bench import make_images
    cfg = get_default_cfg(channels=CHANNELS)

    def build(everything):
        torch.manual_seed(4)
        if everything:
            det = build_detection_head(cfg, BoxCoder((1.0, 1.0, 1.0, 1.0)), CHANNELS, backbone=True, compute_dtype=torch.float16)
        else:
            det = build_detection_head(cfg, BoxCoder((1.0, 1.0, 1.0, 1.0)), CHANNELS,
                                       backbone=build_backbone(cfg, compute_dtype=torch.float16))
        det = det.to(dev).eval()
        D.load(det.backbone.body, D.params(det.backbone.body, D.SEED), dev)
        with torch.no_grad():
            for p in det.rpn_head._params():
                p.normal_(0.0, 0.05)
        return det

    sets = [make_images(N, torch.float32, dev, 21 + k) for k in range(2)]
    size = (NET_HW[1], NET_HW[0])
    steppers = {}
    for f in ("A", "B"):
        if f in forms:
            steppers[f] = (lambda det: lambda k: det.forward_images(sets[k & 1], size)[1])(build(f == "B"))
    out = {"case": "frames_to_detections", "body": "DLA-34-FPN", "images": N, "net_hw": list(NET_HW), "channels": CHANNELS,
           "steps": steps, "repeats": REPEATS}
    before = dict(ops.FALLBACKS)
    out.update(interleave(steppers, steps, warmup, DET_LABELS))
    assert dict(ops.FALLBACKS) == before, "a form took a fallback"
    compare(out, DET_LABELS)
    with torch.no_grad():
        out["detections_per_image"] = {DET_LABELS[f]: [len(x) for x in step(0)] for f, step in steppers.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="one image, FPN only (for the kernel-trace runs)")
    ap.add_argument("--forms", default="A,B,C,D", help="comma-separated forms")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    forms = tuple(f for f in args.forms.split(",") if f)
    assert all(f in LABELS for f in forms), forms
    results = []
    for N in ((1,) if args.quick else (1, 4)):
        results.append(run_fpn_case(N, args.steps, args.warmup, dev, forms))
        print(json.dumps(results[-1]), flush=True)
    for N in (() if args.quick else (1, 4)):
        results.append(run_detection_case(N, max(args.steps // 4, REPEATS), min(args.warmup, 2), dev, forms))
        print(json.dumps(results[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
