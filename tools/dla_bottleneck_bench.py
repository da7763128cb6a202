"""DLA-60 and DLA-169 bodies: the torch composition on the device against the HIP path — the body alone and frames to FPN maps.

    python tools/dla_bottleneck_bench.py [--steps K] [--warmup W] [--out profiles/dla_bottleneck_bench.json]
    python tools/dla_bottleneck_bench.py --quick --body DLA-169-FPN --forms B      (for the kernel-trace runs)

Cases: the headline 704 x 1280 fp32 frame with 1 and with 4 images, DLA-60 (63 launches) and DLA-169 (168), the recipe's
parameters (tests/dla_cases.py).  One step = all images.  Forms, timed in ONE process and interleaved as in tools/dla_bench.py
(four repeats with warm-up; ``A_spread_us`` is the spread of A's per-call time over them):

    A  ``siammot_amd.dla.dla_torch`` on the device (MIOpen convolutions, torch's affines, ReLUs, cats, max-pools and adds);
    B  ``siammot_amd.dla.DLA.forward``: one launch of csrc/dla.hip per convolution;
    C  the same module with ``operands="split16"`` (the trees' 3x3 convolutions on three-part bf16 operands).

``frames_to_fpn``: A = the torch body and ``fpn_torch``, B = ``backbone(images)``, C = B over a split-mode body.

Nothing is promised: the tool reports A, B, C and the spreads as measured, and whether B is below A by more than A's spread.
The 1x1 kernels' share of a call comes from a separate ``rocprofv3 --kernel-trace --stats`` run of the ``--quick`` form
(profiles/dla_bottleneck_kernel_stats.md).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import dla_cases as D  # noqa: E402
from dla_bench import NET_HW, against_b, make_images  # noqa: E402
from rpn_head_bench import interleave  # noqa: E402

CHANNELS = 128
BODIES = ("DLA-60-FPN", "DLA-169-FPN")


def make_body(name, dev, operands="fp32"):
    from siammot_amd.dla import BODIES as factories
    body = factories[name](operands=operands)
    return D.load(body, D.params(body, D.SEED), dev)


def run_body_case(name, N, steps, warmup, dev, forms):
    from siammot_amd import ops
    from siammot_amd.dla import dla_torch
    body = make_body(name, dev)
    sets = [make_images(N, torch.float32, dev, 11 + k) for k in range(2)]
    steppers = {}
    if "A" in forms:
        steppers["A"] = lambda k: dla_torch(body, sets[k & 1])
    if "B" in forms:
        steppers["B"] = lambda k: body(sets[k & 1])
    if "C" in forms:
        split = make_body(name, dev, "split16")
        steppers["C"] = lambda k: split(sets[k & 1])
    out = {"case": "body", "body": name, "images": N, "image_dtype": "float32", "net_hw": list(NET_HW), "steps": steps,
           "launches": len(body.convs()),
           "workspace_bytes": ops.dla_net_ws_bytes(body.levels, body.channels, N, NET_HW[0], NET_HW[1], body.block, body.residual_root)}
    before = ops.FALLBACKS["dla_torch"]
    out.update(against_b(interleave(steppers, steps, warmup)))
    assert ops.FALLBACKS["dla_torch"] == before, "B or C took the torch composition"
    with torch.no_grad():
        if "A" in steppers and "B" in steppers:
            a, b = steppers["A"](0), steppers["B"](0)
            out["max_difference_A_B_of_stage_max"] = [float((x - y).abs().max() / x.abs().max()) for x, y in zip(a, b)]
        if "B" in steppers and "C" in steppers:
            b, c = steppers["B"](0), steppers["C"](0)
            out["max_difference_B_C_of_stage_max"] = [float((x - y).abs().max() / x.abs().max()) for x, y in zip(b, c)]
    return out


def run_fpn_case(name, N, steps, warmup, dev, forms):
    from siammot_amd.backbone import build_backbone
    from siammot_amd.config import get_default_cfg
    from siammot_amd.dla import dla_torch
    from siammot_amd.fpn import fpn_torch
    cfg = get_default_cfg(name, channels=CHANNELS)
    torch.manual_seed(4)
    bb = build_backbone(cfg).to(dev).eval()
    D.load(bb.body, D.params(bb.body, D.SEED), dev)
    sets = [make_images(N, torch.float32, dev, 21 + k) for k in range(2)]
    inner, layer = bb.fpn._blocks()
    steppers = {}
    if "A" in forms:
        steppers["A"] = lambda k: fpn_torch(dla_torch(bb.body, sets[k & 1]), inner, layer, bb.fpn.top_blocks)
    if "B" in forms:
        steppers["B"] = lambda k: bb(sets[k & 1])
    if "C" in forms:
        bb_c = build_backbone(cfg, operands="split16").to(dev).eval()
        bb_c.load_state_dict(bb.state_dict())
        steppers["C"] = lambda k: bb_c(sets[k & 1])
    out = {"case": "frames_to_fpn", "body": name, "images": N, "image_dtype": "float32", "net_hw": list(NET_HW), "channels": CHANNELS,
           "steps": steps}
    out.update(against_b(interleave(steppers, steps, warmup)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="one image, the body only (for the kernel-trace runs)")
    ap.add_argument("--body", default=None, help="one of %s (default: both)" % (BODIES,))
    ap.add_argument("--forms", default="ABC", help="which of the forms A, B, C to run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    results = []
    for name in ((args.body,) if args.body else BODIES):
        for N in ((1,) if args.quick else (1, 4)):
            results.append(run_body_case(name, N, args.steps, args.warmup, dev, args.forms))
            print(json.dumps(results[-1]), flush=True)
            if not args.quick:
                results.append(run_fpn_case(name, N, args.steps, args.warmup, dev, args.forms))
                print(json.dumps(results[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
