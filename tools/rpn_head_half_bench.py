"""RPN head in half compute mode against fp32 mode and the all-fp16 torch composition.

    python tools/rpn_head_half_bench.py [--steps K] [--warmup W] [--out profiles/rpn_head_half_bench.json]
    python tools/rpn_head_half_bench.py --quick --forms A,B,C --steps 24 --warmup 2     (for the kernel-trace runs)

Cases: the headline maps (704 x 1280 input, five levels of strides 4..64, C = 128, A = 3), fp32 maps, with 1 and with 4 images.
One step = the head on all images and levels.  Forms, timed in ONE process and interleaved (``REPEATS`` repeats, each with its
own warm-up; every form's spread over the repeats is reported):

    A  ``RPNHead.forward`` in fp32 mode: the path of tools/rpn_head_bench.py's form B, which this mode leaves as it was — the
       yardstick;
    B  the same with ``compute_dtype=torch.float16``;
    C  the same with ``compute_dtype=torch.bfloat16``;
    D  ``siammot_amd.rpn.rpn_head_torch`` with fp16 maps and weights: what an all-half torch pipeline would run.

What counts: B and C against A, judged by A's spread over the repeats; and B against D.  Nothing is promised: the tool reports
what it measured, and how far B's and C's outputs are from A's.  Kernel times come from a separate ``rocprofv3 --kernel-trace
--stats`` run of this script (profiles/fpn_half_kernel_stats.md).

Head-phase case (one image): the two 1x1 heads stay on the fp32 matrix instruction in every mode.  Their share of the kernel
is estimated from the kernel itself: with A = 12 anchors per cell the heads run four 16-row tiles per K step where A = 3 runs
one, on the same ``t`` reads, so (time(A = 12) - time(A = 3)) / 3 is the cost of one tile's pass and its ratio to time(A = 3)
the head phase's share at A = 3 — a lower bound, since the ``t`` reads and the barriers that all tiles share are not in it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from fpn_half_bench import LABELS, REPEATS, compare, interleave  # noqa: E402
from rpn_head_bench import CHANNELS, NET_HW, make_maps  # noqa: E402


def make_head(dev, anchors=3, **kw):
    from siammot_amd.rpn import RPNHead
    torch.manual_seed(3)
    head = RPNHead(None, CHANNELS, anchors, **kw).to(dev).eval()
    with torch.no_grad():
        for p in head._params():
            p.normal_(0.0, 0.05)
    return head


def run_head_case(N, steps, warmup, dev, forms):
    from siammot_amd import ops
    from siammot_amd.rpn import rpn_head_torch
    head = make_head(dev)
    sets = [make_maps(N, torch.float32, dev, 11 + k) for k in range(2)]       # alternated: no step reads what the last one cached
    steppers, modes = {}, {}
    if "A" in forms:
        steppers["A"] = lambda k: head(sets[k & 1])
    for f, ct in (("B", torch.float16), ("C", torch.bfloat16)):
        if f in forms:
            modes[f] = make_head(dev, compute_dtype=ct)                       # (the same seed: the same parameters)
            steppers[f] = (lambda m: lambda k: m(sets[k & 1]))(modes[f])
    if "D" in forms:
        half = [p.detach().half() for p in head._params()]
        half_sets = [[t.half() for t in s] for s in sets]
        steppers["D"] = lambda k: rpn_head_torch(half_sets[k & 1], *half)
    out = {"case": "head", "images": N, "maps": "float32 (D: float16)", "net_hw": list(NET_HW), "channels": CHANNELS,
           "anchors_per_cell": 3, "steps": steps, "repeats": REPEATS}
    before = ops.FALLBACKS["rpn_head_torch"]
    out.update(interleave(steppers, steps, warmup))
    assert ops.FALLBACKS["rpn_head_torch"] == before, "a device form took the torch composition"
    compare(out)
    if "A" in steppers:
        with torch.no_grad():
            oa, ra = steppers["A"](0)
            for f in modes:
                ob, rb = steppers[f](0)
                out["max_difference_A_%s_of_output_max" % f] = max(float((p - q).abs().max() / p.abs().max())
                                                                   for p, q in zip(oa + ra, ob + rb))
    return out


def run_head_phase_case(steps, warmup, dev):
    sets = [make_maps(1, torch.float32, dev, 31 + k) for k in range(2)]
    out = {"case": "head_phase_share", "images": 1, "net_hw": list(NET_HW), "channels": CHANNELS, "steps": steps, "repeats": REPEATS}
    for mode, ct in (("fp32", None), ("fp16_compute", torch.float16)):
        heads = {a: make_head(dev, a, compute_dtype=ct) for a in (3, 12)}
        labels = {a: "%s_A%d" % (mode, a) for a in heads}
        steppers = {a: (lambda m: lambda k: m(sets[k & 1]))(h) for a, h in heads.items()}
        res = interleave(steppers, steps, warmup, labels)
        out.update(res)
        t3, t12 = res[labels[3]]["us_per_call"], res[labels[12]]["us_per_call"]
        out["%s_one_head_tile_us" % mode] = (t12 - t3) / 3.0
        out["%s_head_phase_share_at_A3" % mode] = (t12 - t3) / 3.0 / t3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="one image (for the kernel-trace runs)")
    ap.add_argument("--forms", default="A,B,C,D", help="comma-separated forms")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    forms = tuple(f for f in args.forms.split(",") if f)
    assert all(f in LABELS for f in forms), forms
    results = []
    for N in ((1,) if args.quick else (1, 4)):
        results.append(run_head_case(N, args.steps, args.warmup, dev, forms))
        print(json.dumps(results[-1]), flush=True)
    if not args.quick:
        results.append(run_head_phase_case(args.steps, args.warmup, dev))
        print(json.dumps(results[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
