"""DLA-34, DLA-60 and DLA-169 bodies in half compute mode against fp32 mode, split mode and the torch compositions.

    python tools/dla_half_bench.py [--steps K] [--warmup W] [--out profiles/dla_half_bench.json]
    python tools/dla_half_bench.py --body DLA-60-FPN --images 4 --out profiles/dla_half_bench.json     (one case; merged into --out)
    python tools/dla_half_bench.py --body DLA-60-FPN --images 1 --forms D16 --steps 4                  (for the kernel-trace runs)

Cases: the headline 704 x 1280 frame with 1 and with 4 images, the recipe's parameters (tests/dla_cases.py).  One step = all
images.  Forms, timed in ONE process and interleaved (four repeats, each with its own warm-up; every form's spread over the
repeats is reported, ``<form>_spread_us``):

    A     ``siammot_amd.dla.dla_torch`` on the device in fp32 (MIOpen convolutions, torch's affines, ReLUs, cats, pools, adds);
    H     the same composition with the module and the images in fp16: what an all-half torch pipeline would run;
    B     ``DLA.forward`` in fp32 mode: one launch of csrc/dla.hip per convolution;
    C     the same with ``operands="split16"``;
    D16   the same with ``compute_dtype=torch.float16``;
    Db16  the same with ``compute_dtype=torch.bfloat16``.

What counts: D against B (the fp32 mode) and D against H, judged by B's spread.  Nothing is promised: the tool reports what it
measured, and per stage how far D's maps are from B's.  A case run alone (``--body`` / ``--images``) replaces its entry in
``--out`` and keeps the others, so that every case can run in a process and under a time limit of its own.
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
from dla_bench import NET_HW, make_images  # noqa: E402
from multi_image_bench import time_loop  # noqa: E402

REPEATS = 4
BODIES = ("DLA-34-FPN", "DLA-60-FPN", "DLA-169-FPN")
LABELS = {"A": "A_torch_fp32", "H": "H_torch_fp16", "B": "B_hip_fp32", "C": "C_hip_split16", "D16": "D16_hip_fp16_compute",
          "Db16": "Db16_hip_bf16_compute"}


def make_body(name, dev, **kw):
    from siammot_amd.dla import BODIES as factories
    body = factories[name](**kw)
    return D.load(body, D.params(body, D.SEED), dev)


def interleave(steppers, steps, warmup):
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
    return {LABELS[f]: {"us_per_call": acc[f][0] / done * 1e6, "host_enqueue_us_per_call": acc[f][1] / done * 1e6,
                        "us_per_call_repeats": per[f], "spread_us": max(per[f]) - min(per[f])} for f in steppers}


def run_case(name, N, steps, warmup, dev, forms):
    from siammot_amd import ops
    from siammot_amd.dla import dla_torch
    body = make_body(name, dev)
    sets = [make_images(N, torch.float32, dev, 11 + k) for k in range(2)]     # alternated: no step reads what the last one cached
    steppers = {}
    if "A" in forms:
        steppers["A"] = lambda k: dla_torch(body, sets[k & 1])
    if "H" in forms:
        half, hsets = copy.deepcopy(body).half(), [s.half() for s in sets]
        steppers["H"] = lambda k: dla_torch(half, hsets[k & 1])
    if "B" in forms:
        steppers["B"] = lambda k: body(sets[k & 1])
    if "C" in forms:
        split = make_body(name, dev, operands="split16")
        steppers["C"] = lambda k: split(sets[k & 1])
    if "D16" in forms:
        d16 = make_body(name, dev, compute_dtype=torch.float16)
        steppers["D16"] = lambda k: d16(sets[k & 1])
    if "Db16" in forms:
        db16 = make_body(name, dev, compute_dtype=torch.bfloat16)
        steppers["Db16"] = lambda k: db16(sets[k & 1])
    out = {"case": "body", "body": name, "images": N, "image_dtype": "float32", "net_hw": list(NET_HW), "steps": steps,
           "repeats": REPEATS, "launches": len(body.convs())}
    before = ops.FALLBACKS["dla_torch"]
    out.update(interleave(steppers, steps, warmup))
    assert ops.FALLBACKS["dla_torch"] == before, "a device form took the torch composition"
    b = out.get(LABELS["B"])
    for f in ("D16", "Db16"):
        d = out.get(LABELS[f])
        if b and d:
            out["B_minus_%s_us" % f] = b["us_per_call"] - d["us_per_call"]
            out["B_over_%s_time" % f] = b["us_per_call"] / d["us_per_call"]
            out["%s_below_B_by_more_than_B_spread" % f] = bool(out["B_minus_%s_us" % f] > b["spread_us"])
            with torch.no_grad():
                x, y = steppers["B"](0), steppers[f](0)
            out["max_difference_B_%s_of_stage_max" % f] = [float((p - q).abs().max() / p.abs().max()) for p, q in zip(x, y)]
        h = out.get(LABELS["H"])
        if h and d and b:
            out["H_minus_%s_us" % f] = h["us_per_call"] - d["us_per_call"]
            out["%s_below_H_by_more_than_B_spread" % f] = bool(out["H_minus_%s_us" % f] > b["spread_us"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="merge the JSON result into this file")
    ap.add_argument("--body", default=None, help="one of %s (default: all)" % (BODIES,))
    ap.add_argument("--images", type=int, default=None, help="1 or 4 (default: both)")
    ap.add_argument("--forms", default="A,H,B,C,D16,Db16", help="comma-separated forms")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    forms = tuple(f for f in args.forms.split(",") if f)
    assert all(f in LABELS for f in forms), forms
    results = []
    for name in ((args.body,) if args.body else BODIES):
        for N in ((args.images,) if args.images else (1, 4)):
            results.append(run_case(name, N, args.steps, args.warmup, dev, forms))
            print(json.dumps(results[-1]), flush=True)
    if args.out:
        doc = {"cases": []}
        if os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        keep = [c for c in doc.get("cases", []) if (c["body"], c["images"]) not in {(r["body"], r["images"]) for r in results}]
        doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": keep + results}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
