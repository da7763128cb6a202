"""fp16 / bf16 feature maps through the EMM head: what a half-precision backbone pays with and without the typed kernels.

    python tools/half_maps_bench.py [--steps K] [--warmup W] [--out profiles/half_maps_bench.json] [--quick]

One step = a frame pair (EMM.forward + EMM.extract_cache) of every image, through the public module.  Three forms are
timed in ONE process, interleaved (A B C A B C) so that clock drift favours none:

    A  fp32 maps through the head (the path that always existed);
    B  half maps, ``.float()`` on every level, then the head (what a half-precision user paid before);
    C  half maps through the head as they are (the ``smot_*_typed_fwd`` kernels).

Timed with device events around a synchronised loop of K steps; ``host_enqueue_us_per_step`` is the host wall time of the
loop's enqueue (before the synchronisation).  Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run
of this script (``--quick --forms A`` / ``--forms C``; profiles/half_maps_kernel_stats.md).
Cases: configs[1] (704x1280, C = 128, 30 tracks), configs[2] (100 tracks), configs[4] (1056x1920, C = 256, 50 tracks); one
camera and a batch of 4; fp16 and bf16.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import bench  # noqa: E402
from multi_image_bench import time_loop  # noqa: E402

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def make_case(B, channels, net_hw, n, dtype, dev):
    import siammot_amd  # noqa: F401
    from siammot_amd.config import get_default_cfg
    from siammot_amd.emm import EMM
    from siammot_amd.structures import BoxList
    from siammot_amd.track_utils import build_track_utils
    H, W = net_hw
    image_wh = (W, H)
    cfg = get_default_cfg(channels=channels)
    emm = EMM(cfg, build_track_utils(cfg)).to(dev).eval()
    boxes = bench.synthetic_boxes(n, image_wh)
    bench.init_predictor(emm.predictor, boxes)
    g = torch.Generator().manual_seed(7)
    half = [tuple(torch.randn((B, channels, H // s, W // s), generator=g).to(dtype).to(dev) for s in (4, 8, 16, 32, 64))
            for _ in range(2)]
    full = [tuple(f.float() for f in fs) for fs in half]          # the same values as fp32: A and C compute the same bits
    dets = []
    for b in range(B):
        d = BoxList(boxes.to(dev), image_wh, mode="xyxy")
        d.add_field("ids", torch.arange(b * n, (b + 1) * n, device=dev))
        d.add_field("labels", torch.ones(n, dtype=torch.int64, device=dev))
        dets.append(d)
    return emm, half, full, dets


def run_case(name, B, channels, net_hw, n, dtype_name, steps, warmup, dev, forms="ABC"):
    emm, half, full, dets = make_case(B, channels, net_hw, n, DTYPES[dtype_name], dev)
    det_arg = dets if B > 1 else dets[0]

    def stepper(maps_of):
        with torch.no_grad():
            state = list(emm.extract_cache(maps_of(1), det_arg))

        def step(k):
            z, sr, d = state
            m = maps_of(k & 1)
            emm(m, d, sr, template_features=z)
            state[:] = emm.extract_cache(m, det_arg)
        return step

    steppers = {"A": stepper(lambda i: full[i]),
                "B": stepper(lambda i: tuple(f.float() for f in half[i])),
                "C": stepper(lambda i: half[i])}
    out = {"case": name, "images": B, "channels": channels, "net_hw": list(net_hw), "tracks_per_image": n,
           "maps": dtype_name, "steps": steps}
    acc = {f: [0.0, 0.0] for f in forms}
    for _ in range(2):                                            # interleaved halves
        for f in forms:
            gpu_s, host_s = time_loop(steppers[f], steps // 2, warmup)
            acc[f][0] += gpu_s
            acc[f][1] += host_s
    done = 2 * (steps // 2)
    labels = {"A": "A_fp32_maps", "B": "B_half_maps_cast_to_fp32", "C": "C_half_maps_typed"}
    for f, (gpu_s, host_s) in acc.items():
        out[labels[f]] = {"frame_pairs_per_s": B * done / gpu_s, "us_per_frame_pair": gpu_s / (B * done) * 1e6,
                          "host_enqueue_us_per_step": host_s / done * 1e6}
    if "A" in acc and "C" in acc:
        out["C_over_A_time"] = acc["C"][0] / acc["A"][0]
    if "B" in acc and "C" in acc:
        out["C_over_B_time"] = acc["C"][0] / acc["B"][0]
    # A and C compute the same thing: check once, bit for bit
    with torch.no_grad():
        res = []
        for maps in (full, half):
            z, sr, d = emm.extract_cache(maps[0], det_arg)
            _, r, _ = emm(maps[1], d, sr, template_features=z)
            res.append((z, [x.bbox for x in r], [x.get_field("scores") for x in r]))
        same = torch.equal(res[0][0], res[1][0])
        for a, b in zip(res[0][1] + res[0][2], res[1][1] + res[1][2]):
            same &= bool(torch.equal(a, b))
    out["C_bitwise_equal_to_A"] = bool(same)
    del emm, half, full, steppers
    torch.cuda.empty_cache()
    return out


CASES = [("configs[1]", 128, (704, 1280), 30), ("configs[2]", 128, (704, 1280), 100), ("configs[4]", 256, (1056, 1920), 50)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="configs[1], one camera, fp16 only (for the kernel-trace runs)")
    ap.add_argument("--forms", default="ABC", help="which of the forms A, B, C to run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    if args.quick:
        todo = [(CASES[0], 1, "fp16")]
    else:
        todo = [(c, B, t) for c in CASES for B in (1, 4) for t in ("fp16", "bf16")]
    results = []
    for (name, C, hw, n), B, t in todo:
        r = run_case(name, B, C, hw, n, t, args.steps, args.warmup, dev, args.forms)
        results.append(r)
        print(json.dumps(r), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
