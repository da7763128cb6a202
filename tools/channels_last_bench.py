"""Channels-last feature maps through the EMM head: what a channels-last backbone pays with and without the in-place kernels.

    python tools/channels_last_bench.py [--steps K] [--warmup W] [--out profiles/channels_last_bench.json] [--quick]

One step = a frame pair (EMM.forward + EMM.extract_cache) of every image, through the public module.  Three forms are
timed in ONE process, interleaved (A B C A B C ...) so that clock drift favours none:

    A  NCHW maps through the head (the path that always existed);
    B  channels-last maps, ``.contiguous()`` on every level made HERE, then the head (what such a user paid before the
       channels-last kernels: the tool makes the copy itself, so that B does not depend on the code under test);
    C  channels-last maps through the head as they are (``SMOT_FEAT_CHANNELS_LAST``).

Timed with device events around a synchronised loop; the K steps of a form are split over ``REPEATS`` interleaved repeats
and ``A_spread_us`` is the spread (max - min) of A's per-frame-pair time over them — the yardstick for "C below B".
Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script (``--quick --forms A`` /
``--forms C``; profiles/channels_last_kernel_stats.md).
Cases: configs[1] (704x1280, C = 128, 30 tracks), configs[2] (100 tracks), configs[4] (1056x1920, C = 256, 50 tracks); one
camera and a batch of 4; fp32 and fp16.
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

DTYPES = {"fp32": torch.float32, "fp16": torch.float16}
REPEATS = 4
CL = torch.channels_last


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
    cl_maps = [tuple(torch.randn((B, channels, H // s, W // s), generator=g).to(dtype).to(dev).to(memory_format=CL)
                  for s in (4, 8, 16, 32, 64)) for _ in range(2)]                   # channels-last
    nchw_maps = [tuple(f.contiguous() for f in fs) for fs in cl_maps]     # the same values as NCHW: A and C compute the same bits
    dets = []
    for b in range(B):
        d = BoxList(boxes.to(dev), image_wh, mode="xyxy")
        d.add_field("ids", torch.arange(b * n, (b + 1) * n, device=dev))
        d.add_field("labels", torch.ones(n, dtype=torch.int64, device=dev))
        dets.append(d)
    return emm, cl_maps, nchw_maps, dets


def run_case(name, B, channels, net_hw, n, dtype_name, steps, warmup, dev, forms="ABC"):
    emm, cl_maps, nchw_maps, dets = make_case(B, channels, net_hw, n, DTYPES[dtype_name], dev)
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

    steppers = {"A": stepper(lambda i: nchw_maps[i]),
                "B": stepper(lambda i: tuple(f.contiguous() for f in cl_maps[i])),
                "C": stepper(lambda i: cl_maps[i])}
    out = {"case": name, "images": B, "channels": channels, "net_hw": list(net_hw), "tracks_per_image": n,
           "maps": dtype_name, "steps": steps}
    acc = {f: [0.0, 0.0] for f in forms}
    per = {f: [] for f in forms}                                  # us per frame pair of every repeat
    part = steps // REPEATS
    for _ in range(REPEATS):                                      # interleaved repeats
        for f in forms:
            gpu_s, host_s = time_loop(steppers[f], part, warmup)
            acc[f][0] += gpu_s
            acc[f][1] += host_s
            per[f].append(gpu_s / (B * part) * 1e6)
    done = REPEATS * part
    labels = {"A": "A_nchw_maps", "B": "B_channels_last_maps_copied_to_nchw", "C": "C_channels_last_maps_in_place"}
    for f, (gpu_s, host_s) in acc.items():
        out[labels[f]] = {"frame_pairs_per_s": B * done / gpu_s, "us_per_frame_pair": gpu_s / (B * done) * 1e6,
                          "host_enqueue_us_per_step": host_s / done * 1e6, "us_per_frame_pair_repeats": per[f]}
    if "A" in per:
        out["A_spread_us"] = max(per["A"]) - min(per["A"])
    if "B" in acc and "C" in acc and "A" in per:
        b_us, c_us = acc["B"][0] / (B * done) * 1e6, acc["C"][0] / (B * done) * 1e6
        out["B_minus_C_us"] = b_us - c_us
        out["C_below_B_by_more_than_A_spread"] = bool(b_us - c_us > out["A_spread_us"])
    if "A" in acc and "C" in acc:
        out["C_over_A_time"] = acc["C"][0] / acc["A"][0]
    if "B" in acc and "C" in acc:
        out["C_over_B_time"] = acc["C"][0] / acc["B"][0]
    # A and C compute the same thing: check once, bit for bit
    with torch.no_grad():
        res = []
        for maps in (nchw_maps, cl_maps):
            z, sr, d = emm.extract_cache(maps[0], det_arg)
            _, r, _ = emm(maps[1], d, sr, template_features=z)
            res.append((z, [x.bbox for x in r], [x.get_field("scores") for x in r]))
        same = torch.equal(res[0][0], res[1][0])
        for a, b in zip(res[0][1] + res[0][2], res[1][1] + res[1][2]):
            same &= bool(torch.equal(a, b))
    out["C_bitwise_equal_to_A"] = bool(same)
    del emm, cl_maps, nchw_maps, steppers
    torch.cuda.empty_cache()
    return out


CASES = [("configs[1]", 128, (704, 1280), 30), ("configs[2]", 128, (704, 1280), 100), ("configs[4]", 256, (1056, 1920), 50)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="configs[1], one camera, fp32 only (for the kernel-trace runs)")
    ap.add_argument("--forms", default="ABC", help="which of the forms A, B, C to run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    if args.quick:
        todo = [(CASES[0], 1, "fp32")]
    else:
        todo = [(c, B, t) for c in CASES for B in (1, 4) for t in ("fp32", "fp16")]
    results = []
    for (name, C, hw, n), B, t in todo:
        r = run_case(name, B, C, hw, n, t, args.steps, args.warmup, dev, args.forms)
        results.append(r)
        print(json.dumps(r), flush=True)
    failed = [(r["case"], r["images"], r["maps"]) for r in results if r.get("C_below_B_by_more_than_A_spread") is False]
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    if failed:
        print("FAILED: C is not below B by more than the spread of A in %s" % (failed,), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
