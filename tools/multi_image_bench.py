"""Several cameras on one GPU: B video streams through ONE batched EMM call per half of a frame pair, against B sequential
single-image calls in the same process.

    python tools/multi_image_bench.py [--steps K] [--warmup W] [--out profiles/multi_image_bench.json]

One step = every stream's frame pair (EMM.forward + EMM.extract_cache), through the public module: batched = one
``forward`` and one ``extract_cache`` over lists of B BoxLists on ``[B, C, H, W]`` maps; sequential = the single-image
calls for image 0, 1, .. B-1 on views of the same maps.  Timed with device events around a synchronised loop of K steps;
``host_enqueue_us_per_step`` is the host wall time of that loop's enqueue (before the synchronisation).  Kernel times come
from a separate ``rocprofv3 --kernel-trace --stats`` run of this script (profiles/).
Cases: configs[1] maps (704x1280, C=128), 30 tracks per image, B = 1, 2, 4, 8; configs[4] maps (1056x1920, C=256), B = 2.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402


def make_case(B, channels, net_hw, n, dev):
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
    feats = [tuple(torch.randn((B, channels, H // s, W // s), generator=g).to(dev) for s in (4, 8, 16, 32, 64))
             for _ in range(2)]
    dets = []
    for b in range(B):
        d = BoxList(boxes.to(dev), image_wh, mode="xyxy")
        d.add_field("ids", torch.arange(b * n, (b + 1) * n, device=dev))
        d.add_field("labels", torch.ones(n, dtype=torch.int64, device=dev))
        dets.append(d)
    return emm, feats, dets


def time_loop(step, steps, warmup):
    with torch.no_grad():
        for k in range(warmup):
            step(k)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        t_host = time.perf_counter() - t0
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, t_host


def run_case(B, channels, net_hw, n, steps, warmup, dev):
    emm, feats, dets = make_case(B, channels, net_hw, n, dev)
    img = [[tuple(f[b:b + 1] for f in fs) for b in range(B)] for fs in feats]

    # batched: one forward + one extract_cache for all B streams
    with torch.no_grad():
        state_b = list(emm.extract_cache(feats[1], dets))

    def step_batched(k):
        z, sr, d = state_b
        emm(feats[k & 1], d, sr, template_features=z)
        state_b[:] = emm.extract_cache(feats[k & 1], dets)

    # sequential: the single-image calls of image 0 .. B-1
    with torch.no_grad():
        state_s = [emm.extract_cache(img[1][b], dets[b]) for b in range(B)]

    def step_seq(k):
        for b in range(B):
            z, sr, d = state_s[b]
            emm(img[k & 1][b], d, sr, template_features=z)
            state_s[b] = emm.extract_cache(img[k & 1][b], dets[b])

    out = {"images": B, "channels": channels, "net_hw": list(net_hw), "tracks_per_image": n, "steps": steps}
    # interleaved halves (A B A B) so that clock drift does not favour either form
    acc = {"batched": [0.0, 0.0], "sequential": [0.0, 0.0]}
    for _ in range(2):
        for name, fn in (("batched", step_batched), ("sequential", step_seq)):
            gpu_s, host_s = time_loop(fn, steps // 2, warmup)
            acc[name][0] += gpu_s
            acc[name][1] += host_s
    done = 2 * (steps // 2)
    for name, (gpu_s, host_s) in acc.items():
        out[name] = {"frame_pairs_per_s": B * done / gpu_s, "us_per_frame_pair": gpu_s / (B * done) * 1e6,
                     "us_per_step": gpu_s / done * 1e6, "host_enqueue_us_per_step": host_s / done * 1e6}
    out["batched_over_sequential"] = out["batched"]["frame_pairs_per_s"] / out["sequential"]["frame_pairs_per_s"]
    # the two forms compute the same thing: check once, bit for bit
    with torch.no_grad():
        zb, srb, db = emm.extract_cache(feats[0], dets)
        _, rb, _ = emm(feats[1], db, srb, template_features=zb)
        same = True
        for b in range(B):
            zs, srs, ds = emm.extract_cache(img[0][b], dets[b])
            _, rs, _ = emm(img[1][b], ds, srs, template_features=zs)
            same &= bool(torch.equal(rs[0].bbox, rb[b].bbox) and torch.equal(rs[0].get_field("scores"), rb[b].get_field("scores")))
    out["bitwise_equal_to_sequential"] = same
    del emm, feats, img, state_b, state_s
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="configs[1] at B = 4 only (for the kernel-trace run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    cases = [(4, 128, (704, 1280), 30)] if args.quick else \
        [(B, 128, (704, 1280), 30) for B in (1, 2, 4, 8)] + [(2, 256, (1056, 1920), 30)]
    results = []
    for B, C, hw, n in cases:
        r = run_case(B, C, hw, n, args.steps, args.warmup, dev)
        results.append(r)
        print(json.dumps(r), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
