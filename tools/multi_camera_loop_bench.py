"""Several cameras on one GPU, the whole tracking step: B video streams through ONE ``MultiCameraTrackingLoop`` (one head
call, one solver launch, one synchronisation, one template extraction per step) against B independent default
``TrackingLoop``s stepped one after the other in the same process.

    python tools/multi_camera_loop_bench.py [--steps K] [--repeats R] [--out profiles/multi_camera_loop_bench.json]

configs[1] maps (704x1280, C=128), 30 tracks per camera held steady as in bench.py's tracking-loop leg (a head that holds
its boxes, no track started or suspended after the first frame), no box-head refinement, B = 1, 2, 4, 8, 16.  The two forms are
interleaved (A B A B ...), R repeats of K steps each; a repeat is wall time around K steps closed by a synchronisation
(every step synchronises once anyway).  Reported: the median repeat and the spread (min, max) of each form in ms per step,
and — from a separate, untimed pass — where the host spends a batched step (``host_timeline_us``).  Kernel durations come
from a ``rocprofv3 --kernel-trace --stats`` run of this script with ``--quick`` (profiles/).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

CHANNELS, NET_HW, TRACKS = 128, (704, 1280), 30


def grid_boxes(n, image_wh, dev):
    """bench.py's layout: one grid cell per track, sizes mixed so that no two boxes overlap above the NMS threshold."""
    cols = max(1, int(math.ceil(math.sqrt(n * image_wh[0] / float(image_wh[1])))))
    rows = int(math.ceil(n / float(cols)))
    bl = []
    for i in range(n):
        w, h = bench.TRACK_SIZES[(i % cols + 2 * (i // cols)) % 4]
        cx, cy = (i % cols + 0.5) * image_wh[0] / cols, (i // cols + 0.5) * image_wh[1] / rows
        x1, y1 = min(max(cx - w / 2, 0), image_wh[0] - w - 1), min(max(cy - h / 2, 0), image_wh[1] - h - 1)
        bl.append([x1, y1, x1 + w, y1 + h])
    return torch.tensor(bl, dtype=torch.float32, device=dev)


def holding_head(emm, boxes):
    """A head that holds its tracks (bench.tracking_loop_throughput): zeroed head convolutions, a regression bias that
    decodes to the box the track came from.  Same kernel work, data that keeps the track count fixed."""
    bench.init_predictor(emm.predictor, boxes.cpu())
    with torch.no_grad():
        pr = emm.predictor
        for name in ("cls", "center", "reg"):
            getattr(pr, name).weight.zero_()
        mw, mh = 2.0 * float(pr.reg.bias[0]), 2.0 * float(pr.reg.bias[1])
        dx, dy = (2.0 * mw + 1.0) / 958.0, (2.0 * mh + 1.0) / 958.0
        pr.reg.bias.copy_(torch.tensor([0.5 * mw + dx, 0.5 * mh + dy, 0.5 * mw - dx, 0.5 * mh - dy]))


def run_case(B, steps, repeats, dev):
    import siammot_amd.ops as ops
    from siammot_amd.config import get_default_cfg
    from siammot_amd.multi_camera import build_multi_camera_tracking_loop
    from siammot_amd.structures import BoxList
    from siammot_amd.track_head import build_tracking_loop
    image_wh = (NET_HW[1], NET_HW[0])
    n = TRACKS
    cfg = get_default_cfg(channels=CHANNELS)
    boxes = grid_boxes(n, image_wh, dev)
    multi = build_multi_camera_tracking_loop(cfg, B, device=dev, refine_tracks=False)
    holding_head(multi.emm, boxes)
    multi.emm.to(dev)
    singles = [build_tracking_loop(cfg, device=dev, refine_tracks=False) for _ in range(B)]
    for lp in singles:
        lp.track.tracker.load_state_dict(multi.emm.state_dict())
    g = torch.Generator(device=dev).manual_seed(7)
    feats = [tuple(torch.randn((B, CHANNELS, NET_HW[0] // s, NET_HW[1] // s), generator=g, device=dev)
                   for s in (4, 8, 16, 32, 64)) for _ in range(2)]
    views = [[tuple(f[b:b + 1] for f in fs) for b in range(B)] for fs in feats]
    ids, labels = torch.full((n,), -1, dtype=torch.int64, device=dev), torch.ones(n, dtype=torch.int64, device=dev)

    def dets(k):
        out = []
        for _ in range(B):
            d = BoxList(boxes + float(k & 1), image_wh, mode="xyxy")
            d.add_field("ids", ids)
            d.add_field("labels", labels)
            d.add_field("scores", torch.full((n,), 0.9, device=dev))
            out.append(d)
        return out

    def step_multi(k, d):
        return multi(feats[k & 1], d)

    def step_singles(k, d):
        return [singles[b](views[k & 1][b], d[b]) for b in range(B)]

    forms = (("multi_camera_loop", step_multi), ("independent_loops", step_singles))
    torch.set_grad_enabled(False)
    for _, fn in forms:                                  # frame 0 starts the n tracks of every camera
        fn(0, dets(0))
    for s_ in list(multi.solvers) + [lp.solver for lp in singles]:
        s_.start_thresh, s_.track_thresh = 2.0, 0.0     # fixed track count from here on (bench.py)
    k = 1
    t0 = time.perf_counter()
    while k < 30 or time.perf_counter() - t0 < 0.3:      # untimed frames until the clocks have ramped
        for _, fn in forms:
            fn(k, dets(k))
        k += 1
    torch.cuda.synchronize()
    k0 = k
    fb0 = ops.FALLBACKS["multi_camera_per_camera"]
    ms = {name: [] for name, _ in forms}
    last = {}
    for r in range(repeats):
        for name, fn in forms:
            ready = [dets(kk) for kk in range(k0, k0 + steps)]      # the detector's finished BoxLists: not tracker work
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for kk in range(steps):
                last[name] = fn(k0 + kk, ready[kk])
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
        k0 += steps                                      # (an even number of steps: the frame parity continues)
    held = {name: all(int((o.get_field("ids") >= 0).sum().item()) == n for o in last[name]) for name, _ in forms}
    same = all(torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("ids"), b.get_field("ids"))
               and torch.equal(a.get_field("scores"), b.get_field("scores"))
               for a, b in zip(last["multi_camera_loop"], last["independent_loops"]))

    # where the host spends a batched step: an untimed pass with clocks around the step's parts
    spent = {}

    def clocked(name, fn):
        def wrapped(*a, **kw):
            t = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                spent[name] = spent.get(name, 0.0) + time.perf_counter() - t
        return wrapped
    real = (multi._propagate, ops.track_solve_batched, ops.track_solve_records, multi.emm.extract_cache,
            [t.get_track_memory for t in multi.tracks])
    multi._propagate = clocked("head: memories to one call, enqueue", real[0])
    ops.track_solve_batched = clocked("solver: tables and launch", real[1])
    ops.track_solve_records = clocked("records: copy + the step's synchronisation (waits for head and solver)", real[2])
    multi.emm.extract_cache = clocked("extraction: enqueue", real[3])
    for t, fn in zip(multi.tracks, real[4]):
        t.get_track_memory = clocked("memories: per camera, on the host", fn)
    ready = [dets(kk) for kk in range(k0, k0 + steps)]
    t0 = time.perf_counter()
    for kk in range(steps):
        step_multi(k0 + kk, ready[kk])
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    del multi._propagate, multi.emm.extract_cache
    ops.track_solve_batched, ops.track_solve_records = real[1], real[2]
    for t in multi.tracks:
        del t.get_track_memory
    timeline = {name: round(v / steps * 1e6, 1) for name, v in spent.items()}
    timeline["everything else in the step (BoxLists, mirrors, Python)"] = round((total - sum(spent.values())) / steps * 1e6, 1)
    torch.set_grad_enabled(True)

    def summary(v):
        return {"ms_per_step_median": round(statistics.median(v), 5), "ms_per_step_min": round(min(v), 5),
                "ms_per_step_max": round(max(v), 5), "ms_per_step_repeats": [round(x, 5) for x in v],
                "ms_per_camera_frame_median": round(statistics.median(v) / B, 5)}
    out = {"cameras": B, "channels": CHANNELS, "net_hw": list(NET_HW), "tracks_per_camera": n, "steps_per_repeat": steps,
           "repeats": repeats, "multi_camera_loop": summary(ms["multi_camera_loop"]),
           "independent_loops": summary(ms["independent_loops"]),
           "multi_over_independent_time": round(statistics.median(ms["multi_camera_loop"])
                                                / statistics.median(ms["independent_loops"]), 4),
           "track_count_held": held, "last_step_equal_to_independent_loops": bool(same),
           "camera_by_camera_steps": ops.FALLBACKS["multi_camera_per_camera"] - fb0, "host_timeline_us": timeline}
    del multi, singles, feats, views
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per repeat (even)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="B = 4 and 8, two short repeats (for the kernel-trace run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    assert args.steps % 2 == 0 and args.repeats >= 1
    dev = torch.device("cuda:0")
    cases, steps, repeats = ((4, 8), 60, 2) if args.quick else ((1, 2, 4, 8, 16), args.steps, args.repeats)
    results = []
    for B in cases:
        r = run_case(B, steps, repeats, dev)
        results.append(r)
        print(json.dumps(r), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
