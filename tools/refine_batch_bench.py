"""Box-head refinement of the propagated tracks for B cameras: one batched library call against B one-image calls, and the
multi-camera tracking step with the batched refinement against the same step refining camera by camera.

    python tools/refine_batch_bench.py [--steps K] [--repeats R] [--out profiles/refine_batch_bench.json]

The headline maps (704 x 1280 input, C = 128, strides 4..32), the yaml's box head (7 x 7 pooler, 1024-1024 MLP, K = 2), 30
tracks per camera, B = 1, 2, 4, 8, 16 cameras with different map contents.

  calls  A  ``RefineTracks.refine_raw`` on each camera in turn (``smot_box_refine_typed_fwd``: six launches per camera, the
            weights streamed once per camera);
         B  one ``RefineTracks.refine_raw_batched`` (``smot_box_refine_batched_typed_fwd``: eight launches whatever B is, the
            weights streamed once per 128 rows).
         Neither form synchronises; a repeat is K calls between two device events.  The outputs of the two forms are compared
         bit for bit.
  loop   A  ``MultiCameraTrackingLoop`` with ``batched_refinement = False``: ``RefineTracks.__call__`` per camera (the torch
            path: library GEMMs and the BoxList post-processor with its host synchronisations);
         B  the same loop with the batched refinement (one call per step).
         A repeat is wall time around K steps closed by a synchronisation, as in tools/multi_camera_loop_bench.py, whose
         holding head and steady 30 tracks per camera are used; the box head's regression is zeroed so that it holds the boxes.

The forms of a pair are interleaved in one process (A B A B ...), R repeats each; reported are the median and the spread (min,
max) over the repeats.  The tool reports; it sets no ratio.  ``--quick``: B = 1 and 4, two short repeats (for a kernel trace).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from multi_camera_loop_bench import CHANNELS, NET_HW, TRACKS, grid_boxes, holding_head  # noqa: E402

STRIDES = (4, 8, 16, 32)


def summary(v, B, unit):
    return {unit + "_median": round(statistics.median(v), 4), unit + "_min": round(min(v), 4), unit + "_max": round(max(v), 4),
            unit + "_repeats": [round(x, 4) for x in v], unit + "_per_camera_median": round(statistics.median(v) / B, 4)}


def make_refine(cfg, dev, hold):
    from siammot_amd.box_refine import TrackBoxHead, build_refine_tracks
    torch.manual_seed(11)
    head = TrackBoxHead(cfg, CHANNELS).to(dev).eval()
    with torch.no_grad():
        head.predictor.cls_score.bias.copy_(torch.tensor([-4.0, 4.0], device=dev))
        if hold:                                             # zero deltas decode to the box that went in
            head.predictor.bbox_pred.weight.zero_()
            head.predictor.bbox_pred.bias.zero_()
    return build_refine_tracks(cfg, CHANNELS, box_head=head)


def run_calls(B, steps, repeats, dev):
    from siammot_amd.config import get_default_cfg
    image_wh = (NET_HW[1], NET_HW[0])
    n = TRACKS
    refine = make_refine(get_default_cfg(channels=CHANNELS), dev, hold=False)
    g = torch.Generator(device=dev).manual_seed(7)
    feats = [tuple(torch.randn((B, CHANNELS, NET_HW[0] // s, NET_HW[1] // s), generator=g, device=dev) for s in STRIDES)
             for _ in range(2)]
    views = [[tuple(f[b:b + 1] for f in fs) for b in range(B)] for fs in feats]
    one = grid_boxes(n, image_wh, dev)
    boxes = torch.cat([one + float(b) for b in range(B)])
    conf = torch.rand((B * n,), generator=g, device=dev)
    ids = torch.arange(B * n, device=dev)
    labels = torch.ones(B * n, dtype=torch.int64, device=dev)
    rows = [n] * B
    per = [tuple(t[b * n:(b + 1) * n].contiguous() for t in (boxes, conf, ids, labels)) for b in range(B)]
    assert refine.refine_batch_ok(rows)

    def one_by_one(k):
        return [refine.refine_raw(views[k & 1][b], *per[b], image_wh) for b in range(B)]

    def batched(k):
        return refine.refine_raw_batched(feats[k & 1], boxes, conf, ids, labels, rows, image_wh)
    forms = (("A_one_call_per_camera", one_by_one), ("B_one_batched_call", batched))
    us = {name: [] for name, _ in forms}
    host = {name: [] for name, _ in forms}
    with torch.no_grad():
        t0 = time.perf_counter()
        k = 0
        while k < 20 or time.perf_counter() - t0 < 0.3:      # untimed calls until the clocks have ramped
            for _, fn in forms:
                fn(k)
            k += 1
        torch.cuda.synchronize()
        for _ in range(repeats):
            for name, fn in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                for kk in range(steps):
                    fn(kk)
                t_host = time.perf_counter() - t0
                e1.record()
                torch.cuda.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / steps)
                host[name].append(t_host / steps * 1e6)
        a, b = one_by_one(0), batched(0)
        same = all(torch.equal(torch.cat([x[j] for x in a]), b[j]) for j in range(4))
    out = {"cameras": B, "tracks_per_camera": n, "steps_per_repeat": steps, "repeats": repeats}
    for name, _ in forms:
        out[name] = summary(us[name], B, "us_per_call")
        out[name]["host_enqueue_us_per_call_median"] = round(statistics.median(host[name]), 2)
    out["A_over_B_time"] = round(out["A_one_call_per_camera"]["us_per_call_median"] / out["B_one_batched_call"]["us_per_call_median"], 4)
    out["outputs_bit_equal"] = bool(same)
    del feats, views
    torch.cuda.empty_cache()
    return out


def run_loop(B, steps, repeats, dev):
    import siammot_amd.ops as ops
    from siammot_amd.config import get_default_cfg
    from siammot_amd.multi_camera import build_multi_camera_tracking_loop
    from siammot_amd.structures import BoxList
    image_wh = (NET_HW[1], NET_HW[0])
    n = TRACKS
    cfg = get_default_cfg(channels=CHANNELS)
    refine = make_refine(cfg, dev, hold=True)
    boxes = grid_boxes(n, image_wh, dev)
    loops = {}
    for name, on in (("A_refine_camera_by_camera", False), ("B_batched_refinement", True)):
        lp = build_multi_camera_tracking_loop(cfg, B, device=dev, refine_tracks=refine)
        if loops:
            lp.emm.load_state_dict(next(iter(loops.values())).emm.state_dict())
        else:
            holding_head(lp.emm, boxes)
            lp.emm.to(dev)
        lp.batched_refinement = on
        loops[name] = lp
    g = torch.Generator(device=dev).manual_seed(7)
    feats = [tuple(torch.randn((B, CHANNELS, NET_HW[0] // s, NET_HW[1] // s), generator=g, device=dev)
                   for s in (4, 8, 16, 32, 64)) for _ in range(2)]
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
    torch.set_grad_enabled(False)
    for lp in loops.values():                                # frame 0 starts the n tracks of every camera
        lp(feats[0], dets(0))
        for s_ in lp.solvers:
            s_.start_thresh, s_.track_thresh = 2.0, 0.0     # fixed track count from here on (bench.py)
    k = 1
    t0 = time.perf_counter()
    while k < 12 or time.perf_counter() - t0 < 0.3:
        for lp in loops.values():
            lp(feats[k & 1], dets(k))
        k += 1
    torch.cuda.synchronize()
    k0 = k
    fb0 = ops.FALLBACKS["refine_per_camera"]
    ms = {name: [] for name in loops}
    last = {}
    for _ in range(repeats):
        for name, lp in loops.items():
            ready = [dets(kk) for kk in range(k0, k0 + steps)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for kk in range(steps):
                last[name] = lp(feats[(k0 + kk) & 1], ready[kk])
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
        k0 += steps
    held = {name: all(int((o.get_field("ids") >= 0).sum().item()) == n for o in last[name]) for name in loops}
    torch.set_grad_enabled(True)
    out = {"cameras": B, "tracks_per_camera": n, "steps_per_repeat": steps, "repeats": repeats}
    for name in loops:
        out[name] = summary(ms[name], B, "ms_per_step")
    out["A_over_B_time"] = round(out["A_refine_camera_by_camera"]["ms_per_step_median"]
                                 / out["B_batched_refinement"]["ms_per_step_median"], 4)
    out["track_count_held"] = held
    out["refine_per_camera_fallbacks"] = ops.FALLBACKS["refine_per_camera"] - fb0
    del loops, feats
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="calls / steps per repeat (even)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="B = 1 and 4, two short repeats (for the kernel-trace run)")
    ap.add_argument("--no-loop", action="store_true", help="the calls only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    assert args.steps % 2 == 0 and args.repeats >= 1
    dev = torch.device("cuda:0")
    cases, steps, repeats = ((1, 4), 40, 2) if args.quick else ((1, 2, 4, 8, 16), args.steps, args.repeats)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "channels": CHANNELS, "net_hw": list(NET_HW),
           "box_head": "7x7 pooler, 1024-1024, K=2", "calls": [], "loop": []}
    for B in cases:
        r = run_calls(B, steps, repeats, dev)
        doc["calls"].append(r)
        print(json.dumps({"calls": r}), flush=True)
    if not args.no_loop:
        for B in cases:
            r = run_loop(B, max(steps // 2, 2) & ~1, repeats, dev)
            doc["loop"].append(r)
            print(json.dumps({"loop": r}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
