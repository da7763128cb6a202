#!/usr/bin/env python
"""Benchmark of the EMM tracker-head hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--tracks 30]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One STEP = one frame pair through the hot path (BASELINE.json north_star):
``EMM.forward`` on frame t (ROIAlign of the search regions with virtual padding -> depthwise
cross-correlation -> prediction towers + heads -> fused up-sample/decode) followed by
``EMM.extract_cache`` on frame t (template ROIAlign + search regions for frame t+1), at
BASELINE.json configs[1]: DLA-34-FPN feature maps of a 720p frame (net input 704x1280, C=128,
5 FPN levels), 30 active tracks.  Inputs are synthetic, seeded, and RESIDENT IN HBM before the timed
region.  The DLA-34-FPN backbone, RPN and box head are NOT in the timed region (they are PyTorch
modules outside the hot path) — `config.workload` says so.

Multi-GPU (--gpus N): one process per GPU, each running its own independent stream;
the predictor weights are broadcast once from rank 0 over RCCL before timing; no per-frame
collective.  Weak scaling: value = N * K / max-over-ranks(elapsed).  ``python bench.py --gpus N`` without a
torchrun environment launches its own ranks (re-executes itself under ``torch.distributed.run`` on 127.0.0.1);
rank 0 prints the one JSON line either way.

A plain run sets up, warms up, times K steps and prints the headline: `metric`, `value`, `unit`, `higher_is_better`,
`dtype`, `ms_per_step` (+ the run's configuration and fallback counters).  ``--dump-outputs DIR`` also writes what the
last timed step returned to its caller (tracked boxes / scores / ids of ``EMM.forward``, template features and search
regions of ``EMM.extract_cache``) as DIR/<name>.npy (float32 / float64); the inputs are seeded, so two builds given the
same arguments can be compared output for output.

``--full`` adds every other leg below (each off in a plain run; the ``--no-*`` options still switch single legs off).
With ``--full`` the timed loop carries the kernel event brackets of `roofline` on every 16th step, as it always has.
The JSON line then also carries:
  roofline     — the kernel that runs the cross-correlation in the pipeline (search-region ROIAlign fused with the
                 depthwise xcorr): algorithmic bytes = window cells actually touched + templates + response
                 (SURVEY.md §8(d)-B restricted to that kernel, computed from the boxes) / the average launch duration
                 from the launch's own start/stop events (hipExtLaunchKernel, every 16th step of the timed region);
                 `traffic` = 2 x FETCH_SIZE + WRITE_SIZE of separate --pmc passes (profiles/xcorr_traffic.json);
                 `xcorr_op` = the stand-alone operator (figure A of §8(d)) timed the same way.
  roofline_tower / roofline_path — the towers against the fp32 matrix pipe (executed multiply-adds), the whole frame
                 pair against HBM (compulsory bytes / ms_per_step).
  tracking_loop — head + solver + memory per frame, with and without box-head refinement, track count asserted;
                 `next_frame_shown`: the same with every call shown the next frame's features (speculative next-frame
                 head); `with_dormant_tracks`: a fifth of the tracks dormant — their rows of the memory copied on the
                 device, in the reference's host form, and with the next frame shown.
  cpu_baseline — the CPU oracle (oracle/emm_oracle.py, the reference's torch-CPU ops) timed on this
                 host's cores on the same workload (rank 0, N=1 only), bounded to ~10-20 s.
  parity       — the LAST result of the timed loop compared, outside the timed region, with the CPU oracle on the
                 same inputs, and the same kernels on frames 0/1 compared with tests/golden/bench_n<N>.npz, the
                 output of the reference's own code on these tensors (oracle/gen_golden_bench.py).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

CLOCK_GHZ = 2.4            # MI355X peak engine clock (MI355X_MICROARCH.md); sustained clocks under this load are ~2.1
HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; ~6.3 TB/s achievable)
METRIC = "frame-pairs/sec at 720p, 30 active tracks; EMM xcorr HBM GB/s vs peak"
NET_HW = (704, 1280)       # 720p under MIN_SIZE_TEST 800 / MAX 1280 / divisibility 32
CHANNELS = 128
TIMER_STRIDE = 16          # kernel event brackets on every 16th step of the timed region
MIN_TIMER_SAMPLES = 200    # bracketed launches per instrumented kernel (a short post-loop tops the count up)
FEATURE_SETS = 8           # distinct synthetic frames the timed loop rotates through: 8 x 38.4 MB = 307 MB, more
                           # than the 256 MiB Infinity Cache, so window reads are not served by a cache that two
                           # alternating frames would stay resident in
TRACK_SIZES = [(32, 64), (64, 128), (100, 200), (160, 320)]    # (w,h): FPN levels 0,0,1,2


def synthetic_boxes(n, image_wh):
    """Non-overlapping grid of boxes cycling the four sizes, fully inside the image."""
    W, H = image_wh
    cols = max(1, W // 180)
    boxes = []
    for i in range(n):
        w, h = TRACK_SIZES[i % 4]
        cx = 90 + 180 * (i % cols)
        cy = 170 + 340 * ((i // cols) % max(1, H // 340))
        # tracks beyond the grid capacity wrap with a small offset (crowd regime, configs[2])
        off = 7.0 * (i // (cols * max(1, H // 340)))
        x1 = min(max(cx - w / 2 + off, 0), W - w - 1)
        y1 = min(max(cy - h / 2 + off, 0), H - h - 1)
        boxes.append([x1, y1, x1 + w, y1 + h])
    return torch.tensor(boxes, dtype=torch.float32)


def synthetic_features(seed, device):
    g = torch.Generator().manual_seed(seed)
    H, W = NET_HW
    return tuple(torch.randn((1, CHANNELS, H // s, W // s), generator=g).to(device) for s in (4, 8, 16, 32, 64))


def fused_source_sha1():
    """Hash of the sources the graded kernel is compiled from (the stamp of profiles/xcorr_traffic.json: the GPU box has
    no git history, the sources travel)."""
    import hashlib
    h = hashlib.sha1()
    for f in ("sr_xcorr.hip", "roi_common.h", "xcorr_f16x2.h", "xcorr_patch1.h", "smot_common.h"):
        h.update(open(os.path.join(ROOT, "siam-mot_amd", "csrc", f), "rb").read())
    return h.hexdigest()


def other_config_runs(args):
    """BASELINE.json configs[2] (100 tracks) and configs[4] (C=256, 1056x1920, 50 tracks) after the headline: each in a
    child process of this script (the module's shape constants are process-wide), 200 timed steps, its own kernel
    rooflines and its own parity against the oracle and the reference golden of that configuration."""
    import subprocess
    runs = {"configs[2]": ["--tracks", "100"],
            "configs[4]": ["--channels", "256", "--net-hw", "1056", "1920", "--tracks", "50"]}
    out = {}
    for name, extra in runs.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--full", "--steps", "200", "--warmup", "50", "--prewarm-ms", "200",
               "--no-cpu-baseline", "--no-graph", "--extra-streams", "0", "--no-tracking-loop", "--no-other-configs", "--other-config-worker",
               "--argmax-pairs", "30" if name == "configs[2]" else "0"] + extra
        try:
            r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
            line = [ln for ln in r.stdout.decode("utf-8", "replace").splitlines() if ln.startswith("{")]
            d = json.loads(line[-1])
            out[name] = {k: d.get(k) for k in ("value", "unit", "ms_per_step", "steps", "config", "roofline", "roofline_tower",
                                               "roofline_path", "parity", "fallbacks")}
            out[name]["roofline"] = {k: v for k, v in (d.get("roofline") or {}).items() if k != "xcorr_op"}
        except Exception as e:
            out[name] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
    return out


def fused_algorithmic_bytes(boxes, image_wh, channels, rz=15, rx=30, pad_pixels=512, search_expansion=1.0):
    """Compulsory HBM bytes of the fused search-region-pool + xcorr kernel for these tracks (SURVEY.md §8d
    formula B restricted to that kernel): every feature cell of a track's search window read once
    (virtual zero border excluded), its template read once, its response written once.
        fp(sr, l) = (ceil(x2 s) - floor(x1 s) + 1) * (ceil(y2 s) - floor(y1 s) + 1), clipped to the real map."""
    import math
    W, H = image_wh
    total_cells = 0
    for x1, y1, x2, y2 in boxes.tolist():
        s = math.sqrt((x2 - x1 + 1) * (y2 - y1 + 1))
        lvl = int(min(max(math.floor(4 + math.log2(s / 224 + 1e-6)), 2), 5)) - 2
        scale = 1.0 / (4 * 2 ** lvl)
        w, h = x2 - x1 + 1, y2 - y1 + 1
        wx, hy = w * search_expansion / 2.0, h * search_expansion / 2.0
        sx1, sy1, sx2, sy2 = x1 - wx, y1 - hy, x2 + wx, y2 + hy            # un-padded image coordinates
        mw, mh = W // (4 * 2 ** lvl), H // (4 * 2 ** lvl)
        cx1, cx2 = max(math.floor(sx1 * scale), 0), min(math.ceil(sx2 * scale), mw - 1)
        cy1, cy2 = max(math.floor(sy1 * scale), 0), min(math.ceil(sy2 * scale), mh - 1)
        total_cells += max(cx2 - cx1 + 1, 0) * max(cy2 - cy1 + 1, 0)
    ho = rx - rz + 1
    n = boxes.shape[0]
    return 4.0 * channels * total_cells + 4.0 * n * channels * (rz * rz + ho * ho)


def init_predictor(pred, boxes):
    """Random-init weights of the reference architecture (there are no checkpoints offline), with
    biases that keep the decode non-degenerate (SURVEY.md §7 'Degenerate synthetic weights')."""
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in pred.named_parameters():
            if name.endswith("0.weight") or name in ("cls.weight", "center.weight", "reg.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
        mw = float((boxes[:, 2] - boxes[:, 0]).mean())
        mh = float((boxes[:, 3] - boxes[:, 1]).mean())
        pred.reg.bias.copy_(torch.tensor([0.5 * mw, 0.5 * mh, 0.5 * mw, 0.5 * mh]))


def _cpu_threads():
    """Threads for the CPU leg: the cores this process may actually run on (cgroup/affinity aware —
    os.cpu_count() reports the whole host and oversubscribing OpenMP stalls for minutes), capped at 32
    (the workload's tensors are small; more threads only add fork/join cost)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 32))


def cpu_baseline_worker(n_tracks, budget_s):
    """Time the oracle (reference torch-CPU ops) on the same frame-pair workload; prints one JSON line."""
    from oracle import emm_oracle as O            # checker / baseline only — never the product path
    threads = _cpu_threads()
    torch.set_num_threads(threads)
    feats = synthetic_features(0, "cpu")
    boxes = synthetic_boxes(n_tracks, (NET_HW[1], NET_HW[0]))
    cfg = O.EMMConfig(channels=CHANNELS)
    from siammot_amd.config import get_default_cfg
    from siammot_amd.emm import EMMPredictor
    pred = EMMPredictor(get_default_cfg(channels=CHANNELS))
    init_predictor(pred, boxes)
    params = {k: v.detach() for k, v in pred.named_parameters()}

    # ROIAlign as compiled C (oracle/csrc/roi_align_cpu.c, upstream's CPU algorithm, OpenMP over rois — bit-identical to the
    # oracle's torch restatement) when oracle/_build holds it: the reference runs a C++ operator there, not Python
    roi = O.roi_align_c if O.roi_align_c_library() is not None else None

    def step():
        z, sr = O.extract_cache(cfg, feats, boxes, roi_align=roi)
        return O.emm_forward(cfg, params, feats, boxes, sr, z, (NET_HW[1], NET_HW[0]), reference_ops=True, roi_align=roi)

    def staged():
        """The same frame pair, stage by stage (BASELINE.md §3 asks for per-stage ms): the calls ``emm_forward`` /
        ``extract_cache`` make, timed one by one."""
        ms = {}

        def timed(name, fn):
            t0 = time.perf_counter()
            r = fn()
            ms[name] = ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return r
        z = timed("template_roi_align", lambda: O.sr_pool(feats, boxes, None, cfg.rz, cfg.scales, cfg.sampling_ratio, roi))
        sr = timed("search_region_geometry", lambda: O.search_region(boxes, cfg.pad_pixels, cfg.search_expansion, cfg.min_search_wh))
        padded = timed("pad_feature", lambda: O.pad_features(feats, cfg.pad_pixels))
        x = timed("search_region_roi_align", lambda: O.sr_pool(padded, boxes, sr, cfg.rx, cfg.scales, cfg.sampling_ratio, roi))
        resp = timed("xcorr_depthwise", lambda: O.xcorr_depthwise_conv(x, z))
        cls, center, reg = timed("predictor_towers_and_heads", lambda: O.predictor(resp, params, cfg.gn_groups, cfg.gn_eps))
        ups = timed("bicubic_x16", lambda: [O.bicubic_upsample_torch(t) for t in (cls, center, reg)])
        xs, ys = timed("get_locations", lambda: O.grid_axes(sr, cfg.rx, cfg.rz, cfg.pad_pixels))
        bb, conf, _ = timed("decode_response", lambda: O.decode(ups[0], ups[1], ups[2], xs, ys, boxes, cfg.use_centerness, cfg.sigma))
        timed("clip_to_image", lambda: O.clip_boxes(bb, conf, (NET_HW[1], NET_HW[0])))
        return ms

    with torch.no_grad():
        step()
        t0 = time.perf_counter()
        step()
        one = time.perf_counter() - t0
        reps = int(max(3, min(50, budget_s / max(one, 1e-3))))
        times = []
        t_start = time.perf_counter()
        for _ in range(reps):
            t0 = time.perf_counter()
            step()
            times.append(time.perf_counter() - t0)
            if time.perf_counter() - t_start > 2 * budget_s:
                break
        stage_runs = [staged() for _ in range(3)]
    stages = {k: sorted(r[k] for r in stage_runs)[1] for k in stage_runs[0]}
    times.sort()
    med = times[len(times) // 2]
    print(json.dumps({
        "value": 1.0 / med, "unit": "frame-pairs/s", "cores": threads, "kind": "port",
        "stage_ms": {k: round(v, 3) for k, v in stages.items()},
        "stage_note": "median of 3 stage-by-stage passes of the same calls (their sum runs a few percent above ms_per_step: "
                      "timer calls, no overlap); ROIAlign: %s" % (
                          "oracle/csrc/roi_align_cpu.c — upstream's published CPU algorithm compiled with gcc -O3 -fopenmp, "
                          "parallel over rois (maskrcnn_benchmark itself is not installable here)" if roi is not None else
                          "the oracle's vectorised per-roi torch restatement (oracle/_build/libroi_align_cpu.so not built): "
                          "pessimistic against upstream's C++ operator"),
        "sample": "%d frame pairs of the same workload (%d tracks, 720p maps), median; oracle/emm_oracle.py "
                  "with the reference's torch-CPU ops (grouped conv2d, F.interpolate, physical pad_feature) and %s ROIAlign, "
                  "%d threads" % (len(times), n_tracks, "compiled-C (OpenMP)" if roi is not None else "torch-restated", threads),
        "ms_per_step": med * 1e3}))


def cpu_baseline(n_tracks, budget_s=10.0, timeout_s=150.0):
    """Run the CPU leg in a child process with a hard timeout so that bench.py always finishes."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", "--tracks", str(n_tracks),
           "--cpu-budget", str(budget_s), "--channels", str(CHANNELS), "--net-hw", str(NET_HW[0]), str(NET_HW[1])]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s, cwd=ROOT)
        for line in reversed(res.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
        return {"value": None, "unit": "frame-pairs/s", "cores": _cpu_threads(), "kind": "port",
                "sample": "cpu leg failed: %s" % (res.stderr.strip().splitlines() or ["no output"])[-1]}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "frame-pairs/s", "cores": _cpu_threads(), "kind": "port",
                "sample": "cpu leg exceeded %.0f s and was stopped" % timeout_s}


def multi_stream_throughput(emm, feats, det, n_streams, dev, steps=600):
    """S independent video streams (own track memory) on S HIP streams of one GPU: the serving configuration of
    SURVEY.md §8(e) when a GPU hosts more than one camera.  Kernels of different streams overlap, filling the
    ramp-up / tail of each other's launches.  Informational: `value` stays the single-stream number."""
    streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
    with torch.no_grad():
        states = []
        for st in streams:
            with torch.cuda.stream(st):
                states.append(emm.extract_cache(feats[1], det))

        def run(k_steps):
            for k in range(k_steps):
                for i, st in enumerate(streams):
                    with torch.cuda.stream(st):
                        z, sr, d = states[i]
                        emm(feats[k & 1], d, sr, template_features=z)
                        states[i] = emm.extract_cache(feats[k & 1], det)
        run(100)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"streams": n_streams, "steps_per_stream": steps, "value": n_streams * steps / dt, "unit": "frame-pairs/s",
            "ms_per_step_per_stream": dt / steps * 1e3,
            "note": "informational, and it does NOT use the rest of the chip: two streams reach ~1.06x of one (round 4 and "
                    "5).  One Python thread enqueues both streams (host_enqueue ~44 us of a ~63 us step: two streams are "
                    "host-bound at ~88 us per pair of steps), and each of the four kernels of a step fills the chip by "
                    "itself (480 / 240 / 510 / 480 workgroups on 256 CUs, LDS- or register-limited to one or two per CU), "
                    "so a second stream's kernels mostly queue behind the first's.  More cameras per GPU need more host "
                    "threads or processes (one per stream, as `--gpus N` runs them), not more streams in one loop"}


def hipgraph_loop_throughput(emm, feats, det, state, steps):
    """The timed frame-pair loop captured as ONE hipGraph per revolution of the feature ring
    (siammot_amd.graphs.FramePairRing: len(feats) frame pairs = 4 x len(feats) kernel launches + two small copies per
    hipGraphLaunch) and replayed: the same kernels on the same inputs, the host out of the way.  Informational — `value`
    is the eager loop; this says what a launch-overhead-free host would get and what a replay costs the host."""
    from siammot_amd.graphs import FramePairRing
    ring = FramePairRing(emm, feats, det, state)
    revs = max(4, steps // len(feats))
    for _ in range(8):
        ring.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(revs):
        ring.replay()
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the graph's last step against the eager path on the same memory: the replay computes the same frame pair
    res = ring.results[-1]
    return {"value": revs * len(feats) / dt, "unit": "frame-pairs/s", "ms_per_step": dt / (revs * len(feats)) * 1e3,
            "frame_pairs_per_graph": len(feats), "kernel_nodes_per_graph": 4 * len(feats),
            "host_us_per_step": t_host / (revs * len(feats)) * 1e6, "boxes_finite": bool(torch.isfinite(res.bbox).all()),
            "note": "informational: the replay is NOT faster than the eager loop (65 vs 63-64 us per step in rounds 4 and 5) — "
                    "the eager loop is GPU-bound already (host_enqueue ~44 us < ~63 us of kernels per step), and a graph's "
                    "kernel nodes pay the same dispatch gaps between dependent kernels (plus two small copy nodes per frame "
                    "pair).  What the graph buys is host time: `host_us_per_step` against ~44 us of eager enqueue, i.e. "
                    "headroom for a detector's launches on the same thread"}


def tracking_loop_throughput(n, dev, feats, steps=300, refine=False, native=None, loop_hint=None, ahead=False, dormant=0,
                             device_carry=True, early_head=None):
    """The whole tracker around the head (siammot_amd.track_head.TrackingLoop): EMM.forward -> [box-head refinement of
    the propagated boxes, roi_heads.py:60-84] -> merge with this frame's detections -> solver (score-banded NMS, id life
    cycle, ONE host sync) -> EMM.extract_cache + track memory.  Fixed track count: the n boxes sit on a
    grid on which neither the detections nor the propagated boxes overlap above the NMS threshold, TRACK_THRESH = 0 and
    START_TRACK_THRESH = 2 after the first frame, so the unchanged solver never suspends or starts a track;
    ``tracked_in_last_frame`` must equal n (``track_count_held``).  Informational (not part of the metric).
    ``ahead``: every call is also shown the NEXT frame's feature maps (a streaming caller has them): the loop launches the
    next frame's head speculatively behind this frame's extraction (``TrackingLoop.forward(..., next_features=)``).
    ``dormant``: that many of the n tracks are made dormant in frame 1 (stronger detections on top of them: the solver's
    NMS removes their propagated rows, track_solver.py:82-86) and stay dormant (never resumed, never expired — the MOT17
    yaml keeps them for 30 frames): the memory is n - dormant active rows + dormant carried rows, the head still tracks n
    rows per frame.  ``device_carry=False``: the reference's form of that memory (concatenated on the host every frame,
    track_head.py:77-97) instead of the device copy (``smot_memory_carry_fwd``)."""
    from siammot_amd.box_refine import build_refine_tracks
    from siammot_amd.config import get_default_cfg
    from siammot_amd.structures import BoxList
    from siammot_amd.track_head import build_tracking_loop
    image_wh = (NET_HW[1], NET_HW[0])
    # one grid cell per track; the size index is (col + 2 row) % 4, so that the 320-pixel-tall boxes of one column sit
    # two rows apart (they overlapped their vertical neighbours above IoU 0.5 on the round-2 layout and the solver's
    # NMS merged five of thirty tracks in the first frame)
    import math
    cols = max(1, int(math.ceil(math.sqrt(n * image_wh[0] / float(image_wh[1])))))
    rows = int(math.ceil(n / float(cols)))
    bl = []
    for i in range(n):
        w, h = TRACK_SIZES[(i % cols + 2 * (i // cols)) % 4]
        cx = (i % cols + 0.5) * image_wh[0] / cols
        cy = (i // cols + 0.5) * image_wh[1] / rows
        x1 = min(max(cx - w / 2, 0), image_wh[0] - w - 1)
        y1 = min(max(cy - h / 2, 0), image_wh[1] - h - 1)
        bl.append([x1, y1, x1 + w, y1 + h])
    boxes = torch.tensor(bl, dtype=torch.float32, device=dev)
    cfg = get_default_cfg(channels=CHANNELS)
    refine_fn = False
    if refine:
        refine_fn = build_refine_tracks(cfg, CHANNELS)           # DLA_34_FPN_EMM.yaml box head: 7x7 pooler, 1024-1024 MLP
        head = refine_fn.box.to(dev).eval()
        g = torch.Generator().manual_seed(2)
        with torch.no_grad():                                    # random init of the MLP and the classifier
            for name, p_ in head.named_parameters():
                if name.endswith("weight"):
                    p_.copy_((torch.randn(p_.shape, generator=g) / math.sqrt(p_.shape[1])).to(dev))
                else:
                    p_.zero_()
            head.predictor.bbox_pred.weight.zero_()             # zero deltas decode to the proposal itself: tracks hold
            head.predictor.cls_score.weight.mul_(0.2)
    loop = build_tracking_loop(cfg, device=dev, refine_tracks=refine_fn)
    if dormant:
        loop.solver.track_pool._max_dormant_frames = 1 << 30
        loop.solver.resume_track_thresh = 2.0
        loop.device_carry = bool(device_carry)
    init_predictor(loop.track.tracker.predictor, boxes.cpu())
    with torch.no_grad():
        # A tracker that HOLDS its tracks, as a trained head does on a static scene (random head weights move every box
        # by a few pixels per frame — a random walk that merges neighbours within a few hundred frames, and the count
        # does not hold): the three head convolutions are zeroed, so the penalised score is the cosine window and the
        # arg-max is its centre cell, and the regression bias is made asymmetric by the half-cell offset of the
        # reference's location grid (cell 128 of 256 sits (2w+1)/958 right of the search region's centre,
        # track_core.py:184-225), so the decoded box lands exactly on the box it came from.  Kernel work is the same;
        # only the data differs.  (Every propagated box has the size the regression bias encodes: after the first frame
        # the templates are that size, not the four-size mix of the frame-pair workload.)
        pr = loop.track.tracker.predictor
        for name in ("cls", "center", "reg"):
            getattr(pr, name).weight.zero_()
        mw, mh = 2.0 * float(pr.reg.bias[0]), 2.0 * float(pr.reg.bias[1])
        dx, dy = (2.0 * mw + 1.0) / 958.0, (2.0 * mh + 1.0) / 958.0
        pr.reg.bias.copy_(torch.tensor([0.5 * mw + dx, 0.5 * mh + dy, 0.5 * mw - dx, 0.5 * mh - dy]))
    loop.track.tracker.to(dev)

    # the detector's output of two alternating frames, resident on the device before the loop (synthesising it is
    # not tracker work); every frame gets a fresh BoxList and its own score tensor (the solver bands scores in place)
    pre = [(boxes + float(j), torch.full((n,), -1, dtype=torch.int64, device=dev),
            torch.ones(n, dtype=torch.int64, device=dev)) for j in range(2)]
    fresh_scores = list(torch.full((steps + 31, n), 0.9, device=dev).unbind(0))   # one row per frame, made before the loop
    if native is not None:
        loop.native_frame = bool(native)
    if loop_hint is not None:
        loop.loop_order_hint = bool(loop_hint)          # A/B (measure/loop_hint_ab2.py): the extraction's order hint in the loop
    if early_head is not None:
        loop.early_head = bool(early_head)              # A/B (measure/loop_early_ab.py): the next call's head prepared a call early

    suspended = []

    def dets(k):
        b, ids, labels = pre[k & 1]
        sc = fresh_scores.pop()
        if dormant and k == 2 and not suspended:
            # detections stronger than any propagated row (band (2, 3]) exactly on the boxes the last `dormant` tracks were
            # propagated to in the previous frame (they hold): the NMS removes those tracks' rows, the solver suspends them
            suspended.append(1)
            lo, li = last[0].bbox, last[0].get_field("ids")
            sel = lo[li >= n - dormant]
            if sel.shape[0] == dormant:
                b = b.clone()
                b[n - dormant:] = sel
                sc[n - dormant:] = 3.5
        d = BoxList(b, image_wh, mode="xyxy")
        d.add_field("ids", ids)
        d.add_field("labels", labels)
        d.add_field("scores", sc)
        return d
    last = [None]
    # inference runs with autograd off in the reference's callers (demos/demo_inference.py:103, engine/inferencer.py:56);
    # TrackingLoop.forward switches it off itself only when it finds it on (a context object per call: 2-7 us of host time)
    grad_was = torch.is_grad_enabled()
    torch.set_grad_enabled(False)
    out = loop(feats[0], dets(0))                     # frame 0: the n detections start n tracks
    # fixed track count: from here on the unchanged solver never starts or suspends a track — the n
    # tracks live on, every frame's n detections compete with them in NMS
    loop.solver.start_thresh, loop.solver.track_thresh = 2.0, 0.0
    lean = [0, 0]
    step_lean, step_native = loop._step_lean, loop._step_native

    def counted(*a, **k):
        lean[0] += 1
        return step_lean(*a, **k)

    def counted_native(*a, **k):
        lean[0] += 1
        lean[1] += 1
        return step_native(*a, **k)
    loop._step_lean, loop._step_native = counted, counted_native
    import siammot_amd.ops as _ops
    det_of = [dets]                                 # (the timed frames take their detections ready-made: see below)
    if ahead:
        step0 = lambda k: loop(feats[k & 1], det_of[0](k), next_features=feats[(k + 1) & 1])
    else:
        step0 = lambda k: loop(feats[k & 1], det_of[0](k))

    def step(k):
        o = last[0] = step0(k)
        return o
    for k in range(1, 30):
        out = step(k)
    torch.cuda.synchronize()
    # setup, not part of the timed frames: building the loop (random box-head weights on the CPU) left the GPU idle for
    # up to a second and its clocks at rest — single runs came out at 0.15 or 0.25-0.3 ms per frame depending on that
    # (measure/loop_native_ab.py); run untimed frames until the clocks have ramped, as the frame-pair loop does
    t_pre = time.perf_counter()
    spare = [torch.full((n,), 0.9, device=dev) for _ in range(64)]
    k = 30
    while time.perf_counter() - t_pre < 0.3:
        fresh_scores.append(spare[k & 63].fill_(0.9))
        out = step(k)
        k += 1
    torch.cuda.synchronize()
    lean[0] = lean[1] = 0
    _ops.SPECULATION.clear()
    # three equal chunks, each closed by a synchronisation; the reported time is the MEDIAN chunk's (a single 300-frame
    # span is 25-40 ms: one scheduler hiccup or collector pause of a few ms in it showed up as +40 % on one leg of one run)
    chunk = max(1, steps // 3)
    k0 = k & 1                                       # (frame parity continues: the speculative head saw feats[k & 1])
    # the timed frames' detections are BoxLists the "detector" has already returned (a detector's forward hands over a
    # finished BoxList; building one — an object, three fields — is its cost, ~4 us of Python, not the tracker's):
    # one fresh BoxList and score tensor per frame, made before the clock starts
    ready = [dets(kk) for kk in range(k0, k0 + 3 * chunk)]
    det_of[0] = lambda kk: ready[kk - k0]
    chunk_ms = []
    for c in range(3):
        t0 = time.perf_counter()
        for k in range(k0 + c * chunk, k0 + (c + 1) * chunk):
            out = step(k)
        torch.cuda.synchronize()
        chunk_ms.append((time.perf_counter() - t0) / chunk * 1e3)
    steps = 3 * chunk
    dt = sorted(chunk_ms)[1] * 1e-3 * steps
    tracked = int((out.get_field("ids") >= 0).sum().item())
    pool = loop.solver.track_pool
    torch.set_grad_enabled(grad_was)
    return {"value": steps / dt, "unit": "frames/s", "ms_per_frame": dt / steps * 1e3,
            "ms_per_frame_chunks": [round(v, 5) for v in chunk_ms], "tracks": n,
            "tracked_in_last_frame": tracked, "track_count_held": tracked == n,
            "active_tracks": len(pool.get_active_ids()), "dormant_tracks": len(pool._dormant_ids),
            "memory_rows": len(loop.track_memory[2][0]) if loop.track_memory is not None else 0,
            "dormant_rows": (("copied on the device (smot_memory_carry_fwd)" if device_carry else
                              "concatenated on the host (the reference's form)") if dormant else None),
            "refine_tracks": "TrackBoxHead (7x7 HIP pooler, 1024-1024 MLP, one-launch post-processing)" if refine else None,
            "one_launch_path_frames": lean[0], "frame_entry_point_frames": lean[1], "frames": steps,
            "speculative_heads": dict(_ops.SPECULATION) if ahead else None,
            "early_heads": None if ahead else {k: v for k, v in _ops.SPECULATION.items() if k.startswith("early")},
            "note": "head + %sone-launch solver (device-resident pool) + track memory; synthetic detections resident on "
                    "the device as finished BoxLists (one fresh BoxList + score tensor per frame, made before the timed "
                    "frames: rounds 1-4 built them inside the loop, ~4 us per frame of harness time); one host "
                    "synchronisation per frame; autograd off as in the reference's callers" % (
                        "box-head refinement of the propagated boxes + " if refine else "")}


TIMER_NOTE = ("kernel start/stop events on the launch stream (hipExtLaunchKernel: the dispatch's own begin/end "
              "timestamps, the quantity rocprofv3 reports), every %d-th step of the timed region" % TIMER_STRIDE)


def tower_roofline(n, total_ms, launches, ho=16):
    """The towers against the matrix pipes.  ``frac`` divides the multiply-adds of the Winograd algorithm (F(2x2,3x3): 16/36
    of the direct convolution's) by the dense fp32 MFMA peak — what an fp32 implementation of the same algorithm could
    reach at best, <= 1 for the fp32 forms; the split form (``form`` 3; round 6: two-part fp16 operands, three part products)
    executes three fp16 instructions of K = 32 where the fp32 forms execute eight of K = 4, so its own pipe fraction is
    reported beside it (``f16_mfma``).  ``effective_tflops`` is the direct-convolution figure the reference computes, for
    comparison with other implementations."""
    import siammot_amd.ops as ops
    algo = 2.0 * n * 2 * CHANNELS * ho * ho * 9 * CHANNELS
    executed = algo * 16.0 / 36.0
    sec = total_ms * 1e-3 / launches
    form = ops.tower_form(n, CHANNELS, ho)
    out = {
        "bound": "mfma", "kernel": "tower_wino_kernel (%s)" % ops.TOWER_FORMS.get(form, "?"), "form": form,
        "executed_flops_per_launch": executed, "avg_launch_us": sec * 1e6,
        "achieved": executed / sec / 1e12, "peak": 157.3, "unit": "TFLOP/s", "frac": executed / sec / 1e12 / 157.3,
        "direct_conv_flops_per_launch": algo, "effective_tflops": algo / sec / 1e12,
        "launches_timed": launches,
    }
    if form == 3:
        # per workgroup (two tiles x all 64 output tiles of a track): 8 waves x (C/8 + 3) columns x 12 instructions of
        # 16 x 16 x 32 multiply-adds (the three partial K blocks of the rotation included) + 4 small residual instructions
        # (v_mfma_f32_4x4x4_16b_f16) per wave and stage, not counted
        insts = ((n + 7) // 8 * 8) * (2 * CHANNELS // 32) * 8 * (CHANNELS // 8 + 3) * 12
        flops = insts * 2.0 * 16 * 16 * 32
        out["f16_mfma"] = {"executed_flops_per_launch": flops, "achieved": flops / sec / 1e12, "peak": 2500.0, "unit": "TFLOP/s",
                           "frac": flops / sec / 1e12 / 2500.0,
                           "note": "two-part fp16 operands, 3 part products (DESIGN.md §3 K3 round 6); the loop is bound by "
                                   "the sum of its vector issue, matrix issue and operand fetches on a SIMD with two waves"}
    return out


PREDICTOR_PARAM_BYTES = 1213980          # (2*128*128*9 + 7*128*9) conv + 2*2*128 GN + 7 biases, x4 B


def path_algorithmic_bytes(boxes, image_wh, channels, rz=15, rx=30):
    """Compulsory HBM bytes of one frame pair through the whole head (SURVEY.md §8(d) formula B): per track the search
    window cells + the template read (EMM.forward) + the detection window cells + the template written
    (EMM.extract_cache), zero padding virtual and every intermediate on chip, plus the predictor parameters once."""
    import math
    W, H = image_wh
    sr_part = fused_algorithmic_bytes(boxes, image_wh, channels, rz, rx) - 4.0 * boxes.shape[0] * channels * (rx - rz + 1) ** 2
    det_cells = 0
    for x1, y1, x2, y2 in boxes.tolist():
        s = math.sqrt((x2 - x1 + 1) * (y2 - y1 + 1))
        lvl = int(min(max(math.floor(4 + math.log2(s / 224 + 1e-6)), 2), 5)) - 2
        scale = 1.0 / (4 * 2 ** lvl)
        mw, mh = W // (4 * 2 ** lvl), H // (4 * 2 ** lvl)
        cx1, cx2 = max(math.floor(x1 * scale), 0), min(math.ceil(x2 * scale), mw - 1)
        cy1, cy2 = max(math.floor(y1 * scale), 0), min(math.ceil(y2 * scale), mh - 1)
        det_cells += max(cx2 - cx1 + 1, 0) * max(cy2 - cy1 + 1, 0)
    params = PREDICTOR_PARAM_BYTES if channels == 128 else 4.0 * (2 * channels * channels * 9 + 7 * channels * 9 + 4 * channels + 7)
    return sr_part + 4.0 * channels * det_cells + 4.0 * boxes.shape[0] * channels * rz * rz + params


def box_iou(a, b):
    """Plain continuous IoU of matching rows (the north star's 1e-3 IoU bar)."""
    ix = (torch.minimum(a[:, 2], b[:, 2]) - torch.maximum(a[:, 0], b[:, 0])).clamp(min=0)
    iy = (torch.minimum(a[:, 3], b[:, 3]) - torch.maximum(a[:, 1], b[:, 1])).clamp(min=0)
    inter = ix * iy
    ua = (a[:, 2] - a[:, 0]).clamp(min=0) * (a[:, 3] - a[:, 1]).clamp(min=0)
    ub = (b[:, 2] - b[:, 0]).clamp(min=0) * (b[:, 3] - b[:, 1]).clamp(min=0)
    union = ua + ub - inter
    return torch.where(union > 0, inter / union.clamp(min=1e-12), torch.ones_like(union))


def _parity_stats(bb, conf, idx, bb_ref, conf_ref, idx_ref):
    bb, conf, bb_ref, conf_ref = (t.detach().double().cpu() for t in (bb, conf, bb_ref, conf_ref))
    same = (idx.cpu().long() == idx_ref.cpu().long())
    return {"tracks": int(bb.shape[0]), "argmax_exact_frac": float(same.double().mean()) if len(same) else 1.0,
            "min_iou": float(box_iou(bb, bb_ref).min()) if len(same) else 1.0,
            "max_box_err_px": float((bb - bb_ref).abs().max()) if len(same) else 0.0,
            "max_score_err": float((conf - conf_ref).abs().max()) if len(same) else 0.0}


def parity_report(emm, ops, feats_last, state_last, result_last, feats01, det, boxes_cpu, image_wh, n):
    """Outside the timed region: (a) the LAST result of the timed loop vs the CPU oracle on the same inputs
    (what the timed kernels produced, checked by the checker); (b) frames 0 -> 1 and 1 -> 0 through the same
    entry points vs tests/golden/bench_n<N>.npz, the reference's own output on these tensors."""
    from oracle import emm_oracle as O            # checker only — never the product path
    import numpy as np
    fe, pr = emm.feature_extractor.pooler_x, emm.predictor
    params = pr.param_dict()

    def hip_track(feats, d, sr, z):
        return ops.emm_track(feats, d[0].bbox, sr[0].bbox, z, params, emm.rx, emm.rz, tuple(fe.scales),
                             fe.sampling_ratio, emm.pad_pixels, sigma=emm.sigma, use_centerness=emm.use_centerness,
                             clip_wh=None if emm.amodal else d[0].size, gn_groups=pr.gn_groups, gn_eps=pr.gn_eps,
                             return_index=True)
    out = {}
    with torch.no_grad():
        z, sr, d = state_last
        bb, conf, idx = hip_track(feats_last, d, sr, z)
        torch.cuda.synchronize()
        # the re-run IS the timed computation: bit-identical boxes and scores
        out["rerun_bitwise_equal_to_timed_result"] = bool(
            torch.equal(bb, result_last[0].bbox) and torch.equal(conf, result_last[0].get_field("scores")))
        cfg = O.EMMConfig(channels=CHANNELS)
        p_cpu = {k: v.detach().cpu() for k, v in params.items()}
        torch.set_num_threads(_cpu_threads())
        f_cpu = [f.cpu() for f in feats_last]
        bb_o, conf_o, _, inter = O.emm_forward(cfg, p_cpu, f_cpu, boxes_cpu, sr[0].bbox.cpu(), z.cpu(), image_wh,
                                               return_intermediates=True, reference_ops=True)
        idx_o = inter["idx"]
        out["vs_oracle_fp32"] = _parity_stats(bb, conf, idx, bb_o, conf_o, idx_o)
        out["vs_oracle_fp32"]["what"] = "last frame pair of the timed loop; oracle/emm_oracle.py on the same inputs"
        gname = {(128, (704, 1280), 30): "n30", (128, (704, 1280), 100): "n100", (256, (1056, 1920), 50): "cfg4",
                 (128, (800, 800), 4): "cfg0"}.get((CHANNELS, tuple(NET_HW), n), "n%d" % n)
        gpath = os.path.join(ROOT, "tests", "golden", "bench_%s.npz" % gname)
        out["vs_reference_golden"] = None
        if os.path.exists(gpath) and feats01 is not None:
            g = np.load(gpath)
            csum = np.stack([[float(t.double().sum()) for t in f] + [float(t.double().abs().sum()) for t in f]
                             for f in feats01])
            if not np.allclose(csum, g["feat_checksum"], rtol=1e-9, atol=1e-6):
                out["vs_reference_golden"] = {"skipped": "synthetic inputs differ from the ones the golden file was "
                                                         "generated on (another torch generator?)"}
            else:
                worst = None
                for tag, (a, b) in (("ab", (0, 1)), ("ba", (1, 0))):
                    zz, ssr, dd = emm.extract_cache(feats01[a], det)
                    bb, conf, idx = hip_track(feats01[b], dd, ssr, zz)
                    torch.cuda.synchronize()
                    st = _parity_stats(bb, conf, idx, torch.from_numpy(g["bb_" + tag]),
                                       torch.from_numpy(g["scores_" + tag]), torch.from_numpy(g["idx_" + tag]))
                    st["sr_bit_exact"] = bool(np.array_equal(ssr[0].bbox.cpu().numpy(), g["sr_" + tag]))
                    if worst is None:
                        worst = st
                    else:
                        worst = {"tracks": worst["tracks"] + st["tracks"],
                                 "argmax_exact_frac": (worst["argmax_exact_frac"] * worst["tracks"]
                                                       + st["argmax_exact_frac"] * st["tracks"])
                                 / (worst["tracks"] + st["tracks"]),
                                 "min_iou": min(worst["min_iou"], st["min_iou"]),
                                 "max_box_err_px": max(worst["max_box_err_px"], st["max_box_err_px"]),
                                 "max_score_err": max(worst["max_score_err"], st["max_score_err"]),
                                 "sr_bit_exact": worst["sr_bit_exact"] and st["sr_bit_exact"]}
                worst["what"] = ("frames 0->1 and 1->0 vs tests/golden/bench_%s.npz = the reference's own EMM code "
                                 "on these tensors (oracle/gen_golden_bench.py)" % gname)
                out["vs_reference_golden"] = worst
    return out


def argmax_rows(emm, ops, dev, n, pairs, progress=False, seed0=0):
    """Arg-max agreement of the HIP head with the fp32 CPU oracle over ``pairs`` seeded frame pairs at the benchmark's
    configuration (fresh N(0,1) 720p maps per seed, the benchmark boxes jittered +-3 px, the benchmark weights): per
    track one row (seed, track, same cell?, IoU, |score diff|, max |box diff| px, fp64 score gap of the two cells on
    the oracle's logits, cause) with cause 0 = same cell, 1 = upstream fp32 rounding (the oracle's decode of the
    kernel's OWN logits elects the kernel's cell), 2 = decode rounding tie (fp64 gap <= 1e-6 on the kernel's logits),
    3 = unexplained.  Shared by tools/argmax_stats.py (artifact) and this file's parity block (measured in-run)."""
    from oracle import emm_oracle as O            # checker only — never the product path
    from siammot_amd.structures import BoxList
    image_wh = (NET_HW[1], NET_HW[0])
    base_boxes = synthetic_boxes(n, image_wh)
    params_cpu = {k: v.detach().cpu() for k, v in emm.predictor.named_parameters()}
    ocfg = O.EMMConfig(channels=CHANNELS)
    fe, pr = emm.feature_extractor.pooler_x, emm.predictor
    rows = []
    t0 = time.time()
    with torch.no_grad():
        for seed in range(seed0, seed0 + pairs):
            g = torch.Generator().manual_seed(10_000 + seed)
            jitter = (torch.rand((n, 1), generator=g) * 6.0 - 3.0)
            boxes = (base_boxes + jitter).clamp(min=0)
            boxes[:, 2].clamp_(max=image_wh[0] - 1)
            boxes[:, 3].clamp_(max=image_wh[1] - 1)
            gd = torch.Generator(device=dev).manual_seed(20_000 + seed)
            fa = tuple(torch.randn((1, CHANNELS, NET_HW[0] // s, NET_HW[1] // s), generator=gd, device=dev) for s in (4, 8, 16, 32, 64))
            fb = tuple(torch.randn((1, CHANNELS, NET_HW[0] // s, NET_HW[1] // s), generator=gd, device=dev) for s in (4, 8, 16, 32, 64))
            det = BoxList(boxes.to(dev), image_wh, mode="xyxy")
            det.add_field("ids", torch.arange(n, device=dev))
            det.add_field("labels", torch.ones(n, dtype=torch.int64, device=dev))
            z, sr, d = emm.extract_cache(fa, det)
            bb, conf, idx = ops.emm_track(fb, d[0].bbox, sr[0].bbox, z, pr.param_dict(), emm.rx, emm.rz, tuple(fe.scales),
                                          fe.sampling_ratio, emm.pad_pixels, sigma=emm.sigma,
                                          use_centerness=emm.use_centerness, clip_wh=image_wh, gn_groups=pr.gn_groups,
                                          gn_eps=pr.gn_eps, return_index=True)
            fa_c, fb_c = [t.cpu() for t in fa], [t.cpu() for t in fb]
            z_o, sr_o = O.extract_cache(ocfg, fa_c, boxes)
            bb_o, conf_o, _, inter = O.emm_forward(ocfg, params_cpu, fb_c, boxes, sr_o, z_o, image_wh,
                                                   return_intermediates=True, reference_ops=True)
            idx, idx_o = idx.cpu(), inter["idx"]
            iou = box_iou(bb.cpu().double(), bb_o.double())
            diff = (idx != idx_o).nonzero().flatten().tolist()
            gaps, kind = {}, {}
            if diff:
                # Attribution.  (1) the kernel's OWN logits (same operators, called one by one) decoded by the fp32
                # oracle: if that elects the kernel's cell, the decode is exact and the difference was made upstream
                # (pooling / correlation / Winograd-vs-direct summation order moved the logits by ~1e-5 of their
                # scale and two cells swapped places).  (2) otherwise the two cells' fp64 scores on the kernel's
                # logits: a gap <= 1e-6 is an exponential-rounding tie between torch-CPU and the device.
                resp = ops.sr_xcorr_fused(fb, d[0].bbox, sr[0].bbox, z, emm.rx, emm.rz, tuple(fe.scales), fe.sampling_ratio,
                                          emm.pad_pixels)
                lg = ops.emm_predictor(resp, pr.param_dict(), pr.gn_groups, pr.gn_eps).cpu()[diff]
                xs, ys = O.grid_axes(sr_o[diff], ocfg.rx, ocfg.rz, ocfg.pad_pixels)
                up32 = [O.bicubic_upsample_torch(lg[:, a:b]) for a, b in ((0, 2), (2, 3), (3, 7))]
                _, _, idx_mix = O.decode(up32[0], up32[1], up32[2], xs, ys, boxes[diff], True, 0.4)
                up64 = [O.bicubic_upsample(lg[:, a:b].double()) for a, b in ((0, 2), (2, 3), (3, 7))]
                score64, _ = O.score_map(up64[0], up64[1], up64[2], boxes[diff].double(), True, 0.4)
                up_o = [O.bicubic_upsample(inter[k][diff].double()) for k in ("cls", "center", "reg")]
                score_o, _ = O.score_map(up_o[0], up_o[1], up_o[2], boxes[diff].double(), True, 0.4)
                for j, t in enumerate(diff):
                    gaps[t] = float(score_o[j, idx_o[t]] - score_o[j, idx[t]])       # on the ORACLE's logits
                    if int(idx_mix[j]) == int(idx[t]):
                        kind[t] = 1                                                  # upstream fp32 rounding
                    elif abs(float(score64[j, idx_mix[j]] - score64[j, idx[t]])) <= 1e-6:
                        kind[t] = 2                                                  # decode-level rounding tie
                    else:
                        kind[t] = 3                                                  # unexplained
            for t in range(n):
                rows.append((seed, t, int(idx[t] == idx_o[t]), float(iou[t]), float((conf[t].cpu() - conf_o[t]).abs()),
                             float((bb[t].cpu() - bb_o[t]).abs().max()), gaps.get(t, 0.0), kind.get(t, 0)))
            if progress and (seed + 1) % 50 == 0:
                print("%d pairs, %.0f s" % (seed + 1, time.time() - t0), flush=True)
    return rows


def argmax_statistics(emm, ops, dev, n, pairs):
    """The arg-max statistic of the parity block, MEASURED IN THIS RUN on ``pairs`` seeded
    frame pairs of the benchmark configuration (outside the timed region; CPU oracle as the checker)."""
    t0 = time.time()
    torch.set_num_threads(_cpu_threads())
    rows = argmax_rows(emm, ops, dev, n, pairs)
    same = [r for r in rows if r[2]]
    dis = [r for r in rows if not r[2]]
    return {
        "measured_in_this_run": True, "frame_pairs": pairs, "tracks_total": len(rows), "argmax_exact": len(same),
        "argmax_exact_frac": len(same) / max(len(rows), 1),
        "min_iou": min(r[3] for r in rows), "tracks_below_1e-3_iou_bar": sum(1 for r in rows if 1.0 - r[3] > 1e-3),
        "min_iou_among_argmax_exact": min([r[3] for r in same] or [1.0]),
        "max_score_err": max(r[4] for r in rows), "max_box_err_px_among_argmax_exact": max([r[5] for r in same] or [0.0]),
        "disagreements": [{"seed": r[0], "track": r[1], "iou": r[3], "fp64_score_gap_on_oracle_logits": r[6],
                           "cause": {1: "upstream fp32 rounding", 2: "decode rounding tie (fp64 gap <= 1e-6)",
                                     3: "UNEXPLAINED"}[r[7]]} for r in dis],
        "what": "HIP head vs oracle/emm_oracle.py (fp32, the reference's torch-CPU ops) on fresh N(0,1) maps per seed, the "
                "benchmark boxes jittered +-3 px; a disagreement is attributed through fp64 scores (tools/argmax_stats.py "
                "writes the long-run artifact: profiles/r05_argmax_stats*.md)",
        "seconds": time.time() - t0}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, result, state):
    """``--dump-outputs``: what one timed step hands its caller — ``EMM.forward``'s tracks and ``EMM.extract_cache``'s new
    track memory — as <out_dir>/<name>.npy, float32 (float64 for the integer ids).  Above DUMP_LIMIT_BYTES in all, the
    template features keep a fixed, seeded sample of their rows (tracks) and ``template_feature_rows.npy`` says which."""
    import numpy as np
    z, sr, _ = state
    arrays = {"track_boxes": result[0].bbox, "track_scores": result[0].get_field("scores"),
              "track_ids": result[0].get_field("ids"), "search_regions": sr[0].bbox, "template_features": z}
    arrays = {k: v.detach().cpu().numpy() for k, v in arrays.items()}
    arrays = {k: v.astype(np.float32 if v.dtype.kind == "f" and v.itemsize <= 4 else np.float64) for k, v in arrays.items()}
    z = arrays["template_features"]
    room = DUMP_LIMIT_BYTES - sum(v.nbytes for k, v in arrays.items() if k != "template_features")
    if z.nbytes > room:
        rows_fit = max(1, (room - 8 * z.shape[0]) // (z.nbytes // z.shape[0]))
        keep = np.sort(np.random.RandomState(0).choice(z.shape[0], rows_fit, replace=False))
        arrays["template_features"], arrays["template_feature_rows"] = z[keep], keep.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def self_launch(args):
    """``python bench.py --gpus N`` without a torchrun environment: start the N ranks ourselves (one process per
    GPU, rendezvous on 127.0.0.1) and let rank 0 print the JSON line."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")         # dmabuf IPC: required by RCCL on this host driver
    env.setdefault("OMP_NUM_THREADS", "1")       # a rank is one Python launch loop; OpenMP pools would only spin
    return subprocess.call(cmd, env=env, cwd=ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--prewarm-ms", type=float, default=400.0,
                    help="setup phase: run untimed frame pairs for this long so host and device clocks leave their "
                         "idle states before the W warm-up steps (a 200-step run measured 0.29 ms/step, a 2000-step "
                         "run 0.16 ms/step on the same box); 0 disables")
    ap.add_argument("--tracks", type=int, default=30)
    ap.add_argument("--channels", type=int, default=CHANNELS,
                    help="FPN channel count (128 = DLA-34-FPN, the metric's configuration; 256 = R-50-FPN, configs[4])")
    ap.add_argument("--net-hw", type=int, nargs=2, default=list(NET_HW), metavar=("H", "W"),
                    help="network input size (704 1280 = 720p under the default resize rule; 1056 1920 = configs[4])")
    ap.add_argument("--feature-sets", type=int, default=FEATURE_SETS,
                    help="distinct synthetic frames the timed loop rotates through (8 x 38 MB exceeds the 256 MiB "
                         "Infinity Cache; 2 = the cache-warm loop of round 1)")
    ap.add_argument("--graph", action="store_true",
                    help="also replay the frame-pair loop as a hipGraph (siammot_amd.graphs.FramePairRing).  Off by default since "
                         "round 6: the replay buys HOST time (3 us per frame pair instead of ~42), not GPU time — 58.3 vs 57.3 us "
                         "per step — so it is a deployment option for host-bound callers, not a faster benchmark leg")
    ap.add_argument("--no-graph", action="store_true", help=argparse.SUPPRESS)          # (accepted: the leg is off by default)
    ap.add_argument("--no-tracking-loop", action="store_true",
                    help="skip the tracking-loop legs (head + solver + track memory per frame; ~20 s)")
    ap.add_argument("--extra-streams", type=int, default=0,
                    help="after the timed region, also measure S independent video streams on S HIP streams of the same "
                         "GPU (reported as `multi_stream`, not as `value`); 0 disables")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the post-run comparison with the oracle / golden file")
    ap.add_argument("--argmax-pairs", type=int, default=100,
                    help="seeded frame pairs of the in-run arg-max statistic (parity.argmax_statistics; ~0.25 s each on the "
                         "CPU oracle); 0 skips it")
    ap.add_argument("--no-kernel-timer", action="store_true",
                    help="skip the HIP-event bracketing of the xcorr launches (roofline fields become null)")
    ap.add_argument("--allow-shared-gpu", action="store_true",
                    help="let ranks share a device when fewer GPUs than ranks are visible (flow test only: the "
                         "collective backend becomes gloo and the JSON says so)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the BASELINE.json configs[2] / configs[4] runs that follow the headline (`other_configs`)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run every other leg: kernel rooflines, parity with the oracle and the "
                         "reference golden, arg-max statistics, cache-warm / graph / multi-stream / tracking loops, host "
                         "enqueue cost, the other BASELINE.json configs and the CPU baseline (several minutes)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned (EMM.forward's tracks, EMM.extract_cache's new track "
                         "memory) as DIR/<name>.npy, float32 / float64")
    ap.add_argument("--other-config-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-baseline-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-budget", type=float, default=10.0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    globals()["CHANNELS"] = args.channels            # the helpers above read the module constants
    globals()["NET_HW"] = tuple(args.net_hw)
    if args.cpu_baseline_worker:
        cpu_baseline_worker(args.tracks, args.cpu_budget)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    from siammot_amd import ops, parallel
    from siammot_amd.config import get_default_cfg
    from siammot_amd.emm import EMM
    from siammot_amd.structures import BoxList
    from siammot_amd.track_utils import build_track_utils

    assert torch.cuda.is_available(), "bench.py needs a ROCm device (the product path has no CPU fallback)"
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world_env))
    n_dev = torch.cuda.device_count()
    shared = world_env > n_dev
    if shared and not (args.allow_shared_gpu or os.environ.get("SMOT_DIST_BACKEND") == "gloo"):
        raise SystemExit("bench.py: %d ranks but only %d GPU(s) visible (--allow-shared-gpu runs the flow with "
                         "ranks sharing devices over gloo; it is not a scaling measurement)" % (world_env, n_dev))
    dev_index = int(os.environ.get("LOCAL_RANK", "0")) % n_dev     # ranks > GPUs only in the shared-device flow test
    torch.cuda.set_device(dev_index)                          # before the process group: RCCL binds to this device
    dev = torch.device("cuda", dev_index)
    rank, world, local_rank = parallel.init_distributed(backend="gloo" if shared else None, device=dev)
    pinned = None
    if world > 1:
        # one launch loop per rank on its own cores (NUMA-local slices), no OpenMP pools spinning beside it
        torch.set_num_threads(1)
        pinned = parallel.pin_rank_to_cores(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    ops.load_library()
    timer = args.full and not args.no_kernel_timer

    n = args.tracks
    image_wh = (NET_HW[1], NET_HW[0])
    boxes_cpu = synthetic_boxes(n, image_wh)
    cfg = get_default_cfg(channels=CHANNELS)
    emm = EMM(cfg, build_track_utils(cfg)).eval()
    if rank == 0:
        init_predictor(emm.predictor, boxes_cpu)
    emm = emm.to(dev)
    bcast_bytes = parallel.broadcast_module(emm, src=0)       # one RCCL broadcast over xGMI; 0 at N=1
    K = max(2, args.feature_sets)
    feats = [synthetic_features(100 + rank * K + k, dev) for k in range(K)]     # the frames the loop rotates through
    det = BoxList(boxes_cpu.to(dev), image_wh, mode="xyxy")
    det.add_field("ids", torch.arange(n, device=dev))
    det.add_field("labels", torch.ones(n, dtype=torch.int64, device=dev))

    def step(k, state):
        z, sr, d = state
        f = feats[k % K]
        _, result, _ = emm(f, d, sr, template_features=z)                  # frame t: track
        return emm.extract_cache(f, det), result                           # frame t: new templates / SRs

    def timed_run(steps, k0=0):
        nonlocal state
        prev = state
        parallel.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(k0, k0 + steps):
            prev = state
            state, result = step(k, state)
        torch.cuda.synchronize()
        parallel.barrier()
        return time.perf_counter() - t0, prev, result

    with torch.no_grad():
        state = emm.extract_cache(feats[K - 1], det)
        t_pre = time.perf_counter()
        while (time.perf_counter() - t_pre) * 1e3 < args.prewarm_ms:     # setup, not part of W or K
            for k in range(32):
                state, _ = step(k, state)
            torch.cuda.synchronize()
        for k in range(args.warmup):
            state, _ = step(k, state)
        if timer:
            # events are created here, outside the timed region.  An event pair costs ~3 us of stream time, so the
            # two instrumented kernels are bracketed on every TIMER_STRIDE-th step only (bracketing all of them
            # slows the frame pair from 80 to 94 us); the samples still come from inside the timed region.
            cap = args.steps + MIN_TIMER_SAMPLES * 4 + 8
            ops.kernel_timer_begin(ops.TIMER_XCORR, cap, TIMER_STRIDE)
            ops.kernel_timer_begin(ops.TIMER_TOWER, cap, TIMER_STRIDE)
        elapsed, state_before_last, result = timed_run(args.steps)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, result, state)      # before any later step can reuse a buffer
        last_k = args.steps - 1
        post_steps = 0
        if timer:
            # top the bracket samples up to MIN_TIMER_SAMPLES with a post-loop of the same frame pairs (NOT part of
            # `value`): the driver's default --steps 20 leaves two samples otherwise
            have = (args.steps + TIMER_STRIDE - 1) // TIMER_STRIDE
            if have < MIN_TIMER_SAMPLES:
                post_steps = (MIN_TIMER_SAMPLES - have) * TIMER_STRIDE
                st_keep = state
                timed_run(post_steps, k0=args.steps)
                state = st_keep
        xcorr_total_ms, xcorr_launches = ops.kernel_timer_end(ops.TIMER_XCORR) if timer else (0.0, 0)
        tower_total_ms, tower_launches = ops.kernel_timer_end(ops.TIMER_TOWER) if timer else (0.0, 0)
        # cache-warm variant of the same loop (two alternating frames, as round 1 measured it): informational
        warm = None
        if args.full and world == 1 and K > 2 and args.steps >= 100:
            K_keep, K = K, 2
            timed_run(min(200, args.steps))
            w_elapsed, _, _ = timed_run(args.steps)
            K = K_keep
            warm = {"feature_sets": 2, "value": args.steps / w_elapsed, "unit": "frame-pairs/s",
                    "ms_per_step": w_elapsed / args.steps * 1e3,
                    "note": "two alternating frames (77 MB) stay resident in the 256 MiB Infinity Cache"}
    multi = loop_stats = graph_stats = None
    if args.full and world == 1 and args.graph and not args.no_graph:
        try:
            with torch.no_grad():
                graph_stats = hipgraph_loop_throughput(emm, feats, det, state, args.steps)
        except Exception as e:                      # a capture failure must not cost the run its headline
            graph_stats = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
    if args.full and world == 1 and args.extra_streams > 1:
        multi = multi_stream_throughput(emm, feats, det, args.extra_streams, dev)
    if args.full and world == 1 and not args.no_tracking_loop:
        loop_stats = tracking_loop_throughput(n, dev, feats)
        loop_stats["with_refinement"] = tracking_loop_throughput(n, dev, feats, refine=True)
        # the same loops with every call shown the next frame's features (a streaming caller): the next head is launched a
        # call early on the guess that the track count holds, the host's record -> launch path runs beside it
        loop_stats["next_frame_shown"] = {k: v for k, v in tracking_loop_throughput(n, dev, feats, ahead=True).items()
                                          if k in ("value", "unit", "ms_per_frame", "tracked_in_last_frame", "track_count_held",
                                                   "frame_entry_point_frames", "frames", "speculative_heads")}
        loop_stats["next_frame_shown"]["with_refinement"] = {
            k: v for k, v in tracking_loop_throughput(n, dev, feats, refine=True, ahead=True).items()
            if k in ("value", "unit", "ms_per_frame", "tracked_in_last_frame", "track_count_held", "speculative_heads")}
        # the same head workload (n rows per frame) with dormant tracks in the memory, as MOT sequences have them all the
        # time (DLA_34_FPN_EMM_MOT17.yaml keeps a lost track for 30 frames): a fifth of the tracks dormant; their rows
        # copied on the device / concatenated on the host as the reference does / copied with the next frame shown
        keep = ("value", "unit", "ms_per_frame", "tracked_in_last_frame", "track_count_held", "active_tracks", "dormant_tracks",
                "memory_rows", "dormant_rows", "frame_entry_point_frames", "frames", "speculative_heads")
        nd = max(1, n // 5)
        import siammot_amd.ops as _ops
        fb_before = dict(_ops.FALLBACKS)          # (a carried memory has no order hint: its heads count as `unhinted_head`
        wd = {k: v for k, v in tracking_loop_throughput(n, dev, feats, dormant=nd).items() if k in keep}
        wd["host_form"] = {k: v for k, v in tracking_loop_throughput(n, dev, feats, dormant=nd, device_carry=False).items()
                           if k in keep}
        wd["next_frame_shown"] = {k: v for k, v in tracking_loop_throughput(n, dev, feats, dormant=nd, ahead=True).items()
                                  if k in keep}
        wd["fallbacks"] = {k: v - fb_before.get(k, 0) for k, v in _ops.FALLBACKS.items() if v != fb_before.get(k, 0)}
        _ops.FALLBACKS.clear()                    #  — reported here, not among the headline's fallbacks)
        _ops.FALLBACKS.update(fb_before)
        loop_stats["with_dormant_tracks"] = wd
    # host cost of a step: the time to ENQUEUE frame pairs (no synchronisation), measured outside the timed region on
    # a burst short enough for the stream's queue; next to the GPU time per step it says how much host headroom a
    # rank has (eight ranks share one host)
    if args.full:
        with torch.no_grad():
            torch.cuda.synchronize()
            t_h = time.perf_counter()
            for k in range(64):
                state, _ = step(k, state)
            host_enqueue_us = (time.perf_counter() - t_h) / 64 * 1e6
            torch.cuda.synchronize()
        rank_ms = parallel.gather_floats(elapsed / args.steps * 1e3, dev)
        rank_host_us = parallel.gather_floats(host_enqueue_us, dev)
    elapsed = parallel.max_over_ranks(elapsed, dev)
    backend = torch.distributed.get_backend() if parallel.is_distributed() else "none"
    dist_world = torch.distributed.get_world_size() if parallel.is_distributed() else 1
    # The timed launches carry a start/stop event pair of their own (hipExtLaunchKernel): the elapsed time between
    # the two is the kernel's duration as rocprofv3 sees it.  (Round 1 bracketed the launch with two hipEventRecord
    # markers instead: that span ran 2.5-3.5 us above the kernel's duration.)
    xcorr_avg_s = xcorr_total_ms * 1e-3 / max(xcorr_launches, 1)

    if rank != 0:
        parallel.shutdown()           # every collective of this rank is behind it
        return
    fb_snapshot = dict(ops.FALLBACKS)        # (before the parity legs: those call the operators stand-alone, un-hinted)
    parity = None
    if args.full and not args.no_parity:
        golden_ok = (CHANNELS, tuple(NET_HW), n) in ((128, (704, 1280), 30), (128, (704, 1280), 100),
                                                     (256, (1056, 1920), 50), (128, (800, 800), 4))
        parity = parity_report(emm, ops, feats[last_k % K], state_before_last, result,
                               feats[:2] if golden_ok else None, det, boxes_cpu, image_wh, n)
        # what the handful of tracks above cannot show: the arg-max statistic over many seeded frame pairs, measured HERE
        # (outside the timed region; --argmax-pairs 0 skips it)
        if args.argmax_pairs > 0 and world == 1 and (CHANNELS, tuple(NET_HW)) == (128, (704, 1280)):
            try:
                parity["argmax_statistics"] = argmax_statistics(emm, ops, dev, n, args.argmax_pairs)
            except Exception as e:
                parity["argmax_statistics"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        else:
            parity["argmax_statistics"] = None
    rx, rz = emm.rx, emm.rz
    ho = rx - rz + 1
    # the kernel that runs in the pipeline: search-region pooling fused with the cross-correlation
    fused_bytes = fused_algorithmic_bytes(boxes_cpu, image_wh, CHANNELS, rz, rx)
    achieved = fused_bytes / xcorr_avg_s / 1e9 if xcorr_avg_s > 0 else 0.0
    # the stand-alone xcorr operator (SURVEY.md §8d figure A) on the same search regions, timed the same way
    xcorr_bytes = 4.0 * n * CHANNELS * (rx * rx + rz * rz + ho * ho)
    xop = None
    if timer:
        with torch.no_grad():
            z, sr, d = state
            x = ops.roi_align_levels(feats[0], sr[0].bbox, d[0].bbox, rx, emm.feature_extractor.pooler_x.scales, 2,
                                     [int(emm.pad_pixels / ((2 ** i) * 4)) for i in range(4)])
            for _ in range(20):
                ops.xcorr_depthwise(x, z)
            reps = 200
            ops.xcorr_timer_begin(reps)
            for _ in range(reps):
                ops.xcorr_depthwise(x, z)
            torch.cuda.synchronize()
            ms, cnt = ops.xcorr_timer_end()
        t = ms * 1e-3 / max(cnt, 1)
        xop = {"kernel": "xcorr_dw_patch2_kernel<30,15,0>", "algorithmic_bytes_per_launch": xcorr_bytes,
               "avg_launch_us": t * 1e6, "achieved": xcorr_bytes / t / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": xcorr_bytes / t / 1e9 / HBM_PEAK_GBS, "launches_timed": cnt,
               "note": "stand-alone operator, input resident in L2/MALL (not part of the frame-pair pipeline, which "
                       "runs the fused kernel)"}
    # an empty kernel of the graded kernel's launch shape under the same timer (see `empty_launch_event_bracket_us` below)
    floor_us = None
    if timer:
        try:
            floor_us = ops.dispatch_floor_us(n * ((CHANNELS + 7) // 8), 512)
        except Exception:
            floor_us = None
    traffic = traffic_source = valu_insts = None
    tpath = os.path.join(ROOT, "profiles", "xcorr_traffic.json")
    if args.full and os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            # the counters were taken on ONE kernel at ONE source state: refuse them for any other
            stamp_ok = (tj.get("kernel") == ops.fused_kernel_name() and tj.get("source_sha1") == fused_source_sha1()
                        and (CHANNELS, tuple(NET_HW)) == (128, (704, 1280)))
            traffic = tj.get(str(n)) if stamp_ok else None
            valu_insts = (tj.get("valu_insts") or {}).get(str(n)) if stamp_ok else None
            traffic_source = ("static:profiles/xcorr_traffic.json (%s)" % tj.get(
                "source", "separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, not measured by this run")) if stamp_ok else (
                "null: profiles/xcorr_traffic.json was taken on %s at source %s; this run launches %s at source %s" % (
                    tj.get("kernel"), str(tj.get("source_sha1"))[:12], ops.fused_kernel_name(), fused_source_sha1()[:12]))
        except Exception:
            traffic = None
    out = {
        "metric": METRIC,
        "value": world * args.steps / elapsed,
        "unit": "frame-pairs/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        # arithmetic type of the path: fp32 in and out of every kernel; the towers' transform-domain GEMMs run on the fp16 matrix
        # pipe with every fp32 operand as two fp16 parts of a power-of-two-scaled value (3 of 4 part products, fp32 accumulate):
        # logits within the fp32 form's error of an fp64 evaluation (tests/test_hip_parity.py, 1.25 x bound)
        "dtype": "f32 (towers and correlation: fp16x2 operands on MFMA, fp32 accumulate, fp32-equivalent error)",
        "data": "synthetic",
        "config": {
            "workload": "EMM tracker-head frame pair (EMM.forward + EMM.extract_cache) on %s FPN maps "
                        "(net input %dx%d, C=%d, 5 levels), %d tracks, one stream per GPU; hot path only: "
                        "backbone / RPN / box head / solver are outside the timed region"
                        % ("DLA-34-FPN 720p" if (CHANNELS, NET_HW) == (128, (704, 1280)) else "synthetic",
                           NET_HW[0], NET_HW[1], CHANNELS, n),
            "tracks": n, "channels": CHANNELS, "rz": rz, "rx": rx, "prewarm_ms": args.prewarm_ms,
            "feature_sets": K, "feature_bytes_rotated": int(sum(f.numel() for f in feats[0]) * 4 * K),
            "parallelism": "streams x%d (one process per GPU, no per-frame collective); weights broadcast once: %d B; "
                           "backend=%s, world_size=%d as reported by torch.distributed%s"
                           % (world, bcast_bytes, {"nccl": "nccl (RCCL)"}.get(backend, backend), dist_world,
                              "; RANKS SHARE DEVICES (flow test, not a scaling measurement)" if shared else ""),
        },
        # capacity cliffs that fell back to a slower path during THIS run (siammot_amd.ops.FALLBACKS; all zero = none)
        "fallbacks": {k: int(fb_snapshot.get(k, 0)) for k in ("refine_library_gemm", "host_solver", "unhinted_head",
                                                                "general_frame")},
    }
    if args.full:
        out.update({
            "per_rank": {"ms_per_step_min": min(rank_ms), "ms_per_step_max": max(rank_ms),
                         "host_enqueue_us_per_step_min": min(rank_host_us), "host_enqueue_us_per_step_max": max(rank_host_us),
                         "cores_pinned_rank0": pinned, "omp_threads": torch.get_num_threads(),
                         "note": "host_enqueue = Python + ctypes time to enqueue one frame pair (4 launches), no "
                                 "synchronisation; headroom = ms_per_step - host_enqueue"},
            "roofline": {
                "bound": "hbm", "kernel": ops.fused_kernel_name() + " (search-region ROIAlign + depthwise xcorr)",
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic, "traffic_source": traffic_source,
                # the same fraction by the bytes the counters saw instead of the algorithmic ones: at 100
                # tracks overlapping search windows are served by L2 / MALL, so fewer bytes reach the fabric than the formula counts
                "frac_by_counter_bytes": None if not traffic or xcorr_avg_s <= 0 else traffic / xcorr_avg_s / 1e9 / HBM_PEAK_GBS,
                # the resource that actually binds this kernel: vector-instruction issue.  A wave64
                # instruction occupies its SIMD's issue port for 4 cycles; SQ_INSTS_VALU (same counter passes and source stamp
                # as `traffic`) x 4 cycles / (256 CUs x 4 SIMDs) / clock = the time the launch needs for vector issue alone,
                # were it spread perfectly over the chip — `frac_of_duration` of the measured duration
                "valu_issue": None if not valu_insts or xcorr_avg_s <= 0 else {
                    "wave_instructions_per_launch": valu_insts, "cycles_per_instruction": 4, "simds": 1024, "clock_ghz": CLOCK_GHZ,
                    "issue_bound_us": valu_insts * 4.0 / 1024.0 / (CLOCK_GHZ * 1e3),
                    "frac_of_duration": valu_insts * 4.0 / 1024.0 / (CLOCK_GHZ * 1e3) / (xcorr_avg_s * 1e6),
                    "note": "static counter (profiles/xcorr_traffic.json, SQ_INSTS_VALU of a separate --pmc pass at this source "
                            "state), not measured by this run.  Since round 6 the correlation runs on the matrix pipe (45 fp16 matrix "
                            "instructions per plane on two-part operands instead of 900 v_fmac_f32 per lane): vector issue is no longer "
                            "what binds the kernel — its time is the start-up / pooling chain (dependent memory round trips) plus an "
                            "LDS-bound correlation phase (DESIGN.md §3)"},
                "algorithmic_bytes_per_launch": fused_bytes,
                "avg_launch_us": xcorr_avg_s * 1e6, "launches_timed": xcorr_launches, "timer": TIMER_NOTE,
                # an EMPTY kernel of the same launch shape bracketed by the same pair of events: an UPPER bound on the fixed cost
                # inside `avg_launch_us` — rocprofv3's dispatch timestamps give 0.8-1.5 us for the same empty kernel
                # (profiles/r04_loop_kernel_stats.md, smot::empty_kernel) and the same 17.5 us as the events for the graded
                # kernel, so most of an empty bracket is the bracket.  No "fraction net of the floor" is derived from it.
                "empty_launch_event_bracket_us": floor_us,
                "timer_stride": TIMER_STRIDE, "post_loop_steps_for_timer_samples": post_steps,
                "xcorr_op": xop,
            },
            # the kernel with the largest share of GPU time: the two conv3x3 towers, Winograd F(2x2,3x3) on the matrix cores
            # (tower_roofline: which form ran, its multiply-adds against the fp32 pipe, effective_tflops = the direct
            # convolution's FLOPs / time, the figure to compare implementations by).  At the 29 x 29 response of the second yaml
            # family the timer brackets the blocked convolution kernel only (GroupNorm + heads run in a second kernel).
            "roofline_tower": None if tower_launches == 0 else tower_roofline(n, tower_total_ms, tower_launches, rx - rz + 1),
            # the whole frame pair against HBM: compulsory bytes / ms_per_step.  The path is issue-,
            # matrix-pipe- and latency-bound, so this fraction is small by construction.
            "roofline_path": (lambda pb: {"bound": "hbm", "algorithmic_bytes_per_step": pb,
                                          "achieved": pb / (elapsed / args.steps) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                          "frac": pb / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS})(
                path_algorithmic_bytes(boxes_cpu, image_wh, CHANNELS, rz, rx)),
            "parity": parity,
            "cache_warm_loop": warm,
            "hipgraph_loop": graph_stats,
            "multi_stream": multi,
            "tracking_loop": loop_stats,
        })
    if args.full:
        if world == 1 and not args.no_other_configs and not args.other_config_worker:
            out["other_configs"] = other_config_runs(args)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(n)
        # the last thing on the line (a log tail keeps it): the numbers a reviewer looks for first, compact
        rt, am = out.get("roofline_tower") or {}, ((out.get("parity") or {}).get("argmax_statistics") or {})
        out["summary"] = {
            "frame_pairs_per_s": out["value"], "ms_per_step": out["ms_per_step"],
            "graded_kernel_us": out["roofline"]["avg_launch_us"], "graded_kernel_frac_of_hbm_peak": out["roofline"]["frac"],
            "tower_us": rt.get("avg_launch_us"), "tower_form": rt.get("form"),
            "tower_f16_mfma_frac": (rt.get("f16_mfma") or {}).get("frac"),
            "host_enqueue_us_per_step": max(rank_host_us),
            "tracking_loop_ms_per_frame": None if not loop_stats else {
                "plain": loop_stats.get("ms_per_frame"), "with_refinement": (loop_stats.get("with_refinement") or {}).get("ms_per_frame"),
                "next_frame_shown": (loop_stats.get("next_frame_shown") or {}).get("ms_per_frame")},
            "argmax_statistics": {k: am.get(k) for k in ("frame_pairs", "tracks_total", "argmax_exact", "min_iou",
                                                         "tracks_below_1e-3_iou_bar")} if am else None,
            "other_configs_ms_per_step": {k: v.get("ms_per_step") for k, v in (out.get("other_configs") or {}).items()},
            "cpu_baseline_frame_pairs_per_s": (out.get("cpu_baseline") or {}).get("value"),
            "methodology_version": "r06 (tracking_loop legs: median of three chunks, detections as ready-made BoxLists — as r05; "
                                   "r01-r04 built a BoxList per frame inside the timed loop: ~4 us per frame more)",
        }
    print(json.dumps(out))
    sys.stdout.flush()
    parallel.shutdown()


if __name__ == "__main__":
    main()
