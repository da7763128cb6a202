"""The frames of B cameras through ONE ``FramePreprocessor.batch`` call, against what a caller does with the single-frame path:
B x ``pre(frame)``, a ``torch.stack``, then ``.to(dtype)`` and ``.contiguous(memory_format=torch.channels_last)`` where the
row asks for them.

    python tools/preprocess_batch_bench.py [--steps K] [--warmup W] [--rounds R] [--out profiles/preprocess_batch_bench.json]

Rows: B = 1, 2, 4, 8 cameras x input sets (all 720p / all 1080p / half 720p and half 1080p — every one goes to 704 x 1280;
the mixed set needs B >= 2) x outputs (fp32 NCHW, fp16 NCHW, fp16 channels-last) x where the frames start ("device": uint8
tensors already on the GPU, i.e. launches + the extra passes only; "host": numpy frames, i.e. staging and host-to-device
copies included).  Both forms run in one process, alternating, for R rounds after a warm-up; a round is a window of K calls
that ends in a synchronise, timed with the host clock; ``host_enqueue_us`` is the host time of the window's enqueue before
that synchronise.  Reported per form: the median over the rounds and the spread (max - min).  ``no_slower`` states the
condition the documents quote: batched median <= baseline median + the larger of the two spreads.
Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script (``--quick``;
profiles/preprocess_batch_kernel_stats.md); ``bytes_in`` / ``bytes_out`` are what the shapes imply for the batched kernel.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SETS = {"720p": ((720, 1280),), "1080p": ((1080, 1920),), "mixed": ((720, 1280), (1080, 1920))}
OUTPUTS = (("fp32_nchw", torch.float32, False), ("fp16_nchw", torch.float16, False), ("fp16_nhwc", torch.float16, True))
NET_HW = (704, 1280)


def input_shapes(B, name):
    kinds = SETS[name]
    return [kinds[(b * len(kinds)) // B] for b in range(B)]          # mixed: the first half 720p, the second half 1080p


def implied_bytes(shapes, dtype):
    """(uint8 bytes read, output bytes written) of one batched call, from the shapes alone."""
    esize = torch.empty((), dtype=dtype).element_size()
    return sum(h * w * 3 for h, w in shapes), len(shapes) * 3 * NET_HW[0] * NET_HW[1] * esize


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) / steps * 1e6, (t1 - t0) / steps * 1e6


def run_row(pre, B, set_name, out_name, dtype, cl, where, steps, warmup, rounds, dev):
    shapes = input_shapes(B, set_name)
    rs = np.random.RandomState(17)
    host = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    frames = host if where == "host" else [torch.from_numpy(a).to(dev) for a in host]
    assert all(pre.get_size((w, h)) == NET_HW for h, w in shapes)

    def batched():
        return pre.batch(frames, dtype=dtype, channels_last=cl)

    def baseline():
        x = torch.stack([pre(f) for f in frames])
        if dtype != torch.float32:
            x = x.to(dtype)
        if cl:
            x = x.contiguous(memory_format=torch.channels_last)
        return x

    same = bool(torch.equal(batched(), baseline()))                  # the two forms compute the same thing, bit for bit
    for fn in (batched, baseline):
        for _ in range(warmup):
            fn()
    acc = {"batched": ([], []), "baseline": ([], [])}
    for _ in range(rounds):                                          # alternating, so that drift favours neither form
        for name, fn in (("batched", batched), ("baseline", baseline)):
            us, enq = window(fn, steps)
            acc[name][0].append(us)
            acc[name][1].append(enq)
    bytes_in, bytes_out = implied_bytes(shapes, dtype)
    row = {"images": B, "inputs": set_name, "output": out_name, "frames_on": where, "steps": steps, "rounds": rounds,
           "bytes_in": bytes_in, "bytes_out": bytes_out, "bitwise_equal_to_baseline": same}
    for name, (us, enq) in acc.items():
        row[name] = {"median_us": statistics.median(us), "spread_us": max(us) - min(us), "rounds_us": us,
                     "host_enqueue_us": statistics.median(enq)}
    b, s = row["batched"], row["baseline"]
    row["baseline_over_batched"] = s["median_us"] / b["median_us"]
    row["no_slower"] = bool(b["median_us"] <= s["median_us"] + max(b["spread_us"], s["spread_us"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", default="both", choices=("device", "host", "both"))
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    ap.add_argument("--quick", action="store_true", help="B = 4, mixed inputs, device frames only (for the kernel-trace run)")
    args = ap.parse_args()
    assert args.rounds >= 5 or args.quick, "at least five rounds"
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    import siammot_amd  # noqa: F401
    from siammot_amd.config import get_default_cfg
    from siammot_amd.preprocess import FramePreprocessor
    pre = FramePreprocessor.from_cfg(get_default_cfg(), device=dev)
    wheres = ("device", "host") if args.frames == "both" else (args.frames,)
    if args.quick:
        cases = [(4, "mixed", "device")]
    else:
        cases = [(B, s, w) for w in wheres for s in SETS for B in (1, 2, 4, 8) if not (s == "mixed" and B == 1)]
    results = []
    for B, set_name, where in cases:
        for out_name, dtype, cl in OUTPUTS:
            steps = args.steps if where == "device" else max(5, args.steps // 4)
            r = run_row(pre, B, set_name, out_name, dtype, cl, where, steps, args.warmup, args.rounds, dev)
            results.append(r)
            print(json.dumps(r), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "net_hw": list(NET_HW), "rows": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
