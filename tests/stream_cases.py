"""Helpers of the stream tests (tests/test_streams.py) — TEST INFRASTRUCTURE.  Imports without a device.

* ``spin(ms)``: a bounded busy kernel on the current stream (``torch.cuda._sleep``), the one deterministic way of making a
  stream late: whatever is enqueued behind it on that stream starts ``ms`` later, whatever was wrongly enqueued on another
  stream does not wait.  The cycles per millisecond are measured once per session between two events (no clock rate is
  assumed); a spin beyond ``SPIN_MAX_MS`` is refused.
* ``fresh_streams(n)``: new side streams of the test device that run beside one another (no shared hardware queue).
* ``bits_equal(a, b)``: the same bits — integer views, so equal NaN patterns compare equal — over tensors, lists / tuples,
  BoxLists (``bbox``, ``size``, ``mode`` and every field) and plain values.
* ``late_pack(real, box)``: the wrapper of section (b) around a pack function (or ``ops.rpn_anchors``).
"""
import time

import torch

DEV = "cuda:0"
SPIN_MS = 20.0                        # what every test asks for
SPIN_MAX_MS = 100.0
PROBE_CYCLES = 10_000_000
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_calibration = {}


def cycles_per_ms():
    """``torch.cuda._sleep``'s cycles per millisecond on this device: one ``_sleep(PROBE_CYCLES)`` timed between two events,
    once per session (after a short one that loads the kernel)."""
    if "cycles_per_ms" not in _calibration:
        torch.cuda.synchronize()
        torch.cuda._sleep(1000)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        torch.cuda._sleep(PROBE_CYCLES)
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end)
        if not ms > 0:
            raise RuntimeError("stream_cases: the calibration spin took %r ms" % (ms,))
        _calibration["probe_ms"] = ms
        _calibration["cycles_per_ms"] = PROBE_CYCLES / ms
    return _calibration["cycles_per_ms"]


def probe_ms():
    """The milliseconds the calibration's ``_sleep(PROBE_CYCLES)`` took."""
    cycles_per_ms()
    return _calibration["probe_ms"]


def spin(ms=SPIN_MS):
    """Keep the current stream busy for ``ms`` milliseconds (at most ``SPIN_MAX_MS``): bounded, not a hang."""
    if not 0 < ms <= SPIN_MAX_MS:
        raise ValueError("stream_cases.spin: %r ms is outside (0, %g]" % (ms, SPIN_MAX_MS))
    torch.cuda._sleep(int(ms * cycles_per_ms()))


PROBE_MS = 2.0
_probes = {"tried": 0, "shared": 0}


def runs_beside(busy, other):
    """Work on stream ``other`` does not wait for work on stream ``busy``: behind a ``PROBE_MS`` spin on ``busy``, an event on
    ``other`` completes while the spin still runs.  Two torch streams may share one hardware queue (the runtime opens a few
    and deals the streams out over them), and a queue runs its packets in the order they were submitted: there a late stream
    delays the other one as well, and a test that relies on one stream being late and the other not proves nothing."""
    with torch.cuda.stream(busy):
        spin(PROBE_MS)
        spun = torch.cuda.Event()
        spun.record()
    with torch.cuda.stream(other):
        reached = torch.cuda.Event()
        reached.record()
    reached.synchronize()
    beside = spun.query() is False
    spun.synchronize()
    _probes["tried"] += 1
    _probes["shared"] += 0 if beside else 1
    return beside


def fresh_streams(n, apart_from=(), device=DEV):
    """``n`` new ``torch.cuda.Stream(device)`` objects, each of which runs beside the others and beside the streams
    ``apart_from`` (``runs_beside`` in both directions is one property: a shared queue).  Raises when the pool's streams do
    not offer that many."""
    chosen = []
    for _ in range(64):
        if len(chosen) == n:
            return chosen
        s = torch.cuda.Stream(device)
        if all(runs_beside(c, s) for c in list(apart_from) + chosen):
            chosen.append(s)
    if len(chosen) == n:
        return chosen
    raise RuntimeError("stream_cases.fresh_streams: found %d of %d streams that run beside %d others (%d probes, %d on a shared "
                       "queue)" % (len(chosen), n, len(apart_from), _probes["tried"], _probes["shared"]))


def _bits(t):
    if t.dtype is torch.bool:
        return t.to(torch.uint8)
    if t.dtype.is_floating_point:
        return t.contiguous().view(_INT_VIEW[t.element_size()])
    return t


def bits_equal(a, b):
    """``a`` and ``b`` have one structure and every tensor in it the same shape, dtype and bits."""
    if isinstance(a, torch.Tensor):
        return (isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype
                and bool(torch.equal(_bits(a.detach()).cpu(), _bits(b.detach()).cpu())))
    if hasattr(a, "bbox") and hasattr(a, "extra_fields"):                     # a BoxList
        return (hasattr(b, "bbox") and hasattr(b, "extra_fields") and tuple(a.size) == tuple(b.size) and a.mode == b.mode
                and bits_equal(a.bbox, b.bbox) and list(a.extra_fields) == list(b.extra_fields)
                and all(bits_equal(a.extra_fields[k], b.extra_fields[k]) for k in a.extra_fields))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(bits_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(bits_equal(x, y) for x, y in zip(a, b))
    if hasattr(a, "dtype") and hasattr(a, "tobytes"):                           # a numpy array
        return hasattr(b, "tobytes") and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


def any_nan(x):
    """Some floating tensor in ``x`` (the structures of ``bits_equal``) holds a NaN."""
    if isinstance(x, torch.Tensor):
        return bool(x.is_floating_point() and torch.isnan(x).any())
    if hasattr(x, "bbox") and hasattr(x, "extra_fields"):
        return any_nan(x.bbox) or any_nan(list(x.extra_fields.values()))
    if isinstance(x, (list, tuple)):
        return any(any_nan(v) for v in x)
    return False


def late_pack(real, box):
    """Section (b)'s wrapper around ``real`` (a pack function, or ``ops.rpn_anchors``).  On the stream that is current when it
    is called: a spin, the event ``spun`` behind it (appended to ``box["spun"]``), the real call — so the image is written
    about ``SPIN_MS`` from now — and, on a third stream, a NaN fill of the returned tensor(s), which alone is waited for on
    the host.  In real time the image is NaN when the wrapper returns and becomes the packed image when the spin ends."""
    def wrapper(*args, **kwargs):
        (third,) = fresh_streams(1, apart_from=[torch.cuda.current_stream()])   # (its fill must not queue up behind the spin)
        box["host_t0"] = time.perf_counter()
        spin(SPIN_MS)
        spun = torch.cuda.Event()
        spun.record()
        out = real(*args, **kwargs)
        with torch.cuda.stream(third):
            for t in (out if isinstance(out, (list, tuple)) else (out,)):
                t.fill_(float("nan"))
        third.synchronize()
        box.setdefault("spun", []).append(spun)
        box["calls"] = box.get("calls", 0) + 1
        return out
    wrapper.__wrapped__ = real
    return wrapper
