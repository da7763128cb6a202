"""Several cameras on one GPU, the host side (no device needed): the batched track solver's entry point
(smot_track_solve_batched_fwd: declared, exported, bound; every refusal before a launch, with the image named) and
``MultiCameraTrackingLoop`` against independent ``TrackingLoop``s around the fake tracker — every step through
``solver.solve_batched``'s camera-by-camera form, which is all a CPU can run.  The device side is
tests/test_multi_camera_gpu.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from fake_tracker import SEQ, FakeTracker, detections
from test_solver import _numpy_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smot_track_solve_batched_fwd"


def test_batched_solver_symbol_is_declared_exported_and_bound():
    import siammot_amd.ops as ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smot_emm.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    assert NAME in ops.EXPORTED_SYMBOLS
    lib = ops.load_library()
    assert hasattr(ctypes.CDLL(ops.LIB_PATH), NAME)
    assert len(getattr(lib, NAME).argtypes) == 29            # num_images, 27 per-image arrays, stream
    assert ops.ABI_VERSION == lib.smot_abi_version() == 14
    assert ops.TRACK_SOLVE_CHUNK == 16 and ops.MAX_IMAGES == 64


class _Tables(object):
    """The 27 per-image host arrays of one call, filled with a legal frame per image (fake, aligned, distinct addresses:
    a call that is refused — or has no rows — never looks behind them)."""
    PTRS = ("det_boxes", "det_scores", "det_ids", "det_labels", "trk_boxes", "trk_scores", "trk_ids", "trk_labels",
            "pool_state", "out_boxes", "out_scores", "out_ids", "out_labels", "act_boxes", "act_ids", "act_labels",
            "act_scores", "record")
    ORDER = ("det_boxes", "det_scores", "det_ids", "det_labels", "n_det", "trk_boxes", "trk_scores", "trk_ids", "trk_labels",
             "n_trk", "bias", "track", "start", "resume", "nms", "max_dormant", "pool_state", "cap", "out_boxes", "out_scores",
             "out_ids", "out_labels", "act_boxes", "act_ids", "act_labels", "act_scores", "record")

    def __init__(self, B, rows=(3, 2)):
        self.B = B
        self.a = {}
        for k, name in enumerate(self.PTRS):
            self.a[name] = np.array([0x10000000 + 0x100000 * k + 0x1000 * b for b in range(B)], dtype=np.uint64)
        self.a["n_det"] = np.full(B, rows[0], np.int32)
        self.a["n_trk"] = np.full(B, rows[1], np.int32)
        self.a["max_dormant"] = np.full(B, 2, np.int32)
        self.a["cap"] = np.full(B, 512, np.int32)
        for name, v in (("bias", 1.0), ("track", 0.3), ("start", 0.5), ("resume", 0.4), ("nms", 0.5)):
            self.a[name] = np.full(B, v, np.float32)
        self.null = set()

    def call(self, lib, num_images=None):
        args = [0 if n in self.null else self.a[n].ctypes.data for n in self.ORDER]
        return lib.smot_track_solve_batched_fwd(self.B if num_images is None else num_images, *args, None)


def test_batched_solver_argument_errors_are_reported_without_a_device():
    """Everything is validated before the first launch and before any per-image pointer is dereferenced."""
    import siammot_amd.ops as ops
    lib = ops.load_library()
    BAD, UNSUPPORTED = -1, -2

    def refused(t, code, *msgs, **kw):
        assert t.call(lib, **kw) == code, msgs
        err = lib.smot_last_error()
        for m in msgs:
            assert m in err, (err, m)

    refused(_Tables(1), BAD, b"num_images=0", num_images=0)
    refused(_Tables(1), BAD, b"num_images=65", num_images=65)
    refused(_Tables(1), BAD, b"num_images=-3", num_images=-3)
    for name in _Tables.ORDER:                               # any of the 27 tables missing
        t = _Tables(3)
        t.null.add(name)
        refused(t, BAD, b"null per-image table")
    for name in ("n_det", "n_trk"):
        t = _Tables(3)
        t.a[name][2] = -1
        refused(t, BAD, b"image 2", b"negative box count")
    # an image with rows: the single entry's null-pointer and alignment checks, with the image named
    for name, msg in (("pool_state", b"null pool state / record"), ("record", b"null pool state / record"),
                      ("det_boxes", b"null detection pointer"), ("det_scores", b"null detection pointer"),
                      ("det_ids", b"null detection pointer"), ("trk_boxes", b"null track pointer"),
                      ("trk_ids", b"null track pointer"), ("out_boxes", b"null output pointer"),
                      ("act_scores", b"null output pointer"), ("out_labels", b"null output pointer")):
        t = _Tables(4)
        t.a[name][1] = 0
        refused(t, BAD, b"image 1", msg)
    t = _Tables(2)
    t.a["cap"][1] = 0
    refused(t, BAD, b"image 1", b"null pool state / record")
    for name in ("out_boxes", "act_boxes"):
        t = _Tables(5)
        t.a[name][4] += 8
        refused(t, BAD, b"image 4", b"16-byte aligned")
    for name in ("det_labels", "trk_labels"):                # labels may be missing per image (1), as in the single entry
        t = _Tables(2, rows=(0, 0))
        t.a[name][:] = 0
        assert t.call(lib) == 0
    # capacities: as the single entry
    t = _Tables(3)
    t.a["n_det"][2], t.a["n_trk"][2] = 500, 13
    refused(t, UNSUPPORTED, b"image 2", b"513 boxes")
    t = _Tables(3)
    t.a["n_det"][0], t.a["n_trk"][0] = 2 ** 31 - 1, 2 ** 31 - 1      # (the sum does not wrap)
    refused(t, UNSUPPORTED, b"image 0")
    t = _Tables(3)
    t.a["cap"][1] = 513
    refused(t, UNSUPPORTED, b"image 1", b"pool capacity 513")
    # two images with rows on one pool or one record would race; an image without rows is not in the way
    for name, msg in (("pool_state", b"share one pool_state"), ("record", b"share one record")):
        t = _Tables(4)
        t.a[name][3] = t.a[name][1]
        refused(t, BAD, b"images 1 and 3", msg)
    # a refused image behind legal ones: nothing was launched for those either (no device here: a launch would fail)
    t = _Tables(20)
    t.a["n_trk"][19] = -5
    refused(t, BAD, b"image 19")
    # legal: no image has rows — nothing is launched, whatever the pointers are
    for B in (3, 64):
        t = _Tables(B, rows=(0, 0))
        assert t.call(lib) == 0
        for name in _Tables.PTRS:
            t.a[name][:] = 0
        assert t.call(lib) == 0


class BatchedFakeTracker(FakeTracker):
    """``FakeTracker``'s arithmetic over B BoxLists, with the batched interface of ``EMM``: ``forward`` on B template /
    search-region BoxLists and the rows of all of them, ``extract_cache`` on a list of B BoxLists, ``wrap_cache``."""

    def forward(self, features, boxes, sr, targets=None, template_features=None):
        assert len(boxes) == len(sr) and template_features.shape[0] == sum(len(b) for b in boxes)
        out, n0 = [], 0
        for b, s_ in zip(boxes, sr):
            t = template_features[n0:n0 + len(b)]
            n0 += len(b)
            if len(b) == 0:
                out.append(b)
                continue
            out.append(FakeTracker.forward(self, features, [b], [s_], template_features=t)[1][0])
        return {}, out, {}

    def extract_cache(self, features, detection):
        if not isinstance(detection, (list, tuple)):
            return FakeTracker.extract_cache(self, features, detection)
        parts = [FakeTracker.extract_cache(self, features, d) for d in detection]
        return torch.cat([p[0] for p in parts]), [p[1][0] for p in parts], list(detection)

    def wrap_cache(self, x, sr_bbox, det, hint=None):
        sr = self.BoxList(sr_bbox, [det.size[0] + 2 * self.pad, det.size[1] + 2 * self.pad], "xyxy")
        for f in det.fields():
            sr.add_field(f, det.get_field(f))
        return x, [sr], [det]


def _starved(d, f):
    """One camera's detections: below every threshold in frames 7-10, none at all in frames 8-9."""
    if 7 <= f <= 10:
        d.add_field("scores", torch.full_like(d.get_field("scores"), 0.05))
        if f in (8, 9):
            d = d[:0]
    return d


def _same_boxlist(a, b, where):
    assert torch.equal(a.bbox, b.bbox), where
    assert sorted(a.fields()) == sorted(b.fields()), where
    for f in a.fields():
        assert torch.equal(a.get_field(f), b.get_field(f)), (where, f)


def _same_pool(pa, pb, where):
    assert pa.get_active_ids() == pb.get_active_ids(), where
    assert list(pa._dormant_ids.items()) == list(pb._dormant_ids.items()), where
    assert pa._kill_ids == pb._kill_ids and pa._max_id == pb._max_id and pa._frame_idx == pb._frame_idx, where


def _same_memory(ma, mb, where):
    assert len(ma[2][0]) == len(mb[2][0]), where
    assert ma[0].numel() == mb[0].numel() and torch.equal(ma[0].reshape(-1), mb[0].reshape(-1)), where
    assert torch.equal(ma[1][0].bbox, mb[1][0].bbox) and torch.equal(ma[2][0].bbox, mb[2][0].bbox), where
    if len(mb[2][0]):
        assert torch.equal(ma[2][0].get_field("ids"), mb[2][0].get_field("ids")), where


def test_multi_camera_loop_equals_independent_loops_on_cpu():
    import siammot_amd.ops as ops
    from siammot_amd.multi_camera import MultiCameraTrackingLoop
    from siammot_amd.solver import TrackPool, TrackSolver
    from siammot_amd.track_head import TrackHead, TrackingLoop
    B, STARVED, FRAMES = 3, 1, 30
    tu = types.SimpleNamespace(pad_pixels=SEQ["pad"])

    def parts(tracker):
        pool = TrackPool(max_dormant_frames=2)
        return TrackHead(tracker, tu, pool).eval(), TrackSolver(pool, *SEQ["thresholds"], nms_mask_fn=_numpy_mask)

    singles = [TrackingLoop(*parts(FakeTracker(SEQ["pad"]))).eval() for _ in range(B)]
    shared = BatchedFakeTracker(SEQ["pad"])
    heads, solvers = zip(*[parts(shared) for _ in range(B)])
    multi = MultiCameraTrackingLoop(shared, list(heads), list(solvers)).eval()
    rs = [[np.random.RandomState(11 + b) for b in range(B)] for _ in range(2)]
    feats = (torch.zeros(B),)
    seen = dict(dormant=False, resumed=False, expired=False, empty=False)
    before = ops.FALLBACKS["multi_camera_per_camera"]
    for f in range(FRAMES):
        dets = [[_starved(detections(r, f), f) if b == STARVED else detections(r, f) for b, r in enumerate(side)] for side in rs]
        dormant_before = [set(s_.track_pool._dormant_ids) for s_ in solvers]
        # the fake tracker scores an id the same in every frame, so nothing it suspends ever comes back by itself: camera 0
        # runs frame 12 with a stricter track threshold (cameras may be configured differently, and re-configured) — what
        # that frame suspends resumes in frame 13 unless a detection takes its place
        solvers[0].track_thresh = singles[0].solver.track_thresh = 0.7 if f == 12 else SEQ["thresholds"][0]
        outs = multi(feats, dets[0])
        assert len(outs) == B
        for b in range(B):
            where = "camera %d, frame %d" % (b, f)
            want = singles[b](tuple(x[b:b + 1] for x in feats), dets[1][b])
            _same_boxlist(outs[b], want, where)
            pa, pb = solvers[b].track_pool, singles[b].solver.track_pool
            _same_pool(pa, pb, where)
            _same_memory(multi.track_memory[b], singles[b].track_memory, where)
            seen["dormant"] |= bool(pa._dormant_ids)
            seen["resumed"] |= bool(dormant_before[b] & pa.get_active_ids())
            seen["expired"] |= bool(dormant_before[b] & pa._kill_ids)
        seen["empty"] |= len(dets[0][STARVED]) == 0
    assert all(seen.values()), seen
    # every step ran camera by camera (a numpy NMS is not the kernel's)
    assert ops.FALLBACKS["multi_camera_per_camera"] == before + FRAMES
    # one camera restarts its video: the others are undisturbed; its first frame has no detections — a camera without rows
    multi.reset(camera=1)
    singles[1].reset()
    assert multi.track_memory[1] is None and multi.track_memory[0] is not None and solvers[1].track_pool._max_id == -1
    assert solvers[0].track_pool._max_id > 5
    dets = [[detections(r, FRAMES)[:0] if b == 1 else detections(r, FRAMES) for b, r in enumerate(side)] for side in rs]
    outs = multi(feats, dets[0])
    assert outs[1] is dets[0][1] and solvers[1].track_pool._frame_idx == 0
    for b in range(B):
        _same_boxlist(outs[b], singles[b](tuple(x[b:b + 1] for x in feats), dets[1][b]), "camera %d after the restart" % b)
        _same_pool(solvers[b].track_pool, singles[b].solver.track_pool, "camera %d after the restart" % b)
        _same_memory(multi.track_memory[b], singles[b].track_memory, "camera %d after the restart" % b)
    multi.reset()
    assert multi.track_memory == [None] * B and all(s_.track_pool._max_id == -1 for s_ in solvers)


def test_solve_batched_leaves_cameras_without_rows_alone():
    from siammot_amd.solver import TrackPool, TrackSolver, solve_batched
    from siammot_amd.structures import BoxList
    solvers = [TrackSolver(TrackPool(max_dormant_frames=2), nms_mask_fn=_numpy_mask) for _ in range(2)]
    empty = [BoxList(torch.zeros((0, 4)), (1280, 704)) for _ in range(2)]
    seen = []
    outs = solve_batched(solvers, empty, [None, None], 1.0, on_record=seen.append)
    assert outs[0] is empty[0] and outs[1] is empty[1] and len(seen) == 1
    assert all(s_.track_pool._frame_idx == 0 for s_ in solvers)
    with pytest.raises(RuntimeError, match="2 solvers, 1 detection lists"):
        solve_batched(solvers, empty[:1])
