"""The tracking step for B cameras that share a GPU: one head call, one box-head refinement call (§3j), one solver launch
per 16 cameras, one host synchronisation and one template extraction per step, whatever B is.

``MultiCameraTrackingLoop`` is the general path of ``TrackingLoop._forward`` (roi_heads.py:38-50 of the reference: head,
[box-head refinement,] solver, track memory) over B independent video streams: ONE ``EMM`` shared by all cameras, and per
camera its own ``TrackPool`` / ``TrackSolver`` / ``TrackHead`` and its own track memory in the reference's form
``(templates, [search regions], [template boxes])``.  Camera b's outputs, pool and memory are bit for bit those of a
``TrackingLoop`` of its own that is fed ``tuple(f[b:b+1] for f in features)``.

It composes parts that exist — ``EMM.forward`` / ``EMM.extract_cache`` over B BoxLists (§3b), ``solver.solve_batched``,
``TrackHead.get_track_memory`` — and owns nothing of ``TrackingLoop``'s lean paths: dormant tracks join a camera's memory on
the host, as in the reference, and the boxes go through BoxLists.
"""
import torch

from . import ops
from .solver import TrackPool, builder_tracker_solver, solve_batched
from .track_head import TrackHead, TrackingLoop


class MultiCameraTrackingLoop(torch.nn.Module):
    """``forward(features, detections) -> [BoxList] * B``: ``features`` a tuple of ``[B, C, H_l, W_l]`` maps (what the batched
    head accepts: fp32 / fp16 / bf16, NCHW or channels-last), ``detections`` one BoxList per camera, all of one image size."""

    # the refinement of the cameras' propagated boxes in ONE ``refine_tracks(features, [tracks_b ...])`` call per step when
    # the callable offers it (``offers_batched``: ``box_refine.RefineTracks`` over a ``TrackBoxHead`` on the device);
    # False: camera by camera, as for any other callable
    batched_refinement = True

    def __init__(self, emm, track_heads, solvers, refine_tracks=None):
        super(MultiCameraTrackingLoop, self).__init__()
        if len(track_heads) != len(solvers) or not track_heads:
            raise ValueError("MultiCameraTrackingLoop: %d track heads, %d solvers" % (len(track_heads), len(solvers)))
        self.emm = emm
        # (plain lists: the heads hold no parameters beside the shared EMM's, which `self.emm` registers once)
        self.tracks = list(track_heads)
        self.solvers = list(solvers)
        self.refine_tracks = refine_tracks
        self.num_cameras = len(track_heads)
        self.track_memory = [None] * self.num_cameras

    def reset(self, camera=None):
        """Forget the tracks of every camera, or of ``camera`` alone (its video restarts while the others run)."""
        for b in (range(self.num_cameras) if camera is None else (camera,)):
            self.track_memory[b] = None
            self.tracks[b].reset_track_pool()

    def forward(self, features, detections):
        with torch.no_grad():
            return self._forward(features, detections)

    def _empty(self, like):
        """A camera without rows in the batched head call: no boxes, the fields the head's wrapper copies."""
        dev = like.bbox.device
        none = torch.zeros((0,), dtype=torch.int64, device=dev)
        e = like.__class__(torch.zeros((0, 4), dtype=like.bbox.dtype, device=dev), like.size, mode="xyxy")
        e.add_field("ids", none)
        e.add_field("labels", none)
        return e

    def _propagate(self, features):
        """The head on the B memories (``TrackHead.forward_inference`` per camera, one call): [tracks or None] * B."""
        B, mems = self.num_cameras, self.track_memory
        tracks = [None] * B
        for b in range(B):
            if mems[b] is None:
                self.tracks[b].track_pool.reset()                                  # track_head.py:38-39
        live = [b for b in range(B) if mems[b] is not None and mems[b][0].numel() > 0]
        if not live:
            return tracks
        if B == 1:
            t, sr, boxes = mems[0]
            tracks[0] = self.emm(features, boxes, sr=sr, template_features=t)[1][0]
            return tracks
        if len(live) == B:
            boxes, srs = [m[2][0] for m in mems], [m[1][0] for m in mems]
        else:
            first, has = mems[live[0]], set(live)
            empty_box, empty_sr = self._empty(first[2][0]), self._empty(first[1][0])
            boxes = [mems[b][2][0] if b in has else empty_box for b in range(B)]
            srs = [mems[b][1][0] if b in has else empty_sr for b in range(B)]
        templates = [mems[b][0] for b in live]
        out = self.emm(features, boxes, sr=srs, template_features=templates[0] if len(live) == 1 else torch.cat(templates))[1]
        for b in live:
            tracks[b] = out[b]
        return tracks

    def _refine_batched(self, features, tracks):
        """The propagated boxes of all cameras through ONE ``refine_tracks`` call, in place in ``tracks``; False when the
        step is to refine camera by camera (a callable without the batched form, the switch, one camera, or row counts the
        batched call does not take — counted in ``ops.FALLBACKS["refine_per_camera"]``).  The row counts are the sizes of the
        memories the head ran on: nothing is read from the device."""
        offers = getattr(self.refine_tracks, "offers_batched", None)
        live = [b for b in range(self.num_cameras) if tracks[b] is not None]
        if offers is None or not self.batched_refinement or self.num_cameras == 1 or not live or not offers():
            return False
        first = tracks[live[0]]
        lists = [tracks[b] if tracks[b] is not None else self._empty(first) for b in range(self.num_cameras)]
        if not self.refine_tracks.batch_ok(lists):
            ops.FALLBACKS["refine_per_camera"] += 1
            return False
        out = self.refine_tracks(features, lists)
        for b in live:
            tracks[b] = out[b]
        return True

    def _forward(self, features, detections):
        B = self.num_cameras
        if len(detections) != B:
            raise RuntimeError("MultiCameraTrackingLoop: %d detection lists for %d cameras" % (len(detections), B))
        mems_before = list(self.track_memory)
        tracks = self._propagate(features)                                         # roi_heads.py:38
        bias = 1.0
        if self.refine_tracks is not None:                                         # roi_heads.py:43-45
            bias = 0.0
            if not self._refine_batched(features, tracks):                         # camera by camera
                for b in range(B):
                    if tracks[b] is not None:
                        tracks[b] = self.refine_tracks(tuple(f[b:b + 1] for f in features), [tracks[b]])[0]
        pre = {}

        def extract(outs):
            # the next memories' templates / search regions of every camera's active rows: ONE launch, enqueued as soon as
            # the records are on the host — it runs while the host mirrors the pools and builds the memories
            acts = [self.tracks[b]._get_track_targets(outs[b]) for b in range(B)]
            if not any(len(a) for a in acts):
                return
            for b in range(B):
                if len(outs[b]) and getattr(outs[b], "active_rows", None) is None:
                    outs[b].active_rows = acts[b]          # (a camera-by-camera step: filtered once, here)
            if B == 1:
                x, srs, _ = self.emm.extract_cache(features, acts[0])
            else:
                x, srs, _ = self.emm.extract_cache(features, acts)
            n0 = 0
            for b in range(B):
                n1 = n0 + len(acts[b])
                pre[b] = (x[n0:n1], srs[b].bbox)
                n0 = n1

        outs = solve_batched(self.solvers, detections, tracks, bias, on_record=extract)      # the step's one synchronisation
        for b in range(B):
            if getattr(outs[b], "nan_track_scores", False):
                TrackingLoop._raise_on_bad_hint(mems_before[b])
            self.track_memory[b] = self.tracks[b].get_track_memory(features, [outs[b]], precomputed=pre.get(b))
        return outs


def build_multi_camera_tracking_loop(cfg, num_cameras, device="cuda", refine_tracks=None):
    """``build_tracking_loop`` for ``num_cameras`` video streams on one device: one EMM head, and a pool, a solver and a
    ``TrackHead`` per camera around it.  ``refine_tracks`` as there (``box_refine.RefineTracks``: one batched call per step, any other callable camera by camera;
    ``False``: none, explicitly)."""
    if refine_tracks is False:
        refine_tracks = None
    elif refine_tracks is None:
        import warnings
        warnings.warn("siammot_amd.build_multi_camera_tracking_loop: no refine_tracks callable — propagated boxes are scored "
                      "track_conf + 1 instead of the reference's box-head refinement (roi_heads.py:60-84)", stacklevel=2)
    from .emm import EMM
    from .track_utils import build_track_utils
    if not 1 <= num_cameras <= ops.MAX_IMAGES:
        raise ValueError("build_multi_camera_tracking_loop: %d cameras, need 1..%d" % (num_cameras, ops.MAX_IMAGES))
    tu = build_track_utils(cfg)
    emm = EMM(cfg, tu).to(device).eval()
    pools = [TrackPool(max_dormant_frames=cfg.MODEL.TRACK_HEAD.MAX_DORMANT_FRAMES) for _ in range(num_cameras)]
    heads = [TrackHead(emm, tu, p).eval() for p in pools]
    return MultiCameraTrackingLoop(emm, heads, [builder_tracker_solver(cfg, p) for p in pools], refine_tracks).eval()
