"""the drop-in claim of INTEGRATION.md §3 against what the REAL reference classes did with this EMM.
CPU-only, no kernel launch.  oracle/check_reference_dropin.py runs the reference's own ``build_track_head`` / ``TrackHead``
/ ``TrackSolver`` / ``TrackPool`` around ``siammot_amd.emm.EMM`` and, with ``--golden``, records what it saw in
tests/golden/reference_dropin.json; this test checks the package against that record."""
import json
import os

import torch


def test_reference_build_track_head_holds_the_hip_emm(golden_dir):
    """``register("EMM", override=True)`` puts ``siammot_amd.emm.EMM`` where ``build_track_head`` looks it up; the
    reference EMM's state_dict loads into it key for key, shape for shape; driven through the reference's TrackHead /
    TrackSolver / TrackPool call sequence (tests/reference_call_sequence.py): the first frame takes the no-tracker path,
    the solver starts the tracks the reference's did, and the head calls ``extract_cache`` / ``forward`` with the
    argument structure the reference's TrackHead used."""
    import golden_inputs as gi
    import reference_call_sequence as rcs
    import siammot_amd.emm as hip_emm
    from oracle.ref_structures import BoxList
    from siammot_amd.config import get_default_cfg
    from siammot_amd.registry import SIAMESE_TRACKER
    from siammot_amd.track_utils import build_track_utils
    want = json.load(open(os.path.join(golden_dir, "reference_dropin.json")))
    assert want["ok"] and want["tracker_class"] == "siammot_amd.emm.EMM"
    assert want["track_head_class"] == "siammot.modelling.track_head.track_head.TrackHead"

    hip_emm.register("EMM", override=True)
    assert SIAMESE_TRACKER["EMM"] is hip_emm.EMM and SIAMESE_TRACKER["EMM_HIP"] is hip_emm.EMM

    case = gi.EMM_CASES["default"]
    cfg = get_default_cfg(channels=case["channels"])
    tracker = SIAMESE_TRACKER["EMM"](cfg, build_track_utils(cfg))
    sd = {k: torch.zeros(v["shape"], dtype=getattr(torch, v["dtype"].split(".")[-1])) for k, v in want["state_dict"].items()}
    missing = tracker.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    assert sorted(tracker.state_dict().keys()) == sorted(sd.keys()) and len(sd) == want["state_dict_keys"] == 12
    assert all(str(v.dtype) == want["state_dict"][k]["dtype"] for k, v in tracker.state_dict().items())

    pool = rcs.TrackPool(max_dormant_frames=1)
    head = rcs.TrackHead(tracker, tracker.track_utils, pool).eval()
    solver = rcs.TrackSolver(pool, 0.4, 0.6, 0.4)          # TRACK_THRESH / START_TRACK_THRESH / RESUME_TRACK_THRESH
    W, H = case["image_wh"]
    feats = tuple(torch.zeros(s) for s in gi.feature_shapes((W, H), case["channels"]))
    assert head(feats, track_memory=None) == ({}, None, {})                  # first frame: no tracker call
    det = BoxList(torch.from_numpy(gi.emm_case_inputs("default")["boxes"][:3].copy()), (W, H), mode="xyxy")
    det.add_field("labels", torch.ones(3, dtype=torch.int64))
    det.add_field("scores", torch.tensor([0.9, 0.8, 0.3]))
    det.add_field("ids", torch.full((3,), -1, dtype=torch.int64))
    dets = solver([det])
    assert dets[0].get_field("ids").tolist() == want["tracks_started"] == [0, 1, -1]

    calls = {}

    def fake_extract_cache(features, detection):
        calls["extract_cache"] = [len(features), len(detection)]
        sr = BoxList(detection.bbox + 512.0, (W + 1024, H + 1024), mode="xyxy")
        for f in detection.fields():
            sr.add_field(f, detection.get_field(f))
        return torch.zeros(len(detection), case["channels"], 15, 15), [sr], [detection]

    def fake_forward(features, boxes, sr, targets=None, template_features=None):
        calls["forward"] = dict(n_feat=len(features), n_boxes=len(boxes[0]), sr_size=list(sr[0].size),
                                z_shape=list(template_features.shape))
        return {}, boxes, {}
    tracker.extract_cache = fake_extract_cache
    tracker.forward = fake_forward
    memory = head.get_track_memory(feats, dets)
    assert calls["extract_cache"] == want["calls"]["extract_cache"]
    head(feats, track_memory=memory)
    assert calls["forward"] == want["calls"]["forward"]
