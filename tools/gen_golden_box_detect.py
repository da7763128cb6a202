#!/usr/bin/env python
"""Generate ``tests/golden/box_detect_post.npz`` with the REFERENCE's own box-head post-processor on the CPU.

Imported UNMODIFIED from the reference checkout ($SIAMMOT_REFERENCE):
    siammot/modelling/box_head/inference.py    PostProcessor.forward / filter_results
Its ``maskrcnn_benchmark`` imports are satisfied by stubs in ``sys.modules``: the oracle's BoxList / cat_boxlist
(oracle/ref_structures.py), the oracle's BoxCoder (oracle/box_head_oracle.py) and a restatement, below, of upstream's
``boxlist_nms`` over the numpy NMS (oracle/solver_oracle.py).

The inputs are ``tests/box_detect_cases.py::case(name)`` for ``GOLDEN_CASES`` — id-less proposals, as the RPN hands them
over; only the rows that exist go in.  Every case must meet ``box_detect_cases.conditions`` (asserted here and again by
tests/test_box_detect.py).  Stored: per case the reference's boxes, scores and labels — outputs only; the tests regenerate
the inputs.  The archive is written with fixed member timestamps, so a regeneration is byte-stable.

Usage:  python tools/gen_golden_box_detect.py            write the archive
        python tools/gen_golden_box_detect.py --search   print, per seeded case, the first of six seeds that meets the
                                                         conditions (what ``box_detect_cases.SEEDS`` holds)
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("SIAMMOT_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import box_detect_cases as B                                  # noqa: E402
from oracle import solver_oracle as SO                        # noqa: E402
from oracle.box_head_oracle import BoxCoder                   # noqa: E402
from oracle.ref_structures import BoxList, cat_boxlist        # noqa: E402


def boxlist_nms(boxlist, nms_thresh, max_proposals=-1, score_field="scores"):
    """[UPSTREAM] structures/boxlist_ops.py over the numpy NMS."""
    if nms_thresh <= 0:
        return boxlist
    mode = boxlist.mode
    boxlist = boxlist.convert("xyxy")
    keep = SO.nms_indices(boxlist.bbox.numpy(), boxlist.get_field(score_field).numpy(), nms_thresh)
    if max_proposals > 0:
        keep = keep[:max_proposals]
    return boxlist[torch.from_numpy(keep)].convert(mode)


def install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod("maskrcnn_benchmark")
    mod("maskrcnn_benchmark.structures")
    mod("maskrcnn_benchmark.structures.bounding_box", BoxList=BoxList)
    mod("maskrcnn_benchmark.structures.boxlist_ops", boxlist_nms=boxlist_nms, cat_boxlist=cat_boxlist)
    mod("maskrcnn_benchmark.modeling")
    mod("maskrcnn_benchmark.modeling.box_coder", BoxCoder=BoxCoder)
    sys.path.insert(0, REFERENCE)


def save_npz_stable(path, arrays):
    """``np.savez_compressed`` with the members' timestamps fixed: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def search():
    for name in B.CASE_NAMES:
        if name not in B.SEEDS:
            continue
        base, found = B.SEEDS[name] // 100 * 100, None
        for seed in range(base, base + 6):
            c = B.build_case(name, seed)
            if B.conditions_hold(c, B.conditions(c)):
                found = seed
                break
        print("%s: %s" % (name, found if found is not None else "no seed of six meets the conditions"))


def load_post_processor():
    """The reference's module, loaded from its file alone (the package's __init__ pulls in the whole model)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "reference_box_head_inference", os.path.join(REFERENCE, "siammot", "modelling", "box_head", "inference.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.PostProcessor


def main():
    if "--search" in sys.argv:
        return search()
    install_stubs()
    PostProcessor = load_post_processor()
    torch.set_grad_enabled(False)
    out = {}
    for name in B.GOLDEN_CASES:
        c = B.case(name)
        cond = B.conditions(c)
        assert B.conditions_hold(c, cond), (name, cond)
        K, KR, n = c["num_classes"], c["reg_classes"], c["count"]
        ho = torch.from_numpy(c["head_out"][:n])
        post = PostProcessor(c["score_thresh"], c["nms_thresh"], 100, BoxCoder(c["weights"]), c["agnostic"], False,
                             c["clip_wh"] is None).eval()
        prop = BoxList(torch.from_numpy(c["boxes"][:n].copy()), c["clip_wh"] or B.IMAGE_WH, mode="xyxy")
        r = post((ho[:, :K].contiguous(), ho[:, K:K + 4 * KR].contiguous()), [prop])[0]
        assert bool((r.get_field("ids") == -1).all())
        out[name + "/boxes"] = r.bbox.numpy()
        out[name + "/scores"] = r.get_field("scores").numpy()
        out[name + "/labels"] = r.get_field("labels").numpy()
        print("%s: %d rows x %d classes -> %d detections (candidates %d), score margin %.2e, gap %.2e, delta %.2e px" % (
            name, n, K, len(r), cond["candidates"], cond["score_margin"], cond["score_gap"], cond["delta"]))
    path = os.path.join(ROOT, "tests", "golden", "box_detect_post.npz")
    save_npz_stable(path, out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 100000


if __name__ == "__main__":
    main()
