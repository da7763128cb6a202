"""A/B of two builds of the product library (e.g. another compiler flag), same session, interleaved: frame pair and
tracking loop.    python measure/lib_ab.py measure/libsmot_emm_preload.so [ALTERNATIONS, default 3]"""
import json, os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench
import siammot_amd.ops as ops
from siammot_amd.structures import BoxList
from siammot_amd.emm import EMM
from siammot_amd.config import get_default_cfg
from siammot_amd.track_utils import build_track_utils
dev = torch.device("cuda:0")
base = ops.load_library()
other = ops._open(os.path.abspath(sys.argv[1]), ops._SIGNATURES)
assert other.smot_abi_version() == ops.ABI_VERSION
feats = [bench.synthetic_features(k, dev) for k in range(4)]
n = 30
boxes = bench.synthetic_boxes(n, (1280, 704)).to(dev)
det = BoxList(boxes, (1280, 704), mode="xyxy")
det.add_field("ids", torch.arange(n, device=dev))
det.add_field("labels", torch.ones(n, dtype=torch.int64, device=dev))
cfg = get_default_cfg(channels=bench.CHANNELS)
emm = EMM(cfg, build_track_utils(cfg)).eval()
bench.init_predictor(emm.predictor, boxes.cpu())
emm = emm.to(dev)
ref = None
for rep in range(int(sys.argv[2]) if len(sys.argv) > 2 else 3):
    for name, lib in (("product", base), ("variant", other)):
        ops._lib = lib
        with torch.no_grad():
            state = emm.extract_cache(feats[3], det)
            def step(k, state):
                z, sr, d = state
                _, res, _ = emm(feats[k % 4], d, sr, template_features=z)
                return emm.extract_cache(feats[k % 4], det), res
            for k in range(100):
                state, res = step(k, state)
            out = torch.cat((res[0].bbox, res[0].get_field("scores")[:, None]), 1).clone()
            ref = out if ref is None else ref
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(300):
                    state, res = step(k, state)
                e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) / 300 * 1e3)
            r = bench.tracking_loop_throughput(30, dev, feats[:2], steps=400, refine=True)
        print(json.dumps({"library": name, "frame_pair_us": round(min(ts), 2), "bitwise_equal": bool(torch.equal(out, ref)),
                          "loop_refine_ms": round(r["ms_per_frame"], 4)}), flush=True)
ops._lib = base
