"""FPN on the device (siammot_amd.fpn.FPN, ops.fpn / fpn_pack, csrc/fpn.hip, csrc/conv3x3_mfma.h) and
``DetectionHead.forward_stages``.

CPU: symbols, ``state_dict`` keys and initialisation, the module on CPU tensors against the yardstick bit for bit, the config's
pyramid, the upstream patch.
GPU: the kernels against torch's ``F.conv2d`` / ``F.interpolate`` / ``F.max_pool2d`` composition on the CPU (tests/fpn_cases.py)
with the bound of the project's other matrix-core convolutions (tests/test_rpn_head.py, tests/test_hip_parity.py::
test_predictor_vs_oracle: 1e-4 of the per-channel scale against fp64, 2e-4 against fp32); exactness with integer data,
non-finite cells, half stage maps and half outputs, independence of the images of a call, fallbacks, repacking, and the
composition from stage maps to detections with one host copy.
"""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import fpn_cases as P
import rpn_head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smot_fpn_packed_floats", "smot_fpn_pack", "smot_fpn_ws_bytes", "smot_fpn_fwd")
_cache = {}


def _cfg(channels=128):
    from siammot_amd.config import get_default_cfg
    return get_default_cfg(channels=channels)


def _reference(C, cin, N, sizes):
    """(maps, parameters, fp64 outputs, fp32 outputs, per-channel scale) of one case: computed once, never modified."""
    key = (C, cin, N, sizes)
    if key not in _cache:
        prm, x = P.params(C, cin), P.maps(cin, N, sizes)
        o64 = P.oracle(x, prm, torch.float64)
        _cache[key] = dict(prm=prm, x=x, o64=o64, o32=P.oracle(x, prm, torch.float32), scale=P.channel_scale(o64))
    return _cache[key]


def _fpn(C, cin, prm, dev="cuda", out_dtype=torch.float32, top=True, **kw):
    from siammot_amd.fpn import FPN, LastLevelMaxPool
    return P.load_fpn(FPN(cin, C, top_blocks=LastLevelMaxPool() if top else None, out_dtype=out_dtype, **kw), prm, dev)


def _dev(levels, dev="cuda"):
    return [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in levels]


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _equal_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _errors(out, ref):
    return H.scaled_error(out, ref["o64"], ref["scale"]), H.scaled_error(out, ref["o32"], ref["scale"])


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_carry_the_new_symbols():
    import siammot_amd.ops as ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smot_emm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smot_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared and name in ops.EXPORTED_SYMBOLS, name
    assert ops.ABI_VERSION == 14 and re.search(r"#define SMOT_ABI_VERSION 14\b", src)
    assert "fpn_torch" in dict(ops.FALLBACKS)                    # registered from import
    assert ops.fpn_shapes_ok(P.DLA, 128) and ops.fpn_shapes_ok(P.R50, 256)
    assert not ops.fpn_shapes_ok((64, 24), 128) and not ops.fpn_shapes_ok(P.DLA, 48) and not ops.fpn_shapes_ok(P.DLA, 544)


def test_state_dict_is_upstreams_and_the_initialisation_is_kaiming_uniform():
    from siammot_amd.fpn import FPN, LastLevelMaxPool
    torch.manual_seed(3)
    fpn = FPN(P.DLA, 128, top_blocks=LastLevelMaxPool())
    keys = [k for i in (1, 2, 3, 4) for k in ("fpn_inner%d.weight" % i, "fpn_inner%d.bias" % i, "fpn_layer%d.weight" % i,
                                                "fpn_layer%d.bias" % i)]
    sd = fpn.state_dict()
    assert list(sd.keys()) == keys
    for i, c in enumerate(P.DLA, 1):
        assert sd["fpn_inner%d.weight" % i].shape == (128, c, 1, 1) and sd["fpn_layer%d.weight" % i].shape == (128, 128, 3, 3)
        assert sd["fpn_inner%d.bias" % i].shape == (128,) and float(sd["fpn_layer%d.bias" % i].abs().max()) == 0.0
        # kaiming_uniform_(a=1): U(-b, b) with b = sqrt(6 / ((1 + a^2) fan_in)) = sqrt(3 / fan_in): all inside, the largest near b
        for w, fan_in in ((sd["fpn_inner%d.weight" % i], c), (sd["fpn_layer%d.weight" % i], 128 * 9)):
            bound = (3.0 / fan_in) ** 0.5
            assert 0.98 * bound < float(w.abs().max()) <= bound
            assert abs(float(w.std()) - bound / 3 ** 0.5) < 0.05 * bound
    assert FPN((0, 32), 32).inner_blocks == ["fpn_inner2"]      # a level without input channels has no blocks


@pytest.mark.parametrize("sizes,cin,C", [(P.ODD4, (16, 32, 64, 128), 32), (P.TWO, (48, 16), 64)])
def test_cpu_module_is_the_yardstick_bit_for_bit(sizes, cin, C):
    import siammot_amd.ops as ops
    ref = _reference(C, cin, 2, sizes)
    fpn = _fpn(C, cin, ref["prm"], "cpu")
    before = ops.FALLBACKS["fpn_torch"]
    with torch.no_grad():
        out = fpn([torch.from_numpy(v) for v in ref["x"]])
    assert isinstance(out, tuple) and _equal_bits(out, ref["o32"])
    assert ops.FALLBACKS["fpn_torch"] == before                  # counted for device tensors only
    half = _fpn(C, cin, ref["prm"], "cpu", out_dtype=torch.float16)
    with torch.no_grad():
        assert _equal_bits(half([torch.from_numpy(v) for v in ref["x"]]), [o.to(torch.float16) for o in ref["o32"]])


@pytest.mark.parametrize("channels", [128, 256])
def test_build_fpn_reads_the_config(channels):
    from siammot_amd.fpn import LastLevelMaxPool, build_fpn
    cfg = _cfg(channels)
    assert cfg.MODEL.FPN.USE_GN is False and cfg.MODEL.FPN.USE_RELU is False
    fpn = build_fpn(cfg)
    assert fpn.in_channels == (64, 128, 256, 512) and fpn.out_channels == channels
    assert type(fpn.top_blocks) is LastLevelMaxPool and len(list(fpn.top_blocks.parameters())) == 0
    assert fpn.fpn_inner3.weight.shape == (channels, 256, 1, 1) and fpn.fpn_layer1.weight.shape == (channels, channels, 3, 3)
    cfg.MODEL.FPN.USE_GN = True
    assert isinstance(build_fpn(cfg).fpn_layer1, torch.nn.Sequential)


def test_patch_upstream_fpn_sets_the_attribute(monkeypatch):
    from siammot_amd.fpn import FPN
    from siammot_amd.layers import patch_upstream_fpn
    names = ["maskrcnn_benchmark", "maskrcnn_benchmark.modeling", "maskrcnn_benchmark.modeling.backbone",
             "maskrcnn_benchmark.modeling.backbone.fpn"]
    mods = [types.ModuleType(n) for n in names]
    for parent, child, name in zip(mods, mods[1:], names[1:]):
        setattr(parent, name.rsplit(".", 1)[1], child)
    mods[-1].FPN = object
    for n, m in zip(names, mods):
        monkeypatch.setitem(sys.modules, n, m)
    assert patch_upstream_fpn() is FPN and mods[-1].FPN is FPN


# ---- GPU ----------------------------------------------------------------------------------------------------------------
ORACLE_CASES = [(C, cin, P.ODD4, N) for C, cin in ((32, (16, 32, 64, 128)), (96, (48, 96, 192, 384)), (128, P.DLA), (256, P.R50))
                for N in (1, 3)] + [(128, P.DLA, P.FLOOR, 2), (64, (48, 16), P.TWO, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("C,cin,sizes,N", ORACLE_CASES)
def test_fpn_against_the_cpu_oracle(C, cin, sizes, N):
    """Measured maxima (scaled error against fp64 / fp32 over all outputs of the call): see INTEGRATION.md §3l."""
    import siammot_amd.ops as ops
    ref = _reference(C, cin, N, sizes)
    fpn = _fpn(C, cin, ref["prm"])
    before = ops.FALLBACKS["fpn_torch"]
    with torch.no_grad():
        out = fpn(_dev(ref["x"]))
    assert ops.FALLBACKS["fpn_torch"] == before
    assert isinstance(out, tuple) and len(out) == len(sizes) + 1
    for o, want in zip(out, ref["o32"]):
        assert o.shape == want.shape and o.dtype is torch.float32 and o.is_contiguous()
    assert out[-1].shape[2:] == ((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2)
    e64, e32 = _errors(out, ref)
    print("fpn C=%d Cin=%s %s N=%d: max scaled error %.3e vs fp64, %.3e vs fp32" % (C, cin, sizes[0], N, e64, e32))
    assert e64 < 1e-4 and e32 < 2e-4
    assert torch.equal(out[-1], out[-2][:, :, ::2, ::2])         # the top block is a subsample of the coarsest map


@pytest.mark.gpu
def test_exact_with_integer_data():
    """Maps, weights and biases in {-1, 0, 1}, two levels at an exact 2x, C = 32, Cin = (16, 32).  last[1] is an integer, |.| <=
    32 + 1.  The resize's weights are 0.25 / 0.75 (1 / 0 at the border): every product w * v and h * (...) is a multiple of
    1/16 of at most 33 in size, so last[0] = lateral (|.| <= 17) + resize is a multiple of 1/16, |.| <= 50.  A 3x3 output sums
    at most 288 such terms and a bias: every partial sum is a multiple of 1/16 with |.| <= 14,401 < 2^14, i.e. an integer
    below 2^18 in units of 1/16 — exact in fp32's 24 bits in ANY summation order.  So the outputs equal the fp32 yardstick
    bit for bit; this pins borders, halo zeros, tap order and the bilinear weights."""
    C, cin, N = 32, (16, 32), 2
    rs = np.random.RandomState(11)
    ints = lambda shape: rs.randint(-1, 2, size=shape).astype(P.F32)
    prm = [(ints((C, c, 1, 1)), ints(C), ints((C, C, 3, 3)), ints(C)) for c in cin]
    x = [ints((N, c, h, w)) for c, (h, w) in zip(cin, P.EXACT)]
    o32 = P.oracle(x, prm, torch.float32)
    o64 = P.oracle(x, prm, torch.float64)
    assert all(torch.equal(a.double(), b) for a, b in zip(o32, o64))            # the yardstick itself is exact
    assert float(o32[0].abs().max()) > 100 and float((o32[0] * 16 - (o32[0] * 16).round()).abs().max()) == 0.0
    assert float((o32[0] - o32[0].round()).abs().max()) > 0                     # sixteenths do occur
    with torch.no_grad():
        out = _fpn(C, cin, prm)(_dev(x))
    for l, (g, w) in enumerate(zip(out, o32)):
        assert torch.equal(g.cpu(), w), "level %d: %d cells differ" % (l, int((g.cpu() != w).sum()))


@pytest.mark.gpu
def test_non_finite_cells_spread_as_in_torch():
    C, cin, N = 32, (16, 32, 64, 128), 3
    ref = _reference(C, cin, N, P.ODD4)
    x = [v.copy() for v in ref["x"]]
    x[0][0, 3, 5, 7] = np.inf                                    # interior of the finest stage map
    x[0][1, 10, 0, 0] = -np.inf                                  # a corner
    x[3][2, 100, 1, 1] = np.nan                                  # interior of the coarsest: spreads down the pyramid
    x[2][1, 7, 3, 5] = np.nan                                    # (and a corner two levels up: reaches part of the finer maps)
    o32 = P.oracle(x, ref["prm"], torch.float32)
    o64 = P.oracle(x, ref["prm"], torch.float64)
    with torch.no_grad():
        out = _fpn(C, cin, ref["prm"])(_dev(x))
    for l, (g, w) in enumerate(zip(out, o32)):
        assert torch.equal(torch.isfinite(g.cpu()), torch.isfinite(w)), "level %d" % l
    assert int((~torch.isfinite(o32[0][0])).sum()) == C * 9 and bool(torch.isfinite(o32[1][0]).all())
    assert not bool(torch.isfinite(o32[0][2]).any()) and not bool(torch.isfinite(o32[4][2]).any())   # taps of weight 0 count
    for l in (0, 1):                                             # image 1: the corner's -inf, and part of the map from x[2]'s NaN
        assert 4 < int((~torch.isfinite(o32[l][1, 0])).sum()) < o32[l][1, 0].numel()
    assert bool(torch.isfinite(o32[3][1]).all())
    e64 = H.scaled_error(out, o64, ref["scale"])
    e32 = H.scaled_error(out, o32, ref["scale"])
    print("fpn with non-finite cells: finite outputs %.3e vs fp64, %.3e vs fp32" % (e64, e32))
    assert e64 < 1e-4 and e32 < 2e-4


@pytest.mark.gpu
@pytest.mark.parametrize("C,cin", [(32, (16, 32, 64, 128)), (128, P.DLA)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_stage_maps_return_the_bits_of_the_float_call(dtype, C, cin):
    ref = _reference(C, cin, 3, P.ODD4)
    fpn = _fpn(C, cin, ref["prm"])
    half = [v.to(dtype) for v in _dev(ref["x"])]
    with torch.no_grad():
        out_h = fpn(half)
        out_f = fpn([v.float() for v in half])
    assert _equal_bits(out_h, out_f) and float(out_h[0].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_outputs_are_the_float_call_rounded_once(dtype):
    C, cin = 128, P.DLA
    ref = _reference(C, cin, 3, P.ODD4)
    x = _dev(ref["x"])
    with torch.no_grad():
        full = _fpn(C, cin, ref["prm"])(x)
        half = _fpn(C, cin, ref["prm"], out_dtype=dtype)(x)
    assert all(h.dtype is dtype and h.is_contiguous() for h in half) and len(half) == 5
    assert _equal_bits(half, [f.to(dtype) for f in full])       # P[L] included


@pytest.mark.gpu
def test_images_are_independent_and_calls_repeat_without_a_sync():
    C, cin, N = 128, P.DLA, 3
    ref = _reference(C, cin, N, P.ODD4)
    fpn = _fpn(C, cin, ref["prm"])
    x = _dev(ref["x"])
    with torch.no_grad():
        out = fpn(x)
        again, syncs = H.count_syncs(lambda: fpn(x))
        assert _equal_bits(out, again)
        assert len(syncs) == 0, [str(s.message)[:80] for s in syncs]
        for i in range(N):
            assert _equal_bits(fpn([v[i:i + 1] for v in x]), [o[i:i + 1] for o in out]), "image %d" % i
        # the two coarsest stages alone: the coarse end of the pyramid does not depend on the finer levels
        two = _fpn(C, cin[2:], ref["prm"][2:])(x[2:])
    assert len(two) == 3
    for g, w in zip(two, out[2:]):
        assert torch.equal(torch.isfinite(g), torch.isfinite(w))
    ref2 = dict(o64=ref["o64"][2:], o32=ref["o32"][2:], scale=ref["scale"])
    e64, e32 = _errors(two, ref2)
    assert e64 < 1e-4 and e32 < 2e-4


def _raw_fwd(C, cin, sizes, N=1, stage_offset=0, out_offset=0):
    """``smot_fpn_fwd`` on valid buffers of these shapes (the stage / output pointers moved by so many bytes) -> its return
    code."""
    import siammot_amd.ops as ops
    lib = ops.load_library()
    L = len(cin)
    stages = [torch.zeros((N, c, h, w), device="cuda") for c, (h, w) in zip(cin, sizes)]
    out = [torch.zeros((N, C, h, w), device="cuda") for (h, w) in sizes]
    packed = torch.zeros(sum(C * c + 2 * C + 9 * C * C for c in cin), device="cuda")
    ws = torch.zeros(sum(N * C * h * w + 4 for (h, w) in sizes), device="cuda")
    arr = lambda vals: (ctypes.c_int * L)(*vals)
    ptrs = lambda ts, off=0: ctypes.cast((ctypes.c_void_p * L)(*[t.data_ptr() + off for t in ts]), ctypes.c_void_p)
    ic, ih, iw = arr(cin), arr([s[0] for s in sizes]), arr([s[1] for s in sizes])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert lib.smot_fpn_ws_bytes(L, cast(ih), cast(iw), N, C) <= ws.numel() * 4
    rc = lib.smot_fpn_fwd(ptrs(stages, stage_offset), 0, cast(ic), cast(ih), cast(iw), L, N, C, ctypes.c_void_p(packed.data_ptr()),
                          ctypes.c_void_p(ws.data_ptr()), ptrs(out, out_offset), 0, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, lib.smot_fpn_packed_floats(L, cast(ic), C), out


@pytest.mark.gpu
def test_shapes_beyond_the_capacities_take_the_torch_composition():
    import siammot_amd.ops as ops
    from siammot_amd.fpn import conv_with_kaiming_uniform
    for C, cin, kw in ((48, (16, 32), {}), (32, (24, 32), {}), (32, (16, 32), {"conv_block": conv_with_kaiming_uniform(True, True, 8)})):
        prm, x = P.params(C, cin), P.maps(cin, 2, P.TWO)
        if kw:                                                   # GroupNorm + ReLU blocks: the module against itself on the CPU
            torch.manual_seed(1)
            from siammot_amd.fpn import FPN, LastLevelMaxPool
            fpn = FPN(cin, C, top_blocks=LastLevelMaxPool(), **kw).eval()
            assert isinstance(fpn.fpn_inner1, torch.nn.Sequential)
            with torch.no_grad():
                want = [o.double() for o in fpn([torch.from_numpy(v) for v in x])]
            fpn = fpn.to("cuda")
        else:
            fpn = _fpn(C, cin, prm)
            want = P.oracle(x, prm, torch.float64)
        before = ops.FALLBACKS["fpn_torch"]
        with torch.no_grad():
            out = fpn(_dev(x))
        assert ops.FALLBACKS["fpn_torch"] == before + 1
        e = H.scaled_error(out, want, P.channel_scale(want))
        assert len(out) == 3 and e < 1e-4, e
        if not kw:
            rc, floats, raw_out = _raw_fwd(C, cin, P.TWO)
            assert rc == -2 and floats == -1                     # SMOT_ERR_UNSUPPORTED; nothing launched
            assert all(float(o.abs().max()) == 0.0 for o in raw_out)
            with pytest.raises(RuntimeError, match="C = 48|Cin = 24"):
                ops.fpn_pack([(torch.from_numpy(p[0]).cuda(), torch.from_numpy(p[1]).cuda()) for p in prm],
                             [(torch.from_numpy(p[2]).cuda(), torch.from_numpy(p[3]).cuda()) for p in prm])
    rc, floats, _ = _raw_fwd(32, (16, 32), P.TWO)               # the same call within the capacities runs
    assert rc == 0 and floats == sum(32 * c + 64 + 9 * 32 * 32 for c in (16, 32))
    for kw in ({"stage_offset": 2}, {"out_offset": 2}):         # fp32 maps at an odd half-word: SMOT_ERR_BAD_ARG, nothing launched
        rc, _, raw_out = _raw_fwd(32, (16, 32), P.TWO, **kw)
        assert rc == -1 and all(float(o.abs().max()) == 0.0 for o in raw_out), kw
    # a CPU call is the composition and is not counted; training mode is counted
    ref = _reference(64, (48, 16), 2, P.TWO)
    before = ops.FALLBACKS["fpn_torch"]
    with torch.no_grad():
        assert _equal_bits(_fpn(64, (48, 16), ref["prm"], "cpu")([torch.from_numpy(v) for v in ref["x"]]), ref["o32"])
        assert ops.FALLBACKS["fpn_torch"] == before
        _fpn(64, (48, 16), ref["prm"]).train()(_dev(ref["x"]))
        assert ops.FALLBACKS["fpn_torch"] == before + 1


@pytest.mark.gpu
def test_a_changed_parameter_is_packed_again():
    C, cin = 32, (16, 32, 64, 128)
    ref = _reference(C, cin, 1, P.ODD4)
    fpn = _fpn(C, cin, ref["prm"])
    x = _dev(ref["x"])
    with torch.no_grad():
        a = [o.clone() for o in fpn(x)]
        fpn.fpn_layer2.weight.mul_(2.0)
        b = fpn(x)
    assert not torch.equal(a[1], b[1])
    assert _equal_bits([a[0]] + a[2:], [b[0]] + list(b[2:]))   # P[1] alone reads fpn_layer2
    prm = [list(p) for p in ref["prm"]]
    prm[1][2] = prm[1][2] * 2.0
    o64 = P.oracle(ref["x"], prm, torch.float64)
    assert H.scaled_error(b, o64, P.channel_scale(o64)) < 1e-4


def _detector(N, dev="cuda"):
    """A seeded ``DetectionHead`` with the config's FPN and an RPN head at C = 128, and DLA stage maps of ``N`` images of
    84 x 52 (``ODD4``: the five FPN maps are rpn_head_cases.ODD)."""
    import rpn_proposal_cases as R
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.detector import build_detection_head
    C = 128
    cfg = _cfg(C)
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    torch.manual_seed(5)
    det = build_detection_head(cfg, BoxCoder(R.WEIGHTS), C, fpn=True).to(dev).eval()
    H.load_head(det.rpn_head, H.params(C, 3, seed=1), dev)
    P.load_fpn(det.fpn, P.params(C, P.DLA, seed=2), dev)
    with torch.no_grad():
        det.box_head.predictor.bbox_pred.weight.mul_(0.02)
        det.box_head.predictor.cls_score.weight.mul_(4.0)
    return det, _dev(P.maps(P.DLA, N, P.ODD4, seed=9), dev), (84, 52)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2])
def test_forward_stages_is_the_composition_with_one_host_copy(N):
    import siammot_amd.ops as ops
    det, stages, size = _detector(N)
    with torch.no_grad():
        feats = det.fpn(stages)
        want = det.forward_features(feats, size)                 # (also: workspaces, the packed weights, the anchors)
    assert [tuple(f.shape[2:]) for f in feats] == list(H.ODD)
    before = dict(ops.FALLBACKS)
    (got_feats, got), syncs = H.count_syncs(lambda: det.forward_stages(stages, size))
    assert dict(ops.FALLBACKS) == before
    assert len(syncs) == 1, "expected ONE device->host copy, saw %d: %s" % (len(syncs), [str(x.message)[:80] for x in syncs])
    assert _equal_bits(got_feats, feats)
    assert len(got) == len(want) == N
    for a, b in zip(got, want):
        assert a.fields() == b.fields() == ["scores", "ids", "labels"] and tuple(a.size) == tuple(size) and len(a) == len(b)
        assert torch.equal(a.bbox.view(torch.int32), b.bbox.view(torch.int32))
        assert torch.equal(a.get_field("scores").view(torch.int32), b.get_field("scores").view(torch.int32))
        assert torch.equal(a.get_field("labels"), b.get_field("labels"))
    print("forward_stages N=%d: detections %s" % (N, [len(a) for a in got]))
