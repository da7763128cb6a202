"""RPN head and anchors on the device (siammot_amd.rpn.RPNHead / AnchorGenerator / RPNModule, ops.rpn_head / rpn_anchors,
csrc/rpn_head.hip) and ``DetectionHead.forward_features``.

CPU: symbols, ``state_dict`` keys, the cell anchors' half-to-even rounding, the grid's order.
GPU: the kernel against torch's ``F.conv2d`` composition on the CPU (tests/rpn_head_cases.py) with the bound of the
project's other matrix-core convolutions (tests/test_hip_parity.py::test_predictor_vs_oracle: 1e-4 of the per-channel
scale against fp64, 2e-4 against fp32); borders, non-finite cells, half maps, independence of the images and levels of a
call, capacities, the anchors bit for bit, and the composition from FPN maps to detections with one host copy.
"""
import os
import re

import numpy as np
import pytest
import torch

import rpn_head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smot_rpn_head_pack", "smot_rpn_head_packed_floats", "smot_rpn_head_fwd", "smot_rpn_anchors_fwd")
HEAD_KEYS = ["conv.weight", "conv.bias", "cls_logits.weight", "cls_logits.bias", "bbox_pred.weight", "bbox_pred.bias"]
_cache = {}


def _cfg(channels=128):
    from siammot_amd.config import get_default_cfg
    return get_default_cfg(channels=channels)


def _reference(C, A, N):
    """(maps, parameters, fp64 outputs, fp32 outputs, per-channel scales) of one case on ``ODD``: computed once."""
    key = (C, A, N)
    if key not in _cache:
        prm, x = H.params(C, A), H.maps(C, N)
        o64, r64 = H.oracle(x, prm, torch.float64)
        o32, r32 = H.oracle(x, prm, torch.float32)
        _cache[key] = dict(prm=prm, x=x, o64=o64, r64=r64, o32=o32, r32=r32, so=H.channel_scale(o64), sr=H.channel_scale(r64))
    return _cache[key]


def _head(C, A, prm, dev="cuda"):
    from siammot_amd.rpn import RPNHead
    return H.load_head(RPNHead(None, C, A), prm, dev)


def _dev(levels, dev="cuda"):
    return [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in levels]


def _equal_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_carry_the_new_symbols():
    import siammot_amd.ops as ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smot_emm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smot_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared and name in ops.EXPORTED_SYMBOLS, name
    assert ops.ABI_VERSION == 14 and re.search(r"#define SMOT_ABI_VERSION 14\b", src)
    assert "rpn_head_torch" in dict(ops.FALLBACKS)               # registered from import


def test_modules_carry_upstreams_state_dict_keys_and_the_cpu_head_is_the_composition():
    import siammot_amd.ops as ops
    from siammot_amd.rpn import AnchorGenerator, RPNHead, RPNModule
    head = RPNHead(_cfg(), 32, 3).eval()
    assert list(head.state_dict().keys()) == HEAD_KEYS
    assert head.conv.weight.shape == (32, 32, 3, 3) and head.cls_logits.weight.shape == (3, 32, 1, 1)
    assert head.bbox_pred.weight.shape == (12, 32, 1, 1) and float(head.conv.bias.detach().abs().max()) == 0.0
    assert 0.005 < float(head.conv.weight.detach().std()) < 0.02
    gen = AnchorGenerator(H.SIZES, H.RATIOS, H.STRIDES)
    assert list(gen.state_dict().keys()) == ["cell_anchors.%d" % l for l in range(5)]
    mod = RPNModule(_cfg(), 128)
    assert sorted(mod.state_dict().keys()) == sorted(["anchor_generator.cell_anchors.%d" % l for l in range(5)]
                                                     + ["head." + k for k in HEAD_KEYS])
    assert hasattr(mod, "box_selector_test") and mod.head.num_anchors == 3
    prm = H.params(32, 3)
    H.load_head(head, prm, "cpu")
    x = [torch.from_numpy(v) for v in H.maps(32, 2)]
    before = ops.FALLBACKS["rpn_head_torch"]
    with torch.no_grad():
        obj, reg = head(x)
    o32, r32 = H.oracle(x, prm, torch.float32)
    assert _equal_bits(obj, o32) and _equal_bits(reg, r32)
    assert ops.FALLBACKS["rpn_head_torch"] == before          # counted for device tensors only
    with pytest.raises(NotImplementedError):
        mod.eval()([(64, 32)], x, targets=[None])
    with pytest.raises(NotImplementedError):
        mod.train()([(64, 32)], x)


def test_cell_anchors_round_half_to_even():
    from siammot_amd.rpn import AnchorGenerator, generate_anchors
    a = generate_anchors(16, (128,), (0.5, 1, 2))
    assert a.tolist() == [[-84, -40, 99, 55], [-56, -56, 71, 71], [-36, -80, 51, 95]]
    assert generate_anchors(32, (256,), (0.5,)).tolist() == [[-164, -72, 195, 103]]          # round(22.5) = 22
    gen = AnchorGenerator(H.SIZES, H.RATIOS, H.STRIDES)
    assert gen.num_anchors_per_location() == [3] * 5
    cells = list(gen.cell_anchors)
    assert all(c.dtype is torch.float32 and c.shape == (3, 4) for c in cells)
    assert cells[2].tolist() == a.tolist() and cells[3][0].tolist() == [-164, -72, 195, 103]
    cfg = _cfg()
    assert tuple(cfg.MODEL.RPN.ANCHOR_SIZES) == H.SIZES and tuple(cfg.MODEL.RPN.ANCHOR_STRIDE) == H.STRIDES
    assert tuple(cfg.MODEL.RPN.ASPECT_RATIOS) == H.RATIOS and cfg.MODEL.RPN.STRADDLE_THRESH == 0


def test_grid_anchors_on_the_cpu_are_the_broadcast_expression():
    from siammot_amd.rpn import AnchorGenerator
    gen = AnchorGenerator(H.SIZES, H.RATIOS, H.STRIDES)
    feats = [torch.zeros(2, 4, h, w) for (h, w) in H.ODD]
    per_image = gen([(84, 52), (84, 52)], feats)
    assert len(per_image) == 2 and all(len(p) == 5 for p in per_image)
    for l, ((h, w), s, cell) in enumerate(zip(H.ODD, H.STRIDES, gen.cell_anchors)):
        want = H.grid_expression(cell, s, h, w)
        got = per_image[0][l]
        assert got.mode == "xyxy" and tuple(got.size) == (84, 52) and got.fields() == []      # no visibility field
        assert got.bbox.shape == (h * w * 3, 4) and torch.equal(got.bbox.view(torch.int32), want.view(torch.int32))
        # the flattened order (y * W + x) * A + a, spelled out at one cell
        y, x, a = h - 1, w - 1, 2
        assert got.bbox[(y * w + x) * 3 + a].tolist() == (cell[a] + torch.tensor([x * s, y * s, x * s, y * s])).tolist()
        assert per_image[1][l].bbox is got.bbox


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("A", [1, 3, 4])
@pytest.mark.parametrize("C", [32, 96, 128, 256])
def test_head_against_the_cpu_oracle(C, A, N):
    """Measured maxima (scaled error against fp64 / fp32, objectness and regression together): see INTEGRATION.md §3k."""
    import siammot_amd.ops as ops
    ref = _reference(C, A, N)
    head = _head(C, A, ref["prm"])
    before = ops.FALLBACKS["rpn_head_torch"]
    with torch.no_grad():
        obj, reg = head(_dev(ref["x"]))
    assert ops.FALLBACKS["rpn_head_torch"] == before
    for l, (h, w) in enumerate(H.ODD):
        assert obj[l].shape == (N, A, h, w) and reg[l].shape == (N, 4 * A, h, w)
        assert obj[l].dtype is torch.float32 and obj[l].is_contiguous() and reg[l].is_contiguous()
    e64 = max(H.scaled_error(obj, ref["o64"], ref["so"]), H.scaled_error(reg, ref["r64"], ref["sr"]))
    e32 = max(H.scaled_error(obj, ref["o32"], ref["so"]), H.scaled_error(reg, ref["r32"], ref["sr"]))
    print("rpn_head C=%d A=%d N=%d: max scaled error %.3e vs fp64, %.3e vs fp32" % (C, A, N, e64, e32))
    assert e64 < 1e-4 and e32 < 2e-4


def _border_map(C, shift=0):
    (h, w), = H.ONE
    x = np.zeros((1, C, h, w), H.F32)
    cells = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2 - 1), (h // 2, 0), (h // 2 + 1, w - 1)]
    for k, (y, xx) in enumerate(cells):
        if 0 <= xx + shift < w:
            x[0, k % C, y, xx + shift] = 1.0 + (k % 3)
    return x


@pytest.mark.gpu
def test_borders_are_exact_with_integer_data():
    C, A = 32, 3
    prm = [np.ones((C, C, 3, 3), H.F32), np.zeros(C, H.F32), np.ones((A, C, 1, 1), H.F32), np.full(A, 2.0, H.F32),
           np.ones((4 * A, C, 1, 1), H.F32), np.full(4 * A, -3.0, H.F32)]
    head = _head(C, A, prm)
    out = {}
    for shift in (0, 1):
        x = _border_map(C, shift)
        o32, r32 = H.oracle([x], prm, torch.float32)
        with torch.no_grad():
            obj, reg = head(_dev([x]))
        assert float(o32[0].max()) >= 2 + 32 * 3 and float((o32[0] - o32[0].round()).abs().max()) == 0.0   # small integers
        assert torch.equal(obj[0].cpu(), o32[0]) and torch.equal(reg[0].cpu(), r32[0])
        out[shift] = (obj[0].cpu(), reg[0].cpu(), o32[0], r32[0])
    for k in (0, 1):                                             # the shift changes exactly the outputs the oracle changes
        changed, want = out[0][k] != out[1][k], out[0][k + 2] != out[1][k + 2]
        assert torch.equal(changed, want) and int(want.sum()) > 0 and not bool(want.all())


@pytest.mark.gpu
def test_non_finite_cells_reach_exactly_their_windows():
    C, A, N = 32, 3, 2
    ref = _reference(C, A, N)
    x = [v.copy() for v in ref["x"]]
    x[0][0, 3, 5, 7] = np.nan
    x[1][1, 10, 0, 0] = np.inf
    x[3][0, 31, 1, 2] = -np.inf
    o32, r32 = H.oracle(x, ref["prm"], torch.float32)
    o64, r64 = H.oracle(x, ref["prm"], torch.float64)
    with torch.no_grad():
        obj, reg = _head(C, A, ref["prm"])(_dev(x))
    bad = 0
    for got, want in zip(list(obj) + list(reg), list(o32) + list(r32)):
        got = got.cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(torch.isposinf(got), torch.isposinf(want)) and torch.equal(torch.isneginf(got), torch.isneginf(want))
        bad += int((~torch.isfinite(want)).sum())
    assert bad > 0 and int((~torch.isfinite(o32[0][0])).sum()) == A * 9 and bool(torch.isfinite(o32[0][1]).all())
    assert bool(torch.isfinite(o32[2]).all()) and bool(torch.isfinite(o32[4]).all())
    e64 = max(H.scaled_error(obj, o64, ref["so"]), H.scaled_error(reg, r64, ref["sr"]))
    e32 = max(H.scaled_error(obj, o32, ref["so"]), H.scaled_error(reg, r32, ref["sr"]))
    print("rpn_head with non-finite cells: finite outputs %.3e vs fp64, %.3e vs fp32" % (e64, e32))
    assert e64 < 1e-4 and e32 < 2e-4


@pytest.mark.gpu
@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_maps_return_the_bits_of_the_float_call(dtype, C):
    ref = _reference(C, 3, 2)
    head = _head(C, 3, ref["prm"])
    half = [v.to(dtype) for v in _dev(ref["x"])]
    with torch.no_grad():
        obj_h, reg_h = head(half)
        obj_f, reg_f = head([v.float() for v in half])
    assert _equal_bits(obj_h, obj_f) and _equal_bits(reg_h, reg_f)
    assert float(obj_h[0].abs().max()) > 0


@pytest.mark.gpu
def test_images_and_levels_of_a_call_are_independent_and_calls_repeat():
    C, A, N = 128, 3, 3
    ref = _reference(C, A, N)
    head = _head(C, A, ref["prm"])
    x = _dev(ref["x"])
    with torch.no_grad():
        obj, reg = head(x)
        obj2, reg2 = head(x)
        assert _equal_bits(obj, obj2) and _equal_bits(reg, reg2)
        for i in range(N):
            oi, ri = head([v[i:i + 1] for v in x])
            assert _equal_bits(oi, [o[i:i + 1] for o in obj]) and _equal_bits(ri, [r[i:i + 1] for r in reg])
        for l in range(len(x)):
            ol, rl = head([x[l]])
            assert _equal_bits(ol, [obj[l]]) and _equal_bits(rl, [reg[l]])


@pytest.mark.gpu
def test_shapes_beyond_the_capacities_take_the_torch_composition():
    import siammot_amd.ops as ops
    for C, A in ((48, 3), (32, 13)):                            # C % 32 != 0; 5 A = 65 rows
        prm, x = H.params(C, A), H.maps(C, 2)
        head = _head(C, A, prm)
        before = ops.FALLBACKS["rpn_head_torch"]
        with torch.no_grad():
            obj, reg = head(_dev(x))
        assert ops.FALLBACKS["rpn_head_torch"] == before + 1
        o64, r64 = H.oracle(x, prm, torch.float64)
        e = max(H.scaled_error(obj, o64, H.channel_scale(o64)), H.scaled_error(reg, r64, H.channel_scale(r64)))
        assert e < 1e-4, e
        with pytest.raises(RuntimeError, match="C = 48|A = 13"):
            ops.rpn_head_pack(*[p.detach() for p in head._params()])
        with pytest.raises(RuntimeError, match="C = 48|A = 13"):
            ops.rpn_head(_dev(x), torch.zeros(1 << 16, device="cuda"), C, A)
    # training mode: the composition, counted
    ref = _reference(32, 3, 2)
    head = _head(32, 3, ref["prm"])
    with torch.no_grad():
        want = head(_dev(ref["x"]))
        before = ops.FALLBACKS["rpn_head_torch"]
        head.train()(_dev(ref["x"]))
        assert ops.FALLBACKS["rpn_head_torch"] == before + 1
        # a channels-last map is copied: the NCHW result bit for bit, on the kernel
        cl = [v.contiguous(memory_format=torch.channels_last) for v in _dev(ref["x"])]
        assert not cl[0].is_contiguous()
        got = head.eval()(cl)
        assert ops.FALLBACKS["rpn_head_torch"] == before + 1
    assert _equal_bits(got[0], want[0]) and _equal_bits(got[1], want[1])


@pytest.mark.gpu
def test_a_changed_parameter_is_packed_again():
    ref = _reference(32, 3, 1)
    head = _head(32, 3, ref["prm"])
    x = _dev(ref["x"])
    with torch.no_grad():
        a = head(x)[0][0].clone()
        head.cls_logits.bias.add_(1.0)
        b = head(x)[0][0]
    assert float((b - a - 1.0).abs().max()) < 1e-5


@pytest.mark.gpu
def test_anchors_on_the_device_are_the_expression_and_are_cached():
    from siammot_amd.rpn import AnchorGenerator
    gen = AnchorGenerator(H.SIZES, H.RATIOS, H.STRIDES).to("cuda")
    feats = [torch.zeros(3, 4, h, w, device="cuda") for (h, w) in H.ODD]
    per_image = gen([(84, 52)] * 3, feats)
    cells = [c.cpu() for c in gen.cell_anchors]
    for l, ((h, w), s) in enumerate(zip(H.ODD, H.STRIDES)):
        want = H.grid_expression(cells[l], s, h, w)
        got = per_image[0][l].bbox
        assert got.is_cuda and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
        assert per_image[1][l].bbox.data_ptr() == got.data_ptr() == per_image[2][l].bbox.data_ptr()    # one tensor per level
    again = gen([(84, 52)] * 3, feats)
    assert all(again[0][l].bbox.data_ptr() == per_image[0][l].bbox.data_ptr() for l in range(5))
    other = gen([(84, 52)], [torch.zeros(1, 4, h + 1, w, device="cuda") for (h, w) in H.ODD])
    assert all(other[0][l].bbox.data_ptr() != per_image[0][l].bbox.data_ptr() for l in range(5))
    assert other[0][0].bbox.shape == (14 * 21 * 3, 4)
    assert torch.equal(other[0][4].bbox.cpu(), H.grid_expression(cells[4], 64, 2, 2))


def _detector(N, dev="cuda"):
    """A seeded ``DetectionHead`` with an RPN head at C = 128 and FPN maps of ``N`` images of 320 x 192."""
    import rpn_proposal_cases as R
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.detector import build_detection_head
    C = 128
    cfg = _cfg(C)
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    torch.manual_seed(5)
    det = build_detection_head(cfg, BoxCoder(R.WEIGHTS), C).to(dev).eval()
    H.load_head(det.rpn_head, H.params(C, 3, seed=1), dev)
    with torch.no_grad():
        det.box_head.predictor.bbox_pred.weight.mul_(0.02)
        det.box_head.predictor.cls_score.weight.mul_(4.0)
    rs = np.random.RandomState(77 + N)
    feats = [torch.from_numpy(rs.standard_normal((N, C, h, w)).astype(H.F32)).to(dev) for (h, w) in R.LEVELS]
    return det, feats, R.IMAGE_WH


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2])
def test_forward_features_is_the_composition_with_one_host_copy(N):
    import siammot_amd.ops as ops
    det, feats, size = _detector(N)
    with torch.no_grad():
        objectness, regression = det.rpn_head(feats)
        anchors = det.anchor_generator([size] * N, feats)
        want = det(anchors, objectness, regression, feats)
        proposals = det.rpn_post(anchors, objectness, regression)
    assert all(len(p) > 20 for p in proposals), [len(p) for p in proposals]      # the box head has something to work on
    det.forward_features(feats, size)                           # (workspaces, the packed weights, the anchors)
    before = dict(ops.FALLBACKS)
    got, syncs = H.count_syncs(lambda: det.forward_features(feats, size))
    assert dict(ops.FALLBACKS) == before
    assert len(syncs) == 1, "expected ONE device->host copy, saw %d: %s" % (len(syncs), [str(x.message)[:80] for x in syncs])
    assert len(got) == len(want) == N
    for a, b in zip(got, want):
        assert a.fields() == b.fields() == ["scores", "ids", "labels"] and tuple(a.size) == tuple(size) and len(a) == len(b)
        assert torch.equal(a.bbox.view(torch.int32), b.bbox.view(torch.int32))
        assert torch.equal(a.get_field("scores").view(torch.int32), b.get_field("scores").view(torch.int32))
        assert torch.equal(a.get_field("labels"), b.get_field("labels"))
    print("forward_features N=%d: proposals %s, detections %s" % (N, [len(p) for p in proposals], [len(a) for a in got]))


@pytest.mark.gpu
def test_rpn_module_is_its_three_parts_composed():
    import rpn_proposal_cases as R
    from siammot_amd.rpn import RPNModule
    C, N = 128, 2
    cfg = _cfg(C)
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    mod = RPNModule(cfg, C)
    H.load_head(mod.head, H.params(C, 3, seed=2), "cuda")
    mod = mod.to("cuda").eval()
    rs = np.random.RandomState(5)
    feats = [torch.from_numpy(rs.standard_normal((N, C, h, w)).astype(H.F32)).cuda() for (h, w) in R.LEVELS]
    got = mod([R.IMAGE_WH] * N, feats)
    with torch.no_grad():
        objectness, regression = mod.head(feats)
        want = mod.box_selector_test(mod.anchor_generator([R.IMAGE_WH] * N, feats), objectness, regression)
    assert len(got) == len(want) == N
    for a, b in zip(got, want):
        assert len(a) == len(b) > 20 and a.fields() == ["objectness"] and tuple(a.size) == R.IMAGE_WH
        assert torch.equal(a.bbox.view(torch.int32), b.bbox.view(torch.int32))
        assert torch.equal(a.get_field("objectness").view(torch.int32), b.get_field("objectness").view(torch.int32))
