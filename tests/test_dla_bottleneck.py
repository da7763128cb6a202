"""Bottleneck DLA bodies and trees of any depth on the device (siammot_amd.dla: DlaBottleneck, residual roots, dla_46_c / dla_60
/ dla_102 / dla_169; ops.dla_net / dla_net_pack / dla_net_ws_bytes / dla_net_num_convs / dla_conv1x1_res; csrc/dla.hip;
INTEGRATION.md §3o).

CPU: symbols, ``state_dict`` keys and shapes, launch counts, the module on CPU tensors against the golden vectors of the
reference's own dla.py with ``block=DlaBottleneck`` (tests/golden/dla_bottleneck_stages.npz,
tools/gen_golden_dla_bottleneck.py), the unused outer ``project``, the config's bodies, capacities, the workspace discipline.
GPU, operator level: the 1x1 kernel with up to eight sources and a residual against torch's CPU operators
(tests/dla_bottleneck_cases.py) with the bounds of tests/test_dla.py (1e-4 of the per-channel scale against fp64, 2e-4 against
fp32); images of a call, half outputs, the bits of ``ops.dla_conv1x1``, exactness with integer data, non-finite residual
cells, refused calls.
GPU, network level: the HIP path against the golden vectors within 4 x the reference's own fp32 error per stage; split
operands; images of a call, half images and half outputs; basic blocks through the new entry point; DLA-60 and DLA-169;
fallbacks; frames to detections with one host copy.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dla_bottleneck_cases as B
import dla_cases as D
import rpn_head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smot_dla_net_num_convs", "smot_dla_net_packed_floats", "smot_dla_net_pack", "smot_dla_net_ws_bytes",
               "smot_dla_net_fwd", "smot_dla_conv1x1_res_fwd")
BODY_CONVS = {"dla_34": 37, "dla_46_c": 48, "dla_60": 63, "dla_102": 105, "dla_169": 168}
BODY_KEYS = {"dla_46_c": 245, "dla_60": 330, "dla_102": 550, "dla_169": 875}
_cache = {}


def _net(case, dev="cpu", **kw):
    """The case's network with the recipe's parameters on ``dev``, and its image."""
    from siammot_amd.dla import DLA
    levels, channels, shape, residual_root = B.NET_CASES[case]
    model = DLA(levels, channels, block="bottleneck", residual_root=residual_root, **kw)
    if ("prm", case) not in _cache:
        _cache[("prm", case)] = D.params(model, B.SEED)
    return D.load(model, _cache[("prm", case)], dev), torch.from_numpy(D.image(shape, B.SEED))


def _cpu_fp32(case):
    """The CPU module's fp32 stage maps of the case: computed once, shared and left unchanged."""
    if ("cpu", case) not in _cache:
        model, x = _net(case)
        with torch.no_grad():
            _cache[("cpu", case)] = [o.clone() for o in model(x)]
    return _cache[("cpu", case)]


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _equal_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_carry_the_new_symbols():
    import siammot_amd.ops as ops
    text = open(os.path.join(ROOT, "include", "smot_emm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(smot_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared and name in ops.EXPORTED_SYMBOLS, name
    assert ops.ABI_VERSION == 14 and re.search(r"#define SMOT_ABI_VERSION 14\b", src)
    assert re.search(r"#define SMOT_DLA_BLOCK_BASIC 0\b", src) and re.search(r"#define SMOT_DLA_BLOCK_BOTTLENECK 1\b", src)
    assert ops.DLA_BLOCKS == {"basic": 0, "bottleneck": 1}


def test_state_dicts_and_launch_counts_are_upstreams():
    import siammot_amd.dla as M
    import siammot_amd.ops as ops
    for name, keys in BODY_KEYS.items():
        model = getattr(M, name)()
        sd = model.state_dict()
        names = list(sd.keys())
        assert len(names) == keys, (name, len(names))
        assert names[:5] == ["base_layer.0.weight", "base_layer.1.weight", "base_layer.1.bias", "base_layer.1.running_mean",
                             "base_layer.1.running_var"]
        assert names[-1] == "level5.project.1.running_var"
        assert len(model.convs()) == BODY_CONVS[name] == ops.dla_net_num_convs(model.levels, model.channels, model.block), name
    model = M.dla_34()
    assert len(model.convs()) == 37 == ops.dla_net_num_convs(model.levels, model.channels)
    sd = M.dla_169().state_dict()
    assert list(sd.keys())[15] == "level2.tree1.tree1.conv1.weight"
    assert sd["level4.tree2.tree2.tree2.tree2.root.conv.weight"].shape == (512, 3328, 1, 1)
    assert sd["level2.tree1.tree1.conv2.weight"].shape == (64, 64, 3, 3)
    sd = M.dla_60().state_dict()
    assert list(sd.keys())[15] == "level2.tree1.conv1.weight" and sd["level2.tree1.conv1.weight"].shape == (64, 32, 1, 1)
    assert sd["level2.tree1.conv3.weight"].shape == (128, 64, 1, 1) and sd["level4.tree2.tree2.root.conv.weight"].shape == (512, 2304, 1, 1)
    # upstream registers conv1, bn1, conv2, bn2, conv3, bn3 in a block and tree1, tree2, root, project in a tree
    level2 = [k for k in sd if k.startswith("level2.")]
    assert [".".join(k.split(".")[1:3]) for k in level2[::5]] == ["tree1.conv1", "tree1.conv2", "tree1.conv3", "tree2.conv1", "tree2.conv2",
                                                                  "tree2.conv3", "root.conv", "project.0"]
    for case, keys in B.NET_KEYS.items():
        model, _ = _net(case)
        assert len(model.state_dict()) == keys, case
    with pytest.raises(TypeError):                               # the new arguments are keyword-only
        M.DLA(D.DLA34[0], D.DLA34[1], torch.float32, "fp32", "bottleneck")


@pytest.mark.parametrize("case", ["D", "E", "F"])
def test_cpu_module_against_the_reference_golden(case):
    """The same operators in the same order as the reference, only the threading differs: 2 x its own fp32 error."""
    import siammot_amd.ops as ops
    g = B.golden(case)
    model, x = _net(case)
    assert g["seed"] == B.SEED and g["shape"] == tuple(x.shape[2:])
    before = ops.FALLBACKS["dla_torch"]
    out = _cpu_fp32(case)
    assert ops.FALLBACKS["dla_torch"] == before                  # counted for device tensors only
    assert [tuple(o.shape) for o in out] == [w.shape for w in g["o64"]]
    err = D.stage_error(out, g["o64"])
    print("dla case %s on the CPU: error / e32 per stage %s" % (case, ["%.2f" % (e / b) for e, b in zip(err, g["e32"])]))
    for k, (e, b) in enumerate(zip(err, g["e32"])):
        assert e <= 2 * b, "stage %d: %.3e against e32 %.3e" % (k + 2, e, b)
    half, _ = _net(case, out_dtype=torch.float16)
    with torch.no_grad():
        assert _equal_bits(half(x), [o.to(torch.float16) for o in out])


def test_the_outer_projects_are_owned_and_unused():
    model, x = _net("D")
    a = _cpu_fp32("D")
    with torch.no_grad():
        model.level4.project[0].weight.mul_(2.0)                 # depth 3: the outer two are not evaluated
        model.level4.tree1.project[0].weight.mul_(2.0)
        assert _equal_bits(a, model(x))
        model.level4.tree1.tree1.project[0].weight.mul_(2.0)     # the depth-1 tree's is
        c = model(x)
    assert _equal_bits(a[:2], c[:2]) and not torch.equal(a[2], c[2])


def test_build_dla_and_build_backbone_take_the_new_bodies():
    import siammot_amd.dla as M
    from siammot_amd.backbone import build_backbone, strip_prefix
    from siammot_amd.config import get_default_cfg
    cfg = get_default_cfg("DLA-169-FPN")
    d = cfg.MODEL.DLA
    assert (d.DLA_STAGE2_OUT_CHANNELS, d.DLA_STAGE3_OUT_CHANNELS, d.DLA_STAGE4_OUT_CHANNELS, d.DLA_STAGE5_OUT_CHANNELS) == (128, 256, 512, 1024)
    d = get_default_cfg().MODEL.DLA
    assert (d.DLA_STAGE2_OUT_CHANNELS, d.DLA_STAGE5_OUT_CHANNELS) == (64, 512)
    want = {"DLA-46-C-FPN": M.dla_46_c, "DLA-60-FPN": M.dla_60, "DLA-102-FPN": M.dla_102, "DLA-169-FPN": M.dla_169}
    for name, factory in want.items():
        ref = factory()
        body = M.build_dla(get_default_cfg(name))
        assert type(body) is M.DLA and (body.levels, body.channels, body.block, body.residual_root) == \
            (ref.levels, ref.channels, "bottleneck", name in ("DLA-102-FPN", "DLA-169-FPN")), name
        assert M.BODIES[name] is factory
    bb = build_backbone(get_default_cfg("DLA-46-C-FPN"))
    assert bb.fpn.in_channels == (64, 64, 128, 256) and bb.out_channels == 128
    ckpt = {"backbone." + k: torch.full_like(v, 0.25) for k, v in bb.state_dict().items()}
    ckpt["rpn.head.conv.weight"] = torch.zeros(1)
    assert len(ckpt) == 245 + 16 + 1
    bb.load_state_dict(strip_prefix(ckpt), strict=True)
    assert float(bb.body.level4.tree1.tree2.bn3.running_var[3]) == 0.25
    assert build_backbone(get_default_cfg("DLA-169-FPN")).fpn.in_channels == (128, 256, 512, 1024)
    for name in ("DLA-46-XC-FPN", "DLA-60-RES2NET-FPN"):
        cfg = get_default_cfg(name)
        with pytest.raises(ValueError, match=name):
            M.build_dla(cfg)
    cfg = get_default_cfg("DLA-60-FPN")
    cfg.MODEL.DLA.STAGE_WITH_DCN = (False, False, False, False, True, False)
    with pytest.raises(ValueError, match="STAGE_WITH_DCN"):
        build_backbone(cfg)
    cfg = get_default_cfg("DLA-60-FPN")
    cfg.MODEL.BACKBONE.CONV_BODY = "DLA-46-C-FPN"                # another body's widths
    with pytest.raises(ValueError, match="DLA-46-C-FPN"):
        M.build_dla(cfg)


def test_capacities():
    import siammot_amd.ops as ops
    ch = (16, 32, 64, 64, 128, 128)
    assert ops.dla_shapes_ok((1, 1, 1, 2, 5, 1), ch, block="bottleneck") and ops.dla_shapes_ok((1, 1, 1, 2, 5, 1), ch, 64, 96, 3, "bottleneck")
    assert not ops.dla_shapes_ok((1, 1, 1, 2, 6, 1), ch, block="bottleneck")
    assert not ops.dla_shapes_ok((1, 1, 1, 2, 3, 1), (16, 32, 64, 96, 128, 128), block="bottleneck")
    assert ops.dla_shapes_ok((1, 1, 1, 2, 3, 1), (16, 32, 64, 96, 128, 128))          # basic: multiples of 32
    assert not ops.dla_shapes_ok((1, 1, 1, 2, 3, 1), ch, block="res2net")
    assert ops.dla_net_num_convs((1, 1, 1, 2, 6, 1), ch, "bottleneck") == -1
    assert ops.dla_net_num_convs((1, 1, 1, 2, 3, 1), (16, 32, 64, 96, 128, 128), "bottleneck") == -1
    assert ops.dla_net_ws_bytes((1, 1, 1, 2, 3, 1), (16, 32, 64, 96, 128, 128), 1, 64, 64, "bottleneck") == -1
    assert ops.dla_net_ws_bytes((1, 1, 1, 2, 3, 1), ch, 1, 40, 72, "bottleneck") == -1
    lib = ops.load_library()
    arr = lambda v: ctypes.cast((ctypes.c_int * 6)(*v), ctypes.c_void_p)
    assert lib.smot_dla_net_num_convs(arr((1, 1, 1, 2, 3, 1)), arr(ch), 2) == -1      # no such block
    # basic blocks at depth <= 2: the packed image and the workspace question have smot_dla_*'s answers
    for levels, channels, _ in (D.NET_CASES["A"], D.NET_CASES["C"]):
        assert lib.smot_dla_net_packed_floats(arr(levels), arr(channels), 0, 0, 0) == lib.smot_dla_packed_floats(arr(levels), arr(channels))
        assert lib.smot_dla_net_packed_floats(arr(levels), arr(channels), 0, 0, 1) == lib.smot_dla_split_packed_floats(arr(levels), arr(channels))


def test_workspace_does_not_grow_with_the_number_of_blocks():
    """Bottleneck, channels (16, 32, 64, 64, 1024, 64), one 64 x 64 image: level4 at depth 5 (32 blocks) against depth 4 (16).

    The walker releases a block's two ``mid`` maps when the block returns and a subtree's maps when its root is written, so a
    depth-n tree holds, at its deepest point, the n - 1 ``tree1`` results of the trees it is inside plus one depth-1 tree's
    maps and one block's intermediates.  One more level of depth is therefore ONE more level-4 output map (1024 x 4 x 4
    floats); a walker that kept every block's temporaries until the level ends would add the maps of 16 more blocks (32)."""
    import siammot_amd.ops as ops
    channels, one_map = (16, 32, 64, 64, 1024, 64), 4 * 1024 * 4 * 4
    ws = [ops.dla_net_ws_bytes((1, 1, 1, 1, depth, 1), channels, 1, 64, 64, "bottleneck") for depth in (1, 2, 3, 4, 5)]
    assert all(w > 0 for w in ws)
    print("ws bytes at level4 depth 1 .. 5: %s (one level-4 map: %d)" % (ws, one_map))
    assert ws[4] - ws[3] == one_map and ws[3] - ws[2] == one_map
    assert ws[4] - ws[3] <= 8 * one_map
    # and it does not depend on residual_root; four images take four times the bytes
    assert ops.dla_net_ws_bytes((1, 1, 1, 1, 5, 1), channels, 1, 64, 64, "bottleneck", True) == ws[4]
    assert ops.dla_net_ws_bytes((1, 1, 1, 1, 5, 1), channels, 4, 64, 64, "bottleneck") == 4 * ws[4]


# ---- GPU, operator level ------------------------------------------------------------------------------------------------
P = (27, 43)                                                     # a pooled map for outputs of 13 x 21
CONV1R = [
    ([(32, False)], 64, (13, 21), True, "plain"),
    ([(32, False)], 64, (13, 21), True, "pooled"),
    ([(32, False), (16, False), (48, P), (96, False), (64, False)], 32, (13, 21), True, "source0"),
    ([(96, False), (16, False), (48, False), (32, P), (64, False), (96, False), (80, False)], 96, (13, 21), False, "source0"),
    ([(32, False), (96, False), (16, P), (48, False), (64, False), (32, False), (80, False), (16, False)], 32, (13, 21), False, "source0"),
    ([(96, False), (64, False), (32, False), (96, P), (16, False), (48, False), (32, False), (64, False)], 96, (13, 21), True, "source0"),
    ([(64, False), (64, False), (192, (2, 10)), (64, False), (64, False)], 64, (1, 5), True, "source0"),
]


def _res_call(ops, c, src, relu, **kw):
    res = None if c["residual"] is None else (src[0] if c["residual"] is c["src"][0] else _cuda(c["residual"]))
    return ops.dla_conv1x1_res(src, c["pooled"], _cuda(c["w"]), _cuda(c["scale"]), _cuda(c["shift"]), relu, residual=res,
                               residual_pooled=c["residual_pooled"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("sources,Cout,size,relu,residual", CONV1R)
def test_conv1x1_res_against_the_cpu_oracle(sources, Cout, size, relu, residual):
    import siammot_amd.ops as ops
    for N in (1, 3):
        c = B.conv1x1_res_case(sources, Cout, size, N, residual)
        o64, o32 = B.conv1x1_res_oracle(c, torch.float64, relu), B.conv1x1_res_oracle(c, torch.float32, relu)
        ch = D.channel_scale(B.conv1x1_res_oracle(c, torch.float64, pre=True))
        src = [_cuda(s) for s in c["src"]]
        out = _res_call(ops, c, src, relu)
        assert out.shape == o32.shape and out.dtype is torch.float32
        e64, e32 = D.scaled_error(out, o64, ch), D.scaled_error(out, o32, ch)
        print("dla_conv1x1_res %d sources -> %d %s N=%d %s: %.3e vs fp64, %.3e vs fp32" % (len(sources), Cout, size, N, residual, e64, e32))
        assert e64 < 1e-4 and e32 < 2e-4
        if N == 3:
            for i in range(N):
                ci = dict(c, src=[s[i:i + 1] for s in c["src"]])
                ci["residual"] = ci["src"][0] if residual == "source0" else c["residual"][i:i + 1]
                assert torch.equal(_bits(_res_call(ops, ci, [s[i:i + 1] for s in src], relu)), _bits(out[i:i + 1])), "image %d" % i
            for dtype in (torch.bfloat16, torch.float16):
                half = _res_call(ops, c, src, relu, out_dtype=dtype)
                assert half.dtype is dtype and torch.equal(_bits(half), _bits(out.to(dtype)))


@pytest.mark.gpu
def test_conv1x1_res_without_a_residual_has_the_bits_of_conv1x1():
    import siammot_amd.ops as ops
    for sources, Cout, relu in (([(32, False), (32, False)], 32, True), ([(96, False), (96, False), (64, P), (96, False)], 96, False),
                                ([(32, (26, 42))], 64, True)):
        c = D.conv1x1_case(sources, Cout, (13, 21), 2)
        src = [_cuda(s) for s in c["src"]]
        args = (c["pooled"], _cuda(c["w"]), _cuda(c["scale"]), _cuda(c["shift"]), relu)
        for dtype in (torch.float32, torch.bfloat16):
            a, b = ops.dla_conv1x1(src, *args, out_dtype=dtype), ops.dla_conv1x1_res(src, *args, out_dtype=dtype)
            assert float(a.float().abs().max()) > 0 and torch.equal(_bits(a), _bits(b))


def _ints(rs, shape, lo=-1, hi=1):
    return rs.randint(lo, hi + 1, size=shape).astype(D.F32)


@pytest.mark.gpu
def test_conv1x1_res_is_exact_with_integer_data():
    """Sources, filters and the residual in {-1, 0, 1} (the pooled ones a max of four integers), scale in {0.5, 1, 2}, shift an
    integer in -2 .. 2: an output sums at most 432 terms of size <= 1, every partial sum an integer below 2^22, exact in fp32
    in any order; times a power of two, plus an integer, plus a residual of size <= 1: a multiple of 1/2 below 2^11.  So the
    output equals the fp32 yardstick bit for bit (and the fp32 and fp64 yardsticks agree): this pins the concatenation order
    over seven sources, the pool's window on a source and on the residual, and the residual's place in front of the ReLU."""
    import siammot_amd.ops as ops
    rs = np.random.RandomState(29)
    sources = [(96, False), (16, False), (48, False), (32, P), (64, False), (96, False), (80, False)]
    for residual, relu in (("source0", True), ("pooled", True), ("plain", False)):
        c = dict(src=[_ints(rs, (2, ch) + (p if p else (13, 21))) for ch, p in sources], pooled=[bool(p) for _, p in sources],
                 w=_ints(rs, (96, 432, 1, 1)), scale=np.asarray([0.5, 1.0, 2.0], dtype=D.F32)[rs.randint(0, 3, size=96)],
                 shift=_ints(rs, 96, -2, 2), residual_pooled=residual == "pooled")
        c["residual"] = c["src"][0] if residual == "source0" else _ints(rs, (2, 96) + (P if residual == "pooled" else (13, 21)))
        o32, o64 = B.conv1x1_res_oracle(c, torch.float32, relu), B.conv1x1_res_oracle(c, torch.float64, relu)
        assert torch.equal(o32.double(), o64) and float(o32.max()) > 30
        assert not torch.equal(o32, D.conv1x1_oracle(c, torch.float32, relu))       # (the residual matters)
        out = _res_call(ops, c, [_cuda(s) for s in c["src"]], relu)
        assert torch.equal(out.cpu(), o32), "%s: %d cells differ" % (residual, int((out.cpu() != o32).sum()))


@pytest.mark.gpu
def test_a_non_finite_residual_cell_reaches_its_own_output_cell():
    import siammot_amd.ops as ops
    sources = [(32, False), (16, False), (48, P), (96, False), (64, False)]
    for residual in ("plain", "pooled"):
        c0 = B.conv1x1_res_case(sources, 32, (13, 21), 2, residual)
        c = dict(c0, residual=c0["residual"].copy())
        if residual == "plain":
            c["residual"][0, 3, 5, 9] = np.nan
            c["residual"][1, 30, 12, 20] = np.inf
            cells = [(0, 3, 5, 9), (1, 30, 12, 20)]
        else:
            c["residual"][0, 3, 11, 19] = np.nan                 # window of output (5, 9)
            c["residual"][1, 30, 24, 41] = np.inf                # window of output (12, 20)
            c["residual"][1, 7, 26, 42] = np.nan                 # the odd map's last row and column: read by no window
            c["residual"][0, 8, 0, 1] = -np.inf                  # -inf loses the max: nothing happens
            cells = [(0, 3, 5, 9), (1, 30, 12, 20)]
        want = torch.zeros((2, 32, 13, 21), dtype=torch.bool)
        for cell in cells:
            want[cell] = True
        for relu in (True, False):
            o32, o64 = B.conv1x1_res_oracle(c, torch.float32, relu), B.conv1x1_res_oracle(c, torch.float64, relu)
            out = _res_call(ops, c, [_cuda(s) for s in c["src"]], relu).cpu()
            assert torch.equal(~torch.isfinite(out), want), residual
            assert torch.equal(torch.isnan(out), torch.isnan(o32)) and float(out[cells[1]]) == np.inf
            ch = D.channel_scale(B.conv1x1_res_oracle(c0, torch.float64, pre=True))
            assert D.scaled_error(out, o64, ch) < 1e-4 and D.scaled_error(out, o32, ch) < 2e-4


def _raw_conv1x1_res(channels, residual_hw, H=4, W=4, Cout=32):
    """``smot_dla_conv1x1_res_fwd`` on valid buffers: sources of these channel counts at H x W, a residual read through the
    pool of a ``residual_hw`` map (None: no residual), a pre-zeroed output -> (code, output)."""
    import siammot_amd.ops as ops
    lib = ops.load_library()
    S = len(channels)
    src = [torch.ones((1, max(c, 1), H, W), device="cuda") for c in channels]
    K = sum(channels)
    w, scale, shift = torch.ones((Cout, K), device="cuda"), torch.ones(Cout, device="cuda"), torch.ones(Cout, device="cuda")
    res = torch.ones((1, Cout) + tuple(residual_hw), device="cuda") if residual_hw else None
    packed, out = torch.zeros(Cout * K + 2 * Cout + 4, device="cuda"), torch.zeros((1, Cout, H, W), device="cuda")
    arr = lambda vals: ctypes.cast((ctypes.c_int * S)(*vals), ctypes.c_void_p)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    sp = ctypes.cast((ctypes.c_void_p * S)(*[t.data_ptr() for t in src]), ctypes.c_void_p)
    rh, rw = residual_hw if residual_hw else (0, 0)
    rc = lib.smot_dla_conv1x1_res_fwd(sp, arr(channels), arr([0] * S), arr([H] * S), arr([W] * S), S, 1, H, W, vp(w), vp(scale), vp(shift),
                                      Cout, 1, vp(res), rh, rw, vp(packed), vp(out), 0,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.gpu
def test_refused_conv1x1_res_calls_launch_nothing():
    import siammot_amd.ops as ops
    for channels, residual_hw, code in (([16] * 9, None, -1),    # nine sources: SMOT_ERR_BAD_ARG
                                        ([32, 24], None, -2),     # a source of 24 channels: SMOT_ERR_UNSUPPORTED
                                        ([32], (6, 8), -1),       # a pooled residual of 6 x 8 for a 4 x 4 output: SMOT_ERR_BAD_ARG
                                        ([32], (8, 12), -1)):
        rc, out = _raw_conv1x1_res(channels, residual_hw)
        assert rc == code and float(out.abs().max()) == 0.0, (channels, residual_hw, rc)
    rc, out = _raw_conv1x1_res([16] * 8, (9, 9))                  # the same call within the capacities runs: 128 + 1 + 1
    assert rc == 0 and float(out.min()) == float(out.max()) == 130.0
    x = torch.zeros((1, 32, 4, 4), device="cuda")
    with pytest.raises(RuntimeError, match="residual has shape"):   # a plain residual of another size: refused by the binding
        ops.dla_conv1x1_res([x], [False], torch.zeros((32, 32, 1, 1), device="cuda"), x[0, :, 0, 0], x[0, :, 0, 0], True,
                            residual=torch.zeros((1, 32, 4, 5), device="cuda"))
    with pytest.raises(RuntimeError, match="code -1"):
        ops.dla_conv1x1_res([x[:, :16]] * 9, [False] * 9, torch.zeros((32, 144, 1, 1), device="cuda"), x[0, :, 0, 0], x[0, :, 0, 0], True)


# ---- GPU, network level -------------------------------------------------------------------------------------------------
def _against_the_golden(case, **kw):
    import siammot_amd.ops as ops
    g = B.golden(case)
    model, x = _net(case, "cuda", **kw)
    before = ops.FALLBACKS["dla_torch"]
    with torch.no_grad():
        out = model(x.cuda())
    assert ops.FALLBACKS["dla_torch"] == before
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [w.shape for w in g["o64"]]
    assert all(o.dtype is torch.float32 and o.is_contiguous() for o in out)
    err = D.stage_error(out, g["o64"])
    print("dla case %s %s on the device: error / e32 per stage %s" % (case, kw, ["%.2f" % (e / b) for e, b in zip(err, g["e32"])]))
    for k, (e, b) in enumerate(zip(err, g["e32"])):
        assert e <= 4 * b, "stage %d: %.3e against e32 %.3e" % (k + 2, e, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["D", "E", "F"])
def test_dla_against_the_reference_golden(case):
    """The bound of tests/test_dla.py::test_dla_against_the_reference_golden: 4 x the reference's own fp32 error per stage.
    Measured ratios: INTEGRATION.md §3o."""
    _against_the_golden(case)


@pytest.mark.gpu
def test_split_operands_against_the_reference_golden():
    _against_the_golden("D", operands="split16")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["D", "E"])
def test_images_half_images_and_half_outputs(case):
    levels, channels, shape, _ = B.NET_CASES[case]
    model, _ = _net(case, "cuda")
    x = torch.from_numpy(D.image(shape, 3, N=3)).cuda()
    with torch.no_grad():
        out = model(x)
        again, syncs = H.count_syncs(lambda: model(x))
        assert _equal_bits(out, again) and float(out[3].abs().max()) > 0
        assert len(syncs) == 0, [str(s.message)[:80] for s in syncs]
        for i in range(3):
            assert _equal_bits(model(x[i:i + 1]), [o[i:i + 1] for o in out]), "image %d" % i
        for dtype in (torch.float16, torch.bfloat16):
            h = x.to(dtype)
            assert _equal_bits(model(h), model(h.float()))      # a half image: the bits of the call on image.float()
            half, _ = _net(case, "cuda", out_dtype=dtype)
            got = half(x)
            assert all(o.dtype is dtype and o.is_contiguous() for o in got)
            assert _equal_bits(got, [o.to(dtype) for o in out])  # rounded once: the next stage read the fp32 value


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A", "C"])
@pytest.mark.parametrize("operands", ["fp32", "split16"])
def test_basic_blocks_through_the_new_entry_point_have_the_bits_of_dla(case, operands):
    import siammot_amd.ops as ops
    from siammot_amd.dla import DLA
    levels, channels, shape = D.NET_CASES[case]
    model = D.load(DLA(levels, channels, operands=operands), D.params(DLA(levels, channels), D.SEED), "cuda")
    x = torch.from_numpy(D.image(shape, 5, N=2)).cuda()
    with torch.no_grad():
        convs = [(c.weight.detach(),) + tuple(t.contiguous() for t in bn.scale_shift()) for c, bn in model.convs()]
        packed = ops.dla_net_pack(convs, levels, channels, operands=operands)
        assert torch.equal(_bits(packed), _bits(ops.dla_pack(convs, levels, channels, operands=operands)))
        for dtype in (torch.float32, torch.bfloat16):
            want = ops.dla(x, packed, levels, channels, out_dtype=dtype, operands=operands)
            got = ops.dla_net(x, packed, levels, channels, out_dtype=dtype, operands=operands)
            assert float(want[3].float().abs().max()) > 0 and _equal_bits(got, want)
        assert _equal_bits(model(x), ops.dla(x, packed, levels, channels, operands=operands))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dla_60", "dla_169"])
def test_the_real_bodies_against_their_own_cpu_module(name):
    """DLA-60 / DLA-169 with the recipe's parameters on one 64 x 64 image, against the same module on the CPU in fp64; the
    bound is 4 x the error of its own CPU fp32 run (the CPU module is pinned to the reference by cases D, E, F)."""
    import siammot_amd.dla as M
    import siammot_amd.ops as ops
    model = getattr(M, name)()
    prm = D.params(model, B.SEED)
    D.load(model, prm)
    x = torch.from_numpy(D.image((64, 64), B.SEED))
    with torch.no_grad():
        o32 = [o.clone() for o in model(x)]
        o64 = [o.clone() for o in model.double()(x.double())]
    e32 = D.stage_error(o32, o64)
    dev = D.load(getattr(M, name)(), prm, "cuda")
    before = ops.FALLBACKS["dla_torch"]
    with torch.no_grad():
        out = dev(x.cuda())
    assert ops.FALLBACKS["dla_torch"] == before
    assert [tuple(o.shape) for o in out] == [tuple(o.shape) for o in o64] and all(bool(torch.isfinite(o).all()) for o in out)
    err = D.stage_error(out, o64)
    print("%s on the device: error %s, the CPU's own fp32 error %s, ratios %s"
          % (name, ["%.2e" % e for e in err], ["%.2e" % e for e in e32], ["%.2f" % (e / b) for e, b in zip(err, e32)]))
    for k, (e, b) in enumerate(zip(err, e32)):
        assert e <= 4 * b, "stage %d: %.3e against e32 %.3e" % (k + 2, e, b)


@pytest.mark.gpu
def test_calls_beyond_the_capacities_take_the_torch_composition():
    import siammot_amd.ops as ops
    from siammot_amd.dla import DLA
    model, x = _net("F", "cuda")
    g = B.golden("F")
    with torch.no_grad():
        want = model(x.cuda())
        before = ops.FALLBACKS["dla_torch"]
        out = model(x.cuda().contiguous(memory_format=torch.channels_last))     # not contiguous NCHW: the composition, counted
        assert ops.FALLBACKS["dla_torch"] == before + 1
        # (torch's device convolutions: the project's bound for a convolution against fp64, of the stage's largest value)
        assert [o.shape for o in out] == [w.shape for w in want] and max(D.stage_error(out, g["o64"])) < 1e-4
    out = model(x.cuda())                                        # grad mode with trainable filters: the composition
    assert ops.FALLBACKS["dla_torch"] == before + 2 and out[0].requires_grad
    narrow = DLA((1, 1, 1, 1, 2, 1), (16, 32, 96, 96, 96, 96), block="bottleneck").cuda().eval()      # mid = 48
    with torch.no_grad():
        assert len(narrow(torch.zeros((1, 3, 32, 32), device="cuda"))) == 4
    assert ops.FALLBACKS["dla_torch"] == before + 3


@pytest.mark.gpu
def test_forward_images_of_a_dla_60_detector_is_the_composition_with_one_host_copy():
    import fpn_cases as FP
    import rpn_proposal_cases as R
    import siammot_amd.ops as ops
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.config import get_default_cfg
    from siammot_amd.detector import build_detection_head
    C, N, size = 128, 2, (96, 64)
    cfg = get_default_cfg("DLA-60-FPN", channels=C)
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    torch.manual_seed(5)
    det = build_detection_head(cfg, BoxCoder(R.WEIGHTS), C, backbone=True).to("cuda").eval()
    H.load_head(det.rpn_head, H.params(C, 3, seed=1), "cuda")
    FP.load_fpn(det.backbone.fpn, FP.params(C, (128, 256, 512, 1024), seed=2), "cuda")
    D.load(det.backbone.body, D.params(det.backbone.body, B.SEED), "cuda")
    with torch.no_grad():
        det.box_head.predictor.bbox_pred.weight.mul_(0.02)
        det.box_head.predictor.cls_score.weight.mul_(4.0)
    images = torch.from_numpy(D.image((64, 96), 9, N=N)).cuda()
    assert det.backbone.body.block == "bottleneck" and len(det.backbone.body.convs()) == 63
    with torch.no_grad():
        stages = det.backbone.body(images)
        want_feats, want = det.forward_stages(stages, size)      # (also: workspaces, the packed weights, the anchors)
        assert _equal_bits(det.backbone(images), want_feats)
    assert [tuple(s.shape[1:]) for s in stages] == [(128, 16, 24), (256, 8, 12), (512, 4, 6), (1024, 2, 3)]
    before = dict(ops.FALLBACKS)
    (got_feats, got), syncs = H.count_syncs(lambda: det.forward_images(images, size))
    assert dict(ops.FALLBACKS) == before
    assert len(syncs) == 1, "expected ONE device->host copy, saw %d: %s" % (len(syncs), [str(x.message)[:80] for x in syncs])
    assert _equal_bits(got_feats, want_feats) and len(got_feats) == 5
    assert len(got) == len(want) == N
    for a, b in zip(got, want):
        assert len(a) == len(b) and torch.equal(a.bbox.view(torch.int32), b.bbox.view(torch.int32))
        assert torch.equal(a.get_field("scores").view(torch.int32), b.get_field("scores").view(torch.int32))
    print("DLA-60 forward_images N=%d: detections %s" % (N, [len(a) for a in got]))
