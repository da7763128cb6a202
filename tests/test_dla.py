"""DLA backbone body on the device (siammot_amd.dla.DLA, siammot_amd.backbone, ops.dla / dla_pack / dla_conv3x3 / dla_conv1x1 /
dla_stem, csrc/dla.hip, csrc/conv3x3_mfma.h) and ``DetectionHead.forward_images``.

CPU: symbols and capacities, ``state_dict`` keys, the module on CPU tensors against the golden vectors of the reference's own
dla.py (tests/golden/dla_stages.npz, tools/gen_golden_dla.py), the unused outer ``project``, the config's body and backbone.
GPU, operator level: the three kernels against torch's ``F.conv2d`` / ``F.max_pool2d`` / ``torch.cat`` on the CPU
(tests/dla_cases.py) with the bound of the project's other matrix-core convolutions (1e-4 of the per-channel scale against
fp64, 2e-4 against fp32; the scale is the per-channel max of the fp64 PRE-ReLU value); exactness with integer data;
non-finite cells; raw calls beyond the capacities.
GPU, network level: the HIP path against the golden vectors within 4 x the reference's own fp32 error per stage; images of a
call, half images and half outputs; fallbacks; repacking; frames to detections with one host copy.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dla_cases as D
import rpn_head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smot_dla_conv3x3_form", "smot_dla_packed_floats", "smot_dla_pack", "smot_dla_ws_bytes", "smot_dla_fwd", "smot_dla_conv3x3_fwd",
               "smot_dla_conv1x1_fwd", "smot_dla_stem_fwd", "smot_dla_conv_packed_floats", "smot_dla_stem_ws_bytes")
_cache = {}


def _cfg(channels=128):
    from siammot_amd.config import get_default_cfg
    return get_default_cfg(channels=channels)


def _net(case, dev="cpu", **kw):
    """The case's network with the recipe's parameters on ``dev``, and its image."""
    from siammot_amd.dla import DLA
    levels, channels, shape = D.NET_CASES[case]
    model = DLA(levels, channels, **kw)
    if ("prm", case) not in _cache:
        _cache[("prm", case)] = D.params(model, D.SEED)
    return D.load(model, _cache[("prm", case)], dev), torch.from_numpy(D.image(shape, D.SEED))


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _equal_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_carry_the_new_symbols():
    import siammot_amd.ops as ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smot_emm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smot_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared and name in ops.EXPORTED_SYMBOLS, name
    assert ops.ABI_VERSION == 14 and re.search(r"#define SMOT_ABI_VERSION 14\b", src)
    assert "dla_torch" in dict(ops.FALLBACKS)                    # registered from import
    assert ops.dla_shapes_ok(*D.DLA34) and ops.dla_shapes_ok(*D.DLA34, H=704, W=1280, N=4)
    levels, channels, (h, w) = D.NET_CASES["C"]
    assert ops.dla_shapes_ok(levels, channels, h, w)
    assert not ops.dla_shapes_ok(*D.DLA34, H=40, W=72)
    assert not ops.dla_shapes_ok(D.DLA34[0], (16, 32, 48, 128, 256, 512))
    assert not ops.dla_shapes_ok((2, 1, 1, 2, 2, 1), D.DLA34[1])


def test_state_dict_is_upstreams():
    from siammot_amd.dla import DLA, FrozenBatchNorm2d, dla_34
    model = dla_34()
    sd = model.state_dict()
    keys = list(sd.keys())
    assert len(keys) == 195
    assert keys[:5] == ["base_layer.0.weight", "base_layer.1.weight", "base_layer.1.bias", "base_layer.1.running_mean",
                        "base_layer.1.running_var"]
    assert keys[15] == "level2.tree1.conv1.weight" and keys[-1] == "level5.project.1.running_var"
    # upstream registers tree1, tree2, root, project in that order
    level2 = [k for k in keys if k.startswith("level2.")]
    assert [k.split(".")[1] for k in level2[::5]] == ["tree1", "tree1", "tree2", "tree2", "root", "project"]
    for k in ("level2.root.conv.weight", "level2.project.0.weight", "level3.tree2.tree1.bn2.running_var", "level3.project.0.weight",
              "level3.tree1.project.0.weight", "level4.tree2.root.bn.running_mean", "level5.tree2.conv2.weight"):
        assert k in sd, k
    assert "level3.tree2.project.0.weight" not in sd and "level3.root.conv.weight" not in sd
    assert sd["base_layer.0.weight"].shape == (16, 3, 7, 7)
    assert sd["level3.tree2.root.conv.weight"].shape == (128, 448, 1, 1)
    assert sd["level4.project.0.weight"].shape == (256, 128, 1, 1)
    assert sd["level2.root.conv.weight"].shape == (64, 128, 1, 1) and sd["level5.root.conv.weight"].shape == (512, 1280, 1, 1)
    bns = [(n, m) for n, m in model.named_modules() if isinstance(m, FrozenBatchNorm2d)]
    assert len(bns) == 39 and not list(bns[0][1].parameters())
    for name, bn in bns:
        conv = sd[name[:-1] + "0.weight"] if name.endswith(".1") else sd[name.replace("bn", "conv") + ".weight"]
        for b in ("weight", "bias", "running_mean", "running_var"):
            assert sd["%s.%s" % (name, b)].shape == (conv.shape[0],), (name, b)
    assert len(model.convs()) == 37                               # the two outer projects are owned, not evaluated
    levels, channels, _ = D.NET_CASES["C"]
    assert len(DLA(levels, channels).state_dict()) == 185


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_cpu_module_against_the_reference_golden(case):
    """The same operators in the same order as the reference, only the threading differs: 2 x its own fp32 error."""
    import siammot_amd.ops as ops
    g = D.golden(case)
    model, x = _net(case)
    assert g["seed"] == D.SEED and g["shape"] == tuple(x.shape[2:]) and len(model.state_dict()) == D.NET_KEYS[case]
    before = ops.FALLBACKS["dla_torch"]
    with torch.no_grad():
        out = model(x)
    assert ops.FALLBACKS["dla_torch"] == before                  # counted for device tensors only
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [w.shape for w in g["o64"]]
    err = D.stage_error(out, g["o64"])
    print("dla case %s on the CPU: error / e32 per stage %s" % (case, ["%.2f" % (e / b) for e, b in zip(err, g["e32"])]))
    for k, (e, b) in enumerate(zip(err, g["e32"])):
        assert e <= 2 * b, "stage %d: %.3e against e32 %.3e" % (k + 2, e, b)
    half, _ = _net(case, out_dtype=torch.float16)
    with torch.no_grad():
        assert _equal_bits(half(x), [o.to(torch.float16) for o in out])


def test_the_outer_project_is_owned_and_unused():
    model, x = _net("A")
    with torch.no_grad():
        a = model(x)
        model.level3.project[0].weight.mul_(2.0)
        b = model(x)
        assert _equal_bits(a, b)
        model.level3.tree1.project[0].weight.mul_(2.0)
        c = model(x)
    assert torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])


def test_build_dla_and_build_backbone_read_the_config():
    from siammot_amd.backbone import build_backbone, strip_prefix
    from siammot_amd.dla import DLA, build_dla
    from siammot_amd.fpn import FPN
    cfg = _cfg(128)
    body = build_dla(cfg)
    assert type(body) is DLA and (body.levels, body.channels) == D.DLA34 and tuple(body.out_channels) == (64, 128, 256, 512)
    for channels in (128, 256):
        bb = build_backbone(_cfg(channels))
        assert [n for n, _ in bb.named_children()] == ["body", "fpn"] and type(bb.body) is DLA and type(bb.fpn) is FPN
        assert bb.out_channels == channels and bb.fpn.in_channels == (64, 128, 256, 512)
    bb = build_backbone(cfg)
    ckpt = {"backbone." + k: torch.full_like(v, 0.25) for k, v in bb.state_dict().items()}
    ckpt["rpn.head.conv.weight"] = torch.zeros(1)
    assert len(ckpt) == 195 + 16 + 1
    bb.load_state_dict(strip_prefix(ckpt), strict=True)
    assert float(bb.body.level4.tree1.root.bn.running_var[3]) == 0.25 and float(bb.fpn.fpn_layer2.bias.detach()[0]) == 0.25
    bad = _cfg()
    bad.MODEL.BACKBONE.CONV_BODY = "DLA-60-FPN"
    with pytest.raises(ValueError, match="DLA-60-FPN"):
        build_dla(bad)
    dcn = _cfg()
    dcn.MODEL.DLA.STAGE_WITH_DCN = (False, False, False, False, True, False)
    with pytest.raises(ValueError, match="STAGE_WITH_DCN"):
        build_backbone(dcn)


# ---- GPU, operator level ------------------------------------------------------------------------------------------------
CONV3 = [(32, 64, 2, (26, 42)), (64, 64, 1, (13, 21)), (48, 96, 2, (25, 41)), (160, 160, 1, (1, 5)), (512, 512, 1, (2, 3))]


def _conv3_ref(Cin, Cout, stride, size, N):
    key = ("c3", Cin, Cout, stride, size, N)
    if key not in _cache:
        c = D.conv3x3_case(Cin, Cout, stride, size, N)
        ref = {}
        for residual in (False, True):
            pre64 = D.conv3x3_oracle(c, torch.float64, residual, pre=True)
            for relu in (False, True):
                ref[(residual, relu)] = (D.conv3x3_oracle(c, torch.float64, residual, relu),
                                         D.conv3x3_oracle(c, torch.float32, residual, relu), D.channel_scale(pre64))
        _cache[key] = (c, ref)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,stride,size", CONV3)
def test_conv3x3_against_the_cpu_oracle(Cin, Cout, stride, size):
    import siammot_amd.ops as ops
    for N in (1, 3):
        c, ref = _conv3_ref(Cin, Cout, stride, size, N)
        x, w, scale, shift, res = (_cuda(c[k]) for k in ("x", "w", "scale", "shift", "residual"))
        for (residual, relu), (o64, o32, ch) in ref.items():
            out = ops.dla_conv3x3(x, w, scale, shift, stride, res if residual else None, relu)
            assert out.shape == o32.shape and out.dtype is torch.float32 and out.is_contiguous()
            e64, e32 = D.scaled_error(out, o64, ch), D.scaled_error(out, o32, ch)
            print("dla_conv3x3 %d->%d stride %d %s N=%d residual=%d relu=%d: %.3e vs fp64, %.3e vs fp32"
                  % (Cin, Cout, stride, size, N, residual, relu, e64, e32))
            assert e64 < 1e-4 and e32 < 2e-4
            if N == 3:                                           # each image is the one-image call, bit for bit
                for i in range(N):
                    one = ops.dla_conv3x3(x[i:i + 1], w, scale, shift, stride, res[i:i + 1] if residual else None, relu)
                    assert torch.equal(_bits(one), _bits(out[i:i + 1])), "image %d" % i


# (Cin, Cout, stride, input size, N of the large call, its form (WR, NM)): the one-image call of each runs (4, .), the
# large call crosses the library's workgroup threshold and runs another form of the kernel — with the cases of CONV3 every
# form the launch site can choose: (4, 1), (4, 2), (2, 2) at both strides, (1, 2) at stride 1
FORMS = [(64, 64, 1, (32, 128), 8, (2, 2)), (32, 64, 2, (63, 127), 16, (2, 2)), (32, 128, 1, (29, 61), 16, (1, 2)),
         (16, 16, 1, (13, 21), 2, (4, 1)), (16, 32, 2, (26, 42), 2, (4, 2))]


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,stride,size,N,form", FORMS)
def test_conv3x3_forms(Cin, Cout, stride, size, N, form):
    """The wave split is chosen by the launch's workgroup count: the large call runs ``form``, its images alone run (4, .), and
    both give the same bits — an output's summation order does not depend on the split."""
    import siammot_amd.ops as ops
    assert ops.dla_conv3x3_form(N, size[0], size[1], Cout, stride) == form
    assert ops.dla_conv3x3_form(1, size[0], size[1], Cout, stride) == (4, form[1])
    c = D.conv3x3_case(Cin, Cout, stride, size, N)
    o64, o32 = D.conv3x3_oracle(c, torch.float64), D.conv3x3_oracle(c, torch.float32)
    ch = D.channel_scale(D.conv3x3_oracle(c, torch.float64, pre=True))
    x, w, scale, shift, res = (_cuda(c[k]) for k in ("x", "w", "scale", "shift", "residual"))
    out = ops.dla_conv3x3(x, w, scale, shift, stride, res, True)
    e64, e32 = D.scaled_error(out, o64, ch), D.scaled_error(out, o32, ch)
    print("dla_conv3x3 form %s: %d->%d stride %d %s N=%d: %.3e vs fp64, %.3e vs fp32" % (form, Cin, Cout, stride, size, N, e64, e32))
    assert e64 < 1e-4 and e32 < 2e-4
    for i in range(N):
        one = ops.dla_conv3x3(x[i:i + 1], w, scale, shift, stride, res[i:i + 1], True)
        assert torch.equal(_bits(one), _bits(out[i:i + 1])), "image %d" % i


def test_conv3x3_forms_reach_every_form():
    """The cases of CONV3 and FORMS together run every form the launch site has (a retune of the threshold must keep that)."""
    import siammot_amd.ops as ops
    seen = set()
    for Cin, Cout, stride, size in CONV3:
        seen |= {(stride,) + ops.dla_conv3x3_form(N, size[0], size[1], Cout, stride) for N in (1, 3)}
    for Cin, Cout, stride, size, N, form in FORMS:
        seen |= {(stride,) + ops.dla_conv3x3_form(n, size[0], size[1], Cout, stride) for n in (1, N)}
    assert seen == {(1, 4, 1), (1, 4, 2), (1, 2, 2), (1, 1, 2), (2, 4, 2), (2, 2, 2)}, seen
    # the headline frame: level2 at WR = 2, the coarser levels at WR = 4; four images move level3 to WR = 1
    assert ops.dla_conv3x3_form(1, 176, 320, 64, 1) == (2, 2) and ops.dla_conv3x3_form(1, 88, 160, 128, 1) == (4, 2)
    assert ops.dla_conv3x3_form(4, 88, 160, 128, 1) == (1, 2) and ops.dla_conv3x3_form(1, 704, 1280, 16, 1) == (4, 1)


CONV1 = [([(32, False), (32, False)], 32, (13, 21), True),
         ([(64, False), (64, False), (32, (26, 42))], 64, (13, 21), True),
         ([(96, False), (96, False), (64, (27, 43)), (96, False)], 96, (13, 21), True),
         ([(32, (26, 42))], 64, (13, 21), False)]


@pytest.mark.gpu
@pytest.mark.parametrize("sources,Cout,size,relu", CONV1)
def test_conv1x1_against_the_cpu_oracle(sources, Cout, size, relu):
    import siammot_amd.ops as ops
    for N in (1, 3):
        c = D.conv1x1_case(sources, Cout, size, N)
        o64, o32 = D.conv1x1_oracle(c, torch.float64, relu), D.conv1x1_oracle(c, torch.float32, relu)
        ch = D.channel_scale(D.conv1x1_oracle(c, torch.float64, pre=True))
        src = [_cuda(s) for s in c["src"]]
        args = (c["pooled"], _cuda(c["w"]), _cuda(c["scale"]), _cuda(c["shift"]), relu)
        out = ops.dla_conv1x1(src, *args)
        assert out.shape == o32.shape and out.dtype is torch.float32
        e64, e32 = D.scaled_error(out, o64, ch), D.scaled_error(out, o32, ch)
        print("dla_conv1x1 %s -> %d N=%d: %.3e vs fp64, %.3e vs fp32" % (sources, Cout, N, e64, e32))
        assert e64 < 1e-4 and e32 < 2e-4
        if N == 3:
            for i in range(N):
                assert torch.equal(_bits(ops.dla_conv1x1([s[i:i + 1] for s in src], *args)), _bits(out[i:i + 1])), "image %d" % i
            half = ops.dla_conv1x1(src, *args, out_dtype=torch.bfloat16)
            assert torch.equal(_bits(half), _bits(out.to(torch.bfloat16)))


@pytest.mark.gpu
@pytest.mark.parametrize("size,N", [((32, 32), 1), ((64, 96), 2), ((32, 160), 1)])
def test_stem_against_the_cpu_oracle(size, N):
    import siammot_amd.ops as ops
    c = D.stem_case(16, 32, size, N)
    o64, o32 = D.stem_oracle(c, torch.float64), D.stem_oracle(c, torch.float32)
    ch = D.channel_scale(D.stem_oracle(c, torch.float64, pre=True))
    layers = [tuple(_cuda(t) for t in layer) for layer in c["layers"]]
    img = _cuda(c["image"])
    out = ops.dla_stem(img, layers)
    assert out.shape == o32.shape == (N, 32, size[0] // 2, size[1] // 2) and out.dtype is torch.float32
    e64, e32 = D.scaled_error(out, o64, ch), D.scaled_error(out, o32, ch)
    print("dla_stem %s N=%d: %.3e vs fp64, %.3e vs fp32" % (size, N, e64, e32))
    assert e64 < 1e-4 and e32 < 2e-4
    for dtype in (torch.float16, torch.bfloat16):                # a half image: the bits of the call on image.float()
        h = img.to(dtype)
        assert torch.equal(_bits(ops.dla_stem(h, layers)), _bits(ops.dla_stem(h.float(), layers)))
    if N > 1:
        for i in range(N):
            assert torch.equal(_bits(ops.dla_stem(img[i:i + 1], layers)), _bits(out[i:i + 1])), "image %d" % i


def _ints(rs, shape, lo=-1, hi=1):
    return rs.randint(lo, hi + 1, size=shape).astype(D.F32)


def _pow2(rs, n, choices):
    return np.asarray(choices, dtype=D.F32)[rs.randint(0, len(choices), size=n)]


def _sparse_filters(rs, cout, cin, k, nonzero):
    """Filters in {-1, 0, 1} with exactly ``nonzero`` non-zero taps per output channel, at random places."""
    w = np.zeros((cout, cin * k * k), dtype=D.F32)
    for o in range(cout):
        idx = rs.permutation(cin * k * k)[:nonzero]
        w[o, idx] = rs.choice(np.asarray([-1.0, 1.0], dtype=D.F32), size=nonzero)
    return w.reshape(cout, cin, k, k)


@pytest.mark.gpu
def test_exact_with_integer_data():
    """Inputs, filters and residuals in {-1, 0, 1}, scale in {0.5, 1, 2}, shift an integer in -2 .. 2.

    conv3x3 (48 -> 96 at stride 2 on 25 x 41, 64 -> 64 at stride 1 on 13 x 21, and 64 -> 64 on 27 x 43 with the residual read
    through the 2 x 2 max-pool of a 54 x 87 map: a max of four integers): an output sums at most 9 * 64 = 576 terms of
    size <= 1: every partial sum is an integer, |.| <= 576 < 2^22, exact in fp32 in ANY order; times a power of two, plus
    an integer, plus a residual of size <= 1: a multiple of 1/2 with |.| <= 1155.  conv1x1 over (96, 96, pooled 64, 96)
    channels: 352 terms, the same argument; the pooled source is a max of four integers.
    Stem (16, 32 channels on 32 x 64): base_layer sums 147 terms, scale in {0.5, 1}: x is a multiple of 1/2, |x| <= 149.
    level0 and level1 have exactly 32 non-zero taps (+-1) per output channel: level0 sums to a multiple of 1/2, |.| <= 32 * 149 =
    4768; with scale in {0.5, 1} and the shift x0 is a multiple of 1/4, |x0| <= 4770, i.e. below 2^15 quarters.  level1 sums 32
    of them: below 2^20 quarters < 2^22, exact in any order, and its scale in {0.5, 1} and shift keep the result a multiple
    of 1/8 below 2^21 eighths.  So every output equals the fp32 yardstick bit for bit (asserted on the CPU first: the fp32
    and fp64 yardsticks agree exactly).  This pins the stride-2 tap alignment, the zero padding of each stem layer (a level0
    cell outside the map is 0, not relu(shift)), the concatenation order, the pool's window and the residual."""
    import siammot_amd.ops as ops
    rs = np.random.RandomState(23)
    for Cin, Cout, stride, size in ((48, 96, 2, (25, 41)), (64, 64, 1, (13, 21))):
        ho, wo = ((size[0] - 1) // 2 + 1, (size[1] - 1) // 2 + 1) if stride == 2 else size
        c = dict(x=_ints(rs, (2, Cin) + size), w=_ints(rs, (Cout, Cin, 3, 3)), scale=_pow2(rs, Cout, (0.5, 1.0, 2.0)),
                 shift=_ints(rs, Cout, -2, 2), residual=_ints(rs, (2, Cout, ho, wo)), stride=stride)
        o32, o64 = D.conv3x3_oracle(c, torch.float32), D.conv3x3_oracle(c, torch.float64)
        assert torch.equal(o32.double(), o64) and float(o32.max()) > 50 and float((o32 - o32.round()).abs().max()) == 0.5
        out = ops.dla_conv3x3(*(_cuda(c[k]) for k in ("x", "w", "scale", "shift")), stride, _cuda(c["residual"]), True)
        assert torch.equal(out.cpu(), o32), "conv3x3 stride %d: %d cells differ" % (stride, int((out.cpu() != o32).sum()))
    # a stage that keeps its width: the residual is the input read through the 2 x 2 max-pool (27 x 43: floor)
    c = dict(x=_ints(rs, (2, 64, 27, 43)), w=_ints(rs, (64, 64, 3, 3)), scale=_pow2(rs, 64, (0.5, 1.0, 2.0)),
             shift=_ints(rs, 64, -2, 2), stride=1, residual=_ints(rs, (2, 64, 54, 87)), residual_pooled=True)
    o32, o64 = D.conv3x3_oracle(c, torch.float32), D.conv3x3_oracle(c, torch.float64)
    assert torch.equal(o32.double(), o64) and float(o32.max()) > 50
    out = ops.dla_conv3x3(*(_cuda(c[k]) for k in ("x", "w", "scale", "shift")), 1, _cuda(c["residual"]), True, residual_pooled=True)
    assert torch.equal(out.cpu(), o32), "conv3x3 with a pooled residual: %d cells differ" % int((out.cpu() != o32).sum())
    sources = [(96, False), (96, False), (64, (27, 43)), (96, False)]
    c = dict(src=[_ints(rs, (2, ch) + (p if p else (13, 21))) for ch, p in sources], pooled=[bool(p) for _, p in sources],
             w=_ints(rs, (96, 352, 1, 1)), scale=_pow2(rs, 96, (0.5, 1.0, 2.0)), shift=_ints(rs, 96, -2, 2))
    o32, o64 = D.conv1x1_oracle(c, torch.float32), D.conv1x1_oracle(c, torch.float64)
    assert torch.equal(o32.double(), o64) and float(o32.max()) > 30
    out = ops.dla_conv1x1([_cuda(s) for s in c["src"]], c["pooled"], _cuda(c["w"]), _cuda(c["scale"]), _cuda(c["shift"]), True)
    assert torch.equal(out.cpu(), o32), "conv1x1: %d cells differ" % int((out.cpu() != o32).sum())
    layers = [(_ints(rs, (16, 3, 7, 7)), _pow2(rs, 16, (0.5, 1.0)), _ints(rs, 16, -2, 2)),
              (_sparse_filters(rs, 16, 16, 3, 32), _pow2(rs, 16, (0.5, 1.0)), _ints(rs, 16, -2, 2)),
              (_sparse_filters(rs, 32, 16, 3, 32), _pow2(rs, 32, (0.5, 1.0)), _ints(rs, 32, -2, 2))]
    c = dict(image=_ints(rs, (2, 3, 32, 64)), layers=layers)
    o32, o64 = D.stem_oracle(c, torch.float32), D.stem_oracle(c, torch.float64)
    assert torch.equal(o32.double(), o64) and float(o32.max()) > 100 and float((o32 * 8 - (o32 * 8).round()).abs().max()) == 0.0
    out = ops.dla_stem(_cuda(c["image"]), [tuple(_cuda(t) for t in layer) for layer in layers])
    assert torch.equal(out.cpu(), o32), "stem: %d cells differ" % int((out.cpu() != o32).sum())


@pytest.mark.gpu
def test_non_finite_cells_spread_as_in_torch():
    import siammot_amd.ops as ops
    for Cin, Cout, stride, size in ((32, 64, 2, (26, 42)), (64, 64, 1, (13, 21))):
        c0, _ = _conv3_ref(Cin, Cout, stride, size, 3)
        c = dict(c0, x=c0["x"].copy(), residual=c0["residual"].copy())
        c["x"][0, 3, 5, 7] = np.nan                              # interior cells
        c["x"][1, 10, 6, 9] = np.inf
        c["x"][1, 11, 11, 4] = -np.inf
        c["x"][2, 0, 0, 0] = -np.inf                             # a corner
        c["residual"][2, 5, 2, 3] = np.nan
        c["residual"][0, 7, 4, 4] = -np.inf                      # -inf behind the ReLU is 0
        ch = D.channel_scale(D.conv3x3_oracle(c0, torch.float64, pre=True))
        for relu in (True, False):
            o32, o64 = D.conv3x3_oracle(c, torch.float32, relu=relu), D.conv3x3_oracle(c, torch.float64, relu=relu)
            out = ops.dla_conv3x3(*(_cuda(c[k]) for k in ("x", "w", "scale", "shift")), stride, _cuda(c["residual"]), relu).cpu()
            assert torch.equal(torch.isnan(out), torch.isnan(o32)) and torch.equal(torch.isfinite(out), torch.isfinite(o32))
            assert int(torch.isnan(o32).sum()) > Cout and bool(torch.isnan(o32[2, 5, 2, 3]))
            assert float(o32[0, 7, 4, 4]) == (0.0 if relu else -np.inf)
            assert D.scaled_error(out, o64, ch) < 1e-4 and D.scaled_error(out, o32, ch) < 2e-4
    # the residual read through the pool: a NaN in the window is the residual, a -inf loses the max, a +inf wins it
    c0, _ = _conv3_ref(64, 64, 1, (13, 21), 3)
    rs = np.random.RandomState(31)
    c = dict(c0, residual=(rs.standard_normal((3, 64, 27, 43)) * 4.0).astype(D.F32), residual_pooled=True)
    c["residual"][0, 3, 5, 9] = np.nan                           # -> output (2, 4)
    c["residual"][1, 8, 0, 1] = -np.inf
    c["residual"][2, 9, 25, 41] = np.inf                         # -> output (12, 20)
    c["residual"][2, 10, 26, 42] = np.nan                        # the odd map's last row and column: read by no window
    o32, o64 = D.conv3x3_oracle(c, torch.float32), D.conv3x3_oracle(c, torch.float64)
    out = ops.dla_conv3x3(*(_cuda(c[k]) for k in ("x", "w", "scale", "shift")), 1, _cuda(c["residual"]), True, residual_pooled=True).cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(o32)) and torch.equal(torch.isfinite(out), torch.isfinite(o32))
    assert int(torch.isnan(o32).sum()) == 1 and bool(torch.isnan(o32[0, 3, 2, 4])) and float(o32[2, 9, 12, 20]) == np.inf
    assert int((~torch.isfinite(o32)).sum()) == 2
    ch = D.channel_scale(D.conv3x3_oracle(dict(c0, residual=np.nan_to_num(c["residual"], nan=0.0, posinf=0.0, neginf=0.0),
                                               residual_pooled=True), torch.float64, pre=True))
    assert D.scaled_error(out, o64, ch) < 1e-4 and D.scaled_error(out, o32, ch) < 2e-4
    sources = [(64, False), (64, False), (32, (26, 42))]
    c0 = D.conv1x1_case(sources, 64, (13, 21), 2)
    c = dict(c0, src=[s.copy() for s in c0["src"]])
    c["src"][2][0, 3, 7, 11] = np.nan                            # the pool hands a NaN on: position (3, 5)
    c["src"][2][1, 8, 0, 1] = -np.inf                            # -inf loses the max: nothing happens
    c["src"][2][1, 9, 25, 41] = np.inf
    c["src"][0][0, 1, 12, 20] = np.nan
    o32, o64 = D.conv1x1_oracle(c, torch.float32), D.conv1x1_oracle(c, torch.float64)
    out = ops.dla_conv1x1([_cuda(s) for s in c["src"]], c["pooled"], _cuda(c["w"]), _cuda(c["scale"]), _cuda(c["shift"]), True).cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(o32)) and torch.equal(torch.isfinite(out), torch.isfinite(o32))
    assert bool(torch.isnan(o32[0, :, 3, 5]).all()) and bool(torch.isfinite(o32[1, :, 0, 0]).all())
    cell = o32[1, :, 12, 20]                                     # +inf times a filter: +inf, or -inf that the ReLU makes 0
    assert bool(((cell == np.inf) | (cell == 0)).all()) and 0 < int((cell == 0).sum()) < 64
    ch = D.channel_scale(D.conv1x1_oracle(c0, torch.float64, pre=True))
    assert D.scaled_error(out, o64, ch) < 1e-4 and D.scaled_error(out, o32, ch) < 2e-4


def _raw_fwd(levels, channels, H, W, N=1, image_offset=0, out_offset=0):
    """``smot_dla_fwd`` on valid buffers of these shapes (the image / output pointers moved by so many bytes) -> its code."""
    import siammot_amd.ops as ops
    lib = ops.load_library()
    arr = lambda vals: ctypes.cast((ctypes.c_int * 6)(*vals), ctypes.c_void_p)
    vp = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    img = torch.zeros((N, 3, H, W), device="cuda")
    out = [torch.zeros((N, channels[k], max(H >> k, 1), max(W >> k, 1)), device="cuda") for k in range(2, 6)]
    floats, nbytes = lib.smot_dla_packed_floats(arr(levels), arr(channels)), lib.smot_dla_ws_bytes(arr(levels), arr(channels), N, H, W)
    packed = torch.zeros(max(floats, 4), device="cuda")
    ws = torch.zeros(max(nbytes // 4, 4), device="cuda")
    po = ctypes.cast((ctypes.c_void_p * 4)(*[t.data_ptr() + out_offset for t in out]), ctypes.c_void_p)
    rc = lib.smot_dla_fwd(vp(img, image_offset), 0, N, H, W, arr(levels), arr(channels), vp(packed), vp(ws), po, 0,
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, floats, nbytes, out


@pytest.mark.gpu
def test_raw_calls_beyond_the_capacities_launch_nothing():
    levels, channels = D.DLA34
    for lv, ch, h, w in ((levels, channels, 40, 72), (levels, (16, 32, 48, 128, 256, 512), 64, 96),
                         ((2, 1, 1, 2, 2, 1), channels, 64, 96), (levels, (24, 32, 64, 128, 256, 512), 64, 96)):
        rc, floats, nbytes, out = _raw_fwd(lv, ch, h, w)
        assert rc == -2 and nbytes == -1 and (floats == -1 or (h, w) == (40, 72)), (lv, ch, h, w)
        assert all(float(o.abs().max()) == 0.0 for o in out)     # SMOT_ERR_UNSUPPORTED; nothing launched
    for kw in ({"image_offset": 2}, {"out_offset": 2}):         # fp32 at an odd half-word: SMOT_ERR_BAD_ARG, nothing launched
        rc, _, _, out = _raw_fwd(levels, channels, 64, 96, **kw)
        assert rc == -1 and all(float(o.abs().max()) == 0.0 for o in out), kw
    rc, floats, nbytes, out = _raw_fwd(levels, channels, 64, 96)  # the same call within the capacities runs
    assert rc == 0 and floats > 0 and nbytes > 0
    import siammot_amd.ops as ops
    x = torch.zeros((1, 32, 4, 4), device="cuda")
    with pytest.raises(RuntimeError, match="Cin = 4|code -2"):
        ops.dla_conv3x3(x[:, :4], torch.zeros((32, 4, 3, 3), device="cuda"), x[0, :, 0, 0], x[0, :, 0, 0], 1)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.dla_conv1x1([x[:, :24].contiguous()], [False], torch.zeros((32, 24, 1, 1), device="cuda"), x[0, :, 0, 0], x[0, :, 0, 0], True)


# ---- GPU, network level -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_dla_against_the_reference_golden(case):
    """The same number of fp32 roundings per output as the reference in another summation order (chunks of four on the matrix
    pipe): 4 x the reference's own fp32 error per stage.  Measured ratios: INTEGRATION.md §3m."""
    import siammot_amd.ops as ops
    g = D.golden(case)
    model, x = _net(case, "cuda")
    before = ops.FALLBACKS["dla_torch"]
    with torch.no_grad():
        out = model(x.cuda())
    assert ops.FALLBACKS["dla_torch"] == before
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [w.shape for w in g["o64"]]
    assert all(o.dtype is torch.float32 and o.is_contiguous() for o in out)
    err = D.stage_error(out, g["o64"])
    print("dla case %s on the device: error / e32 per stage %s" % (case, ["%.2f" % (e / b) for e, b in zip(err, g["e32"])]))
    for k, (e, b) in enumerate(zip(err, g["e32"])):
        assert e <= 4 * b, "stage %d: %.3e against e32 %.3e" % (k + 2, e, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A", "C"])
def test_images_half_images_and_half_outputs(case):
    levels, channels, shape = D.NET_CASES[case]
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
def test_calls_beyond_the_capacities_take_the_torch_composition():
    import siammot_amd.ops as ops
    from siammot_amd.dla import DLA
    model, x = _net("A", "cuda")
    g = D.golden("A")
    with torch.no_grad():
        want = model(x.cuda())
        before = ops.FALLBACKS["dla_torch"]
        nhwc = x.cuda().contiguous(memory_format=torch.channels_last)
        out = model(nhwc)                                        # not contiguous NCHW: the composition, counted
        assert ops.FALLBACKS["dla_torch"] == before + 1
        # (torch's device convolutions: the project's bound for a convolution against fp64, of the stage's largest value)
        assert [o.shape for o in out] == [w.shape for w in want] and max(D.stage_error(out, g["o64"])) < 1e-4
    with pytest.raises(RuntimeError):                            # 40 x 72: the composition, on which torch itself raises
        with torch.no_grad():
            model(torch.zeros((1, 3, 40, 72), device="cuda"))
    assert ops.FALLBACKS["dla_torch"] == before + 2
    out = model(x.cuda())                                        # grad mode with trainable filters: the composition
    assert ops.FALLBACKS["dla_torch"] == before + 3 and out[0].requires_grad
    wide = DLA(D.DLA34[0], (16, 32, 48, 64, 96, 160)).cuda().eval()
    with torch.no_grad():
        assert len(wide(torch.zeros((1, 3, 32, 32), device="cuda"))) == 4
    assert ops.FALLBACKS["dla_torch"] == before + 4


@pytest.mark.gpu
def test_a_changed_parameter_or_buffer_is_packed_again():
    model, x = _net("A", "cuda")
    x = x.cuda()
    with torch.no_grad():
        a = [o.clone() for o in model(x)]
        model.level4.tree1.root.bn.running_var.mul_(4.0)         # a buffer: x4 and x5 change, x2 and x3 do not
        b = [o.clone() for o in model(x)]
        assert _equal_bits(a[:2], b[:2]) and not torch.equal(a[2], b[2]) and not torch.equal(a[3], b[3])
        model.level3.project[0].weight.mul_(2.0)                 # the unused outer project: packed again, the same maps
        assert _equal_bits(model(x), b)
        model.level3.tree1.project[0].weight.mul_(2.0)
        c = model(x)
        assert torch.equal(a[0], c[0]) and not torch.equal(b[1], c[1])
        cpu, _ = _net("A")
        cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        want = [o.double() for o in cpu.double()(x.cpu().double())]
    g = D.golden("A")
    assert all(e <= 4 * b_ for e, b_ in zip(D.stage_error(c, want), g["e32"]))


def _detector(N, dev="cuda"):
    """A seeded ``DetectionHead`` with the config's backbone (the recipe's DLA-34, a seeded FPN) and an RPN head at C = 128,
    and ``N`` images of 64 x 96."""
    import fpn_cases as P
    import rpn_proposal_cases as R
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.detector import build_detection_head
    C = 128
    cfg = _cfg(C)
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    torch.manual_seed(5)
    det = build_detection_head(cfg, BoxCoder(R.WEIGHTS), C, backbone=True).to(dev).eval()
    H.load_head(det.rpn_head, H.params(C, 3, seed=1), dev)
    P.load_fpn(det.backbone.fpn, P.params(C, P.DLA, seed=2), dev)
    D.load(det.backbone.body, D.params(det.backbone.body, D.SEED), dev)
    with torch.no_grad():
        det.box_head.predictor.bbox_pred.weight.mul_(0.02)
        det.box_head.predictor.cls_score.weight.mul_(4.0)
    return det, torch.from_numpy(D.image((64, 96), 9, N=N)).to(dev), (96, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2])
def test_forward_images_is_the_composition_with_one_host_copy(N):
    import siammot_amd.ops as ops
    det, images, size = _detector(N)
    with torch.no_grad():
        stages = det.backbone.body(images)
        want_feats, want = det.forward_stages(stages, size)      # (also: workspaces, the packed weights, the anchors)
        assert _equal_bits(det.backbone(images), want_feats)     # the Sequential is the same composition
    assert [tuple(s.shape[1:]) for s in stages] == [(64, 16, 24), (128, 8, 12), (256, 4, 6), (512, 2, 3)]
    before = dict(ops.FALLBACKS)
    (got_feats, got), syncs = H.count_syncs(lambda: det.forward_images(images, size))
    assert dict(ops.FALLBACKS) == before
    assert len(syncs) == 1, "expected ONE device->host copy, saw %d: %s" % (len(syncs), [str(x.message)[:80] for x in syncs])
    assert _equal_bits(got_feats, want_feats) and len(got_feats) == 5
    assert len(got) == len(want) == N
    for a, b in zip(got, want):
        assert a.fields() == b.fields() == ["scores", "ids", "labels"] and tuple(a.size) == tuple(size) and len(a) == len(b)
        assert torch.equal(a.bbox.view(torch.int32), b.bbox.view(torch.int32))
        assert torch.equal(a.get_field("scores").view(torch.int32), b.get_field("scores").view(torch.int32))
    print("forward_images N=%d: detections %s" % (N, [len(a) for a in got]))
