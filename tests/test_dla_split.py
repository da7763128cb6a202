"""The DLA body's opt-in operand mode ``operands="split16"`` (siammot_amd.dla.DLA, ops.dla / dla_pack / dla_conv3x3 /
dla_conv3x3_form, csrc/dla.hip dla_conv3x3_split_kernel, csrc/conv3x3_mfma.h cvs_block): the trees' 3x3
convolutions on v_mfma_f32_16x16x32_bf16 with three-part bf16 operands and fp32 accumulation.

CPU: the constructor's argument, the unchanged ``state_dict`` and CPU results, the config's builders, the new symbols, the
forms the cases reach.
GPU, operator level: the cases and oracles of tests/dla_cases.py with (A) the project's bounds, 1e-4 of the per-channel scale
against fp64 and 2e-4 against fp32, and (B) the fp32-grade bound ``e_split <= 2 max(e_k32, e_t32)`` against fp64, where e_k32 is
the fp32 kernel's error on the same inputs and e_t32 the torch fp32 oracle's; every form of the launch site; exactness with
integer data; x * 2^k with scale * 2^-k; non-finite cells; an unsupported shape through the raw call.
GPU, network level: the golden vectors within 4 x the reference's own fp32 error; images of a call, half images, half
outputs; repacking; frames to detections with one host copy.
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
NEW_SYMBOLS = ("smot_dla_split_packed_floats", "smot_dla_split_pack", "smot_dla_split_fwd", "smot_dla_conv_split_packed_floats",
               "smot_dla_conv3x3_split_fwd", "smot_dla_conv3x3_split_form")
S16 = "split16"
_cache = {}


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
def test_the_mode_is_a_constructor_argument_and_leaves_the_state_dict_alone():
    from siammot_amd.dla import DLA, dla_34
    model = dla_34(operands=S16)
    assert model.operands == S16 and dla_34().operands == "fp32"
    assert list(model.state_dict().keys()) == list(dla_34().state_dict().keys()) and len(model.state_dict()) == 195
    levels, channels, _ = D.NET_CASES["C"]
    assert len(DLA(levels, channels, operands=S16).state_dict()) == 185
    with pytest.raises(ValueError, match="fp32.*split16"):
        DLA(*D.DLA34, operands="int8")


@pytest.mark.parametrize("case", ["A", "C"])
def test_cpu_tensors_give_the_bits_of_fp32_mode(case):
    import siammot_amd.ops as ops
    a, x = _net(case)
    b, _ = _net(case, operands=S16)
    before = ops.FALLBACKS["dla_torch"]
    with torch.no_grad():
        assert _equal_bits(a(x), b(x))
        half, _ = _net(case, operands=S16, out_dtype=torch.bfloat16)
        assert _equal_bits(half(x), [o.to(torch.bfloat16) for o in a(x)])
    assert ops.FALLBACKS["dla_torch"] == before                  # counted for device tensors only


def test_the_builders_carry_the_mode():
    from siammot_amd.backbone import build_backbone
    from siammot_amd.config import get_default_cfg
    from siammot_amd.dla import build_dla
    cfg = get_default_cfg(channels=128)
    assert build_dla(cfg).operands == "fp32" and build_dla(cfg, operands=S16).operands == S16
    assert build_backbone(cfg).body.operands == "fp32" and build_backbone(cfg, operands=S16).body.operands == S16
    with pytest.raises(ValueError, match="split16"):
        build_backbone(cfg, operands="fp16")


def test_header_and_ctypes_table_carry_the_new_symbols():
    import siammot_amd.ops as ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smot_emm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smot_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared and name in ops.EXPORTED_SYMBOLS, name
    assert ops.DLA_OPERANDS == ("fp32", S16)
    with pytest.raises(ValueError, match="split16"):
        ops.dla_conv3x3_form(1, 8, 8, 32, 1, operands="bf16")


# (Cin, Cout, stride, size): the fp32 mode's cases with Cin a multiple of 32
CONV3 = [(32, 64, 2, (26, 42)), (64, 64, 1, (13, 21)), (96, 96, 2, (25, 41)), (160, 160, 1, (1, 5)), (512, 512, 1, (2, 3))]
# (Cin, Cout, stride, input size, N of the large call, its form (WR, NM)): the one-image call of each runs (4, .); with the
# cases of CONV3 every form the split launch site can choose: (4, 1), (4, 2), (2, 2) at both strides, (1, 2) at stride 1
FORMS = [(64, 64, 1, (32, 128), 8, (2, 2)), (32, 64, 2, (63, 127), 16, (2, 2)), (32, 128, 1, (29, 61), 16, (1, 2)),
         (32, 16, 1, (13, 21), 2, (4, 1)), (32, 32, 2, (26, 42), 2, (4, 2))]


def test_split_forms_reach_every_form():
    """The cases of CONV3 and FORMS together run every form the split launch site has (a retune must keep that)."""
    import siammot_amd.ops as ops
    seen = set()
    for Cin, Cout, stride, size in CONV3:
        seen |= {(stride,) + ops.dla_conv3x3_form(N, size[0], size[1], Cout, stride, operands=S16) for N in (1, 3)}
    for Cin, Cout, stride, size, N, form in FORMS:
        seen |= {(stride,) + ops.dla_conv3x3_form(n, size[0], size[1], Cout, stride, operands=S16) for n in (1, N)}
    assert seen == {(1, 4, 1), (1, 4, 2), (1, 2, 2), (1, 1, 2), (2, 4, 2), (2, 2, 2)}, seen


# ---- GPU, operator level ------------------------------------------------------------------------------------------------
def _conv3_ref(Cin, Cout, stride, size, N, pooled=False):
    """The case and, per (residual, relu): the fp64 oracle, the fp32 oracle, the per-channel scale."""
    key = ("c3", Cin, Cout, stride, size, N, pooled)
    if key not in _cache:
        c = D.conv3x3_case(Cin, Cout, stride, size, N)
        if pooled:
            rs = np.random.RandomState(31)
            c = dict(c, residual=(rs.standard_normal((N, Cout, 2 * size[0] + 1, 2 * size[1] + 1)) * 4.0).astype(D.F32),
                     residual_pooled=True)
        ref = {}
        for residual in ((True,) if pooled else (False, True)):
            pre64 = D.conv3x3_oracle(c, torch.float64, residual, pre=True)
            for relu in (False, True):
                ref[(residual, relu)] = (D.conv3x3_oracle(c, torch.float64, residual, relu),
                                         D.conv3x3_oracle(c, torch.float32, residual, relu), D.channel_scale(pre64))
        _cache[key] = (c, ref)
    return _cache[key]


def _check_bounds(what, out, k32, o64, o32, ch):
    """Bounds A and B of the module docstring; -> e_split / max(e_k32, e_t32)."""
    e_split, e_k32, e_t32 = D.scaled_error(out, o64, ch), D.scaled_error(k32, o64, ch), D.scaled_error(o32, o64, ch)
    e32 = D.scaled_error(out, o32, ch)
    print("%s: vs fp64 split %.3e, fp32 kernel %.3e, torch fp32 %.3e (ratio %.2f); split vs fp32 %.3e"
          % (what, e_split, e_k32, e_t32, e_split / max(e_k32, e_t32), e32))
    assert e_split < 1e-4 and e32 < 2e-4, what
    assert e_split <= 2 * max(e_k32, e_t32), what
    return e_split / max(e_k32, e_t32)


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,stride,size", CONV3)
def test_split_conv3x3_against_the_cpu_oracle(Cin, Cout, stride, size):
    import siammot_amd.ops as ops
    worst = 0.0
    for N in (1, 3):
        c, ref = _conv3_ref(Cin, Cout, stride, size, N)
        x, w, scale, shift, res = (_cuda(c[k]) for k in ("x", "w", "scale", "shift", "residual"))
        for (residual, relu), (o64, o32, ch) in ref.items():
            args = (x, w, scale, shift, stride, res if residual else None, relu)
            out = ops.dla_conv3x3(*args, operands=S16)
            assert out.shape == o32.shape and out.dtype is torch.float32 and out.is_contiguous()
            worst = max(worst, _check_bounds("split conv3x3 %d->%d stride %d %s N=%d residual=%d relu=%d"
                                             % (Cin, Cout, stride, size, N, residual, relu), out, ops.dla_conv3x3(*args), o64, o32, ch))
            if N == 3:                                           # each image is the one-image call, bit for bit
                for i in range(N):
                    one = ops.dla_conv3x3(x[i:i + 1], w, scale, shift, stride, res[i:i + 1] if residual else None, relu, operands=S16)
                    assert torch.equal(_bits(one), _bits(out[i:i + 1])), "image %d" % i
    print("split conv3x3 %d->%d stride %d %s: largest e_split / max(e_k32, e_t32) = %.2f" % (Cin, Cout, stride, size, worst))


@pytest.mark.gpu
def test_split_conv3x3_with_the_pooled_residual():
    import siammot_amd.ops as ops
    c, ref = _conv3_ref(64, 64, 1, (13, 21), 3, pooled=True)
    assert c["residual"].shape == (3, 64, 27, 43)
    x, w, scale, shift, res = (_cuda(c[k]) for k in ("x", "w", "scale", "shift", "residual"))
    for (_, relu), (o64, o32, ch) in ref.items():
        out = ops.dla_conv3x3(x, w, scale, shift, 1, res, relu, residual_pooled=True, operands=S16)
        k32 = ops.dla_conv3x3(x, w, scale, shift, 1, res, relu, residual_pooled=True)
        _check_bounds("split conv3x3 64->64 pooled residual relu=%d" % relu, out, k32, o64, o32, ch)
        for i in range(3):
            one = ops.dla_conv3x3(x[i:i + 1], w, scale, shift, 1, res[i:i + 1], relu, residual_pooled=True, operands=S16)
            assert torch.equal(_bits(one), _bits(out[i:i + 1])), "image %d" % i


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,stride,size,N,form", FORMS)
def test_split_conv3x3_forms(Cin, Cout, stride, size, N, form):
    """The large call runs ``form``, its images alone run (4, .), and both give the same bits."""
    import siammot_amd.ops as ops
    assert ops.dla_conv3x3_form(N, size[0], size[1], Cout, stride, operands=S16) == form
    assert ops.dla_conv3x3_form(1, size[0], size[1], Cout, stride, operands=S16) == (4, form[1])
    c = D.conv3x3_case(Cin, Cout, stride, size, N)
    o64, o32 = D.conv3x3_oracle(c, torch.float64), D.conv3x3_oracle(c, torch.float32)
    ch = D.channel_scale(D.conv3x3_oracle(c, torch.float64, pre=True))
    x, w, scale, shift, res = (_cuda(c[k]) for k in ("x", "w", "scale", "shift", "residual"))
    out = ops.dla_conv3x3(x, w, scale, shift, stride, res, True, operands=S16)
    _check_bounds("split conv3x3 form %s: %d->%d stride %d %s N=%d" % (form, Cin, Cout, stride, size, N), out,
                  ops.dla_conv3x3(x, w, scale, shift, stride, res, True), o64, o32, ch)
    for i in range(N):
        one = ops.dla_conv3x3(x[i:i + 1], w, scale, shift, stride, res[i:i + 1], True, operands=S16)
        assert torch.equal(_bits(one), _bits(out[i:i + 1])), "image %d" % i


def _ints(rs, shape, lo=-1, hi=1):
    return rs.randint(lo, hi + 1, size=shape).astype(D.F32)


def _pow2(rs, shape, choices):
    return np.asarray(choices, dtype=D.F32)[rs.randint(0, len(choices), size=shape)]


@pytest.mark.gpu
def test_split_exact_with_integer_data():
    """Inputs and residuals in {-1, 0, 1}, filters in {0, +-0.5, +-1, +-2}, scale in {0.5, 1, 2}, integer shifts: every value
    is its own first bf16 part (the other two are zero), every product and partial sum a multiple of 1/2 below 2 * 9 * 96 <
    2^22 halves, exact in fp32 in any order: the output equals the fp32 and fp64 oracles exactly.  Odd sizes at both strides
    and the pooled residual: the tap alignment, the stride-2 geometry and the zero halo of the staging."""
    import siammot_amd.ops as ops
    rs = np.random.RandomState(29)
    wvals = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
    for Cin, Cout, stride, size in ((96, 96, 2, (25, 41)), (64, 64, 1, (13, 21)), (32, 32, 2, (17, 35)), (32, 64, 1, (9, 19))):
        ho, wo = ((size[0] - 1) // 2 + 1, (size[1] - 1) // 2 + 1) if stride == 2 else size
        c = dict(x=_ints(rs, (2, Cin) + size), w=_pow2(rs, (Cout, Cin, 3, 3), wvals), scale=_pow2(rs, Cout, (0.5, 1.0, 2.0)),
                 shift=_ints(rs, Cout, -2, 2), residual=_ints(rs, (2, Cout, ho, wo)), stride=stride)
        o32, o64 = D.conv3x3_oracle(c, torch.float32), D.conv3x3_oracle(c, torch.float64)
        assert torch.equal(o32.double(), o64) and float(o32.max()) > 30
        out = ops.dla_conv3x3(*(_cuda(c[k]) for k in ("x", "w", "scale", "shift")), stride, _cuda(c["residual"]), True, operands=S16)
        assert torch.equal(out.cpu(), o32), "%d->%d stride %d: %d cells differ" % (Cin, Cout, stride, int((out.cpu() != o32).sum()))
    c = dict(x=_ints(rs, (2, 64, 27, 43)), w=_pow2(rs, (64, 64, 3, 3), wvals), scale=_pow2(rs, 64, (0.5, 1.0, 2.0)),
             shift=_ints(rs, 64, -2, 2), stride=1, residual=_ints(rs, (2, 64, 54, 87)), residual_pooled=True)
    o32, o64 = D.conv3x3_oracle(c, torch.float32), D.conv3x3_oracle(c, torch.float64)
    assert torch.equal(o32.double(), o64) and float(o32.max()) > 30
    out = ops.dla_conv3x3(*(_cuda(c[k]) for k in ("x", "w", "scale", "shift")), 1, _cuda(c["residual"]), True, residual_pooled=True,
                          operands=S16)
    assert torch.equal(out.cpu(), o32), "pooled residual: %d cells differ" % int((out.cpu() != o32).sum())


@pytest.mark.gpu
def test_split_does_not_depend_on_the_magnitude():
    """x * 2^k with scale * 2^-k, k in {-40, 0, 40}: each run meets bounds A and B against oracles on the same scaled data.
    The three outputs are bit-identical, and that is asserted: the bf16 parts of x * 2^k are the parts of x times 2^k (a power
    of two moves no mantissa bit and nothing here comes near the ends of the exponent range), so every product and every
    fp32 partial sum is its k = 0 value times 2^k, and scale * 2^-k takes the factor out exactly."""
    import siammot_amd.ops as ops
    c0, _ = _conv3_ref(64, 64, 1, (13, 21), 1)
    outs = []
    for k in (-40, 0, 40):
        c = dict(c0, x=c0["x"] * D.F32(2.0 ** k), scale=c0["scale"] * D.F32(2.0 ** -k))
        o64, o32 = D.conv3x3_oracle(c, torch.float64), D.conv3x3_oracle(c, torch.float32)
        ch = D.channel_scale(D.conv3x3_oracle(c, torch.float64, pre=True))
        args = tuple(_cuda(c[n]) for n in ("x", "w", "scale", "shift")) + (1, _cuda(c["residual"]), True)
        out = ops.dla_conv3x3(*args, operands=S16)
        _check_bounds("split conv3x3 64->64 with x * 2^%d" % k, out, ops.dla_conv3x3(*args), o64, o32, ch)
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[2]), _bits(outs[1]))


@pytest.mark.gpu
def test_split_non_finite_cells_stay_local():
    """One inf and one NaN cell in image 0 of two: the outputs whose 3x3 window covers one are non-finite (NaN also where
    the fp32 kernel gives inf: inf - inf appears in the split), every other output and all of image 1 are the bits of the run
    with the two cells set to 0."""
    import siammot_amd.ops as ops
    c0 = D.conv3x3_case(64, 64, 1, (13, 21), 2)
    x = c0["x"].copy()
    bad = [(3, 5, 7), (40, 0, 20)]                               # an interior cell; the first row's last column
    x[0, 3, 5, 7], x[0, 40, 0, 20] = np.inf, np.nan
    clean = x.copy()
    for ch, y, col in bad:
        clean[0, ch, y, col] = 0.0
    hit = torch.zeros((2, 64, 13, 21), dtype=torch.bool)
    for _, y, col in bad:
        hit[0, :, max(y - 1, 0):y + 2, max(col - 1, 0):col + 2] = True
    w, scale, shift, res = (_cuda(c0[k]) for k in ("w", "scale", "shift", "residual"))
    for relu in (False, True):
        out = ops.dla_conv3x3(_cuda(x), w, scale, shift, 1, res, relu, operands=S16).cpu()
        want = ops.dla_conv3x3(_cuda(clean), w, scale, shift, 1, res, relu, operands=S16).cpu()
        assert bool(torch.isfinite(want).all()) and int(hit.sum()) == 64 * (9 + 4)
        assert not bool(torch.isfinite(out[hit]).any())
        assert torch.equal(_bits(out)[~hit], _bits(want)[~hit])


@pytest.mark.gpu
def test_split_raw_call_with_an_unsupported_shape_launches_nothing():
    import siammot_amd.ops as ops
    lib = ops.load_library()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for Cin, want in ((48, -2), (64, 0)):
        x, w = torch.ones((1, Cin, 8, 8), device="cuda"), torch.ones((32, Cin, 3, 3), device="cuda")
        scale = torch.ones(32, device="cuda")
        out = torch.full((1, 32, 8, 8), -7.0, device="cuda")
        n = lib.smot_dla_conv_split_packed_floats(3, Cin, 32)
        assert (n == -1) == (want != 0)
        packed = torch.full((max(n, lib.smot_dla_conv_packed_floats(3, Cin, 32)),), -7.0, device="cuda")
        rc = lib.smot_dla_conv3x3_split_fwd(vp(x), 1, Cin, 8, 8, vp(w), vp(scale), vp(scale), 32, 1, None, 0, 0, 1, vp(packed), vp(out),
                                            stream)
        torch.cuda.synchronize()
        assert rc == want, (Cin, rc)
        if want:                                                 # SMOT_ERR_UNSUPPORTED: output and packed buffer untouched
            assert float(out.min()) == float(out.max()) == -7.0 and float(packed.min()) == float(packed.max()) == -7.0
        else:                                                    # an interior cell: 9 * 64 ones, + 1
            assert float(out[0, 0, 4, 4]) == 9 * 64 + 1.0
    with pytest.raises(RuntimeError, match="Cin = 48|code -2"):
        ops.dla_conv3x3(torch.ones((1, 48, 8, 8), device="cuda"), torch.ones((32, 48, 3, 3), device="cuda"), scale, scale, 1, operands=S16)


# ---- GPU, network level -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_split_dla_against_the_reference_golden(case):
    """The bound of fp32 mode: 4 x the reference's own fp32 error per stage.  Measured ratios: INTEGRATION.md §3n."""
    import siammot_amd.ops as ops
    g = D.golden(case)
    model, x = _net(case, "cuda", operands=S16)
    fp32, _ = _net(case, "cuda")
    before = ops.FALLBACKS["dla_torch"]
    with torch.no_grad():
        out, o32 = model(x.cuda()), fp32(x.cuda())
    assert ops.FALLBACKS["dla_torch"] == before
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [w.shape for w in g["o64"]]
    assert all(o.dtype is torch.float32 and o.is_contiguous() for o in out)
    err, err32 = D.stage_error(out, g["o64"]), D.stage_error(o32, g["o64"])
    print("dla case %s on the device: error / e32 per stage: split16 %s, fp32 %s"
          % (case, ["%.2f" % (e / b) for e, b in zip(err, g["e32"])], ["%.2f" % (e / b) for e, b in zip(err32, g["e32"])]))
    assert not _equal_bits(out, o32)                             # (another kernel ran)
    for k, (e, b) in enumerate(zip(err, g["e32"])):
        assert e <= 4 * b, "stage %d: %.3e against e32 %.3e" % (k + 2, e, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A", "C"])
def test_split_images_half_images_and_half_outputs(case):
    levels, channels, shape = D.NET_CASES[case]
    model, _ = _net(case, "cuda", operands=S16)
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
            half, _ = _net(case, "cuda", operands=S16, out_dtype=dtype)
            got = half(x)
            assert all(o.dtype is dtype and o.is_contiguous() for o in got)
            assert _equal_bits(got, [o.to(dtype) for o in out])  # rounded once: the next stage read the fp32 value


@pytest.mark.gpu
def test_split_a_changed_buffer_is_packed_again():
    model, x = _net("A", "cuda", operands=S16)
    x = x.cuda()
    with torch.no_grad():
        a = [o.clone() for o in model(x)]
        model.level4.tree1.tree1.bn1.running_var.mul_(4.0)       # the BN of a split 3x3: x4 and x5 change, x2 and x3 do not
        b = [o.clone() for o in model(x)]
        assert _equal_bits(a[:2], b[:2]) and not torch.equal(a[2], b[2]) and not torch.equal(a[3], b[3])
        model.operands = "fp32"                                  # the cache key holds the mode: packed again, the fp32 image
        fp32, _ = _net("A", "cuda")
        fp32.load_state_dict(model.state_dict())
        assert _equal_bits(model(x), fp32(x))


@pytest.mark.gpu
def test_split_backbone_frames_to_detections_with_one_host_copy():
    """``DetectionHead.forward_images`` over a split-mode body: one host copy, detections come back.  The counts are printed
    beside fp32 mode's and NOT asserted equal: a score within rounding of a threshold may fall on the other side."""
    import fpn_cases as P
    import rpn_proposal_cases as R
    import siammot_amd.ops as ops
    from siammot_amd.backbone import build_backbone
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.config import get_default_cfg
    from siammot_amd.detector import build_detection_head
    C, N, size = 128, 2, (96, 64)
    cfg = get_default_cfg(channels=C)
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    counts = {}
    for mode in ("fp32", S16):
        torch.manual_seed(5)
        det = build_detection_head(cfg, BoxCoder(R.WEIGHTS), C, backbone=build_backbone(cfg, operands=mode)).to("cuda").eval()
        H.load_head(det.rpn_head, H.params(C, 3, seed=1), "cuda")
        P.load_fpn(det.backbone.fpn, P.params(C, P.DLA, seed=2), "cuda")
        D.load(det.backbone.body, D.params(det.backbone.body, D.SEED), "cuda")
        with torch.no_grad():
            det.box_head.predictor.bbox_pred.weight.mul_(0.02)
            det.box_head.predictor.cls_score.weight.mul_(4.0)
        assert det.backbone.body.operands == mode
        images = torch.from_numpy(D.image((64, 96), 9, N=N)).cuda()
        with torch.no_grad():
            det.forward_images(images, size)                     # (workspaces, the packed weights, the anchors)
        before = dict(ops.FALLBACKS)
        (feats, got), syncs = H.count_syncs(lambda: det.forward_images(images, size))
        assert dict(ops.FALLBACKS) == before
        assert len(syncs) == 1, "expected ONE device->host copy, saw %d: %s" % (len(syncs), [str(s.message)[:80] for s in syncs])
        assert len(feats) == 5 and len(got) == N and all(len(a) > 0 for a in got)
        counts[mode] = [len(a) for a in got]
    print("forward_images N=%d: detections fp32 %s, split16 %s" % (N, counts["fp32"], counts[S16]))
