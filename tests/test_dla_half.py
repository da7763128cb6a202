"""The DLA bodies' opt-in half compute mode ``compute_dtype=torch.float16 | torch.bfloat16`` (siammot_amd.dla.DLA, ops.dla_half /
dla_half_pack / dla_conv3x3_half / dla_conv3x3_half_form / dla_conv1x1_half / dla_conv1x1_half_form; csrc/dla.hip
dla_conv3x3_half_kernel, dla_conv1x1_half_kernel, csrc/conv3x3_mfma.h cvh_block): every tree convolution
with operands rounded to the compute type on v_mfma_f32_16x16x32_f16 / _bf16, exact products, fp32 accumulation.

CPU: the new symbols, the constructor's keyword, the unchanged ``state_dict`` and CPU results, the builders, the forms.
GPU, operator level: the oracles of tests/dla_cases.py / dla_bottleneck_cases.py in fp64 on the case with input and filters
first rounded by ``.to(compute_dtype).float()`` — kernel and oracle then differ in fp32 summation order alone, so the bound is
the project's own for such a pair, 1e-4 of the per-channel scale (tests/test_dla.py); exactness with integer data; non-finite
cells; the fp16 range; powers of two; images of a call; refusals through the raw call.
GPU, network level: ``e_half <= 2 e_emul`` per stage against the goldens, with e_emul the error of the rounded-operand torch
comparator (dla_half_cases.emulate); the half path ran; batch and dtype variants; repacking; frames to detections.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dla_bottleneck_cases as B
import dla_cases as D
import dla_half_cases as C
import rpn_head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smot_dla_half_packed_floats", "smot_dla_half_pack", "smot_dla_half_fwd", "smot_dla_conv_half_packed_floats",
               "smot_dla_conv3x3_half_fwd", "smot_dla_conv3x3_half_form", "smot_dla_conv1x1_half_fwd", "smot_dla_conv1x1_half_form")
TYPES = sorted(C.TYPES)
_cache = {}


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
    assert ops.ABI_VERSION == 14 and ops.DLA_OPERANDS == ("fp32", "split16")
    assert ops.DLA_COMPUTE_TYPES == (torch.float16, torch.bfloat16)
    for fn in ("dla_half_pack", "dla_half", "dla_conv3x3_half", "dla_conv3x3_half_form", "dla_conv1x1_half"):
        assert callable(getattr(ops, fn)), fn


def test_the_mode_is_a_keyword_only_argument_and_leaves_the_state_dict_alone():
    from siammot_amd.dla import DLA, dla_34, dla_46_c, dla_169
    for make, keys in ((dla_34, 195), (dla_46_c, 245), (dla_169, 875)):
        model = make(compute_dtype=torch.float16)
        assert model.compute_dtype is torch.float16 and make().compute_dtype is None and model.operands == "fp32"
        assert list(model.state_dict().keys()) == list(make().state_dict().keys()) and len(model.state_dict()) == keys
    with pytest.raises(TypeError):
        DLA(D.DLA34[0], D.DLA34[1], torch.float32, "fp32", "basic", False, torch.float16)    # not positional
    for bad in (torch.float32, torch.float64, torch.int8, "fp16", 1):
        with pytest.raises(ValueError, match="compute_dtype"):
            DLA(*D.DLA34, compute_dtype=bad)
    for ct in C.TYPES.values():
        with pytest.raises(ValueError, match="split16"):
            DLA(*D.DLA34, operands="split16", compute_dtype=ct)
        assert DLA(*D.DLA34, compute_dtype=ct, block="bottleneck", residual_root=True).compute_dtype is ct


def test_the_builders_carry_the_mode():
    from siammot_amd import dla as M
    from siammot_amd.backbone import build_backbone
    from siammot_amd.config import get_default_cfg
    cfg = get_default_cfg(channels=128)
    assert M.build_dla(cfg).compute_dtype is None and build_backbone(cfg).body.compute_dtype is None
    for ct in C.TYPES.values():
        assert M.build_dla(cfg, compute_dtype=ct).compute_dtype is ct
        assert build_backbone(cfg, compute_dtype=ct).body.compute_dtype is ct
        for make in (M.dla_34, M.dla_46_c, M.dla_60, M.dla_102, M.dla_169):
            assert make(compute_dtype=ct).compute_dtype is ct
    with pytest.raises(ValueError, match="compute_dtype"):
        build_backbone(cfg, compute_dtype=torch.float32)
    with pytest.raises(ValueError, match="split16"):
        build_backbone(cfg, operands="split16", compute_dtype=torch.float16)


@pytest.mark.parametrize("case", ["A", "F"])
@pytest.mark.parametrize("ct", TYPES)
def test_cpu_tensors_give_the_bits_of_fp32_mode(case, ct):
    import siammot_amd.ops as ops
    a, x, _ = C.net(case)
    b, _, _ = C.net(case, compute_dtype=C.TYPES[ct])
    before = ops.FALLBACKS["dla_torch"]
    with torch.no_grad():
        want = a(x)
        assert _equal_bits(want, b(x))
        half, _, _ = C.net(case, compute_dtype=C.TYPES[ct], out_dtype=torch.bfloat16)
        assert _equal_bits(half(x), [o.to(torch.bfloat16) for o in want])
    assert ops.FALLBACKS["dla_torch"] == before                  # counted for device tensors only


def test_half_forms_reach_every_form():
    """The cases of CONV3 and FORMS together run every form the half launch site has, and CONV1 + CONV1_WIDE both forms of
    the 1x1 kernel (a retune must keep that)."""
    import siammot_amd.ops as ops
    seen = set()
    for Cin, Cout, stride, size in C.CONV3:
        seen |= {(stride,) + ops.dla_conv3x3_half_form(N, size[0], size[1], Cout, stride) for N in (1, 3)}
    for Cin, Cout, stride, size, N, form in C.FORMS:
        seen |= {(stride,) + ops.dla_conv3x3_half_form(n, size[0], size[1], Cout, stride) for n in (1, N)}
    assert seen == C.ALL_FORMS, seen
    assert {ops.dla_conv1x1_half_form(N, size[0], size[1], Cout) for _, Cout, size, _, _ in C.CONV1 for N in (1, 3)} == {2}
    _, Cout, size, _, _ = C.CONV1_WIDE
    assert ops.dla_conv1x1_half_form(1, size[0], size[1], Cout) == 4 and (Cout // 16) % 4 != 0     # with an M-block tail


# ---- GPU, operator level: 3x3 -------------------------------------------------------------------------------------------
def _conv3_ref(ct, Cin, Cout, stride, size, N, pooled=False):
    """The case and, per (residual, relu): the fp64 oracle on the rounded case and the per-channel scale.  Computed once."""
    key = ("c3", ct, Cin, Cout, stride, size, N, pooled)
    if key not in _cache:
        c = D.conv3x3_case(Cin, Cout, stride, size, N)
        if pooled:
            rs = np.random.RandomState(31)
            c = dict(c, residual=(rs.standard_normal((N, Cout, 2 * size[0] + 1, 2 * size[1] + 1)) * 4.0).astype(D.F32),
                     residual_pooled=True)
        r, ref = C.rounded3(c, C.TYPES[ct]), {}
        for residual in ((True,) if pooled else (False, True)):
            ch = D.channel_scale(D.conv3x3_oracle(r, torch.float64, residual, pre=True))
            for relu in (False, True):
                ref[(residual, relu)] = (D.conv3x3_oracle(r, torch.float64, residual, relu), ch)
        _cache[key] = (c, ref)
    return _cache[key]


def _check(what, out, o64, ch):
    e = D.scaled_error(out, o64, ch)
    print("%s: %.3e of the channel scale against fp64 on the rounded operands" % (what, e))
    assert out.shape == o64.shape and out.dtype is torch.float32 and out.is_contiguous()
    assert e < 1e-4, what


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,stride,size", C.CONV3)
@pytest.mark.parametrize("ct", TYPES)
def test_half_conv3x3_against_the_cpu_oracle(ct, Cin, Cout, stride, size):
    import siammot_amd.ops as ops
    for N in (1, 3):
        c, ref = _conv3_ref(ct, Cin, Cout, stride, size, N)
        x, w, scale, shift, res = (_cuda(c[k]) for k in ("x", "w", "scale", "shift", "residual"))
        for (residual, relu), (o64, ch) in ref.items():
            out = ops.dla_conv3x3_half(x, w, scale, shift, stride, C.TYPES[ct], res if residual else None, relu)
            _check("half conv3x3 %s %d->%d stride %d %s N=%d residual=%d relu=%d" % (ct, Cin, Cout, stride, size, N, residual, relu),
                   out, o64, ch)
            if N == 3:                                           # each image is the one-image call, bit for bit
                for i in range(N):
                    one = ops.dla_conv3x3_half(x[i:i + 1], w, scale, shift, stride, C.TYPES[ct], res[i:i + 1] if residual else None, relu)
                    assert torch.equal(_bits(one), _bits(out[i:i + 1])), "image %d" % i


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_half_conv3x3_with_the_pooled_residual(ct):
    import siammot_amd.ops as ops
    c, ref = _conv3_ref(ct, 64, 64, 1, (13, 21), 3, pooled=True)
    assert c["residual"].shape == (3, 64, 27, 43)
    x, w, scale, shift, res = (_cuda(c[k]) for k in ("x", "w", "scale", "shift", "residual"))
    for (_, relu), (o64, ch) in ref.items():
        out = ops.dla_conv3x3_half(x, w, scale, shift, 1, C.TYPES[ct], res, relu, residual_pooled=True)
        _check("half conv3x3 %s 64->64 pooled residual relu=%d" % (ct, relu), out, o64, ch)
        for i in range(3):
            one = ops.dla_conv3x3_half(x[i:i + 1], w, scale, shift, 1, C.TYPES[ct], res[i:i + 1], relu, residual_pooled=True)
            assert torch.equal(_bits(one), _bits(out[i:i + 1])), "image %d" % i


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,stride,size,N,form", C.FORMS)
@pytest.mark.parametrize("ct", TYPES)
def test_half_conv3x3_forms(ct, Cin, Cout, stride, size, N, form):
    """The large call runs ``form``, its images alone run (4, .), and both give the same bits."""
    import siammot_amd.ops as ops
    assert ops.dla_conv3x3_half_form(N, size[0], size[1], Cout, stride) == form
    assert ops.dla_conv3x3_half_form(1, size[0], size[1], Cout, stride) == (4, form[1])
    c = D.conv3x3_case(Cin, Cout, stride, size, N)
    r = C.rounded3(c, C.TYPES[ct])
    x, w, scale, shift, res = (_cuda(c[k]) for k in ("x", "w", "scale", "shift", "residual"))
    out = ops.dla_conv3x3_half(x, w, scale, shift, stride, C.TYPES[ct], res, True)
    _check("half conv3x3 %s form %s: %d->%d stride %d %s N=%d" % (ct, form, Cin, Cout, stride, size, N), out,
           D.conv3x3_oracle(r, torch.float64), D.channel_scale(D.conv3x3_oracle(r, torch.float64, pre=True)))
    for i in range(N):
        one = ops.dla_conv3x3_half(x[i:i + 1], w, scale, shift, stride, C.TYPES[ct], res[i:i + 1], True)
        assert torch.equal(_bits(one), _bits(out[i:i + 1])), "image %d" % i


# ---- GPU, operator level: 1x1 -------------------------------------------------------------------------------------------
def _conv1_case(sources, Cout, size, N, residual):
    return B.conv1x1_res_case(C.sources_of(sources, size), Cout, size, N, residual)


def _conv1_call(ops, c, ct, relu, images=None, **kw):
    """``ops.dla_conv1x1_half`` on the (unrounded) case; a residual that is source 0 is passed as that very tensor."""
    pick = (lambda a: a) if images is None else (lambda a: a[images])
    src = [_cuda(pick(s)) for s in c["src"]]
    res = None if c["residual"] is None else (src[0] if c["residual"] is c["src"][0] else _cuda(pick(c["residual"])))
    return ops.dla_conv1x1_half(src, c["pooled"], _cuda(c["w"]), _cuda(c["scale"]), _cuda(c["shift"]), relu, C.TYPES[ct],
                                residual=res, residual_pooled=c["residual_pooled"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("sources,Cout,size,relu,residual", C.CONV1 + [C.CONV1_WIDE])
@pytest.mark.parametrize("ct", TYPES)
def test_half_conv1x1_against_the_cpu_oracle(ct, sources, Cout, size, relu, residual):
    import siammot_amd.ops as ops
    for N in (1, 3):
        c = _conv1_case(sources, Cout, size, N, residual)
        r = C.rounded1(c, C.TYPES[ct])
        o64 = B.conv1x1_res_oracle(r, torch.float64, relu)
        ch = D.channel_scale(B.conv1x1_res_oracle(r, torch.float64, pre=True))
        out = _conv1_call(ops, c, ct, relu)
        _check("half conv1x1 %s %d sources -> %d %s N=%d %s relu=%d (form %d)"
               % (ct, len(sources), Cout, size, N, residual, relu, ops.dla_conv1x1_half_form(N, size[0], size[1], Cout)), out, o64, ch)
        if N == 3:
            for i in range(N):                                   # image i of the call: the bits of its one-image call
                assert torch.equal(_bits(_conv1_call(ops, c, ct, relu, images=slice(i, i + 1))), _bits(out[i:i + 1])), "image %d" % i
            for dtype in (torch.float16, torch.bfloat16):        # a half output: the fp32 result rounded once
                half = _conv1_call(ops, c, ct, relu, out_dtype=dtype)
                assert half.dtype is dtype and torch.equal(_bits(half), _bits(out.to(dtype)))


# ---- exact with integer data --------------------------------------------------------------------------------------------
def _ints(rs, shape, lo=-8, hi=8):
    return rs.randint(lo, hi + 1, size=shape).astype(D.F32)


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_half_exact_with_integer_data(ct):
    """Inputs and filters are integers in [-8, 8]: both types hold them exactly, every product is an integer <= 64 and every
    partial sum is below 64 * 9 * 96 < 2^24, exact in fp32 in any order; scale 1, shift 0, no ReLU.  The output equals torch's
    fp32 convolution bit for bit: a dropped, duplicated or misplaced K slice, tap or source cannot pass."""
    import siammot_amd.ops as ops
    rs = np.random.RandomState(41)
    dt = C.TYPES[ct]
    for Cin, Cout, stride, size in ((96, 96, 2, (25, 41)), (64, 64, 1, (13, 21)), (32, 32, 2, (17, 35)), (32, 64, 1, (9, 19))):
        c = dict(x=_ints(rs, (2, Cin) + size), w=_ints(rs, (Cout, Cin, 3, 3)), scale=np.ones(Cout, D.F32), shift=np.zeros(Cout, D.F32),
                 stride=stride)
        o32, o64 = D.conv3x3_oracle(c, torch.float32, False, False), D.conv3x3_oracle(c, torch.float64, False, False)
        assert torch.equal(o32.double(), o64) and float(o32.abs().max()) > 1000
        out = ops.dla_conv3x3_half(*(_cuda(c[k]) for k in ("x", "w", "scale", "shift")), stride, dt, None, False)
        assert torch.equal(out.cpu(), o32), "3x3 %d->%d stride %d: %d cells differ" % (Cin, Cout, stride, int((out.cpu() != o32).sum()))
    for sources, Cout, size in (([(64, True), (32, False), (96, False), (32, True)], 96, (9, 13)), ([(32, False)] * 8, 64, (5, 7)),
                                ([(32, True)], 160, (75, 75))):
        N = 1 if size[0] > 50 else 2
        c = dict(src=[_ints(rs, (N, ch) + ((2 * size[0] + 1, 2 * size[1] + 1) if p else size)) for ch, p in sources],
                 pooled=[p for _, p in sources], w=_ints(rs, (Cout, sum(ch for ch, _ in sources), 1, 1)),
                 scale=np.ones(Cout, D.F32), shift=np.zeros(Cout, D.F32), residual=None, residual_pooled=False)
        o32, o64 = B.conv1x1_res_oracle(c, torch.float32, False), B.conv1x1_res_oracle(c, torch.float64, False)
        assert torch.equal(o32.double(), o64) and float(o32.abs().max()) > 300
        out = _conv1_call(ops, c, ct, False)
        assert torch.equal(out.cpu(), o32), "1x1 %s -> %d: %d cells differ" % (sources, Cout, int((out.cpu() != o32).sum()))


# ---- non-finite cells, range, powers of two -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_half_non_finite_cells_stay_local_3x3(ct):
    """One inf and one NaN cell in image 0 of two: exactly the outputs whose 3x3 window covers one are non-finite (+-inf around
    the inf cell — an inf operand times a finite filter value, where -inf is 0 behind a ReLU — and NaN around the NaN cell),
    every other output and all of image 1 keep the bits of the run with the two cells set to 0."""
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
        out = ops.dla_conv3x3_half(_cuda(x), w, scale, shift, 1, C.TYPES[ct], res, relu).cpu()
        want = ops.dla_conv3x3_half(_cuda(clean), w, scale, shift, 1, C.TYPES[ct], res, relu).cpu()
        assert bool(torch.isfinite(want).all()) and int(hit.sum()) == 64 * (9 + 4)
        assert torch.equal(_bits(out)[~hit], _bits(want)[~hit])
        assert bool(torch.isnan(out[0, :, 0:2, 19:21]).all())    # the NaN cell's window
        near = out[0, :, 4:7, 6:9]                               # the inf cell's window: +-inf, and -inf is 0 behind the ReLU
        if relu:
            assert bool(((near == np.inf) | (near == 0)).all()) and bool((near == np.inf).any()) and bool((near == 0).any())
        else:
            assert bool(torch.isinf(near).all())


@pytest.mark.gpu
@pytest.mark.parametrize("sources,Cout,size,residual", [([(64, True), (32, False), (32, False)], 96, (9, 13), "plain"),
                                                         ([(32, False)], 160, (75, 75), None)])
@pytest.mark.parametrize("ct", TYPES)
def test_half_non_finite_cells_stay_local_1x1(ct, sources, Cout, size, residual):
    """An inf cell in the first source (for a pooled source: inside one pool window) and a NaN cell in the last one: only
    those two positions of image 0 are non-finite, in every channel; all other outputs — the last, partial tile's live
    positions, the M-block tail's channels, image 1 — keep the bits of the clean call."""
    import siammot_amd.ops as ops
    c0 = _conv1_case(sources, Cout, size, 2, residual)
    c = dict(c0, src=[s.copy() for s in c0["src"]])
    c["residual"] = c0["residual"]
    py, px = size[0] - 1, size[1] - 1                            # the last position of the map: in the last tile
    if sources[0][1]:
        c["src"][0][0, 5, 2 * 2 + 1, 2 * 3] = np.inf             # window of output (2, 3)
    else:
        c["src"][0][0, 5, 2, 3] = np.inf
    if sources[-1][1]:
        c["src"][-1][0, 17, 2 * py, 2 * px + 1] = np.nan
    else:
        c["src"][-1][0, 17, py, px] = np.nan
    hit = torch.zeros((2, Cout) + tuple(size), dtype=torch.bool)
    hit[0, :, 2, 3] = True
    hit[0, :, py, px] = True
    out, want = _conv1_call(ops, c, ct, False).cpu(), _conv1_call(ops, c0, ct, False).cpu()
    assert bool(torch.isfinite(want).all())
    assert torch.equal(~torch.isfinite(out), hit), int((~torch.isfinite(out)).sum())
    assert bool(torch.isnan(out[0, :, py, px]).all()) and bool(torch.isinf(out[0, :, 2, 3]).all())
    assert torch.equal(_bits(out)[~hit], _bits(want)[~hit])


@pytest.mark.gpu
def test_half_range_of_fp16_and_bf16():
    """An input cell of 1e5: fp16 rounds it to +inf, so the outputs that read it are +-inf (NaN where a zero filter tap meets
    it: none here) exactly where the rounded-operand oracle's are; bf16 holds it and every output is finite and within the
    bound.  (The per-channel scale of the bound is the case's own; in fp16 mode, where that is inf, the clean case's: the finite
    outputs do not read the cell.)"""
    import siammot_amd.ops as ops
    c0 = D.conv3x3_case(64, 64, 1, (13, 21), 1)
    x = c0["x"].copy()
    x[0, 9, 6, 11] = 1e5
    c = dict(c0, x=x)
    k0 = _conv1_case([(32, False), (32, False)], 96, (9, 13), 1, None)
    k = dict(k0, src=[s.copy() for s in k0["src"]])
    k["src"][1][0, 4, 3, 8] = -1e5
    for ct in TYPES:
        dt = C.TYPES[ct]
        r = C.rounded3(c, dt)
        o32 = D.conv3x3_oracle(r, torch.float32, False, False)
        out = ops.dla_conv3x3_half(*(_cuda(c[n]) for n in ("x", "w", "scale", "shift")), 1, dt, None, False).cpu()
        assert torch.equal(torch.isinf(out), torch.isinf(o32)) and not bool(torch.isnan(out).any())
        assert int(torch.isinf(out).sum()) == (64 * 9 if ct == "fp16" else 0)
        if ct == "fp16":
            assert torch.equal(out[torch.isinf(out)], o32[torch.isinf(o32)])                     # the signs
        _check("half conv3x3 %s with a cell of 1e5" % ct, out, D.conv3x3_oracle(r, torch.float64, False, False),
               D.channel_scale(D.conv3x3_oracle(C.rounded3(c0 if ct == "fp16" else c, dt), torch.float64, False, pre=True)))
        rk = C.rounded1(k, dt)
        p32 = B.conv1x1_res_oracle(rk, torch.float32, False)
        got = _conv1_call(ops, k, ct, False).cpu()
        assert torch.equal(torch.isinf(got), torch.isinf(p32)) and not bool(torch.isnan(got).any())
        assert int(torch.isinf(got).sum()) == (96 if ct == "fp16" else 0)
        if ct == "fp16":
            assert torch.equal(got[torch.isinf(got)], p32[torch.isinf(p32)])
        _check("half conv1x1 %s with a cell of -1e5" % ct, got, B.conv1x1_res_oracle(rk, torch.float64, False),
               D.channel_scale(B.conv1x1_res_oracle(C.rounded1(k0 if ct == "fp16" else k, dt), torch.float64, pre=True)))


@pytest.mark.gpu
@pytest.mark.parametrize("ct,ks", [("fp16", (-2, 0, 8)), ("bf16", (-40, 0, 40))])
def test_half_powers_of_two_move_no_bit(ct, ks):
    """``x * 2^-k`` with ``scale * 2^k``: |x| in [1, 16), so x * 2^-k stays inside the type's normal range for these k and
    rounds to the rounding of x times 2^-k; every product and fp32 partial sum is its k = 0 value times 2^-k and the scale
    takes the factor out exactly: the three outputs have the same bits."""
    import siammot_amd.ops as ops
    rs = np.random.RandomState(53)
    c0 = D.conv3x3_case(64, 64, 2, (13, 21), 1)
    c0 = dict(c0, x=(rs.uniform(1.0, 16.0, size=c0["x"].shape) * rs.choice([-1.0, 1.0], size=c0["x"].shape)).astype(D.F32))
    k0 = _conv1_case([(64, True), (32, False)], 96, (9, 13), 1, None)
    k0 = dict(k0, src=[(rs.uniform(1.0, 16.0, size=s.shape) * rs.choice([-1.0, 1.0], size=s.shape)).astype(D.F32) for s in k0["src"]])
    outs3, outs1 = [], []
    for k in ks:
        f, g = D.F32(2.0 ** -k), D.F32(2.0 ** k)
        c = dict(c0, x=c0["x"] * f, scale=c0["scale"] * g)
        outs3.append(ops.dla_conv3x3_half(*(_cuda(c[n]) for n in ("x", "w", "scale", "shift")), 2, C.TYPES[ct], None, True))
        kk = dict(k0, src=[s * f for s in k0["src"]], scale=k0["scale"] * g)
        outs1.append(_conv1_call(ops, kk, ct, True))
    for outs in (outs3, outs1):
        assert float(outs[1].abs().max()) > 1 and bool(torch.isfinite(outs[1]).all())
        assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[2]), _bits(outs[1]))


# ---- refusals through the raw call --------------------------------------------------------------------------------------
def _raw_conv1x1_half(channels, ctype, Cout=32, H=4, W=4):
    """``smot_dla_conv1x1_half_fwd`` on valid buffers -> (code, output, packed); both buffers pre-filled with -7."""
    import siammot_amd.ops as ops
    lib = ops.load_library()
    S = len(channels)
    src = [torch.ones((1, c, H, W), device="cuda") for c in channels]
    K = sum(channels)
    w, scale = torch.ones((Cout, K), device="cuda"), torch.ones(Cout, device="cuda")
    packed, out = torch.full((Cout * K + 2 * Cout + 4,), -7.0, device="cuda"), torch.full((1, Cout, H, W), -7.0, device="cuda")
    arr = lambda vals: (ctypes.c_int * S)(*vals)
    sp = (ctypes.c_void_p * S)(*[t.data_ptr() for t in src])
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.smot_dla_conv1x1_half_fwd(sp, arr(channels), arr([0] * S), arr([H] * S), arr([W] * S), S, 1, H, W, vp(w), vp(scale),
                                       vp(scale), Cout, 0, None, 0, 0, ctype, vp(packed), vp(out), 0,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out, packed


@pytest.mark.gpu
def test_half_raw_calls_refuse_what_the_header_says_and_launch_nothing():
    import siammot_amd.ops as ops
    lib = ops.load_library()
    last_error = lambda: lib.smot_last_error().decode("utf-8", "replace")
    untouched = lambda *ts: all(float(t.min()) == float(t.max()) == -7.0 for t in ts)
    for channels, ctype, want in (([32, 16], 1, -2), ([48], 2, -2), ([32, 48, 32], 1, -2), ([32] * 9, 1, -1), ([32], 0, -1), ([32], 3, -1),
                                  ([32, 32], 1, 0), ([32, 32], 2, 0)):
        rc, out, packed = _raw_conv1x1_half(channels, ctype)
        assert rc == want, (channels, ctype, rc)
        if want:
            assert untouched(out, packed), (channels, ctype)
            if want == -2:
                bad = [c for c in channels if c % 32][0]
                assert ("%d channels" % bad) in last_error(), last_error()
        else:
            assert float(out.min()) == float(out.max()) == 64 + 1.0
    assert lib.smot_dla_conv_half_packed_floats(1, 48, 32) == -1 and lib.smot_dla_conv_half_packed_floats(3, 48, 32) == -1
    assert lib.smot_dla_conv_half_packed_floats(1, 64, 32) == 64 * 32 // 2 + 64
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for Cin, ctype, want in ((48, 1, -2), (64, 0, -1), (64, 7, -1), (64, 1, 0), (64, 2, 0)):
        x, w = torch.ones((1, Cin, 8, 8), device="cuda"), torch.ones((32, Cin, 3, 3), device="cuda")
        scale = torch.ones(32, device="cuda")
        out = torch.full((1, 32, 8, 8), -7.0, device="cuda")
        packed = torch.full((lib.smot_dla_conv_packed_floats(3, Cin, 32),), -7.0, device="cuda")
        rc = lib.smot_dla_conv3x3_half_fwd(vp(x), 1, Cin, 8, 8, vp(w), vp(scale), vp(scale), 32, 1, None, 0, 0, 1, ctype, vp(packed),
                                           vp(out), stream)
        torch.cuda.synchronize()
        assert rc == want, (Cin, ctype, rc)
        if want:
            assert untouched(out, packed)
            assert want != -2 or "Cin = 48" in last_error()
        else:                                                    # an interior cell: 9 * 64 ones, + 1
            assert float(out[0, 0, 4, 4]) == 9 * 64 + 1.0
    arr = lambda v: (ctypes.c_int * 6)(*v)
    levels, channels, _ = D.NET_CASES["A"]
    assert lib.smot_dla_half_packed_floats(arr(levels), arr(channels), 0, 0, 0) == -1
    assert lib.smot_dla_half_packed_floats(arr(levels), arr(channels), 0, 0, 3) == -1
    assert lib.smot_dla_half_packed_floats(arr(levels), arr(channels), 0, 0, 1) == lib.smot_dla_half_packed_floats(arr(levels), arr(channels), 0, 0, 2) > 0
    with pytest.raises(ValueError, match="compute_dtype"):
        ops.dla_conv3x3_half(x, w, scale, scale, 1, torch.float32)


# ---- GPU, network level -------------------------------------------------------------------------------------------------
def _e_emul(case, ct):
    """Per stage the error of the rounded-operand torch comparator against the golden's fp64 maps.  Computed once."""
    if ("emul", case, ct) not in _cache:
        model, x, g = C.net(case)
        with torch.no_grad():
            _cache[("emul", case, ct)] = D.stage_error(C.emulate(model, C.TYPES[ct])(x), g["o64"])
    return _cache[("emul", case, ct)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.NET_CASES)
@pytest.mark.parametrize("ct", TYPES)
def test_half_dla_against_the_rounded_operand_comparator(ct, case):
    """``e_half <= 2 e_emul`` per stage: the device path against the torch composition with every tree convolution's input and
    weight rounded to the compute type, both measured against the golden's fp64 maps; 2 is the project's margin for the same
    operators in another summation order.  The half path ran: other bits than fp32 mode's, no fallback counted.
    Measured ratios e_half / e_emul: profiles/dla_half_parity.md."""
    import siammot_amd.ops as ops
    model, x, g = C.net(case, "cuda", compute_dtype=C.TYPES[ct])
    fp32, _, _ = C.net(case, "cuda")
    before = ops.FALLBACKS["dla_torch"]
    with torch.no_grad():
        out, o32 = model(x.cuda()), fp32(x.cuda())
    assert ops.FALLBACKS["dla_torch"] == before
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [w.shape for w in g["o64"]]
    assert all(o.dtype is torch.float32 and o.is_contiguous() for o in out)
    assert all(not torch.equal(_bits(a), _bits(b)) for a, b in zip(out, o32))                # (the half kernels ran)
    e_half, e_emul, e_k32 = D.stage_error(out, g["o64"]), _e_emul(case, ct), D.stage_error(o32, g["o64"])
    print("PARITY case %s %s: e_half %s e_emul %s ratio %s (fp32 mode's error %s)"
          % (case, ct, ["%.3e" % e for e in e_half], ["%.3e" % e for e in e_emul],
             ["%.2f" % (a / b) for a, b in zip(e_half, e_emul)], ["%.3e" % e for e in e_k32]))
    for k, (a, b) in enumerate(zip(e_half, e_emul)):
        assert a <= 2 * b, "stage %d: e_half %.3e against e_emul %.3e" % (k + 2, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A", "F"])
@pytest.mark.parametrize("ct", TYPES)
def test_half_images_half_images_and_half_outputs(ct, case):
    model, x1, _ = C.net(case, "cuda", compute_dtype=C.TYPES[ct])
    x = torch.from_numpy(D.image(tuple(x1.shape[2:]), 3, N=3)).cuda()
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
            half, _, _ = C.net(case, "cuda", compute_dtype=C.TYPES[ct], out_dtype=dtype)
            got = half(x)
            assert all(o.dtype is dtype and o.is_contiguous() for o in got)
            assert _equal_bits(got, [o.to(dtype) for o in out])  # rounded once: the next stage read the fp32 value


@pytest.mark.gpu
def test_half_a_changed_buffer_is_packed_again_and_modes_do_not_share_an_image():
    model, x, _ = C.net("A", "cuda", compute_dtype=torch.float16)
    x = x.cuda()
    with torch.no_grad():
        a = [o.clone() for o in model(x)]
        model.level4.tree1.tree1.bn1.running_var.mul_(4.0)       # the BN of a tree 3x3: x4 and x5 change, x2 and x3 do not
        b = [o.clone() for o in model(x)]
        assert _equal_bits(a[:2], b[:2]) and not torch.equal(a[2], b[2]) and not torch.equal(a[3], b[3])
        other, _, _ = C.net("A", "cuda", compute_dtype=torch.bfloat16)
        other.load_state_dict(model.state_dict())
        c = [o.clone() for o in other(x)]
        assert not any(torch.equal(p, q) for p, q in zip(b, c))  # two models that differ in compute_dtype alone
        assert other.packed().data_ptr() != model.packed().data_ptr() and other.packed().shape == model.packed().shape
        assert not torch.equal(other.packed(), model.packed())
        model.compute_dtype = torch.bfloat16                     # the cache key holds the type: packed again
        assert _equal_bits(model(x), c)
        model.compute_dtype = None                               # ... and the fp32 image
        fp32, _, _ = C.net("A", "cuda")
        fp32.load_state_dict(model.state_dict())
        assert _equal_bits(model(x), fp32(x))


@pytest.mark.gpu
def test_half_backbone_frames_to_detections_with_one_host_copy():
    """``DetectionHead.forward_images`` over a body in fp16 compute mode on the small frame of the split-mode test: one host
    copy, detections come back.  The counts are printed beside fp32 mode's and not asserted equal."""
    import fpn_cases as P
    import rpn_proposal_cases as R
    import siammot_amd.ops as ops
    from siammot_amd.backbone import build_backbone
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.config import get_default_cfg
    from siammot_amd.detector import build_detection_head
    Cw, N, size = 128, 2, (96, 64)
    cfg = get_default_cfg(channels=Cw)
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    counts = {}
    for mode in (None, torch.float16):
        torch.manual_seed(5)
        det = build_detection_head(cfg, BoxCoder(R.WEIGHTS), Cw, backbone=build_backbone(cfg, compute_dtype=mode)).to("cuda").eval()
        H.load_head(det.rpn_head, H.params(Cw, 3, seed=1), "cuda")
        P.load_fpn(det.backbone.fpn, P.params(Cw, P.DLA, seed=2), "cuda")
        D.load(det.backbone.body, D.params(det.backbone.body, D.SEED), "cuda")
        with torch.no_grad():
            det.box_head.predictor.bbox_pred.weight.mul_(0.02)
            det.box_head.predictor.cls_score.weight.mul_(4.0)
        assert det.backbone.body.compute_dtype is mode
        images = torch.from_numpy(D.image((64, 96), 9, N=N)).cuda()
        with torch.no_grad():
            det.forward_images(images, size)                     # (workspaces, the packed weights, the anchors)
        before = dict(ops.FALLBACKS)
        (feats, got), syncs = H.count_syncs(lambda: det.forward_images(images, size))
        assert dict(ops.FALLBACKS) == before
        assert len(syncs) == 1, "expected ONE device->host copy, saw %d: %s" % (len(syncs), [str(s.message)[:80] for s in syncs])
        assert len(feats) == 5 and len(got) == N and all(len(a) > 0 for a in got)
        counts[mode] = [len(a) for a in got]
    print("forward_images N=%d: detections fp32 %s, fp16 compute %s" % (N, counts[None], counts[torch.float16]))
