"""FPN in half compute mode (siammot_amd.fpn.FPN(compute_dtype=), ops.fpn_half / fpn_half_pack, csrc/fpn.hip:
fpn_lateral_half_kernel, fpn_layer_half_kernel), the builders that carry the mode, and frames ->
detections with everything in half mode.

The mode rounds the stage maps, the fp32 ``last`` maps and both convolutions' filters to fp16 / bf16, multiplies exactly on
the 16-bit matrix instruction and accumulates in fp32.  Two yardsticks (tests/fpn_half_cases.py):

* integer data on which every rounding is the identity and every fp32 sum is exact: the kernel equals the CPU composition bit
  for bit, whatever its sum order;
* general data: against the UNROUNDED fp64 oracle of tests/fpn_cases.py the mode's scaled error is at most TWICE that of the
  CPU comparator ``emulate_fpn`` (weights rounded, inputs rounded through pre-hooks): the project's bound for exactly this
  comparison (tests/test_dla_half.py, profiles/dla_half_parity.md).  Measured ratios: profiles/fpn_half_parity.md.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dla_cases as D
import fpn_cases as P
import fpn_half_cases as K
import rpn_head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smot_fpn_half_packed_floats", "smot_fpn_half_pack", "smot_fpn_half_fwd")
FACTOR = 2.0                                         # e_half <= FACTOR * e_emul (module docstring)
_cache = {}


def _cfg(channels=128):
    from siammot_amd.config import get_default_cfg
    return get_default_cfg(channels=channels)


def _fpn(C, cin, prm, dev="cuda", out_dtype=torch.float32, top=True, **kw):
    from siammot_amd.fpn import FPN, LastLevelMaxPool
    return P.load_fpn(FPN(cin, C, top_blocks=LastLevelMaxPool() if top else None, out_dtype=out_dtype, **kw), prm, dev)


def _reference(C, cin, N, shape, ct):
    """(maps, parameters, unrounded fp64 outputs, per-channel scale, the comparator's outputs and its scaled error) of one
    case: computed once, never modified."""
    base = (C, cin, N, shape)
    if base not in _cache:
        prm, x = P.params(C, cin), P.maps(cin, N, K.FPN_SHAPES[shape])
        o64 = P.oracle(x, prm, torch.float64)
        _cache[base] = dict(prm=prm, x=x, o64=o64, scale=P.channel_scale(o64))
    ref = _cache[base]
    if ct not in ref:
        with torch.no_grad():
            emul = K.emulate_fpn(_fpn(C, cin, ref["prm"], "cpu"), K.TYPES[ct])([torch.from_numpy(v) for v in ref["x"]])
        ref[ct] = dict(emul=emul, e_emul=H.scaled_error(emul, ref["o64"], ref["scale"]))
    return ref


def _dev(levels, dev="cuda"):
    return [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in levels]


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _equal_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_carry_the_new_symbols():
    import siammot_amd.ops as ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smot_emm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smot_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared and name in ops.EXPORTED_SYMBOLS, name
    assert ops.ABI_VERSION == 14 and re.search(r"#define SMOT_ABI_VERSION 14\b", src)
    for fn in (ops.fpn_half_pack, ops.fpn_half):
        assert "compute_dtype" in inspect.signature(fn).parameters
    assert ops.fpn_half_shapes_ok(P.DLA, 128) and ops.fpn_half_shapes_ok((32, 64, 96, 160), 160)
    assert ops.fpn_shapes_ok((48, 16), 64) and not ops.fpn_half_shapes_ok((48, 16), 64)      # a K step is 32 channels
    assert not ops.fpn_half_shapes_ok(P.DLA, 48)


def test_the_keyword_is_keyword_only_validated_and_leaves_the_state_dict_alone():
    from siammot_amd.fpn import FPN, LastLevelMaxPool
    p = inspect.signature(FPN.__init__).parameters["compute_dtype"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    with pytest.raises(TypeError):
        FPN(P.DLA, 128, None, LastLevelMaxPool(), torch.float32, torch.float16)
    for bad in (torch.float32, torch.float64, "bf16", 2):
        with pytest.raises(ValueError, match="compute_dtype"):
            FPN(P.DLA, 128, compute_dtype=bad)
    plain = FPN(P.DLA, 128, top_blocks=LastLevelMaxPool())
    assert plain.compute_dtype is None
    for ct in K.TYPES.values():
        half = FPN(P.DLA, 128, top_blocks=LastLevelMaxPool(), compute_dtype=ct)
        assert half.compute_dtype is ct and list(half.state_dict().keys()) == list(plain.state_dict().keys())


def test_the_builders_carry_the_mode():
    from siammot_amd.backbone import build_backbone
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.detector import build_detection_head
    from siammot_amd.fpn import FPN, build_fpn
    cfg = _cfg(128)
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    assert build_fpn(cfg).compute_dtype is None
    assert "compute_dtype" in inspect.signature(build_detection_head).parameters
    for ct in K.TYPES.values():
        assert build_fpn(cfg, compute_dtype=ct).compute_dtype is ct
        assert build_fpn(cfg, torch.float16, ct).out_dtype is torch.float16
        body_only = build_backbone(cfg, compute_dtype=ct)        # keeps meaning "the body only"
        assert body_only.body.compute_dtype is ct and body_only.fpn.compute_dtype is None
        pyramid_only = build_backbone(cfg, fpn_compute_dtype=ct)
        assert pyramid_only.body.compute_dtype is None and pyramid_only.fpn.compute_dtype is ct
        assert list(pyramid_only.state_dict().keys()) == list(build_backbone(cfg).state_dict().keys())
        det = build_detection_head(cfg, BoxCoder((10.0, 10.0, 5.0, 5.0)), 128, backbone=True, compute_dtype=ct)
        assert det.rpn_head.compute_dtype is ct and det.backbone.body.compute_dtype is ct and det.backbone.fpn.compute_dtype is ct
        det = build_detection_head(cfg, BoxCoder((10.0, 10.0, 5.0, 5.0)), 128, fpn=True, compute_dtype=ct)
        assert det.rpn_head.compute_dtype is ct and det.fpn.compute_dtype is ct
        mine = FPN(P.DLA, 128)                                   # a module passed in is left as it is
        det = build_detection_head(cfg, BoxCoder((10.0, 10.0, 5.0, 5.0)), 128, fpn=mine, compute_dtype=ct)
        assert det.fpn is mine and mine.compute_dtype is None and det.rpn_head.compute_dtype is ct
    det = build_detection_head(cfg, BoxCoder((10.0, 10.0, 5.0, 5.0)), 128, backbone=True)
    assert det.rpn_head.compute_dtype is None and det.backbone.body.compute_dtype is None and det.backbone.fpn.compute_dtype is None
    with pytest.raises(ValueError, match="compute_dtype"):
        build_fpn(cfg, compute_dtype=torch.float32)


@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_cpu_tensors_give_the_bits_of_fp32_mode(ct):
    import siammot_amd.ops as ops
    C, cin = 32, (32, 64)
    prm, x = P.params(C, cin), [torch.from_numpy(v) for v in P.maps(cin, 2, P.TWO)]
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        want = _fpn(C, cin, prm, "cpu")(x)
        got = _fpn(C, cin, prm, "cpu", compute_dtype=K.TYPES[ct])(x)
        got16 = _fpn(C, cin, prm, "cpu", out_dtype=torch.float16, compute_dtype=K.TYPES[ct])(x)
    assert _equal_bits(got, want) and _equal_bits(got16, [o.to(torch.float16) for o in want])
    assert dict(ops.FALLBACKS) == before                         # counted for device tensors only


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("C", K.FPN_C)
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_exact_with_integer_data(ct, C, L):
    """``fpn_half_cases.integer_case``: one level, and two at ``EXACT``'s 2x ratio (bilinear weights 0.25 / 0.75)."""
    cin, sizes, N = P.DLA[:L], P.EXACT[:L], 2
    x, prm = K.integer_case(C, cin, sizes, N)
    dt = K.TYPES[ct]
    # the claims the exactness rests on, on the CPU comparator, before the kernel is looked at
    last = K.last_maps(x, prm)
    for l, t in enumerate(last):
        assert torch.equal(t.to(dt).float(), t), "last[%d] does not survive .to(%s)" % (l, ct)
    assert float(last[0].abs().max()) >= 4 and float((last[0] - last[0].round()).abs().max()) == 0.0
    if L == 2:
        up = last[0] - K.last_maps(x[:1], prm[:1])[0]            # the resized coarse level alone
        assert float(up.abs().max()) >= 16 and float((up % 16 != 0).float().mean()) > 0.3   # the 0.25 / 0.75 weights are at work
    o32, o64 = P.oracle(x, prm, torch.float32), P.oracle(x, prm, torch.float64)
    assert all(torch.equal(a.double(), b) for a, b in zip(o32, o64))            # every sum is exact in fp32
    with torch.no_grad():
        emul = K.emulate_fpn(_fpn(C, cin, prm, "cpu"), dt)([torch.from_numpy(v) for v in x])
        assert _equal_bits(emul, o32)                            # the comparator rounds nothing here
        out = _fpn(C, cin, prm, compute_dtype=dt)(_dev(x))
    assert float(o32[0].abs().max()) > 50
    for l, (g, w) in enumerate(zip(out, o32)):
        assert torch.equal(g.cpu(), w), "level %d: %d cells differ" % (l, int((g.cpu() != w).sum()))


GENERAL = [(shape, C, cin[:len(K.FPN_SHAPES[shape])], N) for shape in sorted(K.FPN_SHAPES) for C in K.FPN_C for cin in K.FPN_CIN
           for N in (1, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,C,cin,N", GENERAL)
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_half_fpn_against_the_fp64_oracle_is_within_twice_the_comparator(ct, shape, C, cin, N):
    """Measured ratios e_half / e_emul: profiles/fpn_half_parity.md."""
    import siammot_amd.ops as ops
    ref = _reference(C, cin, N, shape, ct)
    fpn = _fpn(C, cin, ref["prm"], compute_dtype=K.TYPES[ct])
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        out = fpn(_dev(ref["x"]))
    assert dict(ops.FALLBACKS) == before
    sizes = K.FPN_SHAPES[shape]
    assert isinstance(out, tuple) and len(out) == len(sizes) + 1
    for o, want in zip(out, ref["o64"]):
        assert o.shape == want.shape and o.dtype is torch.float32 and o.is_contiguous()
    e_half, e_emul = H.scaled_error(out, ref["o64"], ref["scale"]), ref[ct]["e_emul"]
    print("fpn_half %s %s C=%d Cin=%s N=%d: e_half %.3e e_emul %.3e ratio %.3f" % (ct, shape, C, cin, N, e_half, e_emul, e_half / e_emul))
    assert e_half <= FACTOR * e_emul
    assert torch.equal(out[-1], out[-2][:, :, ::2, ::2])         # the top block is a subsample of the coarsest map, bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("in_dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_half_stage_maps_return_the_bits_of_the_float_call(ct, in_dtype):
    C, cin = 160, P.DLA
    ref = _reference(C, cin, 3, "ODD4", ct)
    fpn = _fpn(C, cin, ref["prm"], compute_dtype=K.TYPES[ct])
    half = [v.to(in_dtype) for v in _dev(ref["x"])]
    with torch.no_grad():
        out_h = fpn(half)
        out_f = fpn([v.float() for v in half])
    assert _equal_bits(out_h, out_f) and float(out_h[0].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_images_are_independent_half_outputs_are_rounded_once_and_calls_do_not_sync(ct):
    C, cin, N = 160, (32, 64, 96, 160), 3
    ref = _reference(C, cin, N, "ODD4", ct)
    fpn = _fpn(C, cin, ref["prm"], compute_dtype=K.TYPES[ct])
    x = _dev(ref["x"])
    with torch.no_grad():
        out = fpn(x)
        again, syncs = H.count_syncs(lambda: fpn(x))
        assert _equal_bits(out, again)
        assert len(syncs) == 0, [str(s.message)[:80] for s in syncs]
        for i in range(N):
            assert _equal_bits(fpn([v[i:i + 1] for v in x]), [o[i:i + 1] for o in out]), "image %d" % i
        for dtype in (torch.float16, torch.bfloat16):
            half = _fpn(C, cin, ref["prm"], out_dtype=dtype, compute_dtype=K.TYPES[ct])(x)
            assert all(h.dtype is dtype and h.is_contiguous() for h in half) and len(half) == 5
            assert _equal_bits(half, [f.to(dtype) for f in out])                # P[L] included
            assert torch.equal(_bits(half[-1]), _bits(half[-2][:, :, ::2, ::2]))


def _bad_cells(x, value_a, value_b):
    x = [v.copy() for v in x]
    x[0][0, 3, 5, 7] = value_a                                   # interior of the finest stage map: 9 cells per channel
    x[3][2, 100, 1, 1] = value_b                                 # the coarsest: spreads down the pyramid through the resizes
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_non_finite_cells_spread_as_in_fp32_modes_oracle(ct):
    C, cin, N = 32, P.DLA, 3
    ref = _reference(C, cin, N, "ODD4", ct)
    x = _bad_cells(ref["x"], np.inf, np.nan)
    o32 = P.oracle(x, ref["prm"], torch.float32)                 # fp32 mode's oracle: the masks the mode must reproduce
    o64 = P.oracle(x, ref["prm"], torch.float64)
    with torch.no_grad():
        emul = K.emulate_fpn(_fpn(C, cin, ref["prm"], "cpu"), K.TYPES[ct])([torch.from_numpy(v) for v in x])
        out = _fpn(C, cin, ref["prm"], compute_dtype=K.TYPES[ct])(_dev(x))
    for l, (g, w) in enumerate(zip(out, o32)):
        assert torch.equal(torch.isfinite(g.cpu()), torch.isfinite(w)), "level %d" % l
    assert int((~torch.isfinite(o32[0][0])).sum()) == C * 9 and bool(torch.isfinite(o32[1][0]).all())
    assert bool(torch.isfinite(o32[0][1]).all()) and not bool(torch.isfinite(o32[0][2]).any()) and not bool(torch.isfinite(o32[4][2]).any())
    e_half, e_emul = H.scaled_error(out, o64, ref["scale"]), H.scaled_error(emul, o64, ref["scale"])
    print("fpn_half %s with non-finite cells: finite outputs e_half %.3e e_emul %.3e" % (ct, e_half, e_emul))
    assert 0 < e_half <= FACTOR * e_emul


@pytest.mark.gpu
def test_seventy_thousand_is_inf_in_fp16_mode_and_finite_in_bf16_mode():
    C, cin, N = 32, P.DLA, 3
    for ct in sorted(K.TYPES):
        ref = _reference(C, cin, N, "ODD4", ct)
        x = _bad_cells(ref["x"], 70000.0, -70000.0)
        inf = _bad_cells(ref["x"], np.inf, -np.inf)
        mask = [torch.isfinite(o) for o in P.oracle(inf if ct == "fp16" else x, ref["prm"], torch.float32)]
        with torch.no_grad():
            out = _fpn(C, cin, ref["prm"], compute_dtype=K.TYPES[ct])(_dev(x))
            plain = _fpn(C, cin, ref["prm"])(_dev(x))
        assert all(bool(torch.isfinite(o).all()) for o in plain)                # fp32 mode has the range
        for l, (g, m) in enumerate(zip(out, mask)):
            assert torch.equal(torch.isfinite(g.cpu()), m), "%s level %d" % (ct, l)
        assert all(bool(m.all()) for m in mask) == (ct == "bf16") and (not bool(mask[0][2].any())) == (ct == "fp16")
        if ct == "bf16":
            o64 = P.oracle(x, ref["prm"], torch.float64)
            with torch.no_grad():
                emul = K.emulate_fpn(_fpn(C, cin, ref["prm"], "cpu"), K.TYPES[ct])([torch.from_numpy(v) for v in x])
            scale = P.channel_scale(o64)
            assert H.scaled_error(out, o64, scale) <= FACTOR * H.scaled_error(emul, o64, scale)


def _raw(C, cin, ct, sizes=P.TWO, N=1, stage_offset=0, out_offset=0, null_ws=False):
    """``smot_fpn_half_fwd`` on valid buffers of these shapes (pointers moved / nulled as asked), the outputs pre-filled with
    7 -> (return code, the packed-size query's answer, the outputs)."""
    import siammot_amd.ops as ops
    lib = ops.load_library()
    L = len(cin)
    stages = [torch.zeros((N, c, h, w), device="cuda") for c, (h, w) in zip(cin, sizes)]
    out = [torch.full((N, C, h, w), 7.0, device="cuda") for (h, w) in sizes]
    packed = torch.zeros(sum(C * c + 2 * C + 9 * C * C for c in cin), device="cuda")
    ws = torch.zeros(sum(N * C * h * w + 4 for (h, w) in sizes), device="cuda")
    arr = lambda vals: (ctypes.c_int * L)(*vals)
    ptrs = lambda ts, off=0: ctypes.cast((ctypes.c_void_p * L)(*[t.data_ptr() + off for t in ts]), ctypes.c_void_p)
    ic, ih, iw = arr(cin), arr([s[0] for s in sizes]), arr([s[1] for s in sizes])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert lib.smot_fpn_ws_bytes(L, cast(ih), cast(iw), N, C) <= ws.numel() * 4          # the workspace is fp32 mode's
    rc = lib.smot_fpn_half_fwd(ptrs(stages, stage_offset), 0, cast(ic), cast(ih), cast(iw), L, N, C, ct,
                               ctypes.c_void_p(packed.data_ptr()), ctypes.c_void_p(None if null_ws else ws.data_ptr()),
                               ptrs(out, out_offset), 0, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, lib.smot_fpn_half_packed_floats(L, cast(ic), C, ct), out


@pytest.mark.gpu
def test_raw_calls_refuse_what_the_header_says_and_launch_nothing():
    import siammot_amd.ops as ops
    lib = ops.load_library()
    untouched = lambda out: all(float((o - 7.0).abs().max()) == 0.0 for o in out)
    rc, floats, out = _raw(32, (32, 64), 1)                      # within the capacities the call runs
    assert rc == 0 and floats == sum(32 * c // 2 + 64 + 9 * 32 * 32 // 2 for c in (32, 64)) and not untouched(out)
    assert all(float(o.abs().max()) == 0.0 for o in out)         # (zero maps, zero image)
    assert _raw(32, (32, 64), 2)[1] == floats                    # bf16: the same size
    for ct in (0, 3, -1, 18):                                    # SMOT_FEAT_F32 and anything else: SMOT_ERR_BAD_ARG
        rc, floats, out = _raw(32, (32, 64), ct)
        assert rc == -1 and floats == -1 and untouched(out), ct
    assert "compute_type" in lib.smot_last_error().decode()
    rc, floats, out = _raw(32, (32, 48), 1)                      # Cin = 48 at level 1: SMOT_ERR_UNSUPPORTED, names the level
    assert rc == -2 and floats == -1 and untouched(out)
    assert re.search(r"Cin = 48 at level 1", lib.smot_last_error().decode())
    for kw in ({"stage_offset": 2}, {"out_offset": 2}, {"null_ws": True}):      # misaligned fp32 maps, a null pointer
        rc, _, out = _raw(32, (32, 64), 1, **kw)
        assert rc == -1 and untouched(out), kw
    prm = P.params(32, (32, 48))
    blocks = ([(torch.from_numpy(p[0]).cuda(), torch.from_numpy(p[1]).cuda()) for p in prm],
              [(torch.from_numpy(p[2]).cuda(), torch.from_numpy(p[3]).cuda()) for p in prm])
    with pytest.raises(RuntimeError, match="Cin = 48"):
        ops.fpn_half_pack(*blocks, torch.float16)
    with pytest.raises(ValueError, match="compute_dtype"):
        ops.fpn_half_pack(*blocks, torch.float32)
    assert ops.fpn_pack(*blocks).numel() > 0                     # fp32 mode takes the level


@pytest.mark.gpu
def test_a_level_of_48_channels_takes_the_torch_composition_with_fp32_modes_bits():
    import siammot_amd.ops as ops
    C, cin = 64, (48, 16)
    prm, x = P.params(C, cin), _dev(P.maps(cin, 2, P.TWO))
    with torch.no_grad():
        before = ops.FALLBACKS["fpn_torch"]
        want = _fpn(C, cin, prm).train()(x)                      # fp32 mode's fallback: the composition on the device
        assert ops.FALLBACKS["fpn_torch"] == before + 1
        got = _fpn(C, cin, prm, compute_dtype=torch.float16)(x)
        assert ops.FALLBACKS["fpn_torch"] == before + 2
    assert _equal_bits(got, want)
    o64 = P.oracle([v.cpu().numpy() for v in x], prm, torch.float64)
    assert H.scaled_error(got, o64, P.channel_scale(o64)) < 1e-4                # it is the fp32 composition, not the mode


@pytest.mark.gpu
def test_packed_images_follow_the_parameters_and_the_mode():
    C, cin = 32, (32, 64, 96, 160)
    ref = _reference(C, cin, 1, "ODD4", "fp16")
    x = _dev(ref["x"])
    plain, half = _fpn(C, cin, ref["prm"]), _fpn(C, cin, ref["prm"], compute_dtype=torch.float16)
    with torch.no_grad():
        old = [o.clone() for o in plain(x)]
        a = [o.clone() for o in half(x)]
        assert not any(torch.equal(p, q) for p, q in zip(a, old))               # the mode is on
        assert plain.packed().data_ptr() != half.packed().data_ptr() and plain.packed().numel() != half.packed().numel()
        assert half.packed() is half.packed()                    # cached
        half.fpn_layer2.weight.mul_(2.0)
        b = [o.clone() for o in half(x)]
        assert not torch.equal(a[1], b[1])
        assert _equal_bits([a[0]] + a[2:], [b[0]] + b[2:])       # P[1] alone reads fpn_layer2
        assert _equal_bits(plain(x), old)                        # the fp32-mode module still returns its old bits
        half.compute_dtype = torch.bfloat16                      # the cache key holds the mode: packed again
        c = half(x)
        assert not any(torch.equal(p, q) for p, q in zip(b, c))
        half.compute_dtype = None                                # ... and the fp32 image
        plain.fpn_layer2.weight.mul_(2.0)
        assert _equal_bits(half(x), plain(x))


@pytest.mark.gpu
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_everything_in_half_mode_frames_to_detections_with_one_host_copy(ct):
    """``build_detection_head(..., backbone=True, compute_dtype=ct)`` on the small frame of
    tests/test_dla_half.py::test_half_backbone_frames_to_detections_with_one_host_copy: body, pyramid and RPN head in half
    compute mode, one host copy, no fallback, finite detections."""
    import rpn_proposal_cases as R
    import siammot_amd.ops as ops
    from siammot_amd.box_refine import BoxCoder
    from siammot_amd.detector import build_detection_head
    Cw, N, size = 128, 2, (96, 64)
    cfg = _cfg(Cw)
    cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM = 64
    cfg.MODEL.RPN.PRE_NMS_TOP_N_TEST, cfg.MODEL.RPN.POST_NMS_TOP_N_TEST, cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 256, 32, 100
    torch.manual_seed(5)
    det = build_detection_head(cfg, BoxCoder(R.WEIGHTS), Cw, backbone=True, compute_dtype=K.TYPES[ct]).to("cuda").eval()
    H.load_head(det.rpn_head, H.params(Cw, 3, seed=1), "cuda")
    P.load_fpn(det.backbone.fpn, P.params(Cw, P.DLA, seed=2), "cuda")
    D.load(det.backbone.body, D.params(det.backbone.body, D.SEED), "cuda")
    with torch.no_grad():
        det.box_head.predictor.bbox_pred.weight.mul_(0.02)
        det.box_head.predictor.cls_score.weight.mul_(4.0)
    assert det.rpn_head.compute_dtype is det.backbone.fpn.compute_dtype is det.backbone.body.compute_dtype is K.TYPES[ct]
    images = torch.from_numpy(D.image((64, 96), 9, N=N)).cuda()
    with torch.no_grad():
        det.forward_images(images, size)                         # (workspaces, the packed weights, the anchors)
    before = dict(ops.FALLBACKS)
    (feats, got), syncs = H.count_syncs(lambda: det.forward_images(images, size))
    assert dict(ops.FALLBACKS) == before
    assert len(syncs) == 1, "expected ONE device->host copy, saw %d: %s" % (len(syncs), [str(s.message)[:80] for s in syncs])
    assert len(feats) == 5 and len(got) == N and all(len(a) > 0 for a in got)
    assert all(bool(torch.isfinite(f).all()) for f in feats)
    for a in got:
        assert bool(torch.isfinite(a.bbox).all()) and bool(torch.isfinite(a.get_field("scores")).all())
    print("forward_images N=%d everything in %s compute mode: detections %s" % (N, ct, [len(a) for a in got]))
