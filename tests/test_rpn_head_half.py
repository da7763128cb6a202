"""RPN head in half compute mode (siammot_amd.rpn.RPNHead(compute_dtype=), ops.rpn_head_half / rpn_head_half_pack,
csrc/rpn_head.hip: rpn_head_half_kernel).

The mode rounds the maps and ``conv.weight`` to fp16 / bf16, multiplies them exactly on the 16-bit matrix instruction and
accumulates in fp32; ``t`` and the two 1x1 heads stay fp32.  Nothing is rounded in between, so the GPU tests are crisp: against
the fp64 oracle of tests/rpn_head_cases.py on the ROUNDED case (tests/fpn_half_cases.py::head_rounded) the kernel differs in fp32
summation order alone and is held to the bound tests/test_rpn_head.py holds the fp32 kernel to: 1e-4 of the per-channel scale.

CPU: symbols, the keyword, ``state_dict``, builders, CPU tensors.  GPU: the oracle over both types, the shapes ``ODD`` / ``ONE``,
C in {32, 160}, A in {1, 3}, N in {1, 3} and fp32 / fp16 / bf16 maps; per-image bits; non-finite cells; fp16's range; the raw
calls' refusals; packed images.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import fpn_half_cases as K
import rpn_head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("smot_rpn_head_half_packed_floats", "smot_rpn_head_half_pack", "smot_rpn_head_half_fwd")
SHAPES = {"ODD": H.ODD, "ONE": H.ONE}
BOUND = 1e-4                                         # tests/test_rpn_head.py's, of the per-channel scale, against fp64
_cache = {}


def _reference(C, A, N, shape, ct, in_dtype=torch.float32):
    """(maps as the call gets them, parameters, fp64 oracle of the rounded case, per-channel scales): computed once."""
    key = (C, A, N, shape, ct, in_dtype)
    if key not in _cache:
        prm = H.params(C, A)
        x = [torch.from_numpy(v).to(in_dtype) for v in H.maps(C, N, SHAPES[shape])]      # what the kernel loads and widens
        xr, pr = K.head_rounded([v.float().numpy() for v in x], prm, K.TYPES[ct])
        o64, r64 = H.oracle(xr, pr, torch.float64)
        _cache[key] = dict(prm=prm, x=x, o64=o64, r64=r64, so=H.channel_scale(o64), sr=H.channel_scale(r64))
    return _cache[key]


def _head(C, A, prm, dev="cuda", **kw):
    from siammot_amd.rpn import RPNHead
    return H.load_head(RPNHead(None, C, A, **kw), prm, dev)


def _equal_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _error(obj, reg, ref):
    return max(H.scaled_error(obj, ref["o64"], ref["so"]), H.scaled_error(reg, ref["r64"], ref["sr"]))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_carry_the_new_symbols():
    import siammot_amd.ops as ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smot_emm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smot_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared and name in ops.EXPORTED_SYMBOLS, name
    assert ops.ABI_VERSION == 14 and re.search(r"#define SMOT_ABI_VERSION 14\b", src)
    assert callable(ops.rpn_head_half_pack) and callable(ops.rpn_head_half)
    for fn in (ops.rpn_head_half_pack, ops.rpn_head_half):
        assert "compute_dtype" in inspect.signature(fn).parameters


def test_the_keyword_is_keyword_only_validated_and_leaves_the_state_dict_alone():
    from siammot_amd.rpn import RPNHead, RPNModule
    for cls in (RPNHead, RPNModule):
        p = inspect.signature(cls.__init__).parameters["compute_dtype"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    with pytest.raises(TypeError):
        RPNHead(None, 32, 3, torch.float16)
    for bad in (torch.float32, torch.float64, "fp16", 1):
        with pytest.raises(ValueError, match="compute_dtype"):
            RPNHead(None, 32, 3, compute_dtype=bad)
    plain = RPNHead(None, 32, 3)
    assert plain.compute_dtype is None
    for ct in K.TYPES.values():
        half = RPNHead(None, 32, 3, compute_dtype=ct)
        assert half.compute_dtype is ct
        assert list(half.state_dict().keys()) == list(plain.state_dict().keys())
        assert [tuple(v.shape) for v in half.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]


def test_rpn_module_carries_the_mode_to_its_head():
    from siammot_amd.config import get_default_cfg
    from siammot_amd.rpn import RPNModule
    cfg = get_default_cfg(channels=32)
    assert RPNModule(cfg, 32).head.compute_dtype is None
    for ct in K.TYPES.values():
        m = RPNModule(cfg, 32, compute_dtype=ct)
        assert m.head.compute_dtype is ct
        assert list(m.state_dict().keys()) == list(RPNModule(cfg, 32).state_dict().keys())
    with pytest.raises(ValueError, match="compute_dtype"):
        RPNModule(cfg, 32, compute_dtype=torch.float32)


@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_cpu_tensors_give_the_bits_of_fp32_mode(ct):
    import siammot_amd.ops as ops
    prm, x = H.params(32, 3), [torch.from_numpy(v) for v in H.maps(32, 2)]
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        want = _head(32, 3, prm, "cpu")(x)
        got = _head(32, 3, prm, "cpu", compute_dtype=K.TYPES[ct])(x)
    assert _equal_bits(got[0], want[0]) and _equal_bits(got[1], want[1])
    assert dict(ops.FALLBACKS) == before                         # counted for device tensors only


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("A", K.HEAD_A)
@pytest.mark.parametrize("C", K.HEAD_C)
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_half_head_against_the_fp64_oracle_of_the_rounded_case(ct, shape, C, A, N):
    """Measured maxima: INTEGRATION.md §3q."""
    import siammot_amd.ops as ops
    ref = _reference(C, A, N, shape, ct)
    head = _head(C, A, ref["prm"], compute_dtype=K.TYPES[ct])
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        obj, reg = head([v.cuda() for v in ref["x"]])
    assert dict(ops.FALLBACKS) == before
    for l, (h, w) in enumerate(SHAPES[shape]):
        assert obj[l].shape == (N, A, h, w) and reg[l].shape == (N, 4 * A, h, w)
        assert obj[l].dtype is torch.float32 and obj[l].is_contiguous() and reg[l].is_contiguous()
    e = _error(obj, reg, ref)
    print("rpn_head_half %s %s C=%d A=%d N=%d: max scaled error %.3e vs fp64 of the rounded case" % (ct, shape, C, A, N, e))
    assert e < BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("C", K.HEAD_C)
@pytest.mark.parametrize("in_dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_half_maps_are_widened_then_rounded(ct, in_dtype, C):
    """A half map is loaded, widened and then rounded to the compute type: the oracle is the rounded case of the WIDENED map,
    and the call returns the bits of the call on ``.float()``.  An fp16 map in fp16 mode (a bf16 map in bf16 mode) is exact."""
    ref = _reference(C, 3, 3, "ODD", ct, in_dtype)
    head = _head(C, 3, ref["prm"], compute_dtype=K.TYPES[ct])
    x = [v.cuda() for v in ref["x"]]
    assert x[0].dtype is in_dtype
    with torch.no_grad():
        obj, reg = head(x)
        obj_f, reg_f = head([v.float() for v in x])
    assert _equal_bits(obj, obj_f) and _equal_bits(reg, reg_f)
    e = _error(obj, reg, ref)
    print("rpn_head_half %s on %s maps C=%d: max scaled error %.3e" % (ct, in_dtype, C, e))
    assert e < BOUND
    if in_dtype is K.TYPES[ct]:
        assert all(torch.equal(torch.from_numpy(K.rnd(v.float().numpy(), in_dtype)), v.float()) for v in ref["x"])


@pytest.mark.gpu
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_each_image_of_a_call_is_its_one_image_call(ct):
    C, A, N = 160, 3, 3
    ref = _reference(C, A, N, "ODD", ct)
    head = _head(C, A, ref["prm"], compute_dtype=K.TYPES[ct])
    x = [v.cuda() for v in ref["x"]]
    with torch.no_grad():
        obj, reg = head(x)
        (obj2, reg2), syncs = H.count_syncs(lambda: head(x))
        assert _equal_bits(obj, obj2) and _equal_bits(reg, reg2)
        assert len(syncs) == 0, [str(s.message)[:80] for s in syncs]
        for i in range(N):
            oi, ri = head([v[i:i + 1] for v in x])
            assert _equal_bits(oi, [o[i:i + 1] for o in obj]) and _equal_bits(ri, [r[i:i + 1] for r in reg]), "image %d" % i


@pytest.mark.gpu
@pytest.mark.parametrize("C", K.HEAD_C)
@pytest.mark.parametrize("ct", sorted(K.TYPES))
def test_non_finite_cells_reach_exactly_their_windows(ct, C):
    A, N = 3, 3
    ref = _reference(C, A, N, "ODD", ct)
    x = [v.numpy().copy() for v in ref["x"]]
    x[0][0, 3, 5, 7] = np.inf                                    # interior of the finest map: A * 9 objectness cells
    x[1][1, C - 1, 0, 0] = np.nan                                # a corner, the last channel
    xr, pr = K.head_rounded(x, ref["prm"], K.TYPES[ct])
    o32, r32 = H.oracle(xr, pr, torch.float32)
    o64, r64 = H.oracle(xr, pr, torch.float64)
    with torch.no_grad():
        obj, reg = _head(C, A, ref["prm"], compute_dtype=K.TYPES[ct])([torch.from_numpy(v).cuda() for v in x])
    for got, want in zip(list(obj) + list(reg), list(o32) + list(r32)):
        assert torch.equal(torch.isfinite(got.cpu()), torch.isfinite(want))
    assert int((~torch.isfinite(o32[0][0])).sum()) == A * 9 and int((~torch.isfinite(o32[1][1])).sum()) == A * 4
    assert bool(torch.isfinite(o32[0][1:]).all()) and bool(torch.isfinite(o32[1][0]).all()) and bool(torch.isfinite(o32[2]).all())
    e = max(H.scaled_error(obj, o64, ref["so"]), H.scaled_error(reg, r64, ref["sr"]))
    print("rpn_head_half %s C=%d with non-finite cells: finite outputs %.3e" % (ct, C, e))
    assert e < BOUND


@pytest.mark.gpu
def test_seventy_thousand_is_inf_in_fp16_mode_and_finite_in_bf16_mode():
    C, A, N = 32, 3, 1
    for ct in sorted(K.TYPES):
        ref = _reference(C, A, N, "ONE", ct)
        x = [v.numpy().copy() for v in ref["x"]]
        x[0][0, 5, 4, 8] = 70000.0
        xr, pr = K.head_rounded(x, ref["prm"], K.TYPES[ct])
        assert bool(np.isinf(xr[0][0, 5, 4, 8])) == (ct == "fp16")
        o64, r64 = H.oracle(xr, pr, torch.float64)
        with torch.no_grad():
            obj, reg = _head(C, A, ref["prm"], compute_dtype=K.TYPES[ct])([torch.from_numpy(v).cuda() for v in x])
        for got, want in zip(list(obj) + list(reg), list(o64) + list(r64)):
            assert torch.equal(torch.isfinite(got.cpu()), torch.isfinite(want))
        bad = int((~torch.isfinite(obj[0])).sum())
        assert bad == (A * 9 if ct == "fp16" else 0)
        so, sr = H.channel_scale([torch.nan_to_num(o, 0.0, 0.0, 0.0) for o in o64]), H.channel_scale([torch.nan_to_num(r, 0.0, 0.0, 0.0) for r in r64])
        assert max(H.scaled_error(obj, o64, so), H.scaled_error(reg, r64, sr)) < BOUND


def _raw(C, A, ct, feat_offset=0, null_out=False, packed_offset=0):
    """``smot_rpn_head_half_fwd`` on valid buffers of ``ONE`` (pointers moved / nulled as asked), the outputs pre-filled with
    7 -> (return code, the packed-size query's answer, the outputs)."""
    import siammot_amd.ops as ops
    lib = ops.load_library()
    (h, w), = H.ONE
    x = torch.zeros((1, max(C, 32), h, w), device="cuda")
    obj, reg = torch.full((1, A, h, w), 7.0, device="cuda"), torch.full((1, 4 * A, h, w), 7.0, device="cuda")
    packed = torch.zeros(1 << 16, device="cuda")
    one = lambda v: ctypes.cast((ctypes.c_void_p * 1)(v), ctypes.c_void_p)
    ints = lambda v: ctypes.cast((ctypes.c_int * 1)(v), ctypes.c_void_p)
    rc = lib.smot_rpn_head_half_fwd(one(x.data_ptr() + feat_offset), 0, ints(h), ints(w), 1, 1, C, A, ct,
                                    ctypes.c_void_p(packed.data_ptr() + packed_offset), one(None if null_out else obj.data_ptr()),
                                    one(reg.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, lib.smot_rpn_head_half_packed_floats(C, A, ct), (obj, reg)


@pytest.mark.gpu
def test_raw_calls_refuse_what_the_header_says_and_launch_nothing():
    import siammot_amd.ops as ops
    untouched = lambda out: all(float((o - 7.0).abs().max()) == 0.0 for o in out)
    rc, floats, out = _raw(32, 3, 1)
    heads = 16 * 32 + 16                                         # 5 A = 15 rows padded to 16, and their biases
    assert rc == 0 and floats == 9 * 32 * 32 // 2 + 32 + heads and not untouched(out)
    assert _raw(32, 3, 2)[1] == floats                           # bf16: the same size
    for ct in (0, 3, -1, 17):                                    # SMOT_FEAT_F32 and anything else: SMOT_ERR_BAD_ARG
        rc, floats, out = _raw(32, 3, ct)
        assert rc == -1 and floats == -1 and untouched(out), ct
    assert "compute_type" in ops.load_library().smot_last_error().decode()
    for C, A in ((48, 3), (32, 13)):                            # the capacities are fp32 mode's: SMOT_ERR_UNSUPPORTED
        rc, floats, out = _raw(C, A, 1)
        assert rc == -2 and floats == -1 and untouched(out), (C, A)
    for kw in ({"null_out": True}, {"packed_offset": 4}):        # a null tensor, a misaligned packed image: SMOT_ERR_BAD_ARG
        rc, _, out = _raw(32, 3, 1, **kw)
        assert rc == -1 and untouched(out), kw
    prm = [torch.from_numpy(p).cuda() for p in H.params(32, 3)]
    with pytest.raises(ValueError, match="compute_dtype"):
        ops.rpn_head_half_pack(*prm, torch.float32)
    with pytest.raises(ValueError, match="compute_dtype"):
        ops.rpn_head_half([torch.zeros(1, 32, 9, 17, device="cuda")], torch.zeros(1 << 14, device="cuda"), 32, 3, None)


@pytest.mark.gpu
def test_packed_images_follow_the_parameters_and_the_mode():
    C, A = 32, 3
    ref = _reference(C, A, 1, "ODD", "fp16")
    x = [v.cuda() for v in ref["x"]]
    plain, half = _head(C, A, ref["prm"]), _head(C, A, ref["prm"], compute_dtype=torch.float16)
    with torch.no_grad():
        old = [o.clone() for o in plain(x)[0]]
        a = [o.clone() for o in half(x)[0]]
        assert not _equal_bits(a, old)                           # the mode is on
        assert plain.packed().data_ptr() != half.packed().data_ptr() and plain.packed().numel() != half.packed().numel()
        assert half.packed() is half.packed()                    # cached
        half.conv.weight.mul_(2.0)
        b = [o.clone() for o in half(x)[0]]
        assert not _equal_bits(a, b)                             # packed again
        prm = [ref["prm"][0] * 2.0] + list(ref["prm"][1:])
        xr, pr = K.head_rounded([v.numpy() for v in ref["x"]], prm, torch.float16)
        o64, _ = H.oracle(xr, pr, torch.float64)
        assert H.scaled_error(b, o64, H.channel_scale(o64)) < BOUND
        assert _equal_bits(plain(x)[0], old)                     # the fp32-mode module still returns its old bits
        half.compute_dtype = torch.bfloat16                      # the cache key holds the mode: packed again
        c = half(x)[0]
        other = _head(C, A, prm, compute_dtype=torch.bfloat16)
        assert _equal_bits(c, other(x)[0]) and not _equal_bits(c, b)
        half.compute_dtype = None                                # ... and the fp32 image
        assert _equal_bits(half(x)[0], _head(C, A, prm)(x)[0])
