"""The half compute mode's contract, read back bit for bit (constructions and tables:
tests/half_rounding_cases.py): operands are rounded with ``tensor.to``'s rounding, the products are exact, the sums fp32.

CPU: the tables against an independent RNE in exact arithmetic, and the conditions that make them bite.
GPU: activation read-back through selection filters and filter read-back through delta images, over every conversion site
(``cvh_block``'s staging for ``dla_conv3x3_half``, ``fpn_half``'s 3x3 stage and ``rpn_head_half``; the stagings of
``dla_conv1x1_half`` and of ``fpn_half``'s lateral; the three pack kernels), both compute types, forms, strides, taps and
partial tiles — ``torch.equal``, no tolerance; the band between the largest finite value and the first that overflows; three
terms of very different size inside one matrix instruction.  Measured outcomes: profiles/half_rounding_parity.md.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dla_cases as D
import dla_half_cases as C
import half_rounding_cases as R
import rpn_head_cases as H

TYPES = sorted(C.TYPES)
F32 = np.float32
BOUND = 1e-4                                         # tests/test_dla_half.py's, of the per-channel scale, against fp64


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def _rnd(a, ct):
    return C.rnd(a, C.TYPES[ct])


def _unit(Cout):
    return torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda")


def _same(out, want, what):
    """Value for value (a selected -0 was summed with +0 terms), and no NaN."""
    got = out.float().cpu()
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not bool(torch.isnan(got).any()), "%s: NaN" % what
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d cells differ, first at %s: got %r (bits %08x), want %r (bits %08x)" % (
            what, int(bad.sum()), bad.numel(), i, float(got[i]), int(_bits(got)[i]) & 0xffffffff, float(want[i]),
            int(_bits(want)[i]) & 0xffffffff))


# ---- CPU: the tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", TYPES)
def test_the_yardstick_is_round_to_nearest_even_on_the_table(ct):
    """``.to(ct).float()`` on the table equals the RNE of exact arithmetic, bit for bit, and every entry stays finite."""
    t = R.edge_table(ct)
    want = R.rne(t, ct)
    assert np.array_equal(_rnd(t, ct).view(np.uint32), want.view(np.uint32))
    assert bool(np.isfinite(want).all())
    assert np.array_equal(np.sort(t.view(np.uint32)), np.sort((-t).view(np.uint32)))            # closed under negation
    assert len(np.unique(t.view(np.uint32))) == len(t)


@pytest.mark.parametrize("ct", TYPES)
def test_the_table_separates_the_roundings(ct):
    """The conditions on the table, met by the reference alone: >= 40 entries are changed by the rounding, for >= 16 RNE is
    not truncation toward zero, for >= 4 it is not round-half-away-from-zero."""
    t = R.edge_table(ct)
    r = R.rne(t, ct)
    changed, trunc, away = int((r != t).sum()), int((r != R.toward_zero(t, ct)).sum()), int((r != R.half_away(t, ct)).sum())
    print("%s table: %d entries, %d changed, %d differ from truncation, %d from half-away" % (ct, len(t), changed, trunc, away))
    assert changed >= 40 and trunc >= 16 and away >= 4
    sub = 2.0 ** (-14 if ct == "fp16" else -126)
    assert int(((np.abs(r) < sub) & (r != 0)).sum()) >= 8                                        # subnormal results
    assert int(((np.abs(t) < sub) & (t != 0) & (r == 0)).sum()) >= 4                             # ... and values that vanish


def test_the_named_entries_round_as_stated():
    p2 = lambda k: F32(2.0 ** k)
    one = lambda v, ct: float(_rnd(np.array([v], dtype=F32), ct)[0])
    up = lambda v: np.nextafter(F32(v), F32(np.inf))
    assert one(1 + p2(-11), "fp16") == 1.0 and one(1 + 3 * p2(-11), "fp16") == 1 + 2.0 ** -9 and one(2 - p2(-11), "fp16") == 2.0
    assert one(p2(-25), "fp16") == 0.0 and one(up(p2(-25)), "fp16") == 2.0 ** -24
    assert one(F32(1.5) * p2(-24), "fp16") == 2.0 ** -23 and one(F32(2.5) * p2(-24), "fp16") == 2.0 ** -23
    assert one(p2(-14) - p2(-25), "fp16") == 2.0 ** -14 and one(p2(-26), "fp16") == 0.0 and one(p2(-130), "fp16") == 0.0
    assert one(1 + p2(-8), "bf16") == 1.0 and one(1 + 3 * p2(-8), "bf16") == 1 + 2.0 ** -6 and one(2 - p2(-8), "bf16") == 2.0
    assert one(p2(-134), "bf16") == 0.0 and one(up(p2(-134)), "bf16") == 2.0 ** -133
    assert one(F32(1.5) * p2(-133), "bf16") == 2.0 ** -132 and one(F32(2.5) * p2(-133), "bf16") == 2.0 ** -132
    assert one(p2(-126) - p2(-134), "bf16") == 2.0 ** -126 and one(p2(-149), "bf16") == 0.0
    for ct in TYPES:
        for v in (p2(-24), 1023 * p2(-24), p2(-14), 65504.0) if ct == "fp16" else (p2(-133), 127 * p2(-133), p2(-126)):
            assert one(v, ct) == float(v) and F32(v) in R.edge_table(ct)


@pytest.mark.parametrize("ct", TYPES)
def test_the_overflow_pairs_straddle_the_edge(ct):
    pairs = R.overflow_pairs(ct)
    assert len(pairs) == 2 and pairs[1] == (-pairs[0][0], -pairs[0][1])
    for lo, hi in pairs:
        assert np.nextafter(lo, hi) == hi                                                        # neighbours in fp32
        r = _rnd(np.array([lo, hi], dtype=F32), ct)
        assert np.isfinite(r[0]) and abs(r[0]) == R.FORMAT[ct][2] and np.isinf(r[1]) and np.sign(r[1]) == np.sign(hi)
        assert np.array_equal(R.rne(np.array([lo, hi], dtype=F32), ct), r)
        assert lo in R.edge_table(ct) and hi not in R.edge_table(ct)
    assert float(pairs[0][1]) == (65520.0 if ct == "fp16" else float(np.uint32(0x7f7f8000).view(F32)))


def test_the_three_term_sums_are_exact_in_any_order():
    """Every partial sum of (+2^a, -2^a, +2^(a - s)) in any order is an fp32 value: an fp32 accumulation returns 2^(a - s)."""
    import itertools
    for s in (12, 20, 23):
        terms = [2.0 ** 10, -2.0 ** 10, 2.0 ** (10 - s)]
        for order in itertools.permutations(terms):
            acc = F32(0.0)
            for v in order:
                exact = float(acc) + v
                acc = F32(exact)
                assert float(acc) == exact
            assert float(acc) == 2.0 ** (10 - s)
        for ct in TYPES:
            assert np.array_equal(_rnd(np.array(terms, dtype=F32), ct), np.array(terms, dtype=F32))


# ---- GPU: activation read-back ------------------------------------------------------------------------------------------
TAPS = {1: ((1, 1), (0, 0), (2, 2)), 2: ((1, 1), (1, 2), (2, 1), (2, 2))}


def _read3(ops, ct, x, Cout, stride, tap, seed, what):
    """One ``dla_conv3x3_half`` call with selection filters on ``x`` (numpy), compared with the slice of ``rnd(x)``."""
    w, ic, sign = R.selection3(Cout, x.shape[1], tap, seed)
    out = ops.dla_conv3x3_half(_cuda(x), _cuda(w), *_unit(Cout), stride, C.TYPES[ct], None, False)
    _same(out, R.shifted(_rnd(x, ct), ic, sign, tap, stride), what)
    return ic


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,size", [(32, 16, (9, 19)), (96, 64, (17, 35)), (32, 64, (17, 35)), (96, 16, (9, 19))])
@pytest.mark.parametrize("ct", TYPES)
def test_activations_read_back_conv3x3(ct, Cin, Cout, size):
    """Cout = 16 is the operator's one width that is no multiple of 32 (a single M-tile); it refuses every other one."""
    import siammot_amd.ops as ops
    with pytest.raises(RuntimeError, match="Cout = 48"):
        ops.dla_conv3x3_half(_cuda(np.zeros((1, 32, 4, 4), F32)), _cuda(np.zeros((48, 32, 3, 3), F32)), *_unit(48), 1, C.TYPES[ct])
    table = R.edge_table(ct)
    x = R.fill((2, Cin) + size, table, 100 + Cin + Cout)
    assert R.holds_every_entry(x, table)
    for stride, taps in TAPS.items():
        for tap in taps:
            ic = _read3(ops, ct, x, Cout, stride, tap, 7 * Cin + Cout + 3 * tap[0] + tap[1] + stride,
                        "conv3x3 %s %d->%d %s stride %d tap %s" % (ct, Cin, Cout, size, stride, tap))
            assert len(set(ic.tolist())) == min(Cin, Cout)


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_activations_read_back_conv3x3_every_form(ct):
    import siammot_amd.ops as ops
    table, seen = R.edge_table(ct), set()
    for Cin, Cout, stride, size, N, form in C.FORMS:
        x = R.fill((N, Cin) + size, table, 200 + Cin + Cout + stride)
        assert ops.dla_conv3x3_half_form(N, size[0], size[1], Cout, stride) == form
        assert ops.dla_conv3x3_half_form(1, size[0], size[1], Cout, stride) == (4, form[1])
        tap = (0, 2) if stride == 1 else (2, 1)
        _read3(ops, ct, x, Cout, stride, tap, 11, "conv3x3 %s form %s stride %d, N = %d" % (ct, form, stride, N))
        _read3(ops, ct, x[N - 1:], Cout, stride, tap, 12, "conv3x3 %s form (4, %d) stride %d, N = 1" % (ct, form[1], stride))
        seen |= {(stride,) + form, (stride, 4, form[1])}
    assert seen == C.ALL_FORMS, seen


def _sources(ct, sources, size, N, table, seed):
    """(the sources as the call gets them, ``rnd`` of their concatenation behind the pool)."""
    src = [R.fill((N, c) + ((2 * size[0] + 1, 2 * size[1] + 1) if p else size), table, seed + i) for i, (c, p) in enumerate(sources)]
    cat = np.concatenate([R.pooled(s) if p else s for s, (_, p) in zip(src, sources)], axis=1)
    assert R.holds_every_entry(np.concatenate([s.ravel() for s in src]), table)
    return src, _rnd(cat, ct)


@pytest.mark.gpu
@pytest.mark.parametrize("sources,Cout,size,form", [([(32, False)], 96, (9, 13), 2), ([(32, False)] * 8, 160, (9, 13), 2),
                                                    ([(64, True), (32, False)], 96, (5, 7), 2), (C.CONV1_WIDE[0], 160, (75, 75), 4)])
@pytest.mark.parametrize("ct", TYPES)
def test_activations_read_back_conv1x1(ct, sources, Cout, size, form):
    import siammot_amd.ops as ops
    N = 1 if form == 4 else 2
    assert ops.dla_conv1x1_half_form(N, size[0], size[1], Cout) == form
    src, want = _sources(ct, sources, size, N, R.edge_table(ct), 300 + Cout)
    if sources[0][1]:                                            # the pooled expectation, in torch's own words
        assert torch.equal(torch.from_numpy(want[:, :64]), F.max_pool2d(torch.from_numpy(src[0]), 2, 2).to(C.TYPES[ct]).float())
    K, read = want.shape[1], set()
    dev, flags = [_cuda(s) for s in src], [p for _, p in sources]
    for start in range(0, K, Cout):                              # Cout < K: further selections until every slot was read
        w, k, sign = R.selection1(Cout, K, 31 + K, start)
        read |= set(k.tolist())
        exp = want[:, k] * sign.reshape(1, -1, 1, 1)
        for od in (torch.float32, torch.float16, torch.bfloat16):
            out = ops.dla_conv1x1_half(dev, flags, _cuda(w), *_unit(Cout), False, C.TYPES[ct], out_dtype=od)
            assert out.dtype is od
            _same(out, torch.from_numpy(exp).to(od).float().numpy(), "conv1x1 %s %s -> %d %s out %s" % (ct, sources, Cout, size, od))
    assert read == set(range(K))


def _fpn_call(ops, ct, x, prm, top_block=False):
    inner = [(_cuda(p[0]), _cuda(p[1])) for p in prm]
    layer = [(_cuda(p[2]), _cuda(p[3])) for p in prm]
    C_ = prm[0][0].shape[0]
    packed = ops.fpn_half_pack(inner, layer, C.TYPES[ct])
    return ops.fpn_half([_cuda(v) for v in x], packed, [p[0].shape[1] for p in prm], C_, C.TYPES[ct], top_block=top_block)


def _fpn_selection(Cn, Cin, seed):
    """A signed permutation as ``inner`` and a signed centre-tap permutation as ``layer`` (biases 0) -> (parameters,
    the channel and the sign each output channel reads)."""
    wi, k1, s1 = R.selection1(Cn, Cin, seed)
    wl, k2, s2 = R.selection3(Cn, Cn, (1, 1), seed + 1)
    zero = np.zeros(Cn, dtype=F32)
    return (wi, zero, wl, zero), k1[k2], s1[k2] * s2


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_activations_read_back_fpn(ct):
    """One level: the output is the signed permutation of ``rnd(x)`` (the second rounding, of ``last``, is idempotent).  Two
    levels at an exact 2x ratio with an all-zero coarse stage map: the top-down term is +0 and the fine level still is."""
    import siammot_amd.ops as ops
    table = R.edge_table(ct)
    x = R.fill((2, 32, 13, 21), table, 400)
    prm, k, sign = _fpn_selection(32, 32, 41)
    assert sorted(k.tolist()) == list(range(32)) and R.holds_every_entry(x, table)
    want = _rnd(x, ct)[:, k] * sign.reshape(1, -1, 1, 1)
    out = _fpn_call(ops, ct, [x], [prm])
    assert len(out) == 1
    _same(out[0], want, "fpn %s, one level" % ct)
    fine = R.fill((2, 32, 12, 20), table, 401)
    prm1, _, _ = _fpn_selection(32, 32, 43)
    out = _fpn_call(ops, ct, [fine, np.zeros((2, 32, 6, 10), dtype=F32)], [prm, prm1])
    _same(out[0], _rnd(fine, ct)[:, k] * sign.reshape(1, -1, 1, 1), "fpn %s, two levels: the fine one" % ct)
    _same(out[1], np.zeros((2, 32, 6, 10), dtype=F32), "fpn %s, two levels: the coarse one" % ct)


RPN_A, RPN_C = 12, 32                                # 5 A = 60 head rows >= C: every mid channel is selected


def _rpn_heads(seed):
    """One-hot rows of ``cls_logits`` and ``bbox_pred`` over the mid channels -> (cls_w, bbox_w, the mid channel per row)."""
    w, mid, _ = R.selection1(5 * RPN_A, RPN_C, seed, signed=False)
    assert set(mid.tolist()) == set(range(RPN_C))
    return w[:RPN_A], w[RPN_A:], mid


def _rpn_call(ops, ct, x, conv_w, cls_w, bbox_w):
    prm = [conv_w, np.zeros(RPN_C, F32), cls_w, np.zeros(RPN_A, F32), bbox_w, np.zeros(4 * RPN_A, F32)]
    packed = ops.rpn_head_half_pack(*[_cuda(p) for p in prm], C.TYPES[ct])
    return ops.rpn_head_half([_cuda(v) for v in x], packed, RPN_C, RPN_A, C.TYPES[ct])


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_activations_read_back_rpn_head(ct):
    """``relu(+-rnd(x))`` at the selected channels; the pack with the signs flipped reads what the ReLU removed."""
    import siammot_amd.ops as ops
    table = R.edge_table(ct)
    sizes = ((9, 19), (17, 35))
    x = [R.fill((2, RPN_C) + s, table, 500 + l) for l, s in enumerate(sizes)]
    assert all(R.holds_every_entry(v, table) for v in x)
    conv_w, ic, sign = R.selection3(RPN_C, RPN_C, (1, 1), 51)
    cls_w, bbox_w, mid = _rpn_heads(52)
    for flip in (1.0, -1.0):
        obj, reg = _rpn_call(ops, ct, x, conv_w * F32(flip), cls_w, bbox_w)
        for l, v in enumerate(x):
            t = np.maximum(_rnd(v, ct)[:, ic] * (sign * F32(flip)).reshape(1, -1, 1, 1), F32(0.0))
            _same(obj[l], t[:, mid[:RPN_A]], "rpn head %s level %d objectness, signs x %d" % (ct, l, flip))
            _same(reg[l], t[:, mid[RPN_A:]], "rpn head %s level %d regression, signs x %d" % (ct, l, flip))


# ---- GPU: filter read-back ------------------------------------------------------------------------------------------------
PARITIES = ((0, 0), (0, 1), (1, 0), (1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cin,Cout,size", [(32, 16, (19, 21)), (96, 64, (31, 33))])
@pytest.mark.parametrize("ct", TYPES)
def test_filters_read_back_conv3x3(ct, Cin, Cout, size, stride):
    import siammot_amd.ops as ops
    table = R.edge_table(ct)
    w = R.fill((Cout, Cin, 3, 3), table, 600 + Cin)
    assert R.holds_every_entry(w, table)
    x, cells, signs = R.deltas3(Cin, size, (1.0, -1.0), PARITIES if stride == 2 else ((0, 0),), seed=Cin)
    want, seen = R.scatter3(_rnd(w, ct), cells, signs, size, stride)
    assert bool(seen.all())                                      # every filter element is read
    out = ops.dla_conv3x3_half(_cuda(x), _cuda(w), *_unit(Cout), stride, C.TYPES[ct], None, False)
    _same(out, want, "conv3x3 %s filters %d->%d stride %d" % (ct, Cin, Cout, stride))


@pytest.mark.gpu
@pytest.mark.parametrize("S,size", [(1, (5, 7)), (8, (16, 17))])
@pytest.mark.parametrize("Cout", [96, 160])
@pytest.mark.parametrize("ct", TYPES)
def test_filters_read_back_conv1x1(ct, Cout, S, size):
    import siammot_amd.ops as ops
    table, K = R.edge_table(ct), 32 * S
    w = R.fill((Cout, K), table, 700 + Cout + S)
    assert R.holds_every_entry(w, table)
    x = R.deltas1(K, size, (1.0, -1.0))
    src = [_cuda(x[:, 32 * s:32 * s + 32]) for s in range(S)]
    out = ops.dla_conv1x1_half(src, [False] * S, _cuda(w.reshape(Cout, K, 1, 1)), *_unit(Cout), False, C.TYPES[ct])
    _same(out, R.gathered1(_rnd(w, ct), size, (1.0, -1.0)), "conv1x1 %s filters K = %d -> %d" % (ct, K, Cout))


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_filters_read_back_fpn(ct):
    """``inner`` (two K steps) through an identity centre-tap ``layer``; ``layer`` through an identity ``inner``."""
    import siammot_amd.ops as ops
    table, Cn = R.edge_table(ct), 32
    zero = np.zeros(Cn, dtype=F32)
    eye3 = np.zeros((Cn, Cn, 3, 3), dtype=F32)
    eye3[np.arange(Cn), np.arange(Cn), 1, 1] = 1.0
    wi = R.fill((Cn, 64), table, 800)
    assert R.holds_every_entry(wi, table)
    out = _fpn_call(ops, ct, [R.deltas1(64, (9, 8), (1.0, -1.0))], [(wi.reshape(Cn, 64, 1, 1), zero, eye3, zero)])
    _same(out[0], R.gathered1(_rnd(wi, ct), (9, 8), (1.0, -1.0)), "fpn %s inner filters" % ct)
    wl = R.fill((Cn, Cn, 3, 3), table, 801)
    assert R.holds_every_entry(wl, table)
    x, cells, signs = R.deltas3(Cn, (19, 21), (1.0, -1.0), seed=8)
    want, seen = R.scatter3(_rnd(wl, ct), cells, signs, (19, 21), 1)
    assert bool(seen.all())
    out = _fpn_call(ops, ct, [x], [(np.eye(Cn, dtype=F32).reshape(Cn, Cn, 1, 1), zero, wl, zero)])
    _same(out[0], want, "fpn %s layer filters" % ct)


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_filters_read_back_rpn_head(ct):
    """``conv.weight`` through the one-hot head rows: the +1 image returns relu(w), the -1 image relu(-w)."""
    import siammot_amd.ops as ops
    table = R.edge_table(ct)
    w = R.fill((RPN_C, RPN_C, 3, 3), table, 900)
    assert R.holds_every_entry(w, table)
    x, cells, signs = R.deltas3(RPN_C, (19, 21), (1.0, -1.0), seed=9)
    want, seen = R.scatter3(_rnd(w, ct), cells, signs, (19, 21), 1)
    assert bool(seen.all())
    t = np.maximum(want, F32(0.0))
    assert np.array_equal(t[0] - t[1], want[0])                  # the two images together hold every element, negative ones too
    cls_w, bbox_w, mid = _rpn_heads(91)
    obj, reg = _rpn_call(ops, ct, [x], w, cls_w, bbox_w)
    _same(obj[0], t[:, mid[:RPN_A]], "rpn head %s conv.weight, objectness" % ct)
    _same(reg[0], t[:, mid[RPN_A:]], "rpn head %s conv.weight, regression" % ct)


# ---- GPU: the band between the largest finite value and the first that overflows ---------------------------------------------
def _band(what, lower, upper, o64_lower, o64_upper, hit):
    """``lower`` / ``upper``: the outputs of the two calls (lists of tensors); ``o64_*``: the fp64 oracle on the rounded operands;
    ``hit``: the outputs that read the cell or element.  The lower call is finite and within the bound; in the upper call
    exactly ``hit`` is +-inf with the oracle's signs and the rest keeps the lower call's bits."""
    for l, (a, b, ra, rb, h) in enumerate(zip(lower, upper, o64_lower, o64_upper, hit)):
        a, b = a.cpu(), b.cpu()
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(ra).all()), "%s [%d]: the lower call" % (what, l)
        scale = ra.abs().amax(dim=(0, 2, 3)).clamp_min(1e-30)
        e = float(((a.double() - ra).abs() / scale.view(1, -1, 1, 1)).max())
        print("%s [%d]: lower call %.3e of the channel scale; %d outputs read the value" % (what, l, e, int(h.sum())))
        assert e < BOUND, what
        assert torch.equal(torch.isinf(b), h) and not bool(torch.isnan(b).any()), "%s [%d]: %d inf, %d NaN, %d expected" % (
            what, l, int(torch.isinf(b).sum()), int(torch.isnan(b).sum()), int(h.sum()))
        assert torch.equal(torch.isinf(rb), h) and torch.equal(b[h].double(), rb[h]), "%s [%d]: the signs" % (what, l)
        assert torch.equal(_bits(a)[~h], _bits(b)[~h]), "%s [%d]: the rest moved" % (what, l)
        assert int(h.sum()) > 0


def _dense(rs, shape):
    return rs.choice(np.array([-1.0, 1.0], dtype=F32), size=shape)


def _conv3_o64(x, w, ct, stride=1):
    c = dict(x=_rnd(x, ct), w=_rnd(w, ct), scale=np.ones(w.shape[0], F32), shift=np.zeros(w.shape[0], F32), stride=stride)
    return D.conv3x3_oracle(c, torch.float64, False, False)


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_band_conv3x3(ct):
    import siammot_amd.ops as ops
    rs = np.random.RandomState(61)
    Cin, Cout, size = 32, 64, (9, 19)
    call = lambda x, w: ops.dla_conv3x3_half(_cuda(x), _cuda(w), *_unit(Cout), 1, C.TYPES[ct], None, False)
    for lo, hi in R.overflow_pairs(ct):
        x, w = (rs.standard_normal((2, Cin) + size) * 4.0).astype(F32), _dense(rs, (Cout, Cin, 3, 3))
        xa, xb = x.copy(), x.copy()
        xa[0, 7, 4, 9], xb[0, 7, 4, 9] = lo, hi
        hit = torch.zeros((2, Cout) + size, dtype=torch.bool)
        hit[0, :, 3:6, 8:11] = True
        _band("conv3x3 %s cell %r" % (ct, float(hi)), [call(xa, w)], [call(xb, w)], [_conv3_o64(xa, w, ct)], [_conv3_o64(xb, w, ct)], [hit])
        x, w = np.ones((2, Cin) + size, dtype=F32), (rs.standard_normal((Cout, Cin, 3, 3)) * 0.05).astype(F32)
        wa, wb = w.copy(), w.copy()
        wa[5, 7, 1, 1], wb[5, 7, 1, 1] = lo, hi                  # the centre tap: it reads no padding
        hit = torch.zeros((2, Cout) + size, dtype=torch.bool)
        hit[:, 5] = True
        _band("conv3x3 %s filter element %r" % (ct, float(hi)), [call(x, wa)], [call(x, wb)], [_conv3_o64(x, wa, ct)], [_conv3_o64(x, wb, ct)], [hit])


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_band_conv1x1(ct):
    import siammot_amd.ops as ops
    rs = np.random.RandomState(62)
    Cout, size = 96, (9, 13)
    call = lambda s, w: ops.dla_conv1x1_half([_cuda(v) for v in s], [False, False], _cuda(w), *_unit(Cout), False, C.TYPES[ct])
    o64 = lambda s, w: F.conv2d(torch.from_numpy(np.concatenate([_rnd(v, ct) for v in s], 1)).double(), torch.from_numpy(_rnd(w, ct)).double())
    for lo, hi in R.overflow_pairs(ct):
        s, w = [(rs.standard_normal((2, 32) + size) * 4.0).astype(F32) for _ in range(2)], _dense(rs, (Cout, 64, 1, 1))
        sa, sb = [v.copy() for v in s], [v.copy() for v in s]
        sa[1][0, 4, 3, 8], sb[1][0, 4, 3, 8] = lo, hi
        hit = torch.zeros((2, Cout) + size, dtype=torch.bool)
        hit[0, :, 3, 8] = True
        _band("conv1x1 %s cell %r" % (ct, float(hi)), [call(sa, w)], [call(sb, w)], [o64(sa, w)], [o64(sb, w)], [hit])
        s, w = [np.ones((2, 32) + size, dtype=F32) for _ in range(2)], (rs.standard_normal((Cout, 64, 1, 1)) * 0.05).astype(F32)
        wa, wb = w.copy(), w.copy()
        wa[5, 40, 0, 0], wb[5, 40, 0, 0] = lo, hi
        hit = torch.zeros((2, Cout) + size, dtype=torch.bool)
        hit[:, 5] = True
        _band("conv1x1 %s filter element %r" % (ct, float(hi)), [call(s, wa)], [call(s, wb)], [o64(s, wa)], [o64(s, wb)], [hit])


def _fpn_o64(x, prm, ct):
    """One level in fp64 on the rounded operands; ``last`` — exact in fp32 by the case's construction (asserted) — is rounded."""
    wi, bi, wl, bl = (torch.from_numpy(v) for v in prm)
    last = F.conv2d(torch.from_numpy(_rnd(x, ct)).double(), torch.from_numpy(_rnd(wi.numpy(), ct)).double(), bi.double())
    assert torch.equal(last.float().double(), last)
    last = last.float().to(C.TYPES[ct]).double()
    return F.conv2d(last, torch.from_numpy(_rnd(wl.numpy(), ct)).double(), bl.double(), padding=1)


SMALL = F32(2.0 ** -14)                              # exact in both types: 1 + 31 SMALL leaves max(bf16) finite in fp32


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_band_fpn(ct):
    """Two stages: all 32 ``last`` channels of the cell's position are +-the value, and the 3x3 stage sums them.  For that sum
    to be finite below the edge and one-signed above it (no inf - inf), ``layer`` is dense with signs s[oc] sigma[ic] tau[tap]
    (sigma: the signs the cell arrives with) and magnitude 1 for one input channel, 2^-14 for the others: in bf16, where the
    edge is the top of fp32's own range, 32 terms of magnitude 1 would overflow the fp32 sum below the edge as well.  The other
    channels are zero at the cell's position and small integers elsewhere: ``last`` is exact in fp32 in any order."""
    import siammot_amd.ops as ops
    rs = np.random.RandomState(63)
    Cn, size = 32, (13, 21)
    zero = np.zeros(Cn, dtype=F32)
    mag = np.full(Cn, SMALL, dtype=F32)
    mag[0] = 1.0
    call = lambda x, prm: _fpn_call(ops, ct, [x], [prm])
    for lo, hi in R.overflow_pairs(ct):
        # a cell of the stage map
        x = rs.randint(-8, 9, size=(2, Cn) + size).astype(F32)
        x[0, :, 5, 7] = 0.0
        xa, xb = x.copy(), x.copy()
        xa[0, 7, 5, 7], xb[0, 7, 5, 7] = lo, hi
        wi = _dense(rs, (Cn, Cn, 1, 1))
        s, tau = _dense(rs, Cn), _dense(rs, (3, 3))
        wl = s.reshape(-1, 1, 1, 1) * (wi[:, 7, 0, 0] * mag).reshape(1, -1, 1, 1) * tau.reshape(1, 1, 3, 3)
        prm = (wi, zero, wl.astype(F32), zero)
        hit = torch.zeros((2, Cn) + size, dtype=torch.bool)
        hit[0, :, 4:7, 6:9] = True
        _band("fpn %s cell %r" % (ct, float(hi)), call(xa, prm), call(xb, prm), [_fpn_o64(xa, prm, ct)], [_fpn_o64(xb, prm, ct)], [hit])
        # an element of ``inner``: its row holds nothing else, so last[5] is the rounded element at every position
        x = np.ones((2, Cn) + size, dtype=F32)
        wi = rs.randint(-1, 2, size=(Cn, Cn, 1, 1)).astype(F32)
        wi[5] = 0.0
        wia, wib = wi.copy(), wi.copy()
        wia[5, 7], wib[5, 7] = lo, hi
        wl = _dense(rs, (Cn, Cn, 3, 3))
        wl[:, 5] = s.reshape(-1, 1, 1) * SMALL                   # one sign per output channel over the nine taps that read last[5]
        wl[:, 5, 1, 1] = s
        hit = torch.ones((2, Cn) + size, dtype=torch.bool)
        pa, pb = (wia, zero, wl, zero), (wib, zero, wl, zero)
        _band("fpn %s inner element %r" % (ct, float(hi)), call(x, pa), call(x, pb), [_fpn_o64(x, pa, ct)], [_fpn_o64(x, pb, ct)], [hit])
        # an element of ``layer``, behind a signed permutation: ``last`` is +-1 everywhere
        wi = R.selection1(Cn, Cn, 64)[0]
        wl = (rs.standard_normal((Cn, Cn, 3, 3)) * 0.05).astype(F32)
        wla, wlb = wl.copy(), wl.copy()
        wla[5, 7, 1, 1], wlb[5, 7, 1, 1] = lo, hi
        hit = torch.zeros((2, Cn) + size, dtype=torch.bool)
        hit[:, 5] = True
        pa, pb = (wi, zero, wla, zero), (wi, zero, wlb, zero)
        _band("fpn %s layer element %r" % (ct, float(hi)), call(x, pa), call(x, pb), [_fpn_o64(x, pa, ct)], [_fpn_o64(x, pb, ct)], [hit])


@pytest.mark.gpu
@pytest.mark.parametrize("ct", TYPES)
def test_band_rpn_head(ct):
    """The ReLU and the fp32 heads stand behind the 3x3 stage: ``conv.weight`` is dense +-1 and gives the cell its own sign
    in ONE mid channel and the opposite one in all others, which the ReLU then zeroes (so that the heads, dense +-1 too, sum
    one value at the edge and not sixteen, and no inf meets a -inf); the element's call has maps of -+1 so that the ReLU
    keeps the element."""
    import siammot_amd.ops as ops
    rs = np.random.RandomState(64)
    size, m0 = (9, 19), 11
    cls_w, bbox_w = _dense(rs, (RPN_A, RPN_C, 1, 1)), _dense(rs, (4 * RPN_A, RPN_C, 1, 1))
    zeros = lambda n: np.zeros(n, dtype=F32)

    def o64(x, conv_w):
        xr, pr = [_rnd(x, ct)], [_rnd(conv_w, ct), zeros(RPN_C), cls_w, zeros(RPN_A), bbox_w, zeros(4 * RPN_A)]
        obj, reg = H.oracle(xr, pr, torch.float64)
        return [obj[0], reg[0]]

    def call(x, conv_w):
        obj, reg = _rpn_call(ops, ct, [x], conv_w, cls_w, bbox_w)
        return [obj[0], reg[0]]

    for lo, hi in R.overflow_pairs(ct):
        x, w = (rs.standard_normal((2, RPN_C) + size) * 4.0).astype(F32), _dense(rs, (RPN_C, RPN_C, 3, 3))
        w[:, 7] = -np.sign(hi)
        w[m0, 7] = np.sign(hi)
        xa, xb = x.copy(), x.copy()
        xa[0, 7, 4, 9], xb[0, 7, 4, 9] = lo, hi
        hit = [torch.zeros((2, n) + size, dtype=torch.bool) for n in (RPN_A, 4 * RPN_A)]
        for h in hit:
            h[0, :, 3:6, 8:11] = True
        _band("rpn head %s cell %r" % (ct, float(hi)), call(xa, w), call(xb, w), o64(xa, w), o64(xb, w), hit)
        x, w = np.full((2, RPN_C) + size, np.sign(hi), dtype=F32), (rs.standard_normal((RPN_C, RPN_C, 3, 3)) * 0.05).astype(F32)
        wa, wb = w.copy(), w.copy()
        wa[5, 7, 1, 1], wb[5, 7, 1, 1] = lo, hi
        hit = [torch.ones((2, n) + size, dtype=torch.bool) for n in (RPN_A, 4 * RPN_A)]
        _band("rpn head %s conv.weight element %r" % (ct, float(hi)), call(x, wa), call(x, wb), o64(x, wa), o64(x, wb), hit)


# ---- GPU: three terms of one sum ----------------------------------------------------------------------------------------------
A_EXP = 10
SHIFTS = (12, 20, 23)


def _terms3(ops, ct, s, Cin, Cout, spread, taps, seed, stride=1, size=(9, 19)):
    """+2^a, -2^a, +2^(a - s) of one output on ``dla_conv3x3_half``: ``taps`` one tap (the three terms then sit in one K block
    of one instruction, or in three chunks) or three (one term each).  The map is constant per channel; the expectation is the
    exact sum of the terms whose tap reads inside the map, which is an fp32 value."""
    values, rows, slots = R.three_terms(Cout, Cin, A_EXP, s, spread, seed)
    x = np.broadcast_to(values.reshape(1, Cin, 1, 1), (2, Cin) + size).copy()
    w = np.zeros((Cout, Cin, 3, 3), dtype=F32)
    want = np.zeros((2, Cout) + ((((size[0] - 1) // 2 + 1, (size[1] - 1) // 2 + 1)) if stride == 2 else size), dtype=np.float64)
    oc = np.arange(Cout)
    for j in range(3):
        tap = taps[j % len(taps)]
        w[oc, slots[:, j], tap[0], tap[1]] = rows[oc, slots[:, j]]
        want += R.shifted(x.astype(np.float64), slots[:, j], rows[oc, slots[:, j]].astype(np.float64), tap, stride)
    assert np.array_equal(want.astype(F32).astype(np.float64), want) and float(np.abs(want).min()) in (0.0, 2.0 ** (A_EXP - s))
    assert np.array_equal(_rnd(x, ct), x) and float(want.max()) > 0
    out = ops.dla_conv3x3_half(_cuda(x), _cuda(w), *_unit(Cout), stride, C.TYPES[ct], None, False)
    return out.cpu(), torch.from_numpy(want.astype(F32))


def _terms1(ops, ct, s, K, Cout, spread, seed, size=(9, 13)):
    values, rows, _ = R.three_terms(Cout, K, A_EXP, s, spread, seed)
    x = np.broadcast_to(values.reshape(1, K, 1, 1), (2, K) + size).copy()
    src = [_cuda(x[:, 32 * i:32 * i + 32]) for i in range(K // 32)]
    out = ops.dla_conv1x1_half(src, [False] * len(src), _cuda(rows.reshape(Cout, K, 1, 1)), *_unit(Cout), False, C.TYPES[ct])
    return out.cpu(), torch.full((2, Cout) + size, 2.0 ** (A_EXP - s))


@pytest.mark.gpu
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("ct", TYPES)
def test_three_terms_through_the_fp32_accumulator(ct, s):
    """The three terms in three chunks (or sources) and in three taps: they meet in the fp32 C operand."""
    import siammot_amd.ops as ops
    for what, (got, want) in (("conv3x3 three chunks", _terms3(ops, ct, s, 96, 64, "blocks", [(1, 1)], 71)),
                              ("conv3x3 three taps", _terms3(ops, ct, s, 32, 16, "groups", [(0, 0), (1, 1), (2, 1)], 72)),
                              ("conv3x3 three taps, stride 2", _terms3(ops, ct, s, 32, 64, "group", [(1, 1), (1, 2), (2, 2)], 73, 2)),
                              ("conv1x1 three sources", _terms1(ops, ct, s, 96, 96, "blocks", 74))):
        assert torch.equal(got, want), "%s %s s = %d: %d cells differ" % (what, ct, s, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("ct", TYPES)
def test_three_terms_inside_one_matrix_instruction(ct, s):
    """The three terms in ONE 32-channel K block at one tap, in one group of 8 k slots and over three groups: the sum
    v_mfma_f32_16x16x32_f16 / _bf16 forms internally.  Measured for s = 12, 20, 23: profiles/half_rounding_parity.md."""
    import siammot_amd.ops as ops
    for what, (got, want) in (("conv3x3 one group", _terms3(ops, ct, s, 32, 16, "group", [(1, 1)], 75)),
                              ("conv3x3 three groups", _terms3(ops, ct, s, 32, 64, "groups", [(0, 2)], 76)),
                              ("conv3x3 three groups, second chunk", _terms3(ops, ct, s, 64, 32, "groups", [(2, 0)], 77, 2)),
                              ("conv1x1 one group", _terms1(ops, ct, s, 32, 96, "group", 78)),
                              ("conv1x1 three groups", _terms1(ops, ct, s, 64, 160, "groups", 79))):
        bad = int((got != want).sum())
        print("ONE-INSTRUCTION %s %s s = %d: %d of %d cells differ%s" % (what, ct, s, bad, got.numel(),
              "" if not bad else ", e.g. got %r for %r" % (float(got[got != want][0]), float(want[got != want][0]))))
        assert bad == 0, "%s %s s = %d: %d cells differ" % (what, ct, s, bad)
