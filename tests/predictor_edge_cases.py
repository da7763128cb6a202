"""Deterministic inputs for tests/test_predictor_edges.py: the predictor (csrc/predictor.hip ``predictor_impl``: two 3x3 conv
towers + GroupNorm + ReLU + three 3x3 heads) at the group sizes, channel counts and map sizes that pick its kernel families
and their code paths.  Every other predictor test calls it with 32 GroupNorm groups, eps 1e-5 and gamma in [0.5, 1.5]; here

  * ``cpg = C / gn_groups`` takes every value the matrix-core families admit (1, 2, 4, 8, 16: the read-lane path at 4, the LDS
    path elsewhere, one group per 16-channel tile at 16) with both K-loop shapes (C = 128 unrolled, the generic loop), and
    values they do not (3, 6, 32: the scalar kernel);
  * C takes the last count the 16 x 16 gate admits (512) and, at 29 x 29, counts that are no power of two (96, 160, 192), one
    above 512 (576), and multiples of 16 that are none of 32 (48, 16: the direct kernel only);
  * Ho takes 1, 2, 15 and 17 beside 16 and 29;
  * eps, gamma (exact zeros, negative entries), beta ~ N(0, 3) and an all-zero track leave the benign regime;

with the CPU oracle's answer (oracle/emm_oracle.py ``predictor``, in fp64 and in fp32) computed ONCE per case and shared by
the CPU and the GPU tests.  Inputs come from seeded ``numpy.random.RandomState`` as in ``golden_inputs.predictor_params``:
responses ~ N(0, 15), filters ~ N(0, 0.05).  ``family`` and ``blocked_tiles`` restate the dispatch of predictor_impl and the
cost table of tower_blocks_tiles_per_workgroup (csrc/tower_wino.hip) so that the choice of N per case is checked on the CPU
and against ``ops.tower_form`` on the device.  Nothing here touches a device."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import golden_inputs as gi
from oracle import emm_oracle as O

F32 = np.float32
BOXES = np.array([[0, 0, 80, 120]], dtype=F32)
TOL64, TOL32 = 1e-4, 2e-4                      # the bounds of test_hip_parity.test_predictor_vs_oracle, for every family
AGREE = {16: 2e-5, 29: 5e-5}                   # Winograd vs direct form, relative to the direct result's channel scale
MATRIX_CPG = (1, 2, 4, 8, 16)
MATRIX_FAMILIES = ("wino16", "direct16", "wino29", "direct29")


def family(c, groups, ho, winograd):
    """The kernel family predictor_impl picks (csrc/predictor.hip: mfma_ok; csrc/tower_conv.hip: the two launchers' gates)."""
    cpg = c // groups
    ok = cpg in MATRIX_CPG
    if ho == 16 and ok and c % 32 == 0 and (c & (c - 1)) == 0 and c <= 512:
        return "wino16" if winograd else "direct16"
    if ho == 29 and ok and c % 32 == 0 and winograd:
        return "wino29"
    if ho == 29 and ok and c % 16 == 0:
        return "direct29"
    return "scalar"


def blocked_tiles(n, c):
    """16-channel tiles per workgroup of the blocked 29 x 29 Winograd towers (tower_blocks_tiles_per_workgroup of the product
    library): 1 = the fp32 form, 2 = the split (two-part fp16) form, which needs the response's plane maxima."""
    tiles = 2 * (c // 16)
    np8 = ((n + 7) // 8) * 8 * 4
    w1, w2 = np8 * tiles, np8 * (tiles // 2)
    c1 = 20.0 if w1 <= 256 else 27.0 * (w1 // 512) + (0.0 if w1 % 512 == 0 else (15.0 if w1 % 512 <= 256 else 27.0))
    c2 = 0.9 * (24.5 * (w2 // 256) + (0.0 if w2 % 256 == 0 else 22.5))
    return 2 if np.float32(c2) < np.float32(c1) else 1


def reported_form(n, c, ho, winograd):
    """What ``ops.tower_form`` (smot_emm_tower_form) must report for the case, or None where it reports no form (it answers
    for power-of-two C <= 512 at Ho 16 / 29 only, and knows nothing of the direct kernels)."""
    if not winograd or ho not in (16, 29) or c % 32 != 0 or (c & (c - 1)) != 0 or c > 512:
        return None
    return 3 if ho == 16 or blocked_tiles(n, c) == 2 else 1


# ---- the cases ----------------------------------------------------------------------------------------------------------
def _case(part, n, c, groups, ho, variant="plain", eps=1e-5, tiles=None):
    name = "n%d_c%d_g%d_h%d" % (n, c, groups, ho) + ("" if variant == "plain" else "_" + variant)
    return name, dict(part=part, n=n, c=c, groups=groups, ho=ho, variant=variant, eps=eps, tiles=tiles, cpg=c // groups)


def _build():
    cs = []
    # part 1, Ho = 16: C = 128 (unrolled K loop) at cpg 1, 2, 8, 16 — the LDS path; C = 64 (generic loop) at cpg 4 — the
    # read-lane path — and at 1, 8, 16; C = 32 at cpg 16; C = 512 (the gate's last count) at one and two tracks
    for g in (128, 64, 16, 8):
        cs.append(_case(1, 2, 128, g, 16))
    for g in (64, 16, 8, 4):
        cs.append(_case(1, 3, 64, g, 16))
    cs.append(_case(1, 3, 32, 2, 16))
    cs.append(_case(1, 1, 512, 32, 16))
    cs.append(_case(1, 2, 512, 32, 16))
    # part 1, Ho = 29: every cpg at C = 64 in the one-tile form (N <= 8) and in the two-tile form (N = 9), at C = 128
    # (two tiles at every N <= 9), C = 512
    for g in (64, 32, 16, 8, 4):
        cs.append(_case(1, 2, 64, g, 29, tiles=1))
    cs.append(_case(1, 8, 64, 16, 29, tiles=1))
    for g in (64, 32, 16, 8, 4):
        cs.append(_case(1, 9, 64, g, 29, tiles=2))
    for g in (128, 64, 32, 16, 8):
        cs.append(_case(1, 2, 128, g, 29, tiles=2))
    cs.append(_case(1, 1, 512, 32, 29, tiles=2))
    # part 1, the scalar kernel: cpg 3, 6, 32 (none divides 16) and Ho 1, 2, 15, 17 (Ho = 1 is rx == rz)
    cs.append(_case(1, 2, 96, 32, 16))
    cs.append(_case(1, 2, 96, 16, 16))
    cs.append(_case(1, 2, 64, 2, 16))
    for ho in (1, 2, 15, 17):
        cs.append(_case(1, 3, 32, 8, ho))
    cs.append(_case(1, 2, 96, 32, 1))
    # part 2: channel counts the 29 x 29 gates admit and nothing has run
    for g in (24, 12):
        cs.append(_case(2, 1, 96, g, 29, tiles=2))
        cs.append(_case(2, 9, 96, g, 29, tiles=1))
    cs.append(_case(2, 9, 160, 20, 29, tiles=2))
    cs.append(_case(2, 1, 192, 24, 29, tiles=1))
    cs.append(_case(2, 9, 192, 24, 29, tiles=2))
    cs.append(_case(2, 1, 576, 36, 29, tiles=2))
    for c, g in ((48, 6), (48, 12), (16, 16), (16, 1)):
        cs.append(_case(2, 2, c, g, 29))
    # part 3: GroupNorm parameters and degenerate groups
    for c, g in ((128, 8), (64, 16), (64, 4)):
        for ho in (16, 29):
            cs.append(_case(3, 2, c, g, ho, "eps1e-3", eps=1e-3))
            cs.append(_case(3, 2, c, g, ho, "eps1", eps=1.0))
            cs.append(_case(3, 2, c, g, ho, "affine"))
            cs.append(_case(3, 3, c, g, ho, "zerotrack"))
    out = dict(cs)
    assert len(out) == len(cs), "duplicate case names"
    return out


CASES = _build()
CASE_NAMES = tuple(CASES)
# (case, winograd): both forms wherever they are different kernels
RUNS = tuple((name, w) for name, c in CASES.items() for w in (True, False)
             if w or family(c["c"], c["groups"], c["ho"], True) != "scalar")
PAIRS = tuple(name for name, c in CASES.items() if family(c["c"], c["groups"], c["ho"], True) in ("wino16", "wino29"))
# the split form against the fp32 form of the measurement library at the new group sizes and channel counts
SPLIT_CASES = ("n2_c128_g8_h16", "n2_c128_g128_h16", "n3_c64_g16_h16", "n3_c64_g4_h16", "n1_c512_g32_h16",
               "n9_c64_g4_h29", "n2_c128_g8_h29", "n1_c96_g24_h29", "n9_c160_g20_h29")
ZERO_TRACK = 1


def _seed(c):
    return 7000 + 13 * c["c"] + 101 * c["groups"] + 7 * c["ho"] + c["n"] + 1009 * len(c["variant"])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(resp [N, C, Ho, Ho], params) of a case as fp32 numpy arrays."""
    c = CASES[name]
    rs = np.random.RandomState(_seed(c))
    params = gi.predictor_params(rs, c["c"], BOXES)
    resp = (rs.standard_normal((c["n"], c["c"], c["ho"], c["ho"])) * 15.0).astype(F32)
    if c["variant"] == "eps1":
        resp = (resp * F32(1e-3)).astype(F32)                    # eps = 1 dominates every group's variance
    if c["variant"] == "affine":
        for t in ("cls_tower", "reg_tower"):
            ga = params[t + ".1.weight"].copy()
            ch = np.arange(c["c"])
            ga[ch % 4 == 1] *= F32(-1.0)                          # negative entries and exact zeros, mixed within every group
            ga[ch % 4 == 3] = F32(0.0)                            # (cpg = 4, 16: a quarter of a group each, half stays positive)
            params[t + ".1.weight"] = ga
            params[t + ".1.bias"] = (rs.standard_normal(c["c"]) * 3.0).astype(F32)
    if c["variant"] == "zerotrack":
        resp[ZERO_TRACK] = 0.0                                    # variance 0, rstd = 1 / sqrt(eps)
    return resp, params


def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The CPU oracle's logits [N, 7, Ho, Ho] in fp64 and fp32, and the fp64 scale of every output channel."""
    c = CASES[name]
    resp, params = inputs(name)
    out = {}
    for key, dt in (("ref64", torch.float64), ("ref32", torch.float32)):
        cls, center, reg = O.predictor(_t(resp, dt), {k: _t(v, dt) for k, v in params.items()}, c["groups"], c["eps"])
        out[key] = torch.cat((cls, center, reg), 1)
    out["scale"] = out["ref64"].abs().amax(dim=(0, 2, 3), keepdim=True)
    return out


def scaled_error(got, ref, scale):
    """The project's measure (test_predictor_vs_oracle): max |out - ref| / max_channel |ref64|, over everything."""
    return float(((got.double() - ref.double()).abs() / scale).max())


def group_variances(name):
    """Biased variance of every (track, tower, GroupNorm group) of the towers' convolution output, in fp64: [N, 2, groups]."""
    c = CASES[name]
    resp, params = inputs(name)
    x = _t(resp, torch.float64)
    v = []
    for t in ("cls_tower", "reg_tower"):
        y = F.conv2d(x, _t(params[t + ".0.weight"], torch.float64), None, padding=1)
        v.append(y.reshape(c["n"], c["groups"], -1).var(dim=2, unbiased=False))
    return torch.stack(v, 1)


# ---- part 4: group membership, exactly ---------------------------------------------------------------------------------
# (C, groups, Ho, group, winograd): one case per cpg in {1, 4, 16} and matrix-core family; the group is an interior one, at
# cpg = 4 inside a 16-channel tile (its neighbours below and above share the tile, the wave and the LDS sums with it)
MEMBERSHIP = tuple((c, g, ho, grp, w) for ho in (16, 29) for w in (True, False)
                   for c, g, grp in ((32, 32, 7), (64, 16, 5), (64, 4, 1)))


def membership_inputs(c, groups, ho, grp, tower):
    """resp [1, C, Ho, Ho], the base parameters with the heads of ``tower`` (0 = cls, 1 = reg) zeroed on every channel
    outside group ``grp``, and four variants of them: the tower filter of one output channel negated (which keeps the pack
    kernel's weight scale and the fp16 parts exact) — the channel just below the group, the one just above it (the logits of
    the tower's heads must not move), the group's first and its last channel (they must)."""
    cpg = c // groups
    first, last = grp * cpg, grp * cpg + cpg - 1
    assert 0 < first and last < c - 1
    rs = np.random.RandomState(4100 + 3 * c + 17 * groups + ho + 1000 * tower)
    params = gi.predictor_params(rs, c, BOXES)
    resp = (rs.standard_normal((1, c, ho, ho)) * 15.0).astype(F32)
    for k in (("cls.weight", "center.weight"), ("reg.weight",))[tower]:
        w = params[k].copy()
        w[:, :first] = 0.0
        w[:, last + 1:] = 0.0
        params[k] = w
    key = ("cls_tower", "reg_tower")[tower] + ".0.weight"

    def negated(ch):
        p = dict(params)
        w = params[key].copy()
        w[ch] = -w[ch]
        p[key] = w
        return p
    return resp, params, dict(below=negated(first - 1), above=negated(last + 1), first=negated(first), last=negated(last))
