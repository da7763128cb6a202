"""Deterministic inputs, references and assertions for tests/test_xcorr_edges.py: the depthwise cross-correlation K2
(csrc/xcorr.hip ``smot_xcorr_dw_fwd``: the two-planes-per-wave 30/15 kernel, the row-patch 35/7 kernel and the generic
kernel behind every other (Rx, Rz)) and the head's general path (the ``else`` branch of ``emm_track_impl`` and the
non-separable branch of ``emm_extract_cache_impl`` in csrc/emm_fused.hip).

Part A.  ``ref64`` is the explicit fp64 sum over taps (``F.unfold`` of the plane times the template, summed: inf * 0 =
NaN is part of the definition), ``mag`` the same sum over absolute values.  The ``check_*`` functions are the assertions
of the GPU tests, written over a callable ``xcorr(x, z) -> out`` on CPU tensors so that the CPU rehearsal can run them
on a correct fp32 stand-in (which must pass all of them) and on mutants of it (each of which must fail one).

Part B.  Seven (rz, search_region, sampling_ratio) cases of the head that reach the general path, plus one at C = 64,
with the CPU oracle's answers (oracle/emm_oracle.py, fp32 and fp64) computed ONCE per case and shared.

Nothing here touches a device."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import decode_edge_cases as D
import golden_inputs as gi
import predictor_edge_cases as P
from oracle import emm_oracle as O

F32 = np.float32
U24 = 2.0 ** -24                     # unit roundoff of fp32: one fmaf step errs by at most U24 * |its result|
PROJECT_RATIO = 1e-6                 # test_hip_parity._xcorr_check: |err| <= 1e-6 * sum |x z|
PROJECT_TAPS = 225                   # ... which the project states for its own shapes: at most 15 x 15 taps


# =========================================================================================================================
# Part A: references
# =========================================================================================================================
def ref64(x, z):
    """out[n, c, i, j] = sum_{u, v} x[n, c, i + u, j + v] * z[n, c, u, v] in fp64, every product formed (so that a
    non-finite x under a zero tap gives NaN, as IEEE arithmetic and the reference's convolution do)."""
    n, c, rx, _ = x.shape
    rz = z.shape[-1]
    ho = rx - rz + 1
    cols = F.unfold(x.double().reshape(n * c, 1, rx, rx), rz)                    # [planes, rz * rz, ho * ho]
    return (cols * z.double().reshape(n * c, rz * rz, 1)).sum(1).reshape(n, c, ho, ho)


def mag(x, z):
    return ref64(x.abs(), z.abs())


def bound(x, z):
    """A-priori error bound of an rz^2-step fp32 fmaf chain (any order): rz^2 * 2^-24 * sum |x z| (+ 1e-30)."""
    rz = z.shape[-1]
    return rz * rz * U24 * mag(x, z) + 1e-30


# =========================================================================================================================
# Part A: cases
# =========================================================================================================================
PATCH2, ROWPATCH, GENERIC = "patch2", "rowpatch", "generic"
GENERIC_SHAPES = ((1, 1), (15, 15), (16, 1), (18, 3), (29, 1), (20, 9), (21, 7), (45, 15), (33, 32), (64, 7))
SHAPES = ((30, 15),) + ((35, 7),) + GENERIC_SHAPES
PLANES = {(30, 15): (1, 2, 3, 7, 45), (35, 7): (1, 5, 33)}
PLANES.update({s: (1, 5) for s in GENERIC_SHAPES})
SPLIT = {1: (1, 1), 2: (2, 1), 3: (1, 3), 5: (5, 1), 7: (1, 7), 33: (3, 11), 45: (5, 9)}      # planes -> (N, C)
NF_PLANES = 7                        # the non-finite cases: five planted planes (0, 1, 2, 4, 5) and two clean ones (3, 6)
NF_CLEAN = (3, 6)
DELTA_SHAPES = {(30, 15): 7, (35, 7): 5, (20, 9): 5}


def kernel_of(rx, rz):
    """The kernel smot_xcorr_dw_fwd launches (csrc/xcorr.hip)."""
    return PATCH2 if (rx, rz) == (30, 15) else ROWPATCH if (rx, rz) == (35, 7) else GENERIC


def _name(kind, rx, rz, planes):
    return "%s_%dx%d_p%d" % (kind, rx, rz, planes)


def _build():
    out = {}
    for rx, rz in SHAPES:
        for p in PLANES[(rx, rz)]:
            for kind in ("exact", "normal", "range"):
                out[_name(kind, rx, rz, p)] = dict(kind=kind, rx=rx, rz=rz, planes=p)
        for kind in ("nfzero", "nfnonzero"):
            out[_name(kind, rx, rz, NF_PLANES)] = dict(kind=kind, rx=rx, rz=rz, planes=NF_PLANES)
        out[_name("zeros", rx, rz, 3)] = dict(kind="zeros", rx=rx, rz=rz, planes=3)
    for (rx, rz), p in DELTA_SHAPES.items():
        out[_name("delta", rx, rz, p)] = dict(kind="delta", rx=rx, rz=rz, planes=p)
    return out


CASES = _build()
EXACT_CASES = tuple(k for k, c in CASES.items() if c["kind"] in ("exact", "delta"))
BOUND_CASES = tuple(k for k, c in CASES.items() if c["kind"] in ("normal", "range"))
NF_CASES = tuple(k for k, c in CASES.items() if c["kind"] in ("nfzero", "nfnonzero"))
ZERO_CASES = tuple(k for k, c in CASES.items() if c["kind"] == "zeros")


def _seed(c, plane):
    kinds = ("exact", "normal", "range", "nfzero", "nfnonzero", "zeros", "delta")
    return 50000 + 997 * c["rx"] + 31 * c["rz"] + 100003 * kinds.index(c["kind"]) + 7 * c["planes"] + 1013 * plane


def delta_tap(rz, plane):
    """(u, v) of the one live tap of a delta template: the four corners first, then interior positions."""
    corners = ((0, 0), (0, rz - 1), (rz - 1, 0), (rz - 1, rz - 1))
    return corners[plane] if plane < 4 else (1 + (3 * plane) % (rz - 2), 1 + (5 * plane) % (rz - 2))


def nf_positions(c):
    """Where the non-finite values of a case sit: {what: (plane, row, col)}; rows / cols of x for the first three, of z for
    the other two.  Corner, edge and interior cells; the two kinds use different ones."""
    rx, rz = c["rx"], c["rz"]
    if c["kind"] == "nfzero":
        return dict(x_nan=(0, 0, 0), x_pinf=(1, 0, rx // 2), x_ninf=(2, rx // 2, rx // 3),
                    z_nan=(4, rz // 2, rz // 2), z_inf=(5, 0, rz // 2))
    return dict(x_nan=(0, rx - 1, rx - 1), x_pinf=(1, rx // 2, rx - 1), x_ninf=(2, rx // 3, rx // 2),
                z_nan=(4, rz - 1, 0), z_inf=(5, rz // 2, rz - 1))


def nf_zero_tap(c):
    """The zero tap that meets the +inf of x in the ``nfzero`` kind (plane 1).  The value sits in row 0 of the plane, which
    only row 0 of the template reaches: tap (0, rz // 2) meets it at output (0, rx // 2 - rz // 2)."""
    return 0, c["rz"] // 2


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x [N, C, Rx, Rx], z [N, C, Rz, Rz]) of a case as fp32 CPU tensors; every plane from a seed of its own.  For the
    non-finite kinds: the data WITHOUT the planted values (``planted`` adds them)."""
    c = CASES[name]
    rx, rz, p = c["rx"], c["rz"], c["planes"]
    xs, zs = [], []
    for k in range(p):
        rs = np.random.RandomState(_seed(c, k))
        if c["kind"] in ("exact", "delta"):
            x = rs.randint(-64, 65, (rx, rx)) / 64.0
            z = rs.randint(-64, 65, (rz, rz)) / 64.0
            if c["kind"] == "delta":
                u, v = delta_tap(rz, k)
                live = (1 + k) / 64.0 * (-1) ** k                                     # a distinct non-zero value per plane
                z = np.zeros((rz, rz))
                z[u, v] = live
        elif c["kind"] == "range":
            x = rs.standard_normal((rx, rx)) * 10.0 ** rs.uniform(-6, 6, (rx, rx))
            z = rs.standard_normal((rz, rz)) * 10.0 ** rs.uniform(-6, 6, (rz, rz))
        else:
            x = rs.standard_normal((rx, rx))
            z = rs.standard_normal((rz, rz))
        if c["kind"] == "zeros":
            sign = np.where(rs.uniform(size=(rx, rx)) < 0.5, -0.0, 0.0)
            if k == 0:
                x = sign                                                            # an all-zero plane of both signs
            if k == 1:
                z = np.where(rs.uniform(size=(rz, rz)) < 0.5, -0.0, 0.0)            # an all-zero template of both signs
        if c["kind"] == "nfzero" and k == 1:
            z[nf_zero_tap(c)] = 0.0
        xs.append(x)
        zs.append(z)
    n, ch = SPLIT[p]
    x = torch.from_numpy(np.stack(xs).astype(F32)).reshape(n, ch, rx, rx)
    z = torch.from_numpy(np.stack(zs).astype(F32)).reshape(n, ch, rz, rz)
    return x, z


@functools.lru_cache(maxsize=None)
def planted(name):
    """(x, z) of a non-finite case with its five values planted."""
    c = CASES[name]
    x, z = [t.clone() for t in inputs(name)]
    xf, zf = x.view(c["planes"], c["rx"], c["rx"]), z.view(c["planes"], c["rz"], c["rz"])
    pos = nf_positions(c)
    xf[pos["x_nan"]] = float("nan")
    xf[pos["x_pinf"]] = float("inf")
    xf[pos["x_ninf"]] = float("-inf")
    zf[pos["z_nan"]] = float("nan")
    zf[pos["z_inf"]] = float("inf")
    return x, z


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref64, mag and the a-priori bound of a case (of the planted data for the non-finite kinds)."""
    x, z = planted(name) if CASES[name]["kind"] in ("nfzero", "nfnonzero") else inputs(name)
    return dict(ref=ref64(x, z), mag=mag(x, z), bound=bound(x, z))


# =========================================================================================================================
# Part A: the assertions (GPU tests and CPU rehearsal alike)
# =========================================================================================================================
def _bits(t):
    return t.contiguous().view(torch.int32)


def check_exact(xcorr, name):
    """Kind 1: on the k / 64 grid every fp32 fmaf is exact in any order: the result IS the fp64 sum.  No tolerance."""
    x, z = inputs(name)
    out = xcorr(x, z)
    want = reference(name)["ref"].float()
    assert out.shape == want.shape, "%s: shape %s, expected %s" % (name, tuple(out.shape), tuple(want.shape))
    assert torch.equal(out, want), "%s: %d of %d outputs differ from the exact sum (max |d| %.3e)" % (
        name, int((out != want).sum()), want.numel(), float((out.double() - want.double()).abs().max()))


def error_ratio(out, ref):
    """max |out - ref64| / mag over the outputs with a finite reference and a non-zero mag."""
    sel = torch.isfinite(ref["ref"]) & (ref["mag"] > 0) & torch.isfinite(ref["mag"])
    if not bool(sel.any()):
        return 0.0
    return float(((out.double() - ref["ref"]).abs()[sel] / ref["mag"][sel]).max())


def check_bound(xcorr, name):
    """Kind 2: |out - ref64| <= rz^2 * 2^-24 * mag (+ 1e-30), and the project's own 1e-6 * mag where it states it (normal
    data, at most 225 taps).  Returns max err / mag."""
    c = CASES[name]
    x, z = inputs(name)
    out = xcorr(x, z)
    ref = reference(name)
    assert out.shape == ref["ref"].shape
    assert bool(torch.isfinite(out).all()), "%s: non-finite output on finite data" % name
    err = (out.double() - ref["ref"]).abs()
    ratio = error_ratio(out, ref)
    assert bool((err <= ref["bound"]).all()), "%s: %d outputs beyond rz^2 2^-24 mag, max err / mag %.3e (bound %.3e)" % (
        name, int((err > ref["bound"]).sum()), ratio, c["rz"] ** 2 * U24)
    if c["kind"] == "normal" and c["rz"] ** 2 <= PROJECT_TAPS:
        assert bool((err <= PROJECT_RATIO * ref["mag"] + 1e-30).all()), "%s: max err / mag %.3e" % (name, ratio)
    return ratio


def check_nonfinite(xcorr, name):
    """Kind 3: the NaN mask and the +-inf cells are the reference's, every other output meets the bound of kind 2, and the
    planes without a planted value are bit-equal to the same call without any planted value.  Returns max err / mag over
    the finite outputs."""
    c = CASES[name]
    x, z = planted(name)
    out = xcorr(x, z)
    clean = xcorr(*inputs(name))
    ref = reference(name)
    r = ref["ref"]
    assert out.shape == r.shape
    assert torch.equal(torch.isnan(out), torch.isnan(r)), "%s: NaN mask differs in %d cells (got %d NaN, reference %d)" % (
        name, int((torch.isnan(out) != torch.isnan(r)).sum()), int(torch.isnan(out).sum()), int(torch.isnan(r).sum()))
    for what, sel in (("+inf", torch.isposinf), ("-inf", torch.isneginf)):
        assert torch.equal(sel(out), sel(r)), "%s: %s cells differ in %d places" % (name, what, int((sel(out) != sel(r)).sum()))
    fin = torch.isfinite(r)
    err = (out.double() - r).abs()
    assert bool((err[fin] <= ref["bound"][fin]).all()), "%s: finite outputs beyond the bound, max err / mag %.3e" % (
        name, error_ratio(out, ref))
    p = c["planes"]
    o, k = out.reshape(p, -1), clean.reshape(p, -1)
    for plane in NF_CLEAN:
        assert torch.equal(_bits(o[plane]), _bits(k[plane])), "%s: clean plane %d changed with its neighbours' values" % (
            name, plane)
    return error_ratio(out, ref)


def check_zeros(xcorr, name):
    """Kind 4: an all-zero plane (plane 0) and an all-zero template (plane 1), of both signs, give exact +0 planes; the
    whole result has the bits of the reference after +0 is added to both (-0 and +0 are one value)."""
    x, z = inputs(name)
    out = xcorr(x, z)
    ref = reference(name)
    p = CASES[name]["planes"]
    o = out.reshape(p, -1)
    for plane in (0, 1):
        assert bool((_bits(o[plane]) == 0).all()), "%s: plane %d is not all +0 (%d cells)" % (
            name, plane, int((_bits(o[plane]) != 0).sum()))
    want = ref["ref"].float().reshape(p, -1)
    assert torch.equal(_bits(o[:2] + 0.0), _bits(want[:2] + 0.0))
    err = (out.double() - ref["ref"]).abs()
    assert bool((err <= ref["bound"]).all())


# ---- stand-ins for the rehearsal ----------------------------------------------------------------------------------------
def standin(x, z):
    """A correct fp32 implementation that is none of the kernels: torch's grouped convolution on the CPU."""
    n, c = x.shape[:2]
    out = F.conv2d(x.reshape(1, n * c, x.shape[2], x.shape[3]), z.reshape(n * c, 1, z.shape[2], z.shape[3]), groups=n * c)
    return out.reshape(n, c, out.shape[2], out.shape[3])


def fma_chain32(x, z, rows=False):
    """The kernels' fp32 accumulation, emulated: the product of two fp32 numbers is exact in fp64, the sum is rounded to
    fp32 once per step (the fp64 rounding before it is 2^-29 of that).  ``rows=False``: one fmaf chain per output over all
    taps, u-major / v-minor (the 30/15 and 35/7 kernels, the oracle); ``rows=True``: one chain per template row, the row
    sums added in row order (the generic kernel)."""
    rz = z.shape[-1]
    ho = x.shape[-1] - rz + 1
    acc = torch.zeros(x.shape[:2] + (ho, ho), dtype=torch.float32)
    for u in range(rz):
        row = torch.zeros_like(acc) if rows else acc
        for v in range(rz):
            row = (x[:, :, u:u + ho, v:v + ho].double() * z[:, :, u:u + 1, v:v + 1].double() + row.double()).float()
        acc = (acc.double() + row.double()).float() if rows else row
    return acc


def _m_drop_last_tap(x, z):
    z = z.clone()
    z[..., -1, -1] = 0.0
    return standin(x, z)


def _m_transposed(x, z):
    return standin(x, z.transpose(-1, -2).contiguous())


def _m_shifted(x, z):
    return standin(torch.roll(x, -1, dims=-1), z)


def _m_last_column(x, z):
    out = standin(x, z).clone()
    if out.shape[-1] >= 2:
        out[..., -1] = out[..., -2]
    return out


def _m_tail_swap(x, z):
    out = standin(x, z)
    n, c = out.shape[:2]
    p = n * c
    if p % 2 == 1 and p >= 3:
        flat = out.reshape(p, -1).clone()
        flat[[p - 2, p - 1]] = flat[[p - 1, p - 2]]
        out = flat.reshape(out.shape)
    return out


def _m_skip_zero_taps(x, z):
    """inf * 0 skipped: a zero tap contributes nothing whatever it meets (a kernel that tests its taps)."""
    rz = z.shape[-1]
    ho = x.shape[-1] - rz + 1
    out = x.new_zeros(x.shape[:2] + (ho, ho))
    for u in range(rz):
        for v in range(rz):
            tap = z[:, :, u:u + 1, v:v + 1]
            term = x[:, :, u:u + ho, v:v + ho] * tap
            out = out + torch.where(tap == 0, torch.zeros_like(term), term)
    return out


MUTANTS = {"last tap dropped": _m_drop_last_tap, "template transposed": _m_transposed,
           "window shifted by one column": _m_shifted, "last output column from Ho - 2": _m_last_column,
           "tail plane pair swapped": _m_tail_swap, "inf * 0 skipped": _m_skip_zero_taps}


def run_checks(xcorr, names):
    """The assertions of kinds 1-3 over ``names`` -> the names of the cases that failed."""
    failed = []
    for name in names:
        kind = CASES[name]["kind"]
        check = check_exact if kind in ("exact", "delta") else check_bound if kind in ("normal", "range") else check_nonfinite
        try:
            check(xcorr, name)
        except AssertionError:
            failed.append(name)
    return failed


# ---- part C: the generic kernel's dynamic LDS --------------------------------------------------------------------------
LDS_OPTIN = (128, 3)                 # (128^2 + 9) * 4 = 65,572 B: the smallest square plane above 64 KiB
LDS_REFUSED = (203, 3)               # (203^2 + 9) * 4 = 164,872 B > 160 KiB: refused before any launch


def lds_bytes(rx, rz):
    return (rx * rx + rz * rz) * 4


@functools.lru_cache(maxsize=None)
def lds_inputs():
    rx, rz = LDS_OPTIN
    rs = np.random.RandomState(128003)
    x = torch.from_numpy((rs.randint(-64, 65, (1, 1, rx, rx)) / 64.0).astype(F32))
    z = torch.from_numpy((rs.randint(-64, 65, (1, 1, rz, rz)) / 64.0).astype(F32))
    return x, z


# =========================================================================================================================
# Part B: the head's general path
# =========================================================================================================================
IMAGE_WH = (256, 128)
SCALES = (0.25, 0.125, 0.0625, 0.03125)
PAD_PIXELS = 128
TRACKS = 6
BATCH_ROWS = (2, 0, 4)
# name -> (rz, search_region, sampling_ratio, channels); rx = int(rz * search_region)
HEAD_CASES = {
    "18_3": (3, 6.0, 2, 32),
    "29_1": (1, 29.0, 2, 32),
    "20_9": (9, 2.25, 2, 32),
    "45_15": (15, 3.0, 2, 32),
    "21_7": (7, 3.0, 2, 32),
    "30_15_ratio1": (15, 2.0, 1, 32),
    "35_7_ratio3": (7, 5.0, 3, 32),
    "18_3_c64": (3, 6.0, 2, 64),
}
HEAD_SHAPES = {"18_3": (18, 16), "29_1": (29, 29), "20_9": (20, 12), "45_15": (45, 31), "21_7": (21, 15),
               "30_15_ratio1": (30, 16), "35_7_ratio3": (35, 29), "18_3_c64": (18, 16)}                  # name -> (rx, Ho)
HEAD_NAMES = tuple(HEAD_CASES)
WINOGRAD_HEADS = tuple(k for k in HEAD_NAMES if HEAD_SHAPES[k][1] in (16, 29))
GN_GROUPS, GN_EPS = 32, 1e-5
HEAD_SEEDS = {k: 8100 + 17 * i for i, k in enumerate(HEAD_NAMES)}
BOX_ATOL, CONF_ATOL = 2e-2, 1e-5     # the bounds of test_hip_parity._check_decode / test_decode_edges._judge


def head_cfg(name):
    rz, region, ratio, channels = HEAD_CASES[name]
    return O.EMMConfig(channels=channels, rz=rz, search_region=region, sampling_ratio=ratio, scales=SCALES,
                       pad_pixels=PAD_PIXELS, min_search_wh=0, use_centerness=True, sigma=0.4, amodal=False,
                       gn_groups=GN_GROUPS, gn_eps=GN_EPS)


def head_boxes(name):
    """Six template boxes whose search regions (about twice the listed size, whatever the case's SEARCH_REGION) lie inside
    the image (tracks 0, 5), cross its border (1, 2) or belong to boxes that are partly outside it themselves (3, 4)."""
    region = HEAD_CASES[name][1]
    W, H = IMAGE_WH
    f = 2.0 / region
    # (centre x, centre y, width, height) at SEARCH_REGION 2
    spec = ((128.0, 64.0, 24.0, 40.0), (20.5, 60.0, 40.0, 24.0), (150.0, 112.25, 16.0, 16.0),
            (W - 8.0, 50.0, 60.0, 50.0), (4.0, 6.5, 30.0, 70.0), (200.0, 40.0, 12.0, 20.0))
    out = []
    for cx, cy, w, h in spec:
        w, h = w * f, h * f
        out.append((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2))
    out = np.array(out, dtype=F32)
    # boxes 3 and 4 stick out of the image at every SEARCH_REGION: their far side is placed outside explicitly
    out[3, 2] = W + 6.0
    out[4, 0], out[4, 1] = -5.0, -4.0
    return out


@functools.lru_cache(maxsize=None)
def head_inputs(name):
    """Maps A and B of three images ([3, C, H_l, W_l] per level, fp32 numpy), the six boxes and the predictor's parameters.
    The one-image tests use image 0 with all six boxes; the batched test gives the images ``BATCH_ROWS`` of them."""
    channels = HEAD_CASES[name][3]
    rs = np.random.RandomState(HEAD_SEEDS[name])
    shapes = [(3,) + s[1:] for s in gi.feature_shapes(IMAGE_WH, channels)]
    feats_a = [rs.standard_normal(s).astype(F32) for s in shapes]
    feats_b = [rs.standard_normal(s).astype(F32) for s in shapes]
    boxes = head_boxes(name)
    # regression biases of half a (SEARCH_REGION 2) box side: the template boxes of a wide search region are a few pixels
    params = gi.predictor_params(rs, channels, boxes)
    return dict(features_a=feats_a, features_b=feats_b, boxes=boxes, params=params)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _image0(feats, dtype):
    return [_t(f[:1], dtype) for f in feats]


def decode_cfg(cfg):
    return dict(rx=cfg.rx, rz=cfg.rz, pad_pixels=cfg.pad_pixels, use_centerness=cfg.use_centerness, sigma=cfg.sigma)


def oracle_eval64(d, cfg):
    """decode_edge_cases.oracle_eval in fp64 for in-regime maps (finite scores: no cell on the overflow border)."""
    t = lambda k: torch.from_numpy(np.asarray(d[k])).double()                       # noqa: E731
    up = [O.bicubic_upsample(t(k)) for k in ("cls", "center", "reg")]
    score, _ = O.score_map(up[0], up[1], up[2], t("boxes"), cfg["use_centerness"], cfg["sigma"])
    score = score.numpy()
    assert np.isfinite(score).all()
    return dict(score=score, idx=D.first_argmax(score), borderline=np.zeros(score.shape, bool))


@functools.lru_cache(maxsize=None)
def head_oracle(name):
    """The CPU oracle on image 0 of a case: templates and search regions (fp32), the whole forward in fp32 and in fp64 with
    every intermediate, and the decode oracle's evaluation of both sets of logits."""
    cfg, inp = head_cfg(name), head_inputs(name)
    out = dict(cfg=cfg)
    for key, dt in (("f32", torch.float32), ("f64", torch.float64)):
        fa, fb = _image0(inp["features_a"], dt), _image0(inp["features_b"], dt)
        boxes = _t(inp["boxes"], dt)
        params = {k: _t(v, dt) for k, v in inp["params"].items()}
        z, sr = O.extract_cache(cfg, fa, boxes)
        bb, conf, keep, inter = O.emm_forward(cfg, params, fb, boxes, sr, z, IMAGE_WH, return_intermediates=True)
        out[key] = dict(z=z, sr=sr, bb=bb, conf=conf, inter=inter)
    i32, i64 = out["f32"]["inter"], out["f64"]["inter"]
    d32 = dict(cls=i32["cls"].numpy(), center=i32["center"].numpy(), reg=i32["reg"].numpy(), boxes=inp["boxes"],
               sr=out["f32"]["sr"].numpy())
    d64 = dict(cls=i64["cls"].numpy(), center=i64["center"].numpy(), reg=i64["reg"].numpy(),
               boxes=inp["boxes"].astype(np.float64))
    out["decode32"] = D.oracle_eval(d32, decode_cfg(cfg), IMAGE_WH)
    out["decode64"] = oracle_eval64(d64, decode_cfg(cfg))
    # the predictor's conditions, on the fp32 oracle's own response (as test_predictor_edges states them)
    resp = i32["response"]
    p32 = {k: _t(v) for k, v in inp["params"].items()}
    p64 = {k: _t(v, torch.float64) for k, v in inp["params"].items()}
    ref64_ = torch.cat(O.predictor(resp.double(), p64, GN_GROUPS, GN_EPS), 1)
    ref32_ = torch.cat(O.predictor(resp, p32, GN_GROUPS, GN_EPS), 1)
    out["pred_scale"] = ref64_.abs().amax(dim=(0, 2, 3), keepdim=True)
    out["pred_err32"] = P.scaled_error(ref32_, ref64_, out["pred_scale"])
    return out


def predictor_refs(resp, params):
    """O.predictor on a response in fp64 and fp32 -> (ref64, ref32, channel scale of ref64)."""
    p32 = {k: _t(v) for k, v in params.items()}
    p64 = {k: _t(v, torch.float64) for k, v in params.items()}
    r64 = torch.cat(O.predictor(resp.double(), p64, GN_GROUPS, GN_EPS), 1)
    r32 = torch.cat(O.predictor(resp.float(), p32, GN_GROUPS, GN_EPS), 1)
    return r64, r32, r64.abs().amax(dim=(0, 2, 3), keepdim=True)


def assert_close(got, ref, rtol, atol, what):
    """test_hip_parity._assert_close: |got - ref| <= atol + rtol * |ref| element-wise."""
    got, ref = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = err > atol + rtol * np.abs(ref)
    assert not bad.any(), "%s: %d/%d elements out of tolerance, max err %.3e" % (what, bad.sum(), bad.size, err.max())


def judge(what, orc, bb, conf, idx):
    """The adjudication of test_decode_edges._judge on numpy results: no failed track, at most 1 in
    ``decode_edge_cases.EXCUSED_PER_TRACKS`` excused, boxes within 2e-2 px and confidences within 1e-5 where the cell is the
    oracle's.  Returns (identical, excused)."""
    verdicts = D.adjudicate(orc, idx)
    same = np.array([v[0] == "same" for v in verdicts])
    excused = ["track %d: %s" % (k, v[1]) for k, v in enumerate(verdicts) if v[0] == "excused"]
    failed = ["track %d: %s" % (k, v[1]) for k, v in enumerate(verdicts) if v[0] == "fail"]
    assert not failed, "%s: %d / %d tracks elect a cell the rule does not admit:\n  %s" % (
        what, len(failed), len(same), "\n  ".join(failed))
    assert len(excused) <= len(same) // D.EXCUSED_PER_TRACKS, "%s: %d of %d tracks excused (at most 1 in %d):\n  %s" % (
        what, len(excused), len(same), D.EXCUSED_PER_TRACKS, "\n  ".join(excused))
    ok_b = D.same_class_close(bb[same], orc["bb"][same], BOX_ATOL)
    ok_c = D.same_class_close(conf[same], orc["conf"][same], CONF_ATOL)
    assert ok_b.all(), "%s: boxes of identical cells differ:\n%s\nvs oracle\n%s" % (what, bb[same], orc["bb"][same])
    assert ok_c.all(), "%s: confidences differ: %s vs oracle %s" % (what, conf[same], orc["conf"][same])
    return int(same.sum()), len(excused)
