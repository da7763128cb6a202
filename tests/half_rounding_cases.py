"""Value tables and constructions of tests/test_half_rounding.py — TEST INFRASTRUCTURE.

The half compute mode rounds activations as they are loaded and filters as they are packed with
``tensor.to``'s rounding — round to nearest, ties to even (RNE), overflow to +-inf — multiplies exactly and accumulates in
fp32.  The tests of that mode compare against ``dla_half_cases.rnd``; this file is what tests the sentence itself, with no
tolerance: each output is made to equal ONE rounded operand times +-1, every other term of its sum being an exact zero.

The value tables
    ``edge_table(ct)``: fp32 values at which a wrong rounding shows, closed under negation, every one finite after the
    rounding.  A probe value b enters as nextafter(b, 0), b, nextafter(b, inf) (fp32 neighbours).  fp16: the ties 1 + 2^-11
    (down to even), 1 + 3 2^-11 (up to even), 2 - 2^-11 (carries into the next binade); 65,504 and the largest fp32 below
    65,520; the subnormals 2^-24, 1023 2^-24, the ties 2^-25 (-> 0), 1.5 2^-24 and 2.5 2^-24 (both -> 2 2^-24) and
    2^-14 - 2^-25 (carries into the normal range), 2^-26 and the fp32 subnormal 2^-130 (-> 0), 2^-14; +-0, 1.0, an ordinary
    value.  bf16: the analogues (8 significant bits; the subnormals lie below 2^-126, where fp32's do).
    ``overflow_pairs(ct)``: (largest fp32 that still rounds to a finite value, smallest fp32 that rounds to inf), and the
    negated pair.
    ``rne`` / ``toward_zero`` / ``half_away``: the three roundings in exact numpy arithmetic (an fp32 value and every power
    of two used are exact in fp64; the quotient by the quantum has at most 24 significant bits) — independent of torch and
    of numpy's own float16.  ``rne`` is what the CPU tests hold ``dla_half_cases.rnd`` to.

Activation read-back (selection filters)
    The input is filled with table entries (``fill``: every entry occurs).  Every output channel's filter has exactly one
    non-zero element, +-1, at input channel ``ic[oc]`` of a seeded map oc -> ic and one tap (``selection3`` / ``selection1``):
    the output is the shifted / strided slice of ``+-rnd(x)`` (``shifted``), zeros from the padding.  Values are compared,
    not bits: a selected -0 is summed with +0 terms.

Filter read-back (delta images)
    The filters are filled with table entries.  Input channel ic is zero except for one cell of +-1 (``deltas3``: cells three
    apart on a grid, so that any 3x3 window holds at most one; ``deltas1``: position p carries channel p).  ``scatter3`` walks
    (channel, tap) and writes ``+-rnd(w)[oc, ic, ky, kx]`` where the output position that reads the cell through that tap
    exists, refuses two writes to one position and returns the coverage mask of the filter elements read.

Sums inside one matrix instruction
    ``three_terms``: channels carrying 2^a or 2^(a - s), filters +1, -1, +1 on two big and one small channel per output
    channel: any fp32 accumulation, in any order, returns 2^(a - s) exactly (every partial sum is representable).
"""
import numpy as np

from dla_half_cases import TYPES, rnd  # noqa: F401  (re-exported: the yardstick under test)

F32 = np.float32
# (significant bits, smallest normal exponent, largest finite value)
FORMAT = {"fp16": (11, -14, 65504.0), "bf16": (8, -126, float(np.uint32(0x7f7f0000).view(F32)))}


# ---- the three roundings, in exact arithmetic -------------------------------------------------------------------------
def _round(a, ct, rule):
    """``a`` (fp32) rounded to ``ct`` under ``rule`` ("even", "zero", "away") -> fp32.  v = n q with the quantum q = 2^(max(e,
    emin) - (bits - 1)), e = floor(log2 |v|): n is exact in fp64, its integer and fractional parts too."""
    bits, emin, top = FORMAT[ct]
    a = np.asarray(a, dtype=F32)
    v = np.abs(a.astype(np.float64))
    _, ex = np.frexp(v)                                          # |v| = m 2^ex, m in [0.5, 1): e = ex - 1
    q = np.ldexp(1.0, np.maximum(ex - 1, emin) - (bits - 1))
    n = v / q
    lo = np.floor(n)
    frac = n - lo
    if rule == "even":
        up = (frac > 0.5) | ((frac == 0.5) & (np.mod(lo, 2.0) == 1.0))
    elif rule == "away":
        up = frac >= 0.5
    else:
        up = np.zeros(n.shape, dtype=bool)
    r = (lo + up) * q
    r = np.where(r > top, np.inf, r)
    out = np.copysign(r, a.astype(np.float64)).astype(F32)
    assert np.array_equal(out.astype(np.float64), np.copysign(r, a.astype(np.float64)))        # nothing rounded on the way back
    return out


def rne(a, ct):
    return _round(a, ct, "even")


def toward_zero(a, ct):
    return _round(a, ct, "zero")


def half_away(a, ct):
    return _round(a, ct, "away")


# ---- the tables ------------------------------------------------------------------------------------------------------
def _f32(v):
    f = F32(v)
    assert float(f) == float(v), "%r is no fp32 value" % (v,)
    return f


def _bits32(u):
    return np.uint32(u).view(F32)


def _triple(b):
    b = _f32(b)
    return [np.nextafter(b, F32(0.0)), b, np.nextafter(b, F32(np.inf))]


def _closed(values):
    """Both signs of every value, one entry per bit pattern (+0 and -0 are two), in a fixed order."""
    a = np.array(values, dtype=F32)
    a = np.concatenate([a, -a])
    _, first = np.unique(a.view(np.uint32), return_index=True)
    return np.ascontiguousarray(a[np.sort(first)])


def overflow_pairs(ct):
    """[(largest fp32 that rounds to a finite ``ct`` value, smallest fp32 that rounds to inf), the negated pair]."""
    hi = _f32(65520.0) if ct == "fp16" else _bits32(0x7f7f8000)
    lo = np.nextafter(hi, F32(0.0))
    return [(lo, hi), (-lo, -hi)]


def edge_table(ct):
    p2 = lambda k: 2.0 ** k
    lo = overflow_pairs(ct)[0][0]
    if ct == "fp16":
        probes = [1 + p2(-11), 1 + 3 * p2(-11), 2 - p2(-11), 65504.0,
                  p2(-24), 1023 * p2(-24), p2(-25), 1.5 * p2(-24), 2.5 * p2(-24), p2(-14) - p2(-25), p2(-26), p2(-130), p2(-14),
                  0.0, 1.0, float(F32(3.14159274)), float(F32(0.1))]
    else:
        probes = [1 + p2(-8), 1 + 3 * p2(-8), 2 - p2(-9), 2 - p2(-8), float(_bits32(0x7f7f0000)),
                  p2(-133), 1.5 * p2(-133), 2.5 * p2(-133), p2(-134), p2(-126) - p2(-134), p2(-149), p2(-126), 127 * p2(-133),
                  0.0, 1.0, float(F32(3.14159274)), float(F32(0.1))]
    values = [v for b in probes for v in _triple(b)] + [np.nextafter(lo, F32(0.0)), lo]
    return _closed(values)


# ---- fills -----------------------------------------------------------------------------------------------------------
def fill(shape, table, seed):
    """An fp32 array of ``shape`` of table entries drawn by ``RandomState(seed)``, every entry at least once."""
    rs = np.random.RandomState(seed)
    n, T = int(np.prod(shape)), len(table)
    assert n >= T, "%d cells cannot hold %d table entries" % (n, T)
    idx = rs.randint(T, size=n)
    idx[rs.permutation(n)[:T]] = np.arange(T)
    return np.ascontiguousarray(table[idx].reshape(shape))


def holds_every_entry(a, table):
    """Every bit pattern of ``table`` occurs in ``a``."""
    return bool(np.isin(table.view(np.uint32), np.asarray(a, dtype=F32).view(np.uint32)).all())


# ---- selection filters -----------------------------------------------------------------------------------------------
def selection(Cout, K, seed, start=0, signed=True):
    """oc -> (k, sign): entries start .. start + Cout of a seeded permutation of the K input slots, continued with fresh
    permutations (calls with start = 0, Cout, 2 Cout, ... up to K read every slot; Cout = K: a permutation), and seeded signs."""
    rs = np.random.RandomState(seed)
    k = np.concatenate([rs.permutation(K) for _ in range((start + Cout + K - 1) // K)])[start:start + Cout]
    sign = rs.choice(np.array([-1.0, 1.0], dtype=F32), size=Cout) if signed else np.ones(Cout, dtype=F32)
    return k, sign


def selection3(Cout, Cin, tap, seed):
    """-> (w [Cout, Cin, 3, 3] with w[oc, ic[oc], tap] = sign[oc] and nothing else, ic, sign)."""
    ic, sign = selection(Cout, Cin, seed)
    w = np.zeros((Cout, Cin, 3, 3), dtype=F32)
    w[np.arange(Cout), ic, tap[0], tap[1]] = sign
    return w, ic, sign


def selection1(Cout, K, seed, start=0, signed=True):
    """-> (w [Cout, K, 1, 1], k, sign)."""
    k, sign = selection(Cout, K, seed, start, signed)
    w = np.zeros((Cout, K, 1, 1), dtype=F32)
    w[np.arange(Cout), k, 0, 0] = sign
    return w, k, sign


def shifted(xr, ic, sign, tap, stride):
    """What a 3x3 convolution (pad 1) with ``selection3``'s filters returns on ``xr``: out[n, oc, oy, ox] = sign[oc]
    xr[n, ic[oc], stride oy - 1 + ky, stride ox - 1 + kx], zero outside the map.  Slices of the zero-framed map."""
    N, _, H, W = xr.shape
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if stride == 2 else (H, W)
    framed = np.zeros((N, xr.shape[1], H + 2, W + 2), dtype=xr.dtype)
    framed[:, :, 1:H + 1, 1:W + 1] = xr
    ky, kx = tap
    cut = framed[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
    return np.ascontiguousarray(cut[:, ic] * sign.reshape(1, -1, 1, 1).astype(xr.dtype))


def pooled(x):
    """``max_pool2d(x, 2, 2)`` of a map [N, C, 2h (+ 1), 2w (+ 1)] by slices."""
    h, w = x.shape[2] // 2, x.shape[3] // 2
    q = [x[:, :, dy:2 * h:2, dx:2 * w:2] for dy in (0, 1) for dx in (0, 1)]
    return np.maximum(np.maximum(q[0], q[1]), np.maximum(q[2], q[3]))


# ---- delta images ----------------------------------------------------------------------------------------------------
def deltas3(Cin, size, signs, shifts=((0, 0),), seed=0):
    """Images [len(signs) * len(shifts), Cin, H, W]: channel ic is zero except at its cell, which holds the image's sign.  The
    cells sit three apart, at (1 + 3 i, 1 + 3 j) of a seeded assignment of the channels to a G x G grid (G = 6 holds 32
    channels on 18 x 18, G = 10 holds 96 on 30 x 30), moved by the image's shift (0 or 1 per axis: the four parities a
    stride-2 convolution reads).  -> (x, cells [image, ic] = (y, x), sign per image)."""
    H, W = size
    G = int(np.ceil(np.sqrt(Cin)))
    assert H >= 3 * G and W >= 3 * G and all(0 <= d <= 1 for sh in shifts for d in sh)
    rs = np.random.RandomState(seed)
    grid = rs.permutation(G * G)[:Cin]
    images = [(s, sh) for sh in shifts for s in signs]
    x = np.zeros((len(images), Cin, H, W), dtype=F32)
    cells = np.zeros((len(images), Cin, 2), dtype=np.int64)
    for n, (s, (dy, dx)) in enumerate(images):
        cells[n, :, 0], cells[n, :, 1] = 1 + 3 * (grid // G) + dy, 1 + 3 * (grid % G) + dx
        x[n, np.arange(Cin), cells[n, :, 0], cells[n, :, 1]] = s
    return x, cells, np.array([s for s, _ in images], dtype=F32)


def scatter3(wr, cells, signs, size, stride):
    """The output of a 3x3 convolution (pad 1) of ``deltas3``'s images with the filters ``wr`` [Cout, Cin, 3, 3], built by
    writing single elements: the output position (oy, ox) with stride oy - 1 + ky = cell y reads the cell through tap (ky, kx).
    No position is written twice (asserted: any 3x3 window holds at most one cell), so every output is one filter element
    times the image's sign.  -> (expected fp32, coverage mask like ``wr``)."""
    Cout, Cin = wr.shape[:2]
    H, W = size
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if stride == 2 else (H, W)
    out = np.zeros((len(signs), Cout, Ho, Wo), dtype=F32)
    seen = np.zeros(wr.shape, dtype=bool)
    for n, s in enumerate(signs):
        written = np.zeros((Ho, Wo), dtype=bool)
        for ic in range(Cin):
            cy, cx = cells[n, ic]
            for ky in range(3):
                for kx in range(3):
                    ny, nx = cy + 1 - ky, cx + 1 - kx
                    if ny % stride or nx % stride or not (0 <= ny // stride < Ho and 0 <= nx // stride < Wo):
                        continue
                    oy, ox = ny // stride, nx // stride
                    assert not written[oy, ox], "two cells in one window"
                    written[oy, ox] = True
                    out[n, :, oy, ox] = F32(s) * wr[:, ic, ky, kx]
                    seen[:, ic, ky, kx] = True
    return out, seen


def deltas1(K, size, signs):
    """Images [len(signs), K, H, W] for a 1x1 convolution: position p (row-major) carries the sign in channel p alone."""
    H, W = size
    assert H * W >= K
    x = np.zeros((len(signs), K, H * W), dtype=F32)
    for n, s in enumerate(signs):
        x[n, np.arange(K), np.arange(K)] = s
    return x.reshape(len(signs), K, H, W)


def gathered1(wr, size, signs):
    """The 1x1 convolution of ``deltas1``'s images with ``wr`` [Cout, K]: out[n, oc, p] = sign[n] wr[oc, p], zero from p = K on."""
    Cout, K = wr.shape
    out = np.zeros((len(signs), Cout, size[0] * size[1]), dtype=F32)
    for n, s in enumerate(signs):
        out[n, :, :K] = F32(s) * wr
    return out.reshape(len(signs), Cout, size[0], size[1])


# ---- three terms of one sum --------------------------------------------------------------------------------------------
def three_terms(Cout, K, a, s, spread, seed):
    """Channel values and filter rows for: +2^a, -2^a, +2^(a - s) per output channel.

    Channel k carries 2^(a - s) where k % 8 == small[k // 8] (one seeded slot per group of 8) and 2^a elsewhere.  Output
    channel oc takes two big channels (+1, -1) and one small one (+1): ``spread`` "group": all three inside one seeded group
    of 8; "groups": in three different groups of one block of 32; "blocks": in three different blocks of 32 (K >= 96).
    -> (values [K], rows [Cout, K], slots [Cout, 3] = the k of (+big, -big, +small))."""
    rs = np.random.RandomState(seed)
    ng = K // 8
    small = rs.randint(8, size=ng)
    values = np.full(K, 2.0 ** a, dtype=F32)
    values[8 * np.arange(ng) + small] = F32(2.0 ** (a - s))
    rows, slots = np.zeros((Cout, K), dtype=F32), np.zeros((Cout, 3), dtype=np.int64)
    for oc in range(Cout):
        if spread == "group":
            g = np.repeat(rs.randint(ng), 3)
        elif spread == "groups":
            g = 4 * rs.randint(K // 32) + rs.permutation(4)[:3]
        else:
            g = 4 * rs.permutation(K // 32)[:3] + rs.randint(4, size=3)
        bigs = lambda grp: [k for k in range(8 * grp, 8 * grp + 8) if k % 8 != small[grp]]
        kp = rs.choice(bigs(g[0]))
        km = rs.choice([k for k in bigs(g[1]) if k != kp])
        ks = 8 * g[2] + small[g[2]]
        rows[oc, kp], rows[oc, km], rows[oc, ks] = 1.0, -1.0, 1.0
        slots[oc] = (kp, km, ks)
    return values, rows, slots
