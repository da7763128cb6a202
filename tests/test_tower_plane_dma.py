"""The split (two-part fp16) form of the 16 x 16 prediction towers (csrc/tower_wino.hip) where its staging of the response
planes can go wrong: the LDS image of a plane (row order, column chunks), the zero halo on all four sides, the ring of stage
buffers over several K blocks, launches that follow one another on one workspace, and a non-finite cell next to the halo.

Everything goes through ``ops.emm_predictor`` / ``smot_emm_predictor_fwd``.  Yardstick: ``oracle.emm_oracle.predictor`` (conv2d
-> GroupNorm -> ReLU -> heads) on the CPU in fp64; measure and bound: test_hip_parity.test_predictor_vs_oracle's, max |out -
ref| / max_channel |ref64| < 1e-4 (no intermediate of the towers is exposed, so the halo cases use this bound too: a missing
or displaced halo cell moves the convolution's border outputs by whole filter taps, four orders of magnitude above it).

Shapes: C = 32 (one K block: prologue fetches, ring wrap and tail overlap), 64 (the generic loop) and 128 (the unrolled loop),
each at N = 1 — the smallest N at which ``smot_emm_tower_form`` reports the split form — and N = 2 (no multiple of 8: the
grid is padded to the XCD count)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import emm_oracle as O

DEV = "cuda:0"
F32 = np.float32
TOL64 = 1e-4
BOXES = np.array([[0, 0, 80, 120]], dtype=F32)
CHANNELS = (32, 64, 128)
SHAPES = tuple((c, n) for c in CHANNELS for n in (1, 2))
# the four corners and one cell on each of the four edges of the 16 x 16 map
BORDER_CELLS = ((0, 0), (0, 15), (15, 0), (15, 15), (0, 6), (15, 9), (5, 0), (10, 15))


@functools.lru_cache(maxsize=None)
def params_of(c):
    return gi.predictor_params(np.random.RandomState(3100 + c), c, BOXES)


@functools.lru_cache(maxsize=None)
def ones_params(c):
    p = dict(params_of(c))
    for t in ("cls_tower", "reg_tower"):
        p[t + ".0.weight"] = np.ones((c, c, 3, 3), dtype=F32)
    return p


def oracle64(resp, params):
    out = O.predictor(torch.from_numpy(resp).double(), {k: torch.from_numpy(v).double() for k, v in params.items()}, 32, 1e-5)
    return torch.cat(out, 1)


def scaled_error(got, ref):
    scale = ref.abs().amax(dim=(0, 2, 3), keepdim=True)
    assert float(scale.min()) >= 1e-3
    return float(((got.double() - ref).abs() / scale).max())


@functools.lru_cache(maxsize=None)
def random_resp(c, n):
    return (np.random.RandomState(3200 + 7 * c + n).standard_normal((n, c, 16, 16)) * 15.0).astype(F32)


@functools.lru_cache(maxsize=None)
def distinct_resp(c, n):
    """cell = f(track, channel, row, col), no two equal: an odd multiplier permutes the cell index modulo a power of two."""
    count = n * c * 256
    mod = 1 << int(np.ceil(np.log2(count)))
    idx = (np.arange(count, dtype=np.int64) * 40503 + 977) % mod
    resp = ((idx.astype(np.float64) - mod / 2) * (30.0 / mod)).astype(F32).reshape(n, c, 16, 16)
    assert np.unique(resp).size == count
    return resp


@functools.lru_cache(maxsize=None)
def impulse_resp(c):
    """Track t: one impulse per plane at BORDER_CELLS[t], its size and sign depending on the channel."""
    resp = np.zeros((len(BORDER_CELLS), c, 16, 16), dtype=F32)
    amp = (8.0 + np.arange(c) % 7) * np.where(np.arange(c) % 3 == 0, -1.0, 1.0)
    for t, (r, col) in enumerate(BORDER_CELLS):
        resp[t, :, r, col] = amp
    return resp


@functools.lru_cache(maxsize=None)
def expected(kind, c, n):
    if kind == "random":
        return oracle64(random_resp(c, n), params_of(c))
    if kind == "distinct":
        return oracle64(distinct_resp(c, n), params_of(c))
    if kind == "ones":
        return oracle64(np.ones((n, c, 16, 16), dtype=F32), ones_params(c))
    assert kind == "impulse"
    return oracle64(impulse_resp(c), params_of(c))


# ---- CPU: what the inputs are meant to be --------------------------------------------------------------------------------
def test_inputs_are_what_the_cases_need():
    assert all(n % 8 for _, n in SHAPES)
    for c in CHANNELS:
        imp = impulse_resp(c)
        assert all(int((imp[t, ch] != 0).sum()) == 1 for t in range(len(BORDER_CELLS)) for ch in (0, c - 1))
        assert {(r in (0, 15)) + (col in (0, 15)) for r, col in BORDER_CELLS} == {1, 2}
        # all-ones response and filters: the convolution is 9 C inside, 6 C on an edge, 4 C in a corner
        y = torch.nn.functional.conv2d(torch.ones(1, c, 16, 16, dtype=torch.float64),
                                       torch.ones(1, c, 3, 3, dtype=torch.float64), padding=1)[0, 0]
        assert y[5, 5] == 9 * c and y[0, 5] == 6 * c and y[5, 15] == 6 * c and y[0, 0] == 4 * c and y[15, 15] == 4 * c
        distinct_resp(c, 2)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import siammot_amd.ops as ops_mod
    ops_mod.load_library()
    return ops_mod


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


_dev_params_cache = {}


def _dev_params(key, params):
    if key not in _dev_params_cache:
        _dev_params_cache[key] = {k: _dev(v) for k, v in params.items()}
    return _dev_params_cache[key]


def _run(ops, resp, pkey, params):
    n, c = resp.shape[:2]
    assert ops.tower_form(n, c, 16) == 3, "N = %d, C = %d does not select the split form" % (n, c)
    out = ops.emm_predictor(_dev(resp), _dev_params(pkey, params))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CHANNELS)
def test_smallest_split_form_track_count(ops, c):
    assert next(n for n in range(1, 65) if ops.tower_form(n, c, 16) == 3) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("c,n", SHAPES)
def test_random_response_against_the_oracle(ops, c, n):
    e = scaled_error(_run(ops, random_resp(c, n), ("p", c), params_of(c)), expected("random", c, n))
    print("plane-dma random   C %3d N %d  vs fp64 %.3e" % (c, n, e))
    assert e < TOL64


@pytest.mark.gpu
@pytest.mark.parametrize("c,n", SHAPES)
def test_every_row_and_column_distinct(ops, c, n):
    """A permuted, duplicated or dropped 16-byte chunk of a plane changes the convolution everywhere around it."""
    e = scaled_error(_run(ops, distinct_resp(c, n), ("p", c), params_of(c)), expected("distinct", c, n))
    print("plane-dma distinct C %3d N %d  vs fp64 %.3e" % (c, n, e))
    assert e < TOL64


@pytest.mark.gpu
@pytest.mark.parametrize("c,n", SHAPES)
def test_halo_all_ones(ops, c, n):
    """Response and tower filters all ones: border and corner outputs of the convolution are 6 C and 4 C against 9 C inside;
    a halo cell that is not zero, or an interior cell taken for one, changes them by a multiple of C."""
    out = _run(ops, np.ones((n, c, 16, 16), dtype=F32), ("ones", c), ones_params(c))
    e = scaled_error(out, expected("ones", c, n))
    print("plane-dma ones     C %3d N %d  vs fp64 %.3e" % (c, n, e))
    assert e < TOL64


@pytest.mark.gpu
@pytest.mark.parametrize("c", CHANNELS)
def test_halo_impulses_on_edges_and_corners(ops, c):
    """One impulse per plane on each of the four edges and in each of the four corners (one track each): a wrong row order
    or a wrong column neighbour shows as a displaced or wrapped stencil."""
    out = _run(ops, impulse_resp(c), ("p", c), params_of(c))
    ref = expected("impulse", c, len(BORDER_CELLS))
    for t, cell in enumerate(BORDER_CELLS):
        e = scaled_error(out[t:t + 1], ref[t:t + 1])
        print("plane-dma impulse  C %3d at %-8s vs fp64 %.3e" % (c, cell, e))
        assert e < TOL64, "impulse at %s" % (cell,)


def _entry(ops, resp, params, tower_ws, logits):
    """The C entry on the caller's workspace and output buffers."""
    lib = ops.load_library()
    n, c = resp.shape[:2]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                                       # noqa: E731
    rc = lib.smot_emm_predictor_fwd(ptr(resp), n, c, 16, *[ptr(params[k]) for k in ops.PREDICTOR_KEYS], 32, 1e-5,
                                    ptr(ops.tower_packed(params)), ptr(tower_ws), ptr(logits),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.smot_last_error()
    torch.cuda.synchronize()
    return logits[:n].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CHANNELS)
def test_second_launch_on_the_same_workspace(ops, c):
    """Three tracks of large values, then two tracks of other data on the same workspace and output buffers: the second
    result is the fresh-workspace run's, bit for bit."""
    params = _dev_params(("p", c), params_of(c))
    first = _dev(random_resp(c, 2)[[0, 1, 0]] * F32(1000.0))
    second = _dev(distinct_resp(c, 2))
    tower_ws = torch.empty((3, 2 * c, 16, 16), device=DEV)
    logits = torch.empty((3, 7, 16, 16), device=DEV)
    _entry(ops, first, params, tower_ws, logits)
    got = _entry(ops, second, params, tower_ws, logits)
    fresh = ops.emm_predictor(second, params).cpu()
    assert torch.equal(got, fresh)
    assert scaled_error(got, expected("distinct", c, 2)) < TOL64


@pytest.mark.gpu
@pytest.mark.parametrize("c", CHANNELS)
def test_zero_track_between_two_large_ones(ops, c):
    """Nothing of the neighbours' planes leaks into a track of zeros through the gaps of the staging image."""
    params = _dev_params(("p", c), params_of(c))
    resp = random_resp(c, 2)[[0, 1, 1]] * F32(1000.0)
    resp[1] = 0.0
    out = ops.emm_predictor(_dev(resp), params).cpu()
    alone = ops.emm_predictor(_dev(resp[1:2]), params).cpu()
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out[1], alone[0])
    assert scaled_error(out, oracle64(resp, params_of(c))) < TOL64


@pytest.mark.gpu
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("cell", [(0, 3), (7, 15), (15, 15)])
def test_infinite_cell_on_the_edge_stays_in_its_track(ops, c, cell):
    """One inf on the map's edge, next to the zero halo, in the middle track of three: the other tracks' logits are those
    of the run without it, bit for bit."""
    params = _dev_params(("p", c), params_of(c))
    resp = random_resp(c, 2)[[0, 1, 0]].copy()
    clean = ops.emm_predictor(_dev(resp), params).cpu()
    resp[1, c // 2, cell[0], cell[1]] = np.inf
    out = ops.emm_predictor(_dev(resp), params).cpu()
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("c,n", SHAPES)
def test_three_launches_are_bitwise_equal(ops, c, n):
    params = _dev_params(("p", c), params_of(c))
    resp = _dev(random_resp(c, n))
    runs = [ops.emm_predictor(resp, params).cpu() for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
