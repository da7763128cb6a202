"""The host binding's paths to the head and the extraction (ops._head_call / ops._extract_call): ``PairPlan`` — the per-frame
fast path of ``EMM.forward`` / ``EMM.extract_cache`` — against the general functions, and the rule that chooses the library
entry point.  The entry also chooses the kernels (the untyped entries run the single-image kernels, the typed entries the
batched ones even for one image), and a wrong choice raises no error: the calls are recorded by a proxy around the loaded
library that forwards every call unchanged.

The 30 / 15 head on two levels of small maps; 32 channels: the smallest count with a packed tower image (16-channel tiles)
that the 32 GroupNorm groups divide — ``PairPlan.track`` declines without the image.  One track writes no order hint, two
are the smallest count that does."""
import ctypes
import types

import numpy as np
import pytest
import torch

import golden_inputs as gi

DEV = "cuda:0"
C, WH, SCALES = 32, (160, 96), (0.25, 0.125)
RX, RZ, PAD, EXPANSION, MIN_WH, SIGMA = 30, 15, 512, 1.0, 0, 0.4
TU = types.SimpleNamespace(pad_pixels=PAD, search_expansion=EXPANSION, min_search_wh=MIN_WH)
FORMS = ["fp32", "fp16", "fp32_channels_last"]
BOXES = np.array([[10, 8, 60, 70], [70, 20, 150, 90], [5, 40, 40, 60], [90, 4, 120, 50], [30, 30, 130, 80]], dtype=np.float32)


class Recorder(object):
    """Forwards every call to the library and keeps (entry name, arguments)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def forward(*args):
            self.calls.append((name, args))
            return fn(*args)
        return forward

    def take(self, prefix):
        """The one recorded launch (``*_fwd``) whose entry name starts with ``prefix``; the record starts anew."""
        hits = [c for c in self.calls if c[0].startswith(prefix) and c[0].endswith("_fwd")]
        assert len(hits) == 1, [c[0] for c in self.calls]
        self.calls = []
        return hits[0]


@pytest.fixture
def rec(monkeypatch):
    import siammot_amd.ops as ops
    r = Recorder(ops.load_library())
    monkeypatch.setattr(ops, "_lib", r)
    return r


def _maps(form, seed, B=1):
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in (4, 8):
        f = torch.randn((B, C, WH[1] // s, WH[0] // s), generator=g).to(DEV)
        if form == "fp16":
            f = f.half()
        elif form == "fp32_channels_last":
            f = f.to(memory_format=torch.channels_last)
        out.append(f)
    return tuple(out)


def _inputs(form, N, B=1):
    boxes = torch.from_numpy(BOXES[:N].copy()).to(DEV)
    p = gi.predictor_params(np.random.RandomState(3), C, BOXES[:N])
    return _maps(form, 1, B), _maps(form, 2, B), boxes, {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}


def _plain(args, names):
    """A recorded argument tuple as plain values: handles as integers, host arrays as tuples, and the addresses that are the
    call's own — its outputs, the tensors an earlier call of the same chain put out (``names``: address -> label) and the
    scratch workspace (kept per stream handle, and the two paths spell the null stream differently) — as labels."""
    import siammot_amd.ops as ops
    names = dict(names)
    names.update({buf.data_ptr(): "workspace" for buf in ops._ws_cache.values()})
    out = []
    for a in args:
        if isinstance(a, ctypes.c_void_p):
            a = a.value or 0
        elif isinstance(a, ctypes.Array):
            a = tuple(a)
        out.append(names.get(a, a) if isinstance(a, int) and not isinstance(a, bool) else a)
    return tuple(out)


def _labels(**tensors):
    return {t.data_ptr(): k for k, t in tensors.items() if t is not None}


def _hint_body(oh):
    """An order hint without its status word (raised by a head that rejects the hint; not part of the list)."""
    import siammot_amd.ops as ops
    flat = oh.reshape(-1).clone()
    flat[ops.HINT_STATUS_WORD] = 0
    return flat


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("form", FORMS)
def test_pair_plan_equals_the_general_functions_in_results_entries_and_arguments(rec, form, N):
    import siammot_amd.ops as ops
    fa, fb, boxes, params = _inputs(form, N)
    dev = boxes.device
    assert ops.tower_packed(params) is not None
    typed = form != "fp32"
    if form == "fp32_channels_last":
        assert ops._levels_layout(fa, 2) == ops.FEAT_CHANNELS_LAST
    rec.calls = []

    # extraction
    z, sr, oh = ops.emm_extract_cache(fa, boxes, RZ, SCALES, 2, PAD, EXPANSION, MIN_WH, hint=True)
    name_g, args_g = rec.take("smot_emm_extract_cache")
    plan = ops.PairPlan(fa, dev, params, RX, RZ, SCALES, 2, PAD, TU)
    rec.calls = []
    got = plan.extract(fa, boxes, True)
    assert got is not None
    zp, srp, ohp = got
    name_p, args_p = rec.take("smot_emm_extract_cache")
    assert name_g == name_p == ("smot_emm_extract_cache_typed_fwd" if typed else "smot_emm_extract_cache_fwd")
    assert _plain(args_g, _labels(z=z, sr=sr, hint=oh)) == _plain(args_p, _labels(z=zp, sr=srp, hint=ohp))
    if typed:
        assert args_g[-3] == 1 and tuple(args_g[-2]) == (0, N) and args_g[-1] is None
    assert (oh is not None) == (N >= 2) and (ohp is not None) == (N >= 2)
    assert torch.equal(zp, z) and torch.equal(srp, sr)
    if oh is not None:
        assert torch.equal(_hint_body(ohp), _hint_body(oh))

    # head, each on its own extraction's outputs
    bb, conf = ops.emm_track(fb, boxes, sr, z, params, RX, RZ, SCALES, 2, PAD, sigma=SIGMA, use_centerness=True,
                             clip_wh=WH, order_hint=oh)
    name_g, args_g = rec.take("smot_emm_track")
    got = plan.track(fb, boxes, srp, zp, SIGMA, True, float(WH[0]), float(WH[1]), 32, 1e-5, ohp)
    assert got is not None
    bbp, confp = got
    name_p, args_p = rec.take("smot_emm_track")
    assert name_g == name_p == ("smot_emm_track_typed_fwd" if typed else "smot_emm_track_fwd")
    assert _plain(args_g, _labels(z=z, sr=sr, hint=oh, bb=bb, conf=conf)) == \
        _plain(args_p, _labels(z=zp, sr=srp, hint=ohp, bb=bbp, conf=confp))
    if typed:
        assert args_g[-2] == 1 and tuple(args_g[-1]) == (0, N)
        assert args_g[1] == ops.FEAT_TYPES[fa[0].dtype] | (ops.FEAT_CHANNELS_LAST if form == "fp32_channels_last" else 0)
    torch.cuda.synchronize()
    assert torch.equal(bbp, bb) and torch.equal(confp, conf)
    assert bool(torch.isfinite(bb).all()) and bool(torch.isfinite(conf).all())
    if oh is not None:
        assert ops.order_hint_status(oh) == 0 and ops.order_hint_status(ohp) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_masked_and_batched_rows_of_the_selection_table(rec, form):
    import siammot_amd.ops as ops
    N = 5
    typed = form != "fp32"
    fa, fb, boxes, params = _inputs(form, N)
    n_valid = torch.tensor([N], dtype=torch.int32, device=DEV)
    rec.calls = []

    # one image with a row count on the device: the masked entry on fp32 NCHW maps, the typed one (n_valid last) otherwise
    z, sr = ops.emm_extract_cache(fa, boxes, RZ, SCALES, 2, PAD, EXPANSION, MIN_WH, n_valid=n_valid)
    name, args = rec.take("smot_emm_extract_cache")
    if typed:
        assert name == "smot_emm_extract_cache_typed_fwd"
        assert args[-3] == 1 and tuple(args[-2]) == (0, N) and args[-1] == n_valid.data_ptr()
    else:
        assert name == "smot_emm_extract_cache_masked_fwd" and args[8] == n_valid.data_ptr()
    z0, sr0 = ops.emm_extract_cache(fa, boxes, RZ, SCALES, 2, PAD, EXPANSION, MIN_WH)
    rec.calls = []
    assert torch.equal(z, z0) and torch.equal(sr, sr0)

    # several images: the typed entries whatever the maps are, with the batch's row ranges and no device row count
    fa2, fb2, _, _ = _inputs(form, N, B=2)
    z2, sr2 = ops.emm_extract_cache_batched(fa2, boxes, [3, 2], RZ, SCALES, 2, PAD, EXPANSION, MIN_WH)
    name, args = rec.take("smot_emm_extract_cache")
    assert name == "smot_emm_extract_cache_typed_fwd"
    assert args[-3] == 2 and tuple(args[-2]) == (0, 3, 5) and args[-1] is None
    ops.emm_track_batched(fb2, boxes, sr2, z2, [3, 2], params, RX, RZ, SCALES, 2, PAD, sigma=SIGMA, clip_wh=WH)
    name, args = rec.take("smot_emm_track")
    assert name == "smot_emm_track_typed_fwd" and args[-2] == 2 and tuple(args[-1]) == (0, 3, 5)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_one_image_through_the_batched_functions_takes_the_typed_entries_on_fp32_maps(rec):
    """(That the results equal ``emm_track``'s bit for bit: test_multi_image.py,
    test_edges_empty_images_single_image_many_rows_and_max_images, "B=1".)"""
    import siammot_amd.ops as ops
    N = 5
    fa, fb, boxes, params = _inputs("fp32", N)
    rec.calls = []
    z, sr = ops.emm_extract_cache_batched(fa, boxes, [N], RZ, SCALES, 2, PAD, EXPANSION, MIN_WH)
    name, args = rec.take("smot_emm_extract_cache")
    assert name == "smot_emm_extract_cache_typed_fwd" and args[1] == 0
    assert args[-3] == 1 and tuple(args[-2]) == (0, N) and args[-1] is None
    ops.emm_track_batched(fb, boxes, sr, z, [N], params, RX, RZ, SCALES, 2, PAD, sigma=SIGMA, clip_wh=WH)
    name, args = rec.take("smot_emm_track")
    assert name == "smot_emm_track_typed_fwd" and args[1] == 0 and args[-2] == 1 and tuple(args[-1]) == (0, N)
    torch.cuda.synchronize()
