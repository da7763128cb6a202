"""The frames of several cameras in one call (``smot_preprocess_batch_fwd``, ``ops.preprocess_frames``,
``FramePreprocessor.batch``): every image bit for bit ``PIL.Image.resize(BILINEAR)`` + the torch ToTensor / Normalize chain,
followed by ``.to(dtype)`` for a half output — never the code under test.  The CPU part pins the C entry's argument checks,
the symbol tables and the staging plan."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), False)
BGR = ((102.9801, 115.9465, 122.7717), (1.0, 1.0, 1.0), True)
DEV = "cuda:0"

# one call = (input sizes of its frames, the one output size)
CALL_MIXED = (((90, 160), (54, 96), (64, 128)), (64, 128))        # down-scale, up-scale, identity
CALL_ODD = (((100, 37), (31, 77)), (31, 77))                      # odd width, last tile < 128, OH % 8 != 0, an identity frame
CALL_TILES = (((33, 250), (12, 100)), (16, 160))                  # a 128-wide and a 32-wide tile
CALL_CHUNKS = (((20, 24),) * 17, (16, 32))                        # crosses the 16-image launch chunk


def _frame(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _frames(call):
    return [_frame(h, w, seed=31 + i) for i, (h, w) in enumerate(call[0])]


def _torch_chain(img_u8, mean, std, to_bgr255):
    """ToTensor + Normalize with the torch ops the reference's transforms run (transforms.py [UPSTREAM])."""
    t = torch.from_numpy(np.array(img_u8, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    if to_bgr255:
        t = t[[2, 1, 0]] * 255
    m = torch.as_tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.as_tensor(std, dtype=torch.float32)[:, None, None]
    return t.sub_(m).div_(s)


@functools.lru_cache(maxsize=None)
def _reference(call, bgr):
    """fp32 ``[B, 3, OH, OW]`` of a call from Pillow + torch; computed once, shared, never written to."""
    PIL_Image = pytest.importorskip("PIL.Image")
    mean, std, _ = BGR if bgr else RGB
    oh, ow = call[1]
    out = [_torch_chain(np.asarray(PIL_Image.fromarray(a, "RGB").resize((ow, oh), PIL_Image.BILINEAR)), mean, std, bgr)
           for a in _frames(call)]
    return torch.stack(out)


def _pre(bgr=False, **kw):
    from siammot_amd.preprocess import FramePreprocessor
    mean, std, flag = BGR if bgr else RGB
    return FramePreprocessor(kw.get("min_size", 800), kw.get("max_size", 1280), 32, mean, std, flag, device=DEV)


def _run(call, bgr=False, dtype=torch.float32, channels_last=False, out=None, frames=None):
    import siammot_amd.ops as ops
    pre = _pre(bgr)
    host = _frames(call) if frames is None else frames
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    tables = [pre.tables(a.shape[:2], call[1]) for a in host]
    return ops.preprocess_frames(dev, tables, call[1], pre.pixel_mean, pre.pixel_std, bgr, dtype=dtype,
                                 channels_last=channels_last, out=out)


def _assert_images_equal(got, ref, what):
    got = got.cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    for b in range(ref.shape[0]):
        assert torch.equal(got[b], ref[b]), "%s: image %d differs in %d elements, max abs diff %g" % (
            what, b, int((got[b] != ref[b]).sum()), float((got[b].float() - ref[b].float()).abs().max()))


# ------------------------------------------------------------------------------------------------ CPU
def _header_symbols():
    src = open(os.path.join(ROOT, "include", "smot_emm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(smot_[a-z0-9_]+)\s*\(", src))


def test_batch_entry_is_declared_bound_and_exported_and_the_abi_stays_14():
    import siammot_amd.ops as ops
    assert "smot_preprocess_batch_fwd" in _header_symbols()
    assert "smot_preprocess_batch_fwd" in ops.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(ops.LIB_PATH)
    assert hasattr(lib, "smot_preprocess_batch_fwd")
    assert lib.smot_abi_version() == 14 and ops.ABI_VERSION == 14
    assert "#define SMOT_ABI_VERSION 14" in open(os.path.join(ROOT, "include", "smot_emm.h")).read()


class _Args(object):
    """A well-formed argument list of ``n`` images for the C entry (pointers that are never followed: every check under test
    happens before the first launch), with one field changed per case."""

    def __init__(self, n):
        P, I = ctypes.c_void_p * max(n, 1), ctypes.c_int * max(n, 1)
        fake = 0x10000
        self.n = n
        self.frames, self.xb, self.xk, self.yb, self.yk = (P(*[fake] * max(n, 1)) for _ in range(5))
        self.H, self.W = I(*[90] * max(n, 1)), I(*[160] * max(n, 1))
        self.kx, self.ky = I(*[5] * max(n, 1)), I(*[5] * max(n, 1))
        self.rows = I(*[15] * max(n, 1))
        self.OH, self.OW = 64, 128
        self.mean, self.std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        self.out, self.out_type = ctypes.c_void_p(fake), 0

    def call(self, lib):
        c = lambda a: ctypes.cast(a, ctypes.c_void_p)
        rc = lib.smot_preprocess_batch_fwd(self.n, c(self.frames), c(self.H), c(self.W), c(self.xb), c(self.xk), c(self.kx),
                                           c(self.yb), c(self.yk), c(self.ky), c(self.rows), self.OH, self.OW, c(self.mean),
                                           c(self.std), 0, self.out, self.out_type, ctypes.c_void_p(0))
        return rc, lib.smot_last_error().decode()


def test_batch_entry_refuses_bad_arguments_before_any_launch():
    import siammot_amd.ops as ops
    lib = ops.load_library()
    BAD_ARG, UNSUPPORTED = -1, -2
    for n in (0, 65):
        rc, msg = _Args(n).call(lib)
        assert rc == BAD_ARG and "num_images=%d" % n in msg, (n, rc, msg)
    a = _Args(3)
    a.xk[1] = None                                  # a null entry
    rc, msg = a.call(lib)
    assert rc == BAD_ARG and "image 1" in msg and "null" in msg, (rc, msg)
    a = _Args(3)
    a.out = ctypes.c_void_p(0)
    rc, msg = a.call(lib)
    assert rc == BAD_ARG and "null" in msg, (rc, msg)
    a = _Args(3)
    a.W[2] = 0                                      # a zero size
    rc, msg = a.call(lib)
    assert rc == BAD_ARG and "image 2" in msg, (rc, msg)
    a = _Args(2)
    a.OH = 0
    rc, msg = a.call(lib)
    assert rc == BAD_ARG and "0x128" in msg, (rc, msg)
    for ot in (3, 16 | 3):
        a = _Args(2)
        a.out_type = ot
        rc, msg = a.call(lib)
        assert rc == BAD_ARG and "out_type=%d" % ot in msg, (ot, rc, msg)
    a = _Args(3)
    a.rows[1] = 170                                 # 170 * 384 = 65,280 bytes fit ...
    a.rows[2] = 171                                 # ... 171 * 384 = 65,664 do not: refused, named by its index
    rc, msg = a.call(lib)
    assert rc == UNSUPPORTED and "image 2" in msg and "LDS" in msg and "171" in msg, (rc, msg)


def test_staging_plan_is_aligned_disjoint_and_stable():
    from siammot_amd.preprocess import staging_plan
    shapes = [(720, 1280, 3), (1080, 1920, 3), (5, 7, 3), (720, 1280, 3), (1, 1, 3)]
    for align in (256, 64, 1):
        offs, total = staging_plan(shapes, align=align)
        sizes = [h * w * c for h, w, c in shapes]
        assert len(offs) == len(shapes) and all(o % align == 0 for o in offs)
        assert offs[0] == 0 and all(offs[i] + sizes[i] <= offs[i + 1] for i in range(len(shapes) - 1))   # in order, disjoint
        assert total >= offs[-1] + sizes[-1] and total >= sum(sizes)
        assert staging_plan(shapes, align=align) == (offs, total)                                        # a pure function
        assert staging_plan(list(shapes), align=align)[0][:2] == staging_plan(shapes[:2], align=align)[0]
    assert staging_plan([(2, 3, 3)] * 3) == ([0, 256, 512], 768)
    assert staging_plan([]) == ([], 0)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_batch_equals_pillow_plus_torch(dtype, channels_last, bgr):
    for call in (CALL_MIXED, CALL_ODD):
        B, (oh, ow) = len(call[0]), call[1]
        got = _run(call, bgr, dtype, channels_last)
        assert tuple(got.shape) == (B, 3, oh, ow) and got.dtype == dtype and got.is_cuda
        if channels_last:
            assert got.is_contiguous(memory_format=torch.channels_last)
            assert tuple(got.stride()) == (oh * ow * 3, 1, ow * 3, 3)
        else:
            assert got.is_contiguous() and tuple(got.stride()) == (3 * oh * ow, oh * ow, ow, 1)
        _assert_images_equal(got, _reference(call, bgr).to(dtype), "%s cl=%s bgr=%s %s" % (dtype, channels_last, bgr, call[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,channels_last", [(torch.float32, False), (torch.float32, True), (torch.float16, False),
                                                 (torch.bfloat16, True)])
def test_batch_tile_boundary(dtype, channels_last):
    _assert_images_equal(_run(CALL_TILES, False, dtype, channels_last), _reference(CALL_TILES, False).to(dtype), "tiles")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,channels_last", [(torch.float32, False), (torch.float16, True)])
def test_batch_of_17_images_crosses_the_launch_chunk(dtype, channels_last):
    got = _run(CALL_CHUNKS, True, dtype, channels_last)
    assert got.shape[0] == 17
    _assert_images_equal(got, _reference(CALL_CHUNKS, True).to(dtype), "17 images")


@pytest.mark.gpu
def test_batch_fp32_nchw_equals_the_single_frame_call():
    import siammot_amd.ops as ops
    pre = _pre()
    for call in (CALL_MIXED, CALL_ODD):
        got = _run(call)
        for b, a in enumerate(_frames(call)):
            one = ops.preprocess_frame(torch.from_numpy(a).to(DEV), pre.tables(a.shape[:2], call[1]), call[1], pre.pixel_mean,
                                       pre.pixel_std, False)
            assert torch.equal(got[b], one), "image %d of %s" % (b, call[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,channels_last", [(torch.float32, False), (torch.float16, True)])
def test_batch_images_are_isolated_and_runs_are_deterministic(dtype, channels_last):
    base = _run(CALL_MIXED, False, dtype, channels_last)
    again = _run(CALL_MIXED, False, dtype, channels_last)
    assert torch.equal(base.cpu().view(torch.int16 if dtype != torch.float32 else torch.int32),
                       again.cpu().view(torch.int16 if dtype != torch.float32 else torch.int32))       # the same BITS
    frames = _frames(CALL_MIXED)
    frames[1] = 255 - frames[1]
    changed = _run(CALL_MIXED, False, dtype, channels_last, frames=frames)
    assert torch.equal(changed[0], base[0]) and torch.equal(changed[2], base[2])
    assert not torch.equal(changed[1], base[1])


@pytest.mark.gpu
def test_out_is_written_in_place_and_a_wrong_out_raises_before_anything_is_written():
    B, (oh, ow) = len(CALL_MIXED[0]), CALL_MIXED[1]
    for dtype, cl in ((torch.float32, False), (torch.float16, True)):
        fmt = torch.channels_last if cl else torch.contiguous_format
        out = torch.full((B, 3, oh, ow), 7.0, dtype=dtype, device=DEV).contiguous(memory_format=fmt)
        ptr = out.data_ptr()
        got = _run(CALL_MIXED, False, dtype, cl, out=out)
        assert got is out and out.data_ptr() == ptr
        _assert_images_equal(out, _reference(CALL_MIXED, False).to(dtype), "out=")
    wrong = [
        (torch.float32, False, torch.full((B, 3, oh, ow + 1), 7.0, device=DEV)),                                  # shape
        (torch.float32, False, torch.full((B + 1, 3, oh, ow), 7.0, device=DEV)),                                  # images
        (torch.float16, False, torch.full((B, 3, oh, ow), 7.0, device=DEV)),                                      # dtype
        (torch.float32, True, torch.full((B, 3, oh, ow), 7.0, device=DEV)),                                       # layout
        (torch.float32, False, torch.full((B, 3, oh, ow), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)),
        (torch.float32, False, torch.full((B, 3, oh, 2 * ow), 7.0, device=DEV)[..., ::2]),                        # a strided view
        (torch.float32, False, torch.full((B, 3, oh, ow), 7.0)),                                                  # device
    ]
    for dtype, cl, out in wrong:
        with pytest.raises(RuntimeError, match="out must be"):
            _run(CALL_MIXED, False, dtype, cl, out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused out= tensor was written to"


@pytest.mark.gpu
def test_binding_refuses_bad_frames_and_tables():
    import siammot_amd.ops as ops
    pre = _pre()
    f = torch.zeros((4, 4, 3), dtype=torch.uint8, device=DEV)
    t = pre.tables((4, 4), (4, 4))
    args = ((4, 4), pre.pixel_mean, pre.pixel_std, False)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.preprocess_frames([f, f.float()], [t, t], *args)
    with pytest.raises(RuntimeError, match="uint8 device"):
        ops.preprocess_frames([f, f.cpu()], [t, t], *args)
    with pytest.raises(RuntimeError, match="1 table tuples for 2 frames"):
        ops.preprocess_frames([f, f], [t], *args)
    with pytest.raises(RuntimeError, match="tables.1. are for 8x8, asked for 4x4"):
        ops.preprocess_frames([f, f], [t, pre.tables((4, 4), (8, 8))], *args)
    with pytest.raises(RuntimeError, match="0 frames"):
        ops.preprocess_frames([], [], *args)
    with pytest.raises(RuntimeError, match="LDS"):               # image 1's 8 output rows need > 64 KiB of input rows
        big = torch.zeros((4000, 8, 3), dtype=torch.uint8, device=DEV)
        small = torch.zeros((8, 8, 3), dtype=torch.uint8, device=DEV)
        ops.preprocess_frames([small, big], [pre.tables((8, 8), (8, 8)), pre.tables((4000, 8), (8, 8))], (8, 8),
                              pre.pixel_mean, pre.pixel_std, False)


@pytest.mark.gpu
def test_preprocessor_batch_of_mixed_cameras_and_its_refusals():
    pre = _pre(min_size=64, max_size=128)
    frames = [_frame(90, 160, 3), _frame(135, 240, 4)]           # 720p-like and 1080p-like: both go to 64 x 96
    got = pre.batch(frames)
    assert tuple(got.shape) == (2, 3, 64, 96) and got.dtype == torch.float32
    assert pre.image_sizes(frames) == [(160, 90), (240, 135)]
    for b, a in enumerate(frames):
        ref = torch.from_numpy(PO.preprocess(a, 64, 128, 32, pre.pixel_mean, pre.pixel_std, False))
        assert torch.equal(got[b].cpu(), ref), "image %d" % b
    half = pre.batch(frames, dtype=torch.float16, channels_last=True)
    assert half.is_contiguous(memory_format=torch.channels_last) and torch.equal(half, got.to(torch.float16))
    with pytest.raises(RuntimeError, match="one network size"):
        pre.batch([_frame(90, 160), _frame(160, 90)])
    with pytest.raises(RuntimeError, match="0 frames"):
        pre.batch([])
    with pytest.raises(RuntimeError, match="uint8"):
        pre.batch([frames[0], frames[1].astype(np.float32)])
    with pytest.raises(RuntimeError, match="65 frames"):
        pre.batch([frames[0]] * 65)


@pytest.mark.gpu
def test_batch_is_one_copy_and_one_library_call(monkeypatch):
    import siammot_amd.ops as ops
    pre = _pre(min_size=64, max_size=128)
    host = [_frame(90, 160, 5), _frame(135, 240, 6), _frame(90, 160, 7), _frame(135, 240, 8)]
    dev = pre.upload_many(host)
    assert len({d.untyped_storage().data_ptr() for d in dev}) == 1           # views of ONE device buffer
    assert all(d.data_ptr() % 256 == 0 for d in dev)
    for d, a in zip(dev, host):
        assert d.is_cuda and torch.equal(d.cpu(), torch.from_numpy(a))
    again = pre.upload_many(dev)                                             # device frames pass through by identity
    assert all(x is y for x, y in zip(again, dev))
    mixed = pre.upload_many([dev[0], host[1]])
    assert mixed[0] is dev[0] and torch.equal(mixed[1].cpu(), torch.from_numpy(host[1]))

    lib = ops.load_library()
    real, calls = lib.smot_preprocess_batch_fwd, []

    def counted(*args):
        calls.append(args[0])
        return real(*args)
    monkeypatch.setattr(lib, "smot_preprocess_batch_fwd", counted)
    first = pre.batch(host)
    assert calls == [4]                                                      # one library call for the four frames
    newer = [255 - a for a in host]
    second = pre.batch(newer)                                                # the staging buffers are reused
    assert calls == [4, 4]
    for b in range(4):
        ref_a = torch.from_numpy(PO.preprocess(host[b], 64, 128, 32, pre.pixel_mean, pre.pixel_std, False))
        ref_b = torch.from_numpy(PO.preprocess(newer[b], 64, 128, 32, pre.pixel_mean, pre.pixel_std, False))
        assert torch.equal(first[b].cpu(), ref_a) and torch.equal(second[b].cpu(), ref_b)
