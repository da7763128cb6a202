"""Cases of the RPN head / anchor tests and their yardstick — TEST INFRASTRUCTURE.

The yardstick of the head's arithmetic is torch's own ``F.conv2d`` / ``F.relu`` on the CPU, in fp64 and in fp32; of the
anchors, upstream's broadcast expression ``shifts + cell`` in torch fp32.  Weights ~ N(0, 0.05), biases ~ N(0, 0.5), maps
~ N(0, 4) (mean, standard deviation), all from seeded ``numpy.random.RandomState``s.
"""
import warnings

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
# no side is a multiple of the kernel's 8 x 16 tile, 13 x 21 takes four tiles, 1 x 2 is smaller than one, five levels
ODD = ((13, 21), (7, 11), (4, 6), (2, 3), (1, 2))
ONE = ((9, 17),)
STRIDES = (4, 8, 16, 32, 64)
SIZES = (32, 64, 128, 256, 512)
RATIOS = (0.5, 1.0, 2.0)


def params(C, A, seed=0):
    """Upstream's six tensors as fp32 numpy arrays, in ``RPNHead._params()`` order."""
    rs = np.random.RandomState(1000 + 7 * C + A + seed)
    return [(rs.standard_normal((C, C, 3, 3)) * 0.05).astype(F32), (rs.standard_normal(C) * 0.5).astype(F32),
            (rs.standard_normal((A, C, 1, 1)) * 0.05).astype(F32), (rs.standard_normal(A) * 0.5).astype(F32),
            (rs.standard_normal((4 * A, C, 1, 1)) * 0.05).astype(F32), (rs.standard_normal(4 * A) * 0.5).astype(F32)]


def maps(C, N, levels=ODD, seed=0):
    rs = np.random.RandomState(2000 + C + 13 * N + seed)
    return [(rs.standard_normal((N, C, h, w)) * 4.0).astype(F32) for (h, w) in levels]


def oracle(feature_maps, prm, dtype=torch.float64):
    """The composition on the CPU in ``dtype``: (objectness list, regression list) of torch tensors."""
    p = [torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for v in prm]
    obj, reg = [], []
    for x in feature_maps:
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        t = F.relu(F.conv2d(x.to(dtype), p[0], p[1], stride=1, padding=1))
        obj.append(F.conv2d(t, p[2], p[3]))
        reg.append(F.conv2d(t, p[4], p[5]))
    return obj, reg


def channel_scale(levels64):
    """max |fp64| per output channel over every image, level and position of a call (the weights are shared by the levels:
    a channel has one scale) -> ``[channels]``."""
    return torch.stack([t.abs().amax(dim=(0, 2, 3)) for t in levels64]).amax(dim=0)


def scaled_error(got, ref, scale):
    """max over a call of |got - ref| / scale[channel], over the positions where ``ref`` is finite."""
    worst = 0.0
    for g, r in zip(got, ref):
        e = (g.double().cpu() - r.double()).abs() / scale.view(1, -1, 1, 1)
        e = e[torch.isfinite(r)]
        if e.numel():
            worst = max(worst, float(e.max()))
    return worst


def load_head(head, prm, dev):
    """``prm`` into an ``rpn.RPNHead`` on ``dev`` (eval mode)."""
    with torch.no_grad():
        for dst, src in zip(head._params(), prm):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    return head.to(dev).eval()


def grid_expression(cell, stride, h, w):
    """Upstream's ``grid_anchors`` for one level in torch fp32 on the CPU: rows (y * W + x) * A + a."""
    sx = torch.arange(0, w * stride, step=stride, dtype=torch.float32)
    sy = torch.arange(0, h * stride, step=stride, dtype=torch.float32)
    sy, sx = torch.meshgrid(sy, sx, indexing="ij")
    sx, sy = sx.reshape(-1), sy.reshape(-1)
    shifts = torch.stack((sx, sy, sx, sy), dim=1)
    return (shifts.view(-1, 1, 4) + cell.view(1, -1, 4)).reshape(-1, 4)


def count_syncs(fn):
    """``fn()`` and the synchronising calls torch saw during it (tests/test_rpn_proposals.py's helper)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
        syncs = [x for x in w if "synchroniz" in str(x.message).lower()]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, syncs
