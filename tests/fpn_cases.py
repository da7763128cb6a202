"""Cases of the FPN tests and their yardstick — TEST INFRASTRUCTURE.

The yardstick is torch's own ``F.conv2d`` / ``F.interpolate`` / ``F.max_pool2d`` on the CPU, in fp64 and in fp32, written from
the operator's contract (include/smot_emm.h, FEATURE PYRAMID):

    last[L-1] = conv1x1(x[L-1]) + b
    last[l]   = conv1x1(x[l]) + b + interpolate(last[l+1], size=(H_l, W_l), mode="bilinear", align_corners=False)
    P[l]      = conv3x3(last[l], pad 1) + b
    P[L]      = max_pool2d(P[L-1], kernel 1, stride 2)

Weights ~ N(0, 0.05), biases ~ N(0, 0.5), maps ~ N(0, 4) (mean, standard deviation), all from seeded
``numpy.random.RandomState``s, as in rpn_head_cases.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
# no side is a multiple of the layer kernel's 8 x 16 tile, 13 x 21 takes four tiles, the resizes are not 2x, the top block
# gives (1, 2); 13 * 21 = 273 positions are four full 64-position workgroups of the lateral kernel and one of 17
ODD4 = ((13, 21), (7, 11), (4, 6), (2, 3))
FLOOR = ((9, 17), (4, 8), (2, 4), (1, 2))            # a one-row level; the top block gives (1, 1)
TWO = ((10, 7), (3, 2))                              # ratios 3.33 and 3.5; two levels
EXACT = ((12, 20), (6, 10))                          # an exact 2x: weights 0.25 / 0.75
DLA = (64, 128, 256, 512)
R50 = (256, 512, 1024, 2048)


def params(C, cin, seed=0):
    """Per level, finest first: (inner weight [C, Cin_l, 1, 1], inner bias, layer weight [C, C, 3, 3], layer bias), fp32."""
    rs = np.random.RandomState(3000 + 7 * C + 3 * len(cin) + cin[0] + seed)
    return [((rs.standard_normal((C, c, 1, 1)) * 0.05).astype(F32), (rs.standard_normal(C) * 0.5).astype(F32),
             (rs.standard_normal((C, C, 3, 3)) * 0.05).astype(F32), (rs.standard_normal(C) * 0.5).astype(F32)) for c in cin]


def maps(cin, N, sizes, seed=0):
    rs = np.random.RandomState(4000 + cin[0] + 13 * N + 17 * sizes[0][0] + seed)
    return [(rs.standard_normal((N, c, h, w)) * 4.0).astype(F32) for c, (h, w) in zip(cin, sizes)]


def _t(v, dtype):
    return (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(dtype)


def oracle(stage_maps, prm, dtype=torch.float64, top_block=True):
    """The composition on the CPU in ``dtype``: the list of L (+ 1) maps, finest first."""
    L = len(stage_maps)
    x = [_t(v, dtype) for v in stage_maps]
    p = [[_t(v, dtype) for v in level] for level in prm]
    last = [None] * L
    last[L - 1] = F.conv2d(x[L - 1], p[L - 1][0], p[L - 1][1])
    for l in range(L - 2, -1, -1):
        lateral = F.conv2d(x[l], p[l][0], p[l][1])
        last[l] = lateral + F.interpolate(last[l + 1], size=lateral.shape[-2:], mode="bilinear", align_corners=False)
    out = [F.conv2d(last[l], p[l][2], p[l][3], stride=1, padding=1) for l in range(L)]
    if top_block:
        out.append(F.max_pool2d(out[-1], 1, 2, 0))
    return out


def channel_scale(levels64):
    """rpn_head_cases.channel_scale's definition over all outputs of the call: max |fp64| per output channel over every image,
    level and position -> ``[C]``."""
    return torch.stack([t.abs().amax(dim=(0, 2, 3)) for t in levels64]).amax(dim=0)


def load_fpn(fpn, prm, dev):
    """``prm`` into an ``fpn.FPN`` on ``dev`` (eval mode)."""
    with torch.no_grad():
        for l, (iw, ib, lw, lb) in enumerate(prm):
            inner, layer = getattr(fpn, "fpn_inner%d" % (l + 1)), getattr(fpn, "fpn_layer%d" % (l + 1))
            for dst, src in ((inner.weight, iw), (inner.bias, ib), (layer.weight, lw), (layer.bias, lb)):
                dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    return fpn.to(dev).eval()
