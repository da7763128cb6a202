"""Cases of the bottleneck / deep-tree DLA tests and their yardsticks — TEST INFRASTRUCTURE.

Network level: the golden vectors tests/golden/dla_bottleneck_stages.npz (tools/gen_golden_dla_bottleneck.py: the reference's
own dla.py with ``block=DlaBottleneck`` in fp64, and per stage the error ``e32`` of the reference's own fp32 run), with the
parameter recipe and the images of tests/dla_cases.py (``params``, ``image``, seed 7).

Operator level: the 1x1 convolution over a virtual concatenation with a residual, written from the contract
(include/smot_emm.h, DLA BACKBONE, BOTTLENECK BLOCKS AND DEEPER TREES) with torch's CPU operators in fp64 and fp32:

    conv1x1_res:  relu?(conv2d(cat([max_pool2d(s, 2, 2) if pooled else s for s in sources], 1), w) * scale + shift
                        + (max_pool2d(residual, 2, 2) if residual_pooled else residual))
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import dla_cases as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dla_bottleneck_stages.npz")
SEED = D.SEED
# case -> (levels, channels, (H, W), residual_root); block = bottleneck, N = 1, seed 7
NET_CASES = {
    # the pooled residual on a conv3 (64 -> 64 and 128 -> 128 at stride 2); a five-source root
    "D": ((1, 1, 1, 2, 3, 1), (16, 32, 64, 64, 128, 128), (64, 96), False),
    # DLA-169's depths; a seven-source root with K = 1,280; a 96-channel mid; a 1 x 5 last stage
    "E": ((1, 1, 2, 3, 5, 1), (16, 32, 64, 128, 192, 64), (32, 160), True),
    # the smallest residual-root network
    "F": ((1, 1, 1, 1, 2, 1), (16, 32, 64, 64, 64, 128), (64, 64), True),
}
NET_KEYS = {"D": 315, "E": 875, "F": 200}

_golden = {}


def golden(case):
    """{"o64": the four fp64 stage maps, "e32": the reference's own fp32 error per stage, "shape", "seed"}."""
    if not _golden:
        z = np.load(GOLDEN)
        for c in NET_CASES:
            _golden[c] = dict(o64=[z["%s_o64_%d" % (c, k)] for k in range(4)], e32=[float(v) for v in z["%s_e32" % c]],
                              shape=tuple(int(v) for v in z["%s_shape" % c]), seed=int(z["%s_seed" % c]))
    return _golden[case]


# ---- operator level -----------------------------------------------------------------------------------------------------
def conv1x1_res_case(sources, Cout, size, N, residual, seed=0):
    """sources: [(channels, pooled: False, or the (H, W) of the finer map)]; residual: None, "plain", "pooled" (a map of
    ``2 * size + 1``, as the pooled sources') or "source0" (the residual IS source 0: its width must be ``Cout``)."""
    c = D.conv1x1_case(sources, Cout, size, N, seed=seed)
    rs = np.random.RandomState(8000 + 3 * Cout + len(sources) + size[1] + seed)
    c["residual_pooled"] = residual == "pooled"
    if residual == "plain":
        c["residual"] = (rs.standard_normal((N, Cout) + tuple(size)) * 4.0).astype(D.F32)
    elif residual == "pooled":
        c["residual"] = (rs.standard_normal((N, Cout, 2 * size[0] + 1, 2 * size[1] + 1)) * 4.0).astype(D.F32)
    elif residual == "source0":
        assert sources[0][0] == Cout
        c["residual"], c["residual_pooled"] = c["src"][0], bool(sources[0][1])
    else:
        c["residual"] = None
    return c


def conv1x1_res_oracle(c, dtype, relu=True, pre=False):
    y = D.conv1x1_oracle(c, dtype, pre=True)
    if c["residual"] is not None:
        r = D._t(c["residual"], dtype)
        y = y + (F.max_pool2d(r, 2, 2) if c["residual_pooled"] else r)
    return y if (pre or not relu) else F.relu(y)
