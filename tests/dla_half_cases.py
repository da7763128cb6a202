"""Cases of the DLA half-compute-mode tests (tests/test_dla_half.py) and their yardsticks — TEST INFRASTRUCTURE.

The mode (``dla.DLA(compute_dtype=torch.float16 | torch.bfloat16)``, ``ops.dla_half`` and its operators) multiplies operands
ROUNDED to the compute type, exactly, and accumulates in fp32.  The yardsticks are therefore the existing ones of
tests/dla_cases.py / tests/dla_bottleneck_cases.py applied to the case whose inputs and filters were first rounded with
``.to(compute_dtype).float()`` (``rounded``): kernel and oracle then differ in fp32 summation order alone.
"""
import copy

import numpy as np
import torch
from torch import nn

import dla_bottleneck_cases as B
import dla_cases as D

TYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}

# ---- 3x3: CONV3 and FORMS of tests/test_dla_split.py, as data ------------------------------------------------------------
# (Cin, Cout, stride, size)
CONV3 = [(32, 64, 2, (26, 42)), (64, 64, 1, (13, 21)), (96, 96, 2, (25, 41)), (160, 160, 1, (1, 5)), (512, 512, 1, (2, 3))]
# (Cin, Cout, stride, input size, N of the large call, its form (WR, NM)): the one-image call of each runs (4, .)
FORMS = [(64, 64, 1, (32, 128), 8, (2, 2)), (32, 64, 2, (63, 127), 16, (2, 2)), (32, 128, 1, (29, 61), 16, (1, 2)),
         (32, 16, 1, (13, 21), 2, (4, 1)), (32, 32, 2, (26, 42), 2, (4, 2))]
ALL_FORMS = {(1, 4, 1), (1, 4, 2), (1, 2, 2), (1, 1, 2), (2, 4, 2), (2, 2, 2)}

# ---- 1x1 ------------------------------------------------------------------------------------------------------------------
# (sources [(channels, pooled)], Cout, output size, relu, residual: None, "plain", "pooled", "source0"); a pooled source of
# an h x w output is a (2h + 1) x (2w + 1) map.  5 x 7: fewer positions than a workgroup's 64; 9 x 13: a partial last tile.
CONV1 = [
    ([(32, False)], 32, (5, 7), True, None),
    ([(32, False)], 96, (9, 13), False, "plain"),
    ([(64, True), (32, False), (32, False)], 160, (9, 13), True, "pooled"),
    ([(64, True), (32, False), (32, False)], 96, (5, 7), False, None),
    ([(32, False)] * 8, 32, (9, 13), True, "source0"),
    ([(96, False)], 96, (9, 13), True, "source0"),                # three K steps inside one source
    ([(96, True), (32, False)], 160, (5, 7), False, "plain"),
]
# the form with four M-tiles per workgroup, with an M-block tail (160 = 64 + 64 + 32): it needs >= 256 workgroups
CONV1_WIDE = ([(32, False)], 160, (75, 75), True, "plain")


def sources_of(sources, size):
    """CONV1's source list in the form ``dla_cases.conv1x1_case`` takes."""
    return [(c, (2 * size[0] + 1, 2 * size[1] + 1) if p else False) for c, p in sources]


def rnd(a, dtype):
    """``a.to(dtype).float()`` on a numpy fp32 array: round to nearest even, fp16 beyond 65,504 -> +-inf."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def rounded3(c, dtype):
    """A ``conv3x3_case`` with the input and the filters rounded to the compute type (residual, scale, shift stay fp32)."""
    return dict(c, x=rnd(c["x"], dtype), w=rnd(c["w"], dtype))


def rounded1(c, dtype):
    """A ``conv1x1_res_case`` likewise.  Rounding is monotone, so rounding before the pool is rounding behind it.  A residual
    that IS source 0 stays the unrounded map, as in the kernel."""
    return dict(c, src=[rnd(s, dtype) for s in c["src"]], w=rnd(c["w"], dtype))


# ---- network level ------------------------------------------------------------------------------------------------------
NET_CASES = ("A", "B", "C", "D", "E", "F")


def net(case, dev="cpu", **kw):
    """The case's network (A, B, C: tests/dla_cases.py; D, E, F: tests/dla_bottleneck_cases.py) with the recipe's parameters
    -> (model on ``dev``, image, golden)."""
    from siammot_amd.dla import DLA
    if case in D.NET_CASES:
        levels, channels, shape = D.NET_CASES[case]
        model, g = DLA(levels, channels, **kw), D.golden(case)
    else:
        levels, channels, shape, rr = B.NET_CASES[case]
        model, g = DLA(levels, channels, block="bottleneck", residual_root=rr, **kw), B.golden(case)
    if case not in _prm:
        _prm[case] = D.params(model, D.SEED)
    return D.load(model, _prm[case], dev), torch.from_numpy(D.image(shape, D.SEED)), g


_prm = {}


def emulate(model, dtype):
    """The comparator of the network tests, in torch on the CPU: a copy of ``model`` (fp32 mode) in which every TREE
    convolution, 3x3 and 1x1, gets its weight rounded with ``.to(dtype).float()`` and, through a forward pre-hook, its input
    likewise, before the fp32 ``conv2d``; ``dla_torch`` over it.  The stem is untouched."""
    m = copy.deepcopy(model).cpu().eval()
    m.compute_dtype = None
    for level in (m.level2, m.level3, m.level4, m.level5):
        for mod in level.modules():
            if isinstance(mod, nn.Conv2d):
                with torch.no_grad():
                    mod.weight.copy_(mod.weight.to(dtype).float())
                mod.register_forward_pre_hook(lambda _, args: (args[0].to(dtype).float(),))
    return m
