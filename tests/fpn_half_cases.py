"""Cases of the FPN / RPN-head half-compute-mode tests (tests/test_fpn_half.py, tests/test_rpn_head_half.py) and their
yardsticks — TEST INFRASTRUCTURE.

The mode (``fpn.FPN(compute_dtype=)``, ``rpn.RPNHead(compute_dtype=)``, ``ops.fpn_half`` / ``ops.rpn_head_half``) multiplies
operands ROUNDED to the compute type, exactly, and accumulates in fp32.

* RPN head: nothing is rounded between the 3x3 stage and the outputs, so the yardstick is ``rpn_head_cases.oracle`` in fp64 on
  the case whose maps and ``conv.weight`` were first rounded with ``dla_half_cases.rnd`` (``head_rounded``): kernel and oracle
  differ in fp32 summation order alone.
* FPN: ``last`` is rounded between the two stages, where a value's rounding depends on the fp32 sum before it.  The
  yardsticks are integer data on which every rounding is the identity (``integer_case``) and, for general data, the
  comparator ``emulate_fpn`` — built like ``dla_half_cases.emulate`` — measured against the unrounded fp64 oracle.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import fpn_cases as P
from dla_half_cases import rnd

TYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
FPN_SHAPES = {"ODD4": P.ODD4, "FLOOR": P.FLOOR, "TWO": P.TWO, "EXACT": P.EXACT}
FPN_CIN = ((32, 64, 96, 160), P.DLA)                 # the first L of either
FPN_C = (32, 160)                                    # one pair; two blocks of 128 with idle waves in the second
HEAD_C, HEAD_A = (32, 160), (1, 3)


def head_rounded(x, prm, dtype):
    """(maps, parameters) of an RPN-head case as the mode multiplies them: the maps and ``conv.weight`` rounded to ``dtype``;
    the biases and the two 1x1 heads untouched."""
    return [rnd(v, dtype) for v in x], [rnd(prm[0], dtype)] + list(prm[1:])


def emulate_fpn(fpn, dtype):
    """The comparator of the general-data FPN tests, in torch on the CPU: a copy of ``fpn`` in fp32 mode in which every
    ``Conv2d`` gets its weight rounded with ``.to(dtype).float()`` and, through a forward pre-hook, its input likewise, before
    the fp32 ``conv2d``; ``fpn_torch`` runs over it (the module on CPU tensors)."""
    m = copy.deepcopy(fpn).cpu().eval()
    m.compute_dtype = None
    for mod in m.modules():
        if isinstance(mod, nn.Conv2d):
            with torch.no_grad():
                mod.weight.copy_(mod.weight.to(dtype).float())
            mod.register_forward_pre_hook(lambda _, args: (args[0].to(dtype).float(),))
    return m


def last_maps(x, prm, dtype=torch.float32):
    """``fpn_cases.oracle``'s ``last`` maps (the inputs of the 3x3 stage), finest first."""
    L = len(x)
    t = [torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for v in x]
    p = [[torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for v in level] for level in prm]
    last = [None] * L
    last[L - 1] = F.conv2d(t[L - 1], p[L - 1][0], p[L - 1][1])
    for l in range(L - 2, -1, -1):
        lateral = F.conv2d(t[l], p[l][0], p[l][1])
        last[l] = lateral + F.interpolate(last[l + 1], size=lateral.shape[-2:], mode="bilinear", align_corners=False)
    return last


def integer_case(C, cin, sizes, N, seed=11):
    """Small-integer parameters and SPARSE small-integer maps (-> (maps, parameters)) on which the half compute mode rounds
    nothing, in fp16 and in bf16 (8 significant bits):

    * filters and biases are in {-1, 0, 1}: exact in either type;
    * a finer map has entries in {-1, 0, 1}, about three non-zero channels per cell: its lateral is an integer of a few units;
    * the coarsest map of a two-level case has entries in {-16, 0, 16}, about two non-zero channels per cell, and a bias in
      {-16, 0, 16}: ``last[1]`` is a multiple of 16 of a few tens, so its 2x resize (weights 1/16, 3/16, 9/16; 1/4, 3/4, 1 at the
      border) is an INTEGER, and ``last[0]`` = lateral + resize is an integer well below 256;
    * a 3x3 output sums at most 9 C such integers times a filter in {-1, 0, 1}: below 2^24 by orders of magnitude, so every
      partial sum is exact in fp32 in ANY order.

    The test checks the claims it relies on (``last`` survives the rounding, fp32 == fp64) before it looks at the kernel."""
    rs = np.random.RandomState(seed + C + 7 * len(cin))
    ints = lambda shape: rs.randint(-1, 2, size=shape).astype(P.F32)
    L = len(cin)
    prm, x = [], []
    for l, (c, (h, w)) in enumerate(zip(cin, sizes)):
        coarse = L > 1 and l == L - 1
        unit = 16.0 if coarse else 1.0
        prm.append((ints((C, c, 1, 1)), ints(C) * np.float32(unit), ints((C, C, 3, 3)), ints(C)))
        keep = rs.random_sample((N, c, h, w)) < (2.0 if coarse else 3.0) / c
        x.append(ints((N, c, h, w)) * keep.astype(P.F32) * np.float32(unit))
    return x, prm
