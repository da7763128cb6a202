"""Feature pyramid: [UPSTREAM] maskrcnn_benchmark's ``FPN`` in the form the reference patches in (its top-down path is resized
bilinearly to the lateral's size, so stage maps need not halve exactly), under upstream's constructor signature and
``state_dict`` keys (``fpn_inner{i}.*``, ``fpn_layer{i}.*``), so that a reference checkpoint's ``backbone.fpn.*`` loads.

    last[L-1] = fpn_inner{L}(x[L-1])
    last[l]   = fpn_inner{l+1}(x[l]) + F.interpolate(last[l+1], size=x[l].shape[-2:], mode="bilinear", align_corners=False)
    P[l]      = fpn_layer{l+1}(last[l])
    P[L]      = max_pool2d(P[L-1], 1, 2, 0)                      (``LastLevelMaxPool``)

Two forms of the operator live here:

* ``FPN.forward`` in eval mode on device maps within ``ops.fpn``'s capacities: the laterals (one launch per level) and the
  3x3 convolutions of all levels and images (one launch) on the fp32 matrix cores, no host synchronisation; ``out_dtype``
  half stores the maps the head and poolers read fastest with no cast in between; ``compute_dtype=torch.float16`` or
  ``torch.bfloat16`` (opt-in) runs both convolutions on the 16-bit matrix cores instead (``ops.fpn_half``);
* ``fpn_torch``: the same as a plain torch composition.  It is the path for CPU tensors, training, GroupNorm / ReLU conv
  blocks, ``LastLevelP6P7``, a skipped level (``in_channels`` 0) and shapes beyond the capacities (counted in
  ``ops.FALLBACKS["fpn_torch"]`` for device tensors), and the baseline of tools/fpn_bench.py.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import ops


def conv_with_kaiming_uniform(use_gn=False, use_relu=False, num_groups=32, eps=1e-5):
    """Upstream's factory of conv blocks: ``make_conv(in_channels, out_channels, kernel_size, stride=1, dilation=1)`` -> a
    ``Conv2d`` with "same" padding, ``kaiming_uniform_(a=1)`` weights and (without GroupNorm) a zero bias; with ``use_gn``
    / ``use_relu`` a ``Sequential`` of the convolution, ``GroupNorm(num_groups)`` and ``ReLU``."""
    def make_conv(in_channels, out_channels, kernel_size, stride=1, dilation=1):
        conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride,
                         padding=dilation * (kernel_size - 1) // 2, dilation=dilation, bias=not use_gn)
        nn.init.kaiming_uniform_(conv.weight, a=1)
        if not use_gn:
            nn.init.constant_(conv.bias, 0)
        module = [conv]
        if use_gn:
            module.append(nn.GroupNorm(num_groups, out_channels, eps))
        if use_relu:
            module.append(nn.ReLU(inplace=True))
        return nn.Sequential(*module) if len(module) > 1 else conv
    return make_conv


class LastLevelMaxPool(nn.Module):
    """Upstream's top block: one more level by subsampling the coarsest map (no parameters)."""

    def forward(self, x):
        return [F.max_pool2d(x, 1, 2, 0)]


class LastLevelP6P7(nn.Module):
    """Upstream's RetinaNet top block (``p6``, ``p7``: 3x3 stride-2 convolutions).  Always on the torch composition."""

    def __init__(self, in_channels, out_channels):
        super(LastLevelP6P7, self).__init__()
        self.p6 = nn.Conv2d(in_channels, out_channels, 3, 2, 1)
        self.p7 = nn.Conv2d(out_channels, out_channels, 3, 2, 1)
        for module in (self.p6, self.p7):
            nn.init.kaiming_uniform_(module.weight, a=1)
            nn.init.constant_(module.bias, 0)
        self.use_P5 = in_channels == out_channels

    def forward(self, c5, p5):
        p6 = self.p6(p5 if self.use_P5 else c5)
        return [p6, self.p7(F.relu(p6))]


def fpn_torch(x, inner_blocks, layer_blocks, top_blocks=None):
    """The operator as torch operators on any device.  x: the stage maps of the levels that have blocks, finest first (half
    maps are upcast first, as the kernel converts on load); inner_blocks / layer_blocks: one module per level."""
    dtype = next(inner_blocks[-1].parameters()).dtype
    x = [t.to(dtype) for t in x]
    last = inner_blocks[-1](x[-1])
    results = [layer_blocks[-1](last)]
    for l in range(len(x) - 2, -1, -1):
        lateral = inner_blocks[l](x[l])
        last = lateral + F.interpolate(last, size=lateral.shape[-2:], mode="bilinear", align_corners=False)
        results.insert(0, layer_blocks[l](last))
    if isinstance(top_blocks, LastLevelP6P7):
        results.extend(top_blocks(x[-1], results[-1]))
    elif top_blocks is not None:
        results.extend(top_blocks(results[-1]))
    return results


def _plain_conv(m, kernel_size):
    return (type(m) is nn.Conv2d and m.bias is not None and m.kernel_size == (kernel_size, kernel_size)
            and m.stride == (1, 1) and m.dilation == (1, 1) and m.groups == 1 and m.padding_mode == "zeros"
            and m.padding == ((kernel_size - 1) // 2,) * 2)


class FPN(nn.Module):
    """Upstream's ``FPN(in_channels_list, out_channels, conv_block, top_blocks=None)``; ``conv_block`` None: plain
    convolutions (``conv_with_kaiming_uniform()``).  ``forward(x)``: the stage maps, finest first -> a tuple of maps, finest
    first (+ the top block's).  A level whose ``in_channels`` is 0 has no blocks and its stage map is not read, as upstream.
    ``out_dtype``: the element type of the returned maps (float32, float16 or bfloat16: the fp32 result rounded once).
    ``compute_dtype`` (keyword-only): None (the default: nothing changes), ``torch.float16`` or ``torch.bfloat16``: the half
    compute mode — the laterals and the 3x3 convolutions multiply operands rounded to that type (stage maps and the fp32
    ``last`` maps as they are loaded, filters when packed) with fp32 accumulation; every ``Cin_l`` a multiple of 32, else the
    torch composition.  CPU tensors and every fallback give the bits of the fp32 mode.  The ``state_dict`` is the same.
    On the device path the packed weights are rebuilt when a parameter's ``_version``, storage or device changes."""

    def __init__(self, in_channels_list, out_channels, conv_block=None, top_blocks=None, out_dtype=torch.float32, *,
                 compute_dtype=None):
        super(FPN, self).__init__()
        if compute_dtype is not None and compute_dtype not in ops.DLA_COMPUTE_TYPES:
            raise ValueError("FPN: compute_dtype must be None, torch.float16 or torch.bfloat16, got %r" % (compute_dtype,))
        self.compute_dtype = compute_dtype
        if conv_block is None:
            conv_block = conv_with_kaiming_uniform()
        self.inner_blocks, self.layer_blocks = [], []
        for idx, in_channels in enumerate(in_channels_list, 1):
            if in_channels == 0:
                continue
            inner, layer = "fpn_inner%d" % idx, "fpn_layer%d" % idx
            self.add_module(inner, conv_block(in_channels, out_channels, 1))
            self.add_module(layer, conv_block(out_channels, out_channels, 3, 1))
            self.inner_blocks.append(inner)
            self.layer_blocks.append(layer)
        if not self.inner_blocks:
            raise RuntimeError("FPN: no level with input channels")
        self.top_blocks = top_blocks
        self.in_channels_list = tuple(int(c) for c in in_channels_list)
        self.in_channels = tuple(c for c in self.in_channels_list if c != 0)
        self.out_channels = int(out_channels)
        self.out_dtype = out_dtype
        self._packed_key, self._packed = None, None

    def _blocks(self):
        return [getattr(self, n) for n in self.inner_blocks], [getattr(self, n) for n in self.layer_blocks]

    def kernel_ok(self, x):
        """This call takes ``ops.fpn``."""
        if self.training or len(self.in_channels) != len(self.in_channels_list) or len(x) != len(self.in_channels):
            return False
        if not (self.top_blocks is None or type(self.top_blocks) is LastLevelMaxPool) or self.out_dtype not in ops.FEAT_TYPES:
            return False
        inner, layer = self._blocks()
        if not (all(_plain_conv(m, 1) for m in inner) and all(_plain_conv(m, 3) for m in layer)):
            return False
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 for t in x):
            return False
        dev, dt = x[0].device, x[0].dtype
        params = list(self.parameters())
        if dt not in ops.FEAT_TYPES or not all(p.dtype is torch.float32 and p.device == dev for p in params):
            return False
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return False
        N = x[0].shape[0]
        if not (1 <= N <= ops.RPN_MAX_IMAGES and all(t.device == dev and t.dtype is dt and t.shape[0] == N and t.numel() > 0
                                                     and t.shape[1] == c for t, c in zip(x, self.in_channels))):
            return False
        if self.compute_dtype is not None:
            return ops.fpn_half_shapes_ok(self.in_channels, self.out_channels)
        return ops.fpn_shapes_ok(self.in_channels, self.out_channels)

    def packed(self):
        """The packed weights for a launch on the current stream: packed on the stream of the first call after a change and
        ordered for every other stream by ``ops.StreamImage`` (an event wait on the device, no host synchronisation)."""
        inner, layer = self._blocks()
        params = [p for m in inner + layer for p in (m.weight, m.bias)]
        key = (self.compute_dtype,) + tuple((p.data_ptr(), p._version, p.device) for p in params)
        if key != self._packed_key:
            blocks = ([(m.weight.detach(), m.bias.detach()) for m in inner], [(m.weight.detach(), m.bias.detach()) for m in layer])
            if self.compute_dtype is not None:
                self._packed = ops.StreamImage(lambda: ops.fpn_half_pack(*blocks, self.compute_dtype), params[0].device)
            else:
                self._packed = ops.StreamImage(lambda: ops.fpn_pack(*blocks), params[0].device)
            self._packed_key = key
        return self._packed.get()

    def forward(self, x):
        x = list(x)
        if self.kernel_ok(x):
            if self.compute_dtype is not None:
                return tuple(ops.fpn_half(x, self.packed(), self.in_channels, self.out_channels, self.compute_dtype,
                                          out_dtype=self.out_dtype, top_block=self.top_blocks is not None))
            return tuple(ops.fpn(x, self.packed(), self.in_channels, self.out_channels, out_dtype=self.out_dtype,
                                 top_block=self.top_blocks is not None))
        if any(isinstance(t, torch.Tensor) and t.is_cuda for t in x):
            ops.FALLBACKS["fpn_torch"] += 1
        inner, layer = self._blocks()
        results = fpn_torch(x[len(x) - len(inner):], inner, layer, self.top_blocks)
        if self.out_dtype is not torch.float32:
            results = [r.to(self.out_dtype) for r in results]
        return tuple(results)


def build_fpn(cfg, out_dtype=torch.float32, compute_dtype=None):
    """The pyramid of the config's backbone, as the reference builds it: DLA-34 stages ``MODEL.DLA.DLA_STAGE{2..5}_OUT_CHANNELS``
    -> ``MODEL.DLA.BACKBONE_OUT_CHANNELS`` channels, plain or GroupNorm / ReLU conv blocks by ``MODEL.FPN.USE_GN`` /
    ``USE_RELU``, and a ``LastLevelMaxPool``.  ``compute_dtype``: the pyramid's half compute mode (``FPN``)."""
    dla = cfg.MODEL.DLA
    stages = [dla.DLA_STAGE2_OUT_CHANNELS, dla.DLA_STAGE3_OUT_CHANNELS, dla.DLA_STAGE4_OUT_CHANNELS, dla.DLA_STAGE5_OUT_CHANNELS]
    gn = cfg.MODEL.GROUP_NORM
    block = conv_with_kaiming_uniform(cfg.MODEL.FPN.USE_GN, cfg.MODEL.FPN.USE_RELU, num_groups=gn.NUM_GROUPS, eps=gn.EPSILON)
    return FPN(stages, dla.BACKBONE_OUT_CHANNELS, block, top_blocks=LastLevelMaxPool(), out_dtype=out_dtype,
               compute_dtype=compute_dtype)
