"""DLA backbone body: the reference's ``siammot/modelling/backbone/dla.py`` for its ``DlaBasic`` networks (DLA-34, the
``CONV_BODY`` of the default config) and its ``DlaBottleneck`` networks at cardinality 1 (DLA-46-C, DLA-60, DLA-102, DLA-169:
trees up to five levels deep, residual roots) with [UPSTREAM] maskrcnn_benchmark's ``FrozenBatchNorm2d``, under upstream's
module tree and ``state_dict`` keys (``base_layer.0.weight``, ``level3.tree2.root.conv.weight``, ...: 195 for DLA-34, 875 for
DLA-169), so that a reference checkpoint's ``backbone.body.*`` loads.  Inference only.

    x  = cbr7x7(image, 3 -> c0)                           base_layer.{0,1}       cbr = conv (no bias), frozen BN, ReLU
    x0 = cbr3x3(x, c0 -> c0)                              level0.{0,1}           cb  = conv, frozen BN
    x1 = cbr3x3(x0, c0 -> c1, stride 2)                   level1.{0,1}
    x2 .. x5 = level2 .. level5 (DlaTree, stride 2 each)  -> [x2, x3, x4, x5]

Two forms of the operator live here:

* ``DLA.forward`` on device images within the kernels' capacities (``ops.dla_shapes_ok``): every convolution on the fp32
  matrix cores with the BN, the residual and the ReLU in its epilogue, the ``cat`` and the max-pool read in place by the 1x1
  kernel, one launch per evaluated convolution (37 for DLA-34, 63 for DLA-60, 168 for DLA-169), no host synchronisation;
  ``out_dtype`` half stores the stage maps rounded once; ``operands="split16"`` runs the trees' 3x3 convolutions on the
  16-bit matrix instruction with three-part bf16 operands and fp32 accumulation instead (fp32-grade results in another
  summation order, no dependence on the data's range).  ``DlaBasic`` networks with trees of depth <= 2
  take ``ops.dla``, every other one ``ops.dla_net``; ``compute_dtype=torch.float16`` or
  ``torch.bfloat16`` runs EVERY tree convolution (3x3 and 1x1) with operands rounded to that type on the 16-bit matrix
  instruction, fp32 accumulation and the fp32 epilogue (``ops.dla_half``): a half-precision result,
  not an fp32-grade one;
* ``dla_torch``: the same as a plain torch composition over the module tree.  It is the path for CPU tensors, images that
  are not contiguous NCHW, trainable parameters under grad mode and shapes beyond the capacities (counted in
  ``ops.FALLBACKS["dla_torch"]`` for device tensors), and the baseline of tools/dla_bench.py and
  tools/dla_bottleneck_bench.py.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import ops


class FrozenBatchNorm2d(nn.Module):
    """[UPSTREAM] ``maskrcnn_benchmark.layers.FrozenBatchNorm2d``: four buffers, ``y = x * scale + shift`` with ``scale =
    weight * running_var.rsqrt()`` (no epsilon) and ``shift = bias - running_mean * scale``."""

    def __init__(self, n):
        super(FrozenBatchNorm2d, self).__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))

    def scale_shift(self):
        scale = self.weight * self.running_var.rsqrt()
        return scale, self.bias - self.running_mean * scale

    def forward(self, x):
        scale, shift = self.scale_shift()
        return x * scale.to(x.dtype).reshape(1, -1, 1, 1) + shift.to(x.dtype).reshape(1, -1, 1, 1)


def _conv(cin, cout, k, stride=1):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=(k - 1) // 2, bias=False)


class DlaBasic(nn.Module):
    """``relu(bn2(conv2(relu(bn1(conv1(x))))) + residual)``, ``conv1`` with the stride; ``residual`` None: ``x``."""

    def __init__(self, cin, cout, stride=1):
        super(DlaBasic, self).__init__()
        for i, (c, s) in enumerate(((cin, stride), (cout, 1)), 1):
            self.add_module("conv%d" % i, _conv(c, cout, 3, s))
            self.add_module("bn%d" % i, FrozenBatchNorm2d(cout))

    def forward(self, x, residual=None):
        out = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(out)) + (x if residual is None else residual))


class DlaBottleneck(nn.Module):
    """Upstream's ``DlaBottleneck`` at cardinality 1 and base width 64: ``relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x))))))))
    + residual)`` with ``conv1`` 1x1 ``cin -> mid`` at the input's resolution, ``conv2`` 3x3 ``mid -> mid`` with the stride,
    ``conv3`` 1x1 ``mid -> cout`` and ``mid = cout // 2``; ``residual`` None: ``x``."""

    def __init__(self, cin, cout, stride=1):
        super(DlaBottleneck, self).__init__()
        mid = cout // 2
        for i, (a, b, k, s) in enumerate(((cin, mid, 1, 1), (mid, mid, 3, stride), (mid, cout, 1, 1)), 1):
            self.add_module("conv%d" % i, _conv(a, b, k, s))
            self.add_module("bn%d" % i, FrozenBatchNorm2d(b))

    def forward(self, x, residual=None):
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        return F.relu(self.bn3(self.conv3(out)) + (x if residual is None else residual))


BLOCKS = {"basic": DlaBasic, "bottleneck": DlaBottleneck}


def _block_convs(block):
    """(conv, bn) of a block in its launch order."""
    return [(getattr(block, "conv%d" % i), getattr(block, "bn%d" % i)) for i in (1, 2, 3) if hasattr(block, "conv%d" % i)]


class DlaRoot(nn.Module):
    """``relu(bn(conv1x1(cat(x))))``; ``residual``: ``relu(bn(conv1x1(cat(x))) + x[0])``."""

    def __init__(self, cin, cout, residual=False):
        super(DlaRoot, self).__init__()
        self.conv, self.bn = _conv(cin, cout, 1), FrozenBatchNorm2d(cout)
        self.residual = residual

    def forward(self, *x):
        y = self.bn(self.conv(torch.cat(x, 1)))
        return F.relu(y + x[0] if self.residual else y)


class DlaTree(nn.Module):
    """The aggregation tree over ``block`` blocks ("basic" or "bottleneck"; keys ``tree1``, ``tree2``, ``root``, ``project``,
    in that order) of any depth.  A ``levels`` = 1 tree is two blocks and a root over (x2, x1, what the parent handed down:
    ``handed`` channels, [bottom if ``level_root``]); a deeper tree is two trees one level shallower, the second at stride 1
    and handed what this tree was handed, its bottom (if ``level_root``) and the first one's output (only the outermost
    tree of a level has ``level_root``, and it is handed nothing).  ``project`` exists wherever ``cin != cout``, as upstream;
    the one of a tree with ``levels`` > 1 is evaluated and discarded there and is not evaluated here (its parameters are
    kept for the ``state_dict``).  ``residual_root``: every root adds its first argument before the ReLU."""

    def __init__(self, levels, cin, cout, stride=1, level_root=False, handed=0, block="basic", residual_root=False):
        super(DlaTree, self).__init__()
        own = cin if level_root else 0                            # the channels of `bottom`, where it joins the root
        if levels == 1:
            self.tree1, self.tree2 = BLOCKS[block](cin, cout, stride), BLOCKS[block](cout, cout)
            self.root = DlaRoot(2 * cout + own + handed, cout, residual_root)
        else:
            self.tree1 = DlaTree(levels - 1, cin, cout, stride, block=block, residual_root=residual_root)
            self.tree2 = DlaTree(levels - 1, cout, cout, handed=handed + own + cout, block=block, residual_root=residual_root)
        self.project = nn.Sequential(_conv(cin, cout, 1), FrozenBatchNorm2d(cout)) if cin != cout else None
        self.levels, self.level_root, self.stride = levels, level_root, stride

    def forward(self, x, children=()):
        bottom = F.max_pool2d(x, self.stride, self.stride) if self.stride > 1 else x
        children = list(children) + ([bottom] if self.level_root else [])
        if self.levels == 1:
            x1 = self.tree1(x, bottom if self.project is None else self.project(bottom))
            return self.root(self.tree2(x1), x1, *children)
        x1 = self.tree1(x)
        return self.tree2(x1, children + [x1])

    def convs(self):
        """(conv, bn) in the launch order of ``ops.dla`` / ``ops.dla_net``."""
        if self.levels > 1:
            return self.tree1.convs() + self.tree2.convs()
        head = [tuple(self.project)] if self.project is not None else []
        return head + _block_convs(self.tree1) + _block_convs(self.tree2) + [(self.root.conv, self.root.bn)]


def dla_torch(model, images):
    """The body as torch operators on any device: -> [x2, x3, x4, x5] in the parameters' dtype (half images are upcast
    first, as the kernels convert on load)."""
    x = images.to(model.base_layer[0].weight.dtype)
    x = model.level1(model.level0(model.base_layer(x)))
    out = []
    for level in (model.level2, model.level3, model.level4, model.level5):
        x = level(x)
        out.append(x)
    return out


class DLA(nn.Module):
    """Upstream's ``DLA(levels, channels, block=DlaBasic or DlaBottleneck, residual_root=...)`` as a feature extractor: ``forward(images [N, 3, H, W])`` -> the
    list of the four stage maps (strides 4, 8, 16, 32), H and W multiples of 32.  ``out_dtype``: the element type of the
    returned maps (float32, float16 or bfloat16: the fp32 result rounded once; the next stage reads the fp32 value).  On
    the device path the packed weights are rebuilt when a parameter's or buffer's ``_version``, storage or device changes.
    ``operands``: "fp32" (the default) or "split16": which kernel the device path runs for the trees' 3x3 convolutions
    (module docstring); the torch composition, the ``state_dict`` and what ``kernel_ok`` admits do not depend on it.
    ``block`` ("basic" or "bottleneck") and ``residual_root`` are upstream's, keyword-only.
    ``compute_dtype`` (keyword-only): None (the default: ``operands`` decides, nothing changes), ``torch.float16`` or
    ``torch.bfloat16``: the device path runs every tree convolution, 3x3 and 1x1, with its input (as it is loaded) and its
    filters (once, when packed) rounded to that type — ``tensor.to``'s rounding; an fp16 operand beyond 65,504 is +-inf —
    with exact products and fp32 accumulation; the stem, the BN, the residuals and the maps between layers stay fp32, and
    ``out_dtype`` keeps its meaning.  It excludes ``operands="split16"`` (two answers to one question).  The torch
    composition ``dla_torch`` does not depend on it, exactly as it does not depend on ``operands``: CPU tensors and every
    fallback give the bits of fp32 mode.  The ``state_dict`` and what ``kernel_ok`` admits do not depend on it either.
    ``half_storage`` (keyword-only, default False): a refinement of ``compute_dtype``, which it needs, with ``out_dtype``
    given as that same type: the device path stores every map a tree convolution writes — block intermediates and outputs,
    ``project`` outputs, roots, the four stage maps — in ``compute_dtype``, the fp32 epilogue value rounded once
    (``ops.dla_half_storage``).  No convolution operand changes by a bit against half compute mode
    (rounding a stored value again is idempotent, the max-pool commutes with the rounding); a residual that is a stored map
    is added as the rounded value, and the returned stage maps ARE the stored maps (no copy, no second rounding).  The
    stem and its output ``x1`` stay fp32.  The ``state_dict``, ``kernel_ok``, the packed weights (``ops.dla_half_pack``'s)
    and the launches do not depend on it; CPU tensors and every fallback give fp32 mode's result ``.to(out_dtype)``.
    NOT RECOMMENDED FOR SPEED: measured, it is 1.15 ... 1.86 x slower than half compute mode without it in every case
    (DESIGN.md §7); what it buys is the smaller workspace and half stage maps for the pyramid without a conversion."""

    def __init__(self, levels, channels, out_dtype=torch.float32, operands="fp32", *, block="basic", residual_root=False,
                 compute_dtype=None, half_storage=False):
        super(DLA, self).__init__()
        if operands not in ops.DLA_OPERANDS:
            raise ValueError("DLA: operands must be \"fp32\" or \"split16\", got %r" % (operands,))
        if compute_dtype is not None and compute_dtype not in ops.DLA_COMPUTE_TYPES:
            raise ValueError("DLA: compute_dtype must be None, torch.float16 or torch.bfloat16, got %r" % (compute_dtype,))
        if compute_dtype is not None and operands != "fp32":
            raise ValueError("DLA: compute_dtype=%r excludes operands=%r: the half compute mode and the split operands are two "
                             "answers to one question" % (compute_dtype, operands))
        if half_storage and compute_dtype is None:
            raise ValueError("DLA: half_storage=True needs compute_dtype=torch.float16 or torch.bfloat16: it stores the maps "
                             "between layers in the compute type")
        if half_storage and out_dtype is not compute_dtype:
            raise ValueError("DLA: half_storage=True returns the stored maps themselves, so out_dtype must be given as the "
                             "compute_dtype %r, got out_dtype=%r" % (compute_dtype, out_dtype))
        self.compute_dtype, self.half_storage = compute_dtype, bool(half_storage)
        if block not in BLOCKS:
            raise ValueError("DLA: block must be \"basic\" or \"bottleneck\", got %r" % (block,))
        self.operands, self.block, self.residual_root = operands, block, bool(residual_root)
        levels, channels = tuple(int(v) for v in levels), tuple(int(v) for v in channels)
        if len(levels) != 6 or len(channels) != 6:
            raise ValueError("DLA: six levels and six channel counts, got %r and %r" % (levels, channels))
        self.levels, self.channels = levels, channels
        self.out_dtype = out_dtype
        self.base_layer = nn.Sequential(_conv(3, channels[0], 7), FrozenBatchNorm2d(channels[0]), nn.ReLU(inplace=True))
        self.level0 = self._conv_level(channels[0], channels[0], levels[0])
        self.level1 = self._conv_level(channels[0], channels[1], levels[1], stride=2)
        for k in range(2, 6):
            self.add_module("level%d" % k, DlaTree(levels[k], channels[k - 1], channels[k], 2, level_root=k > 2, block=block,
                                                   residual_root=self.residual_root))
        # the DlaBasic networks of depth <= 2 keep the entry point they had (ops.dla); every other one takes ops.dla_net
        self._net = block != "basic" or self.residual_root or max(levels[2:]) > 2
        self.out_channels = channels[2:]
        self._packed_key, self._packed = None, None

    @staticmethod
    def _conv_level(cin, cout, count, stride=1):
        """``count`` cbr3x3 layers, the first with the stride and the change of width: keys 0, 1, (2: the ReLU), 3, 4, ..."""
        layers = []
        for i in range(count):
            layers += [_conv(cout if i else cin, cout, 3, 1 if i else stride), FrozenBatchNorm2d(cout), nn.ReLU(inplace=True)]
        return nn.Sequential(*layers)

    def convs(self):
        """(conv, bn) of every convolution that is evaluated, in the launch order of ``ops.dla``."""
        out = [(self.base_layer[0], self.base_layer[1])]
        if len(self.level0) == 3 and len(self.level1) == 3:
            out += [(self.level0[0], self.level0[1]), (self.level1[0], self.level1[1])]
        for level in (self.level2, self.level3, self.level4, self.level5):
            out += level.convs()
        return out

    def kernel_ok(self, images):
        """This call takes ``ops.dla``."""
        if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dim() == 4 and images.shape[1] == 3):
            return False
        if images.dtype not in ops.FEAT_TYPES or self.out_dtype not in ops.FEAT_TYPES or not images.is_contiguous():
            return False
        tensors = list(self.parameters()) + list(self.buffers())
        if not all(t.dtype is torch.float32 and t.device == images.device for t in tensors):
            return False
        if torch.is_grad_enabled() and (images.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        N, _, H, W = images.shape
        return N >= 1 and ops.dla_shapes_ok(self.levels, self.channels, H, W, N, self.block)

    def _pack(self):
        with torch.no_grad():
            convs = [(c.weight.detach(),) + tuple(t.contiguous() for t in bn.scale_shift()) for c, bn in self.convs()]
            if self.compute_dtype is not None:
                return ops.dla_half_pack(convs, self.levels, self.channels, self.compute_dtype, block=self.block,
                                         residual_root=self.residual_root)
            if self._net:
                return ops.dla_net_pack(convs, self.levels, self.channels, block=self.block, residual_root=self.residual_root,
                                        operands=self.operands)
            return ops.dla_pack(convs, self.levels, self.channels, operands=self.operands)

    def packed(self):
        """The packed weights for a launch on the current stream: packed on the stream of the first call after a change and
        ordered for every other stream by ``ops.StreamImage`` (an event wait on the device, no host synchronisation)."""
        tensors = list(self.parameters()) + list(self.buffers())
        key = (self.operands, self.compute_dtype) + tuple((t.data_ptr(), t._version, t.device) for t in tensors)
        if key != self._packed_key:
            self._packed = ops.StreamImage(self._pack, tensors[0].device)
            self._packed_key = key
        return self._packed.get()

    def forward(self, images):
        if self.kernel_ok(images):
            if self.compute_dtype is not None and self.half_storage:
                return ops.dla_half_storage(images, self.packed(), self.levels, self.channels, self.compute_dtype, block=self.block,
                                            residual_root=self.residual_root)
            if self.compute_dtype is not None:
                return ops.dla_half(images, self.packed(), self.levels, self.channels, self.compute_dtype, block=self.block,
                                    residual_root=self.residual_root, out_dtype=self.out_dtype)
            if self._net:
                return ops.dla_net(images, self.packed(), self.levels, self.channels, block=self.block,
                                   residual_root=self.residual_root, out_dtype=self.out_dtype, operands=self.operands)
            return ops.dla(images, self.packed(), self.levels, self.channels, out_dtype=self.out_dtype, operands=self.operands)
        if isinstance(images, torch.Tensor) and images.is_cuda:
            ops.FALLBACKS["dla_torch"] += 1
        out = dla_torch(self, images)
        if self.out_dtype is not torch.float32:
            out = [o.to(self.out_dtype) for o in out]
        return out


def dla_34(out_dtype=torch.float32, operands="fp32", compute_dtype=None, half_storage=False):
    return DLA((1, 1, 1, 2, 2, 1), (16, 32, 64, 128, 256, 512), out_dtype=out_dtype, operands=operands, compute_dtype=compute_dtype,
               half_storage=half_storage)


def dla_46_c(out_dtype=torch.float32, operands="fp32", compute_dtype=None, half_storage=False):
    return DLA((1, 1, 1, 2, 2, 1), (16, 32, 64, 64, 128, 256), out_dtype=out_dtype, operands=operands, block="bottleneck",
               compute_dtype=compute_dtype, half_storage=half_storage)


def dla_60(out_dtype=torch.float32, operands="fp32", compute_dtype=None, half_storage=False):
    return DLA((1, 1, 1, 2, 3, 1), (16, 32, 128, 256, 512, 1024), out_dtype=out_dtype, operands=operands, block="bottleneck",
               compute_dtype=compute_dtype, half_storage=half_storage)


def dla_102(out_dtype=torch.float32, operands="fp32", compute_dtype=None, half_storage=False):
    return DLA((1, 1, 1, 3, 4, 1), (16, 32, 128, 256, 512, 1024), out_dtype=out_dtype, operands=operands, block="bottleneck",
               residual_root=True, compute_dtype=compute_dtype, half_storage=half_storage)


def dla_169(out_dtype=torch.float32, operands="fp32", compute_dtype=None, half_storage=False):
    return DLA((1, 1, 2, 3, 5, 1), (16, 32, 128, 256, 512, 1024), out_dtype=out_dtype, operands=operands, block="bottleneck",
               residual_root=True, compute_dtype=compute_dtype, half_storage=half_storage)


BODIES = {"DLA-34-FPN": dla_34, "DLA-46-C-FPN": dla_46_c, "DLA-60-FPN": dla_60, "DLA-102-FPN": dla_102, "DLA-169-FPN": dla_169}
# upstream's other registered bodies: grouped 3x3 convolutions (DLA-46-XC) and Res2Net blocks, which this package does not have
UNSUPPORTED_BODIES = ("DLA-46-XC-FPN", "DLA-60-RES2NET-FPN")


def build_dla(cfg, out_dtype=torch.float32, operands="fp32", compute_dtype=None, half_storage=False):
    """The body of the config's ``MODEL.BACKBONE.CONV_BODY``: one of ``BODIES``.  Any other body, any true entry of
    ``MODEL.DLA.STAGE_WITH_DCN`` (deformable convolutions) and stage widths in ``MODEL.DLA.DLA_STAGE*_OUT_CHANNELS`` that
    are not the body's raise a ``ValueError`` that names the body or the entry."""
    name = cfg.MODEL.BACKBONE.CONV_BODY
    if name in UNSUPPORTED_BODIES:
        raise ValueError("build_dla: CONV_BODY %r needs grouped 3x3 convolutions or Res2Net blocks, which this package does not "
                         "have (it has %s)" % (name, ", ".join(sorted(BODIES))))
    if name not in BODIES:
        raise ValueError("build_dla: CONV_BODY %r is not in this package (it has %s)" % (name, ", ".join(sorted(BODIES))))
    dcn = tuple(getattr(cfg.MODEL.DLA, "STAGE_WITH_DCN", ()) or ())
    if any(dcn):
        raise ValueError("build_dla: MODEL.DLA.STAGE_WITH_DCN = %r asks for deformable convolutions, which this package does "
                         "not have" % (dcn,))
    body = BODIES[name](out_dtype=out_dtype, operands=operands, compute_dtype=compute_dtype, half_storage=half_storage)
    dla = cfg.MODEL.DLA
    stages = (dla.DLA_STAGE2_OUT_CHANNELS, dla.DLA_STAGE3_OUT_CHANNELS, dla.DLA_STAGE4_OUT_CHANNELS, dla.DLA_STAGE5_OUT_CHANNELS)
    if tuple(stages) != tuple(body.out_channels):
        raise ValueError("build_dla: %s has stage widths %r, the config's MODEL.DLA.DLA_STAGE*_OUT_CHANNELS are %r"
                         % (name, tuple(body.out_channels), tuple(stages)))
    return body
