"""The backbone as the reference builds it (siammot/modelling/backbone/backbone_ext.py): ``nn.Sequential(OrderedDict(body=DLA,
fpn=FPN))`` with ``.out_channels``, so that a reference checkpoint's ``backbone.body.*`` / ``backbone.fpn.*`` keys load with the
``backbone.`` prefix stripped.  Frames ``[N, 3, H, W]`` -> the five FPN maps, on this package's kernels from end to end."""
from collections import OrderedDict

import torch
from torch import nn

from .dla import build_dla
from .fpn import build_fpn


def build_backbone(cfg, out_dtype=torch.float32, operands="fp32", compute_dtype=None, fpn_compute_dtype=None, half_storage=False):
    """``out_dtype``: the element type of the FPN's maps; the body hands the pyramid fp32 stage maps.  ``operands``: the
    body's operand mode (``dla.DLA``: "fp32" or "split16").  ``compute_dtype``: the BODY's half compute mode (``dla.DLA``:
    None, ``torch.float16`` or ``torch.bfloat16``), and the body's alone; ``fpn_compute_dtype``: the pyramid's (``fpn.FPN``).
    ``half_storage``: the body stores its maps between layers in ``compute_dtype`` (``dla.DLA``, which needs ``compute_dtype``
    set) and hands the pyramid stage maps of that type; ``out_dtype`` keeps meaning the pyramid's."""
    if half_storage:
        body = build_dla(cfg, out_dtype=compute_dtype, operands=operands, compute_dtype=compute_dtype, half_storage=True)
    else:
        body = build_dla(cfg, operands=operands, compute_dtype=compute_dtype)
    fpn = build_fpn(cfg, out_dtype=out_dtype, compute_dtype=fpn_compute_dtype)
    if tuple(fpn.in_channels_list) != tuple(body.out_channels):
        raise ValueError("build_backbone: the body's stage widths %r are not the pyramid's inputs %r"
                         % (tuple(body.out_channels), tuple(fpn.in_channels_list)))
    model = nn.Sequential(OrderedDict([("body", body), ("fpn", fpn)]))
    model.out_channels = fpn.out_channels
    return model


def strip_prefix(state_dict, prefix="backbone."):
    """The entries of a checkpoint's ``state_dict`` under ``prefix``, with it removed (for ``load_state_dict``)."""
    return OrderedDict((k[len(prefix):], v) for k, v in state_dict.items() if k.startswith(prefix))
