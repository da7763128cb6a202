"""Golden vectors of the DLA backbone body: tests/golden/dla_stages.npz.

Imported UNMODIFIED from the reference checkout ($SIAMMOT_REFERENCE): siammot/modelling/backbone/dla.py, loaded by path with
``sys.modules`` stubs for what it imports and this body does not use:

    maskrcnn_benchmark.layers            Conv2d = nn.Conv2d, FrozenBatchNorm2d restated ([UPSTREAM]: four buffers, scale =
                                         weight * running_var.rsqrt(), y = x * scale + (bias - running_mean * scale)),
                                         DFConv2d = None
    torchvision.models.utils, timm.models.layers, maskrcnn_benchmark.utils.registry / .model_serialization   empty names

Per case of tests/dla_cases.py (N = 1, seed 7, block = DlaBasic) the file holds the seed, the image's shape, the four stage
maps of ``module.double()`` and, per stage, ``e32 = max|o32 - o64| / max|o64|`` of the reference's own fp32 run: the tests'
bounds are multiples of it.  No weights and no fp32 maps are stored: dla_cases.params / image regenerate the inputs.

    python tools/gen_golden_dla.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("SIAMMOT_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dla_cases as D  # noqa: E402


class FrozenBatchNorm2d(nn.Module):
    def __init__(self, n):
        super(FrozenBatchNorm2d, self).__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))

    def forward(self, x):
        scale = self.weight * self.running_var.rsqrt()
        bias = self.bias - self.running_mean * scale
        return x * scale.reshape(1, -1, 1, 1) + bias.reshape(1, -1, 1, 1)


def reference_dla():
    stubs = {
        "maskrcnn_benchmark": {}, "maskrcnn_benchmark.utils": {}, "torchvision.models.utils": {"load_state_dict_from_url": None},
        "maskrcnn_benchmark.layers": {"Conv2d": nn.Conv2d, "FrozenBatchNorm2d": FrozenBatchNorm2d, "DFConv2d": None},
        "timm": {}, "timm.models": {}, "timm.models.layers": {"SelectAdaptivePool2d": None},
        "maskrcnn_benchmark.utils.registry": {"Registry": dict},
        "maskrcnn_benchmark.utils.model_serialization": {"load_state_dict": None},
    }
    for name, attrs in stubs.items():
        mod = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
    path = os.path.join(REFERENCE, "siammot", "modelling", "backbone", "dla.py")
    spec = importlib.util.spec_from_file_location("reference_dla", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = reference_dla()
    out = {}
    for case, (levels, channels, shape) in D.NET_CASES.items():
        model = ref.DLA(list(levels), list(channels), block=ref.DlaBasic, dcn_config=(False,) * 6)
        assert len(model.state_dict()) == D.NET_KEYS[case], (case, len(model.state_dict()))
        D.load(model, D.params(model, D.SEED))
        x = torch.from_numpy(D.image(shape, D.SEED))
        with torch.no_grad():
            o32 = [o.clone() for o in model(x.clone())]
            o64 = [o.clone() for o in model.double()(x.double())]
        e32 = D.stage_error(o32, o64)
        for k, (o, e) in enumerate(zip(o64, e32)):
            nz = float((o != 0).double().mean())
            print("case %s stage %d %s: max|o64| %.2f, non-zero %.1f %%, e32 %.2e" % (case, k + 2, tuple(o.shape), float(o.abs().max()),
                                                                                  100 * nz, e))
            assert 1e-7 < e < 2e-6 and nz > 0.4, (case, k, e, nz)
            out["%s_o64_%d" % (case, k)] = o.numpy()
        out["%s_e32" % case] = np.asarray(e32, dtype=np.float64)
        out["%s_shape" % case] = np.asarray(shape, dtype=np.int64)
        out["%s_seed" % case] = np.asarray(D.SEED, dtype=np.int64)
    np.savez_compressed(D.GOLDEN, **out)
    print("%s: %d bytes" % (D.GOLDEN, os.path.getsize(D.GOLDEN)))


if __name__ == "__main__":
    main()
