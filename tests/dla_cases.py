"""Cases of the DLA backbone tests and their yardsticks — TEST INFRASTRUCTURE.

Network level: the golden vectors tests/golden/dla_stages.npz (tools/gen_golden_dla.py: the reference's own dla.py in fp64, and
per stage the error ``e32`` of the reference's own fp32 run) and the parameter recipe ``params`` that the generator and the
tests share.

Operator level: torch's ``F.conv2d`` / ``F.max_pool2d`` / ``torch.cat`` on the CPU in fp64 and fp32, written from the contract
(include/smot_emm.h, DLA BACKBONE):

    conv3x3:  relu?(conv2d(x, w, stride, padding 1) * scale + shift (+ residual, or + max_pool2d(residual, 2, 2)))
    conv1x1:  relu?(conv2d(cat([max_pool2d(s, 2, 2) if pooled else s for s in sources], 1), w) * scale + shift)
    stem:     cbr3x3(cbr3x3(cbr7x7(image, pad 3)), stride 2)

with weights ~ N(0, 0.05), maps ~ N(0, 4), and ``scale`` / ``shift`` from the recipe's frozen BN.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dla_stages.npz")
DLA34 = ((1, 1, 1, 2, 2, 1), (16, 32, 64, 128, 256, 512))
# case -> (levels, channels, (H, W)); N = 1, seed 7
NET_CASES = {
    "A": DLA34 + ((64, 96),),                                     # stage maps 16 x 24 down to 2 x 3
    "B": DLA34 + ((32, 160),),                                    # stage 5 is one row, 1 x 5
    # a levels = 2 tree without level_root; widths that are no powers of two and no multiples of the 128-channel block
    "C": ((1, 1, 2, 1, 2, 1), (16, 32, 32, 64, 96, 160), (64, 96)),
}
NET_KEYS = {"A": 195, "B": 195, "C": 185}
SEED = 7


def params(module_or_keys, seed):
    """The recipe: one ``RandomState(seed)`` walked over the ``state_dict`` in key order -> {key: fp32 array}.
    ``running_var ~ U(0.5, 2)``, ``running_mean ~ N(0, 0.2)``, BN ``bias ~ N(0.2, 0.3)``, BN ``weight ~ U(0.5, 1.5)``, conv
    weights ``~ N(0, sqrt(1 / fan_in))``.  module_or_keys: a module, or [(key, shape)]."""
    items = ([(k, tuple(v.shape)) for k, v in module_or_keys.state_dict().items()] if hasattr(module_or_keys, "state_dict")
             else list(module_or_keys))
    rs = np.random.RandomState(seed)
    out = {}
    for key, shape in items:
        if key.endswith("running_var"):
            v = rs.uniform(0.5, 2.0, size=shape)
        elif key.endswith("running_mean"):
            v = rs.standard_normal(shape) * 0.2
        elif key.endswith(".bias"):
            v = 0.2 + rs.standard_normal(shape) * 0.3
        elif len(shape) == 1:
            v = rs.uniform(0.5, 1.5, size=shape)
        else:
            v = rs.standard_normal(shape) * (1.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        out[key] = v.astype(F32)
    return out


def image(shape, seed, N=1):
    rs = np.random.RandomState(1000 + seed + 31 * shape[0] + shape[1])
    return rs.standard_normal((N, 3) + tuple(shape)).astype(F32)


def load(module, prm, dev="cpu"):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in prm.items()}, strict=True)
    return module.to(dev).eval()


def stage_error(out, o64):
    """Per stage ``max|out - o64| / max|o64|`` over the whole map."""
    return [float((o.detach().double().cpu() - torch.as_tensor(w)).abs().max() / torch.as_tensor(w).abs().max())
            for o, w in zip(out, o64)]


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
def _t(v, dtype):
    return (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(dtype)


def bn_scale_shift(C, rs):
    """scale, shift of a frozen BN drawn by the recipe (fp32 arithmetic, as the module's)."""
    var, mean = rs.uniform(0.5, 2.0, size=C).astype(F32), (rs.standard_normal(C) * 0.2).astype(F32)
    bias, weight = (0.2 + rs.standard_normal(C) * 0.3).astype(F32), rs.uniform(0.5, 1.5, size=C).astype(F32)
    scale = (torch.from_numpy(weight) * torch.from_numpy(var).rsqrt()).numpy()
    return scale, (torch.from_numpy(bias) - torch.from_numpy(mean) * torch.from_numpy(scale)).numpy()


def conv3x3_case(Cin, Cout, stride, size, N, seed=0):
    rs = np.random.RandomState(5000 + Cin + 3 * Cout + 7 * stride + size[0] + seed)
    ho, wo = ((size[0] - 1) // 2 + 1, (size[1] - 1) // 2 + 1) if stride == 2 else size
    scale, shift = bn_scale_shift(Cout, rs)
    return dict(x=(rs.standard_normal((N, Cin) + tuple(size)) * 4.0).astype(F32),
                w=(rs.standard_normal((Cout, Cin, 3, 3)) * 0.05).astype(F32), scale=scale, shift=shift,
                residual=(rs.standard_normal((N, Cout, ho, wo)) * 4.0).astype(F32), stride=stride)


def conv3x3_oracle(c, dtype, residual=True, relu=True, pre=False):
    y = F.conv2d(_t(c["x"], dtype), _t(c["w"], dtype), stride=c["stride"], padding=1)
    y = y * _t(c["scale"], dtype).reshape(1, -1, 1, 1) + _t(c["shift"], dtype).reshape(1, -1, 1, 1)
    if residual:                                                 # ("residual_pooled": a map twice as fine, read through the pool)
        r = _t(c["residual"], dtype)
        y = y + (F.max_pool2d(r, 2, 2) if c.get("residual_pooled") else r)
    return y if (pre or not relu) else F.relu(y)


def conv1x1_case(sources, Cout, size, N, seed=0):
    """sources: [(channels, pooled: False, or the (H, W) of the finer map)]."""
    rs = np.random.RandomState(6000 + 5 * Cout + len(sources) + size[0] + seed)
    K = sum(c for c, _ in sources)
    scale, shift = bn_scale_shift(Cout, rs)
    return dict(src=[(rs.standard_normal((N, c) + tuple(p if p else size)) * 4.0).astype(F32) for c, p in sources],
                pooled=[bool(p) for _, p in sources], w=(rs.standard_normal((Cout, K, 1, 1)) * 0.05).astype(F32),
                scale=scale, shift=shift)


def conv1x1_oracle(c, dtype, relu=True, pre=False):
    cat = torch.cat([F.max_pool2d(_t(s, dtype), 2, 2) if p else _t(s, dtype) for s, p in zip(c["src"], c["pooled"])], 1)
    y = F.conv2d(cat, _t(c["w"], dtype))
    y = y * _t(c["scale"], dtype).reshape(1, -1, 1, 1) + _t(c["shift"], dtype).reshape(1, -1, 1, 1)
    return y if (pre or not relu) else F.relu(y)


def stem_case(c0, c1, size, N, seed=0):
    rs = np.random.RandomState(7000 + c0 + c1 + size[0] + size[1] + seed)
    layers = []
    for cout, cin, k in ((c0, 3, 7), (c0, c0, 3), (c1, c0, 3)):
        w = (rs.standard_normal((cout, cin, k, k)) * (1.0 / (cin * k * k)) ** 0.5).astype(F32)
        layers.append((w,) + bn_scale_shift(cout, rs))
    return dict(image=rs.standard_normal((N, 3) + tuple(size)).astype(F32), layers=layers)


def stem_oracle(c, dtype, pre=False):
    y = _t(c["image"], dtype)
    for i, (w, scale, shift) in enumerate(c["layers"]):
        y = F.conv2d(y, _t(w, dtype), stride=2 if i == 2 else 1, padding=w.shape[-1] // 2)
        y = y * _t(scale, dtype).reshape(1, -1, 1, 1) + _t(shift, dtype).reshape(1, -1, 1, 1)
        if i < 2 or not pre:
            y = F.relu(y)
    return y


def channel_scale(pre64):
    """max |fp64 pre-ReLU value| per output channel over every image and position -> ``[C]`` (no channel has scale 0)."""
    return pre64.abs().amax(dim=(0, 2, 3))


def scaled_error(out, ref, scale):
    """max over the FINITE reference cells of |out - ref| / scale[channel]."""
    ref = ref.double()
    d = (out.detach().double().cpu() - ref).abs() / scale.reshape(1, -1, 1, 1)
    ok = torch.isfinite(ref)
    return float(d[ok].max()) if bool(ok.any()) else 0.0
