"""Golden vectors of the bottleneck / deep-tree DLA bodies: tests/golden/dla_bottleneck_stages.npz.

The reference's siammot/modelling/backbone/dla.py, imported UNMODIFIED by path with the stubs of tools/gen_golden_dla.py
(``reference_dla``), run as ``DLA(levels, channels, block=DlaBottleneck, residual_root=...)`` on the cases of
tests/dla_bottleneck_cases.py with the recipe of tests/dla_cases.py (``params``, ``image``, N = 1, seed 7).  Per case the file
holds the seed, the image's shape, the four stage maps of ``module.double()`` and, per stage, ``e32 = max|o32 - o64| /
max|o64|`` of the reference's own fp32 run: the tests' bounds are multiples of it.  No weights and no fp32 maps are stored.

    python tools/gen_golden_dla_bottleneck.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dla_bottleneck_cases as B  # noqa: E402
import dla_cases as D  # noqa: E402
from gen_golden_dla import reference_dla  # noqa: E402


def main():
    ref = reference_dla()
    out = {}
    for case, (levels, channels, shape, residual_root) in B.NET_CASES.items():
        model = ref.DLA(list(levels), list(channels), block=ref.DlaBottleneck, residual_root=residual_root, dcn_config=(False,) * 6)
        assert len(model.state_dict()) == B.NET_KEYS[case], (case, len(model.state_dict()))
        D.load(model, D.params(model, B.SEED))
        x = torch.from_numpy(D.image(shape, B.SEED))
        with torch.no_grad():
            o32 = [o.clone() for o in model(x.clone())]
            o64 = [o.clone() for o in model.double()(x.double())]
        e32 = D.stage_error(o32, o64)
        for k, (o, e) in enumerate(zip(o64, e32)):
            nz, top = float((o != 0).double().mean()), float(o.abs().max())
            print("case %s stage %d %s: max|o64| %.2f, non-zero %.1f %%, e32 %.2e" % (case, k + 2, tuple(o.shape), top, 100 * nz, e))
            # (a deep residual-root level grows: every root adds its first source; it stays far inside fp32's range)
            assert 1e-7 < e < 2e-6 and nz >= 0.5 and bool(torch.isfinite(o).all()) and top < 1e5, (case, k, e, nz, top)
            out["%s_o64_%d" % (case, k)] = o.numpy()
        out["%s_e32" % case] = np.asarray(e32, dtype=np.float64)
        out["%s_shape" % case] = np.asarray(shape, dtype=np.int64)
        out["%s_seed" % case] = np.asarray(B.SEED, dtype=np.int64)
    np.savez_compressed(B.GOLDEN, **out)
    size = os.path.getsize(B.GOLDEN)
    assert size < 1 << 20, size
    print("%s: %d bytes" % (B.GOLDEN, size))


if __name__ == "__main__":
    main()
