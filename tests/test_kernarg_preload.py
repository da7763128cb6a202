"""The frame pair's kernels get their leading arguments in user SGPRs (kernel-argument preload): read back from the kernel
descriptors of the gfx950 code objects inside the two built libraries.  Needs no GPU."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_module():
    spec = importlib.util.spec_from_file_location("smot_build", os.path.join(ROOT, "siam-mot_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def build_mod():
    return _build_module()


def test_flag_is_in_the_build_of_both_libraries(build_mod):
    assert "-amdgpu-kernarg-preload-count=16" in build_mod.FLAGS
    assert build_mod.FLAGS[build_mod.FLAGS.index("-amdgpu-kernarg-preload-count=16") - 1] == "-mllvm"


@pytest.mark.parametrize("which", ["LIB", "LIB_DEBUG"])
def test_every_instantiation_of_the_four_kernels_has_preloaded_arguments(build_mod, which):
    lib = getattr(build_mod, which)
    assert os.path.exists(lib), "%s is not built" % lib
    kds = build_mod.kernel_descriptors(lib)
    assert len(kds) > 100                                        # the whole library's kernels were found
    fam = {k: v for k, v in kds.items() if any("%d%sI" % (len(f), f) in k for f in build_mod.PRELOAD_FAMILIES)}
    # every family is there, in all its forms: single image, batched, fp16 / bf16, channels-last; 16 x 16 and 29 x 29 towers;
    # the three thread-group splits of the decode
    for f in build_mod.PRELOAD_FAMILIES:
        assert any("%d%sI" % (len(f), f) in k for k in fam), f
    assert sum("13decode_kernelI" in k for k in fam) == 3
    assert sum("17tower_wino_kernelI" in k for k in fam) >= 3
    assert sum("sr_xcorr_fused9_" in k for k in fam) >= 36
    none = sorted(k for k, v in fam.items() if v["preload"] == 0)
    assert not none, "no kernel arguments preloaded: %s" % none
    # kernels that do not lead with plain arguments get none: the field read above is the preload length, not a constant
    assert any(v["preload"] == 0 for k, v in kds.items() if k not in fam)
    # ... and the build's own check passes on the library as built (LDS, scratch and registers of the hot forms included)
    build_mod.check_preload(lib, verbose=False)
