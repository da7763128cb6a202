"""Build ``csrc/libsmot_emm.so`` (HIP, gfx950) in-tree with hipcc.

    python siam-mot_amd/build.py            # build if stale
    python siam-mot_amd/build.py --force

Two libraries come out of the same sources:
  csrc/libsmot_emm.so        the product: no environment variable is read, no kernel A/B switch, no ablation;
  csrc/libsmot_emm_debug.so  the measurement build (-DSMOT_DEBUG, + measure/csrc/*.hip and *.inc): older kernel generations,
                             A/B switches and timing ablations for tools/ and the A/B tests (csrc/knobs.h).

The library is plain HIP behind a C ABI (include/smot_emm.h): no torch headers, so it is
compiled with hipcc directly rather than through torch.utils.cpp_extension.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libsmot_emm.so")
LIB_DEBUG = os.path.join(CSRC, "libsmot_emm_debug.so")
MEASURE_CSRC = os.path.join(os.path.dirname(HERE), "measure", "csrc")      # measurement-only sources (not product)
DEBUG_ONLY_SOURCES = ["xcorr_variants.hip", "sr_xcorr_plan.hip"]
SOURCES = ["common.hip", "roi_align.hip", "xcorr.hip", "predictor.hip", "decode.hip", "sr_xcorr.hip", "sr_xcorr_small.hip", "nms.hip", "tower_wino.hip", "tower_conv.hip", "preprocess.hip",
           "emm_fused.hip", "track_solver.hip", "box_refine.hip", "linear_rows.hip", "memory_carry.hip", "rpn_proposals.hip",
           "box_detect.hip", "rpn_head.hip", "fpn.hip", "dla.hip"]
ARCH = "gfx950"
# -fno-slp-vectorize: keeps the xcorr FMA stream as v_fma_f32 with an SGPR tap operand instead of
# v_pk_fma_f32 + register shuffles (measured: 450 pk_fma + 204 movs vs 900 fma + 4 movs).
# -ffp-contract=off: the reference's torch kernels round every mul/add separately; coordinate and
# score arithmetic must do the same (a contracted `start + p*bin` moves a bilinear sample point by
# 1 ulp ~ 1e-5 in the output).  FMAs are written explicitly (fmaf) where they are wanted.
# (tower_wino.hip without -fno-slp-vectorize was measured: the packed adds hipcc then forms in the operand transform make
# both forms of the kernel slower — fp32 main loop 40.6 k -> 42.4 k cycles, bf16 x 3 32.7 k -> 37.9 k)
# -mllvm -amdgpu-kernarg-preload-count=16: leading scalar / pointer kernel arguments are delivered in user SGPRs with the
# wave instead of through an s_load from the kernel-argument segment (gfx950 takes 14 dwords beside the segment pointer; a
# by-value struct ends the preloaded run, so the four frame-pair kernels lead with plain arguments — see the "Argument order"
# comments at sr_xcorr_fused9_kernel, tower_wino_kernel and decode_kernel).  Their first data loads then need no scalar
# round trip in front of them.  check_preload() below reads the result back from the built libraries.
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-ffp-contract=off", "--offload-arch=" + ARCH,
         "-mllvm", "-amdgpu-kernarg-preload-count=16"]

# The frame pair's kernels, every instantiation of which must have its leading arguments preloaded, and what a workgroup of
# the product's hot forms may use without losing its workgroups per CU: (substring of the mangled name, LDS bytes, VGPRs).
PRELOAD_FAMILIES = ("sr_xcorr_fused9_kernel", "sr_xcorr_fused9_batched_kernel", "sr_xcorr_fused9_half_kernel",
                    "sr_xcorr_fused9_half_batched_kernel", "sr_xcorr_fused9_nhwc_kernel", "tower_wino_kernel", "decode_kernel")
HOT_FORMS = (
    ("22sr_xcorr_fused9_kernelILi30ELi15ELi2ELb1ELi8ELb0ELi1EE", 76176, 128),     # two workgroups of eight waves per CU
    ("22sr_xcorr_fused9_kernelILi15ELi15ELi2ELb0ELi8ELb0ELi0EE", 51728, 80),      # three (launch bound: 6 waves per SIMD)
    ("17tower_wino_kernelILi0ELi2ELi0ELb1EE", 0, 256),                            # one of 512 threads (dynamic LDS: 122,880 B)
    ("13decode_kernelILi2EE", 5072, 64),                                          # eight waves per SIMD
)


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def _src(name):
    return os.path.join(MEASURE_CSRC if name in DEBUG_ONLY_SOURCES else CSRC, name)


def _deps(sources):
    hdrs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".h")]
    if any(s in DEBUG_ONLY_SOURCES for s in sources):      # the measurement build also includes measure/csrc/*.inc
        hdrs += [os.path.join(MEASURE_CSRC, f) for f in sorted(os.listdir(MEASURE_CSRC)) if f.endswith(".inc")]
    return [_src(s) for s in sources] + hdrs + [
        os.path.join(os.path.dirname(HERE), "include", "smot_emm.h"), os.path.abspath(__file__)]


def _stale(lib, sources):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(d) > t for d in _deps(sources))


def _build_one(lib, sources, extra_flags, objdir, verbose):
    from concurrent.futures import ThreadPoolExecutor
    hipcc = _hipcc()
    os.makedirs(objdir, exist_ok=True)
    lib_t = os.path.getmtime(lib) if os.path.exists(lib) else 0.0
    hdr_t = max(os.path.getmtime(d) for d in _deps([]))
    jobs, objs = [], []
    for s in sources:
        obj = os.path.join(objdir, s.replace(".hip", ".o"))
        objs.append(obj)
        src = _src(s)
        # per-object staleness: recompile only what changed (a header change recompiles everything)
        if os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(src), hdr_t) and lib_t:
            continue
        jobs.append([hipcc] + FLAGS + extra_flags + ["-I", CSRC, "-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(run, jobs))
    run([hipcc, "-shared", "-fPIC", "--offload-arch=" + ARCH] + objs + ["-o", lib])
    return lib


def code_objects(lib):
    """The gfx950 code objects (ELF images) inside a built library: one per source file, in its offload bundles."""
    data = open(lib, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, pos = [], data.find(magic)
    while pos >= 0:
        n = int.from_bytes(data[pos + 24:pos + 32], "little")
        q = pos + 32
        for _ in range(n):
            off, size, tl = (int.from_bytes(data[q + 8 * k:q + 8 * k + 8], "little") for k in range(3))
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if triple.startswith("hip") and ARCH in triple and size:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(magic, pos + 1)
    return out


def kernel_descriptors(lib):
    """{mangled kernel name: {"preload", "lds", "scratch", "vgprs"}} from the kernel descriptors (the 64-byte `<name>.kd`
    objects, LLVM AMDGPUUsage "Kernel Descriptor") of every gfx950 code object in ``lib``."""
    import struct
    out = {}
    for elf in code_objects(lib):
        assert elf[:4] == b"\x7fELF" and elf[4] == 2 and elf[5] == 1, "code object: not a little-endian ELF64"
        shoff, = struct.unpack_from("<Q", elf, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
        secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
        symtabs = [sec for sec in secs if sec[1] == 2] or [sec for sec in secs if sec[1] == 11]
        for sec in symtabs:
            stroff = secs[sec[6]][4]
            for i in range(sec[5] // 24):
                name_i, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, sec[4] + 24 * i)
                name = elf[stroff + name_i:elf.index(b"\0", stroff + name_i)].decode()
                if not name.endswith(".kd") or size != 64 or not 0 < shndx < shnum:
                    continue
                kd = elf[secs[shndx][4] + value - secs[shndx][3]:][:64]
                lds, scratch = struct.unpack_from("<II", kd, 0)
                rsrc1, = struct.unpack_from("<I", kd, 48)
                preload, = struct.unpack_from("<H", kd, 58)          # KERNARG_PRELOAD_SPEC_LENGTH: bits 470:464
                out[name[:-3]] = {"preload": preload & 0x7F, "lds": lds, "scratch": scratch, "vgprs": ((rsrc1 & 0x3F) + 1) * 8}
    return out


def check_preload(lib, verbose=True):
    """State the preload length the compiler gave each of the frame pair's kernels in ``lib``; raise if one got none, or
    if a hot form's static LDS, scratch or register allocation left the budget of its workgroups per CU."""
    kds = kernel_descriptors(lib)
    fam = {k: v for k, v in kds.items() if any("%d%sI" % (len(f), f) in k for f in PRELOAD_FAMILIES)}
    if not fam:
        raise RuntimeError("%s: no kernel descriptor of the frame pair's kernels found" % lib)
    lengths = sorted(set(v["preload"] for v in fam.values()))
    if verbose:
        print("%s: %d frame-pair kernel instantiations, preloaded kernel-argument dwords: %s" % (
            os.path.basename(lib), len(fam), ", ".join(str(n) for n in lengths)), flush=True)
    none = sorted(k for k, v in fam.items() if v["preload"] == 0)
    if none:
        raise RuntimeError("%s: no kernel arguments preloaded for %s" % (lib, ", ".join(none)))
    for key, lds, vgprs in HOT_FORMS:
        hits = [(k, v) for k, v in fam.items() if key in k]
        if not hits:
            raise RuntimeError("%s: hot kernel form %s not found" % (lib, key))
        for k, v in hits:
            if verbose:
                print("  %s: preload %d dwords, LDS %d B, scratch %d B, %d VGPRs allocated" % (
                    k, v["preload"], v["lds"], v["scratch"], v["vgprs"]), flush=True)
            if v["lds"] != lds or v["scratch"] != 0 or v["vgprs"] > vgprs:
                raise RuntimeError("%s: %s left its occupancy budget (LDS %d B, %d VGPRs, no scratch): %r" % (
                    lib, k, lds, vgprs, v))
    return fam


def build(force=False, verbose=True, debug=True):
    """Compile every HIP source for gfx950 and link the product library (and, with ``debug``, the measurement
    library next to it).  Returns the product library's path."""
    if force:
        for lib in (LIB, LIB_DEBUG):
            if os.path.exists(lib):
                os.remove(lib)
    if force or _stale(LIB, SOURCES):
        _build_one(LIB, SOURCES, [], os.path.join(CSRC, "obj"), verbose)
        check_preload(LIB, verbose)
    if debug and (force or _stale(LIB_DEBUG, SOURCES + DEBUG_ONLY_SOURCES)):
        _build_one(LIB_DEBUG, SOURCES + DEBUG_ONLY_SOURCES, ["-DSMOT_DEBUG"], os.path.join(CSRC, "obj_debug"), verbose)
        check_preload(LIB_DEBUG, verbose)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, debug="--no-debug" not in sys.argv))
