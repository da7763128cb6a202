#!/usr/bin/env python
"""Compare the device code of two source trees of this project, kernel by kernel, without a GPU.

    python tools/kernel_isa_diff.py OLD_TREE NEW_TREE [--md profiles/x.md] [--jobs 8] [--title "..."]

For every file of each tree's ``siam-mot_amd/build.py`` SOURCES the product's device code is compiled alone
(``hipcc <build.py FLAGS> --cuda-device-only -c``), the gfx950 code object is taken out of the bundle
(``clang-offload-bundler --unbundle``) and, for every function symbol of it, three things are compared between the trees:
the function's bytes, its kernel descriptor (the ``<name>.kd`` object) and its entry in the code object's metadata note
(``llvm-readelf --notes``: register counts, LDS, kernarg and scratch sizes, argument layout).  Of the descriptor every
field but one is compared: bytes 16..23 hold the distance from the descriptor to the kernel's first instruction, which
changes with the ORDER in which a file's kernels are emitted and says nothing about a kernel.  It is a plain diff of two
builds.  A refactoring of host code must come out as "identical" for every kernel both trees have; kernels only one tree has
are listed by name.  Exit status 1 when a kernel both trees have differs.
"""
import argparse
import importlib.util
import os
import shutil
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _build_module(tree):
    spec = importlib.util.spec_from_file_location("smot_build_%d" % abs(hash(tree)), os.path.join(tree, "siam-mot_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _llvm_tool(hipcc, name):
    cands = [shutil.which(name)]
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    cands += [os.path.join(root, "llvm", "bin", name), os.path.join(root, "lib", "llvm", "bin", name)]
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise RuntimeError("%s not found beside %s" % (name, hipcc))


def _elf_symbols(path):
    """{name: (type, bytes)} of the FUNC and OBJECT symbols of an ELF64 little-endian file."""
    data = open(path, "rb").read()
    assert data[:6] == b"\x7fELF\x02\x01", path
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for sec in secs:
        if sec[1] != 2:                      # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for k in range(sec[5] // sec[9]):
            name_off, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", data, sec[4] + k * sec[9])
            typ = info & 15
            if typ not in (1, 2) or shndx == 0 or shndx >= shnum or size == 0:
                continue
            name = data[stroff + name_off:data.index(b"\0", stroff + name_off)].decode()
            s = secs[shndx]
            off = s[4] + (value - s[3])
            out[name] = (typ, data[off:off + size])
    return out


def _metadata(readelf, path):
    """{kernel symbol: the text of its entry in the amdhsa.kernels list of the metadata note}."""
    text = subprocess.check_output([readelf, "--notes", path]).decode()
    out, cur, inside = {}, None, False
    for line in text.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if inside and line and not line.startswith(" "):
            inside = False
        if not inside:
            continue
        if line.startswith("  - "):
            cur = []
            out[len(out)] = cur
        if cur is not None:
            cur.append(line)
    named = {}
    for lines in out.values():
        sym = [l.split(":", 1)[1].strip() for l in lines if l.strip().lstrip("- ").startswith(".symbol:")]
        named[sym[0][:-3] if sym and sym[0].endswith(".kd") else (sym[0] if sym else "?")] = "\n".join(lines)
    return named


def device_code(tree, source, workdir):
    """{function: dict(code=bytes, kd=bytes or None, meta=text or None)} of one product source of a tree."""
    b = _build_module(tree)
    hipcc = b._hipcc()
    bundler, readelf = _llvm_tool(hipcc, "clang-offload-bundler"), _llvm_tool(hipcc, "llvm-readelf")
    obj = os.path.join(workdir, source + ".bundle")
    co = os.path.join(workdir, source + ".co")
    subprocess.check_call([hipcc] + b.FLAGS + ["-I", b.CSRC, "--cuda-device-only", "-c", b._src(source), "-o", obj],
                          stderr=subprocess.DEVNULL)
    subprocess.check_call([bundler, "--type=o", "--targets=" + TARGET, "--input=" + obj, "--output=" + co, "--unbundle"])
    syms, meta = _elf_symbols(co), _metadata(readelf, co)
    funcs = {}
    for name, (typ, code) in syms.items():
        if typ == 2:
            kd = syms.get(name + ".kd")
            # (kernel_code_entry_byte_offset, bytes 16..23: where the code lies relative to the descriptor)
            funcs[name] = dict(code=code, kd=kd[1][:16] + kd[1][24:] if kd else None, meta=meta.get(name))
    return funcs


def compare(old_tree, new_tree, jobs):
    bo, bn = _build_module(old_tree), _build_module(new_tree)
    cxxfilt = shutil.which("c++filt") or _llvm_tool(bn._hipcc(), "llvm-cxxfilt")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        work = []
        for tag, tree, b in (("old", old_tree, bo), ("new", new_tree, bn)):
            os.makedirs(os.path.join(tmp, tag))
            work += [(tag, tree, s) for s in b.SOURCES]
        with ThreadPoolExecutor(max_workers=jobs) as ex:
            res = list(ex.map(lambda w: device_code(w[1], w[2], os.path.join(tmp, w[0])), work))
    code = {(w[0], w[2]): r for w, r in zip(work, res)}
    for s in sorted(set(bo.SOURCES) | set(bn.SOURCES), key=lambda s: (bn.SOURCES + bo.SOURCES).index(s)):
        o, n = code.get(("old", s), {}), code.get(("new", s), {})
        row = dict(source=s, old=o, new=n, removed=sorted(set(o) - set(n)), added=sorted(set(n) - set(o)), differ=[])
        for name in sorted(set(o) & set(n)):
            what = [k for k in ("code", "kd", "meta") if o[name][k] != n[name][k]]
            if what:
                row["differ"].append((name, what))
        rows.append(row)
    names = sorted({x for r in rows for x in r["removed"] + r["added"]} | {x for r in rows for x, _ in r["differ"]})
    pretty = dict(zip(names, subprocess.check_output([cxxfilt] + names).decode().splitlines())) if names else {}
    return rows, pretty


def _kernels(funcs):
    return {k: v for k, v in funcs.items() if v["kd"] is not None}


def to_markdown(rows, pretty, title):
    out = ["# %s" % title, "",
           "Device-only compile of every product source at both trees (`build.py` FLAGS, gfx950); per function symbol the "
           "bytes, the kernel descriptor and the metadata entry are compared (`tools/kernel_isa_diff.py`).", "",
           "| source | kernels old | kernels new | code bytes old | code bytes new | removed | added | differing | others |",
           "|---|---|---|---|---|---|---|---|---|"]
    tot = [0, 0, 0, 0]
    for r in rows:
        ko, kn = _kernels(r["old"]), _kernels(r["new"])
        bo, bn = sum(len(v["code"]) for v in r["old"].values()), sum(len(v["code"]) for v in r["new"].values())
        tot = [tot[0] + len(ko), tot[1] + len(kn), tot[2] + bo, tot[3] + bn]
        same = len(set(r["old"]) & set(r["new"])) - len(r["differ"])
        out.append("| `%s` | %d | %d | %d | %d | %d | %d | %d | %d identical |" % (
            r["source"], len(ko), len(kn), bo, bn, len(r["removed"]), len(r["added"]), len(r["differ"]), same))
    out.append("| **all** | %d | %d | %d | %d | | | | |" % tuple(tot))
    for key, head in (("removed", "Only in the old tree"), ("added", "Only in the new tree")):
        items = [(r["source"], x, r["old" if key == "removed" else "new"][x]) for r in rows for x in r[key]]
        out += ["", "## %s" % head, ""]
        out += ["- `%s`: `%s` (%d bytes)" % (s, pretty.get(x, x), len(v["code"])) for s, x, v in items] or ["none"]
    out += ["", "## In both trees and different", ""]
    out += ["- `%s`: `%s` (%s)" % (r["source"], pretty.get(x, x), ", ".join(w)) for r in rows for x, w in r["differ"]] or [
        "none: every function both trees have is identical in code, kernel descriptor and metadata"]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--md")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--title", default="Device code of two trees, kernel by kernel")
    a = ap.parse_args()
    rows, pretty = compare(os.path.abspath(a.old_tree), os.path.abspath(a.new_tree), a.jobs)
    md = to_markdown(rows, pretty, a.title)
    if a.md:
        open(a.md, "w").write(md)
    print(md)
    sys.exit(1 if any(r["differ"] for r in rows) else 0)
