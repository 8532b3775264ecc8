#!/usr/bin/env python3
"""Are the kernels of one tree still the kernels of another?  CPU only (hipcc cross-compiles to gfx950 without a GPU).

    python tools/kernel_isa_diff.py OLD_TREE NEW_TREE [gemm.hip gemm256.hip ...] [--work DIR] [--reuse-old]

For every named file of ppt_amd/csrc (default: gemm.hip gemm256.hip) the file is compiled in both trees to gfx950 assembly with
that tree's ppt_amd/build.py flags for the file plus `--cuda-device-only -S`, the assembly is cut into kernels (from the symbol's
label up to and including its `.amdhsa_kernel ... .end_amdhsa_kernel` descriptor: instructions, register counts, LDS bytes, scratch
size), and each kernel is normalised: comments, `.size` / `.type` / `.p2align` / `.globl` lines and the kernel's own symbol name
dropped, `.LBB<n>_<m>` rewritten to `.LBB_<m>` (the function index <n> shifts when kernels come or go).  Kernels are then paired by
the hash of the normalised text -- template parameter lists change in a refactor, bodies must not -- and every kernel of the new tree
is reported as "identical to <old kernel>" or with the first differing lines against the old kernel of the closest name.

The tool compares text and hashes.  It looks at no instruction and judges none.  Exit status 0: every new kernel has an identical
old one.  Compiling takes minutes per file, which is why this is a tool and not a test.
"""
import argparse
import concurrent.futures
import difflib
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

DROP = re.compile(r"^\s*\.(size|type|p2align|globl)\b")
LBB = re.compile(r"\.LBB\d+_(\d+)")


def build_flags(tree, name):
    """(hipcc, flags) ppt_amd/build.py of `tree` uses for csrc/`name`"""
    spec = importlib.util.spec_from_file_location("_ppt_build_" + hashlib.md5(tree.encode()).hexdigest(),
                                                  os.path.join(tree, "ppt_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, mod.COMMON + mod.PER_FILE.get(name, [])


def compile_asm(tree, name, out):
    hipcc, flags = build_flags(tree, name)
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(tree, "ppt_amd", "csrc", name), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    return out


def kernels(path):
    """{symbol: normalised text} of every kernel (every symbol with an .amdhsa_kernel descriptor) of an assembly file"""
    with open(path) as fh:
        lines = fh.read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    label = {n + ":": n for n in names}
    out, cur, body = {}, None, []
    for ln in lines:
        head = ln.split(";", 1)[0].strip()
        if cur is None:
            if head in label:
                cur, body = label[head], []
            continue
        code = ln.split(";", 1)[0].rstrip()                # (comment lines and trailing comments)
        if code.strip() and not DROP.match(code):
            # the kernel's own name, also where it is part of another symbol (its static LDS array: _ZZ<name without _Z>E4smem)
            code = code.replace(cur, "<kernel>").replace(cur[2:], "<kernel>")
            body.append(LBB.sub(r".LBB_\1", code))
        if head == ".end_amdhsa_kernel":
            out[cur] = "\n".join(body)
            cur = None
    missing = [n for n in names if n not in out]
    if missing:
        raise RuntimeError("%s: no body found for %s" % (path, ", ".join(missing)))
    return out


def demangle(names):
    tool = next((t for t in ("llvm-cxxfilt", "c++filt", "/opt/rocm/llvm/bin/llvm-cxxfilt") if shutil.which(t)), None)
    if not tool or not names:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True)
    plain = r.stdout.split("\n")[:len(names)] if r.returncode == 0 else names
    return {n: (d.replace("(anonymous namespace)::", "") or n) for n, d in zip(names, plain)}


def compare(name, old_s, new_s, context):
    old, new = kernels(old_s), kernels(new_s)
    dm = demangle(sorted(set(old) | set(new)))
    digest = lambda text: hashlib.sha256(text.encode()).hexdigest()
    by_hash = {}
    for sym, text in old.items():
        by_hash.setdefault(digest(text), []).append(sym)
    print("== %s: %d kernels in the old tree, %d in the new" % (name, len(old), len(new)))
    differing, partners = 0, set()
    # the old symbol whose demangled name is closest (two symbols may demangle alike: the mangled name settles it)
    by_name = lambda name, syms: max(sorted(syms), key=lambda s: difflib.SequenceMatcher(None, name, dm[s]).ratio())
    for sym in sorted(new, key=lambda s: dm[s]):
        h = digest(new[sym])
        same = by_hash.get(h)
        if same:
            osym = by_name(dm[sym], same)
            partners.add(osym)
            print("  %s  %s\n      identical to  %s" % (h[:12], dm[sym], dm[osym]))
            continue
        differing += 1
        osym = by_name(dm[sym], old) if old else None
        print("  %s  %s\n      DIFFERS; closest old name  %s" % (h[:12], dm[sym], dm[osym] if osym else None))
        if osym:
            diff = difflib.unified_diff(old[osym].split("\n"), new[sym].split("\n"), "old", "new", n=1, lineterm="")
            for i, ln in enumerate(diff):
                if i >= context:
                    print("        ...")
                    break
                print("        " + ln)
    gone = sorted(dm[s] for s in old if s not in partners)
    if gone:
        print("  -- %d old kernels without a partner in the new tree:" % len(gone))
        for g in gone:
            print("      " + g)
    return differing


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("files", nargs="*", default=["gemm.hip", "gemm256.hip"])
    ap.add_argument("--work", help="directory for the assembly files (default: a temporary one)")
    ap.add_argument("--reuse-old", action="store_true", help="do not recompile old-tree assembly already present in --work")
    ap.add_argument("--lines", type=int, default=24, help="diff lines shown per differing kernel")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="kernel_isa_diff_")
    os.makedirs(work, exist_ok=True)
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        for f in a.files:
            for side, tree in (("old", a.old_tree), ("new", a.new_tree)):
                out = os.path.join(work, "%s.%s.s" % (f[:-4] if f.endswith(".hip") else f, side))
                if side == "old" and a.reuse_old and os.path.exists(out):
                    continue
                jobs[out] = ex.submit(compile_asm, os.path.abspath(tree), f, out)
        for j in jobs.values():
            j.result()
    differing = 0
    for f in a.files:
        stem = os.path.join(work, f[:-4] if f.endswith(".hip") else f)
        differing += compare(f, stem + ".old.s", stem + ".new.s", a.lines)
    print("== %s" % ("every kernel of the new tree is identical to a kernel of the old tree" if not differing
                     else "%d kernels of the new tree DIFFER from every kernel of the old tree" % differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
