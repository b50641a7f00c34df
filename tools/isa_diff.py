#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel: python tools/isa_diff.py OLD_TREE NEW_TREE [--jobs N]

Every splice_amd/csrc/*.hip of both trees is compiled to device assembly with the Makefile's flags (as tools/isa.sh does).  A kernel is
the same when its instruction stream (local label numbers normalised, comments dropped) and its .amdhsa_* descriptor block (registers, LDS, scratch,
user-SGPR / kernarg-preload counts) are equal.  Kernels are matched by symbol over the whole tree, so a kernel may move between
translation units.  Prints the kernels that differ, the ones only one tree has, and "N kernels compared, N equal"; exit status 1 if any
differ.  What a refactor that must not move device code checks after every step."""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-mllvm", "-amdgpu-kernarg-preload-count=16",
         "-Wno-unused-result", "-S", "--cuda-device-only"]


def compile_unit(tree, hip, out):
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *FLAGS, f"-I{tree}/include", "-o", out, hip]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{hip}: {r.stderr}")
    return out


def normalise(text):
    text = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", text)
    text = re.sub(r"\.L(func_(?:begin|end)|tmp|JTI|__unnamed_)\d+(_\d+)?", r".L\1", text)
    # comments go (the "; %bb.N" block marks, and loop notes whose column depends on the label's length)
    lines = (re.sub(r"\s*;.*$", "", l) for l in text.split("\n"))
    return "\n".join(l for l in lines if l)


def kernels(asm_path):
    """symbol -> (unit, body, descriptor)"""
    s = open(asm_path).read()
    unit = os.path.basename(asm_path)[:-2]
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", s, re.M | re.S):
        name = m.group(1)
        i = s.index(f"\n{name}:") + 1
        j = s.index(".Lfunc_end", i)
        out[name] = (unit, normalise(s[i:j]), m.group(2))
    return out


def tree_kernels(tree, tmp, tag, pool):
    hips = sorted(glob.glob(os.path.join(tree, "splice_amd", "csrc", "*.hip")))
    futs = [pool.submit(compile_unit, tree, h, os.path.join(tmp, tag, os.path.basename(h)[:-4] + ".s")) for h in hips]
    all_k = {}
    for f in futs:
        for name, v in kernels(f.result()).items():
            if name in all_k:
                sys.exit(f"{tree}: kernel {name} defined in {all_k[name][0]} and {v[0]}")
            all_k[name] = v
    return all_k


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        os.makedirs(os.path.join(tmp, "old")); os.makedirs(os.path.join(tmp, "new"))
        old = tree_kernels(os.path.abspath(a.old_tree), tmp, "old", pool)
        new = tree_kernels(os.path.abspath(a.new_tree), tmp, "new", pool)
    for name in sorted(set(old) - set(new)):
        print(f"only in old ({old[name][0]}): {name}")
    for name in sorted(set(new) - set(old)):
        print(f"only in new ({new[name][0]}): {name}")
    common = sorted(set(old) & set(new))
    bad = 0
    for name in common:
        what = [w for w, k in (("instructions", 1), ("descriptor", 2)) if old[name][k] != new[name][k]]
        if what:
            bad += 1
            print(f"DIFFERS ({', '.join(what)}): {name}  [{old[name][0]} -> {new[name][0]}]")
    moved = sum(1 for n in common if old[n][0] != new[n][0])
    print(f"{len(common)} kernels compared, {len(common) - bad} equal ({moved} moved to another unit)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
