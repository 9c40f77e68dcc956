"""Compare the compiler's resource figures of every kernel of librspt.so between two source trees, without a GPU: each tree's rs_pbrt_amd/csrc/*.hip
is compiled for the device only with -Rpass-analysis=kernel-resource-usage (the Makefile's flags), the remarks are read per mangled kernel name, and the two
sets are compared.  Prints the file kept as profiles/*_kernel_resource_usage.txt: the kernels whose figures changed or that went away, the new kernels,
and every kernel of both builds.  Exit status 1 if a kernel of the first tree changed or went away.
usage: python tools/kernel_resource_diff.py PARENT_TREE THIS_TREE [-j N]      (a tree = a checkout's root; `git worktree add` makes the parent's)"""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fPIC",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null"]
KEYS = (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
        ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"))


FAST_FLAGS = ["-fno-hip-fp32-correctly-rounded-divide-sqrt", "-Xarch_device", "-fapprox-func"]   # csrc/Makefile FAST_FLAGS: the fast-math shade units, tu_shade_f*.hip


def remarks(tu):
    name = os.path.basename(tu)
    fast = FAST_FLAGS if name.startswith("tu_shade_f") and name not in ("tu_shade_fc.hip", "tu_shade_fmc.hip") else []   # (the generic set keeps exact division)
    r = subprocess.run([HIPCC] + FLAGS + fast + [os.path.basename(tu)], cwd=os.path.dirname(tu), stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, errors="replace")
    if r.returncode != 0:
        sys.exit("%s failed on %s:\n%s" % (HIPCC, tu, r.stderr[-2000:]))
    return r.stderr


def figures(tree, jobs):
    tus = sorted(glob.glob(os.path.join(tree, "rs_pbrt_amd", "csrc", "*.hip")))
    out = {}
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for text in pool.map(remarks, tus):
            cur = None
            for line in text.splitlines():
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    cur = out.setdefault(m.group(1), {})
                    continue
                if cur is not None:
                    for key, pat in KEYS:
                        m = re.search(pat, line)
                        if m:
                            cur[key] = int(m.group(1))
    return out


def row(f):
    return "  ".join(str(f[k]) for k, _ in KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    before, after = figures(a.parent, a.j), figures(a.tree, a.j)
    changed = [k for k in before if k not in after or before[k] != after[k]]
    print("kernels before: %d   kernels after: %d   kernels whose figures changed or that went away: %d" % (len(before), len(after), len(changed)))
    for k in changed:
        print("  CHANGED  %s\n      %s  ->  %s" % (k, row(before[k]), row(after[k]) if k in after else "gone"))
    print("\nnew kernels:")
    for k in after:
        if k not in before:
            print("  %s\n      %s" % (k, row(after[k])))
    print("\nevery kernel of both builds, identical figures:")
    for k in sorted(before):
        if k not in changed:
            print("  %s  %s" % (row(before[k]), k))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
