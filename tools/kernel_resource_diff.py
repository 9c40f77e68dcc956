"""Compare the compiler's resource figures of every kernel of librspt.so between two source trees, without a GPU: each tree's own rs_pbrt_amd/csrc/Makefile
writes the -Rpass-analysis=kernel-resource-usage remarks of every unit, compiled for the device only with that unit's flags (`make unit-remarks`), the remarks
are read per mangled kernel name, and the two sets are compared.  Prints the file kept as profiles/*_kernel_resource_usage.txt: the kernels whose figures
changed or that went away, the new kernels, and every kernel of both builds.  Exit status 1 if a kernel of the first tree changed or went away.
Both trees need a Makefile with the unit-remarks target: a tree from before the one-unit-source build (57 tu_*.hip files) cannot be read.
usage: python tools/kernel_resource_diff.py PARENT_TREE THIS_TREE [-j N]      (a tree = a checkout's root; `git worktree add` makes the parent's)
The remarks are kept under each tree's build/obj/*.ru and made again only when a source changed."""
import argparse
import glob
import os
import re
import subprocess
import sys

KEYS = (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
        ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"))


def figures(tree, jobs):
    objdir = os.path.join(os.path.abspath(tree), "build", "obj")
    r = subprocess.run(["make", "-s", "-j%d" % jobs, "-C", os.path.join(tree, "rs_pbrt_amd", "csrc"), "OBJDIR=" + objdir, "unit-remarks"], stderr=subprocess.PIPE, text=True, errors="replace")
    if r.returncode != 0:
        sys.exit("make unit-remarks failed in %s:\n%s" % (tree, r.stderr[-2000:]))
    out = {}
    for ru in sorted(glob.glob(os.path.join(objdir, "*.ru"))):
        cur = None
        for line in open(ru, errors="replace"):
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
