"""profiles/fast_shade_static.txt from the resource-usage remarks and the gfx950 assembly of the shade units (tools/static_kernel_facts.sh fast): every fast-math
shade kernel (k_shade_fast*, the SHADE_F* groups of tu.hip) beside its exact twin.  usage: python tools/fast_shade_static.py WORK_DIR REPO"""
import re
import subprocess
import sys

work, repo = sys.argv[1], sys.argv[2]
KEYS = (("VGPRs", r" VGPRs: (\d+)"), ("AGPRs", r"AGPRs: (\d+)"), ("SGPRs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
        ("LDS", r"LDS Size \[bytes/block\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"))
OPS = ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_rcp_f32", "v_sqrt_f32", "v_sin_f32", "v_cos_f32", "v_log_f32", "v_exp_f32")

facts = {}
for block in open(work + "/ru.txt").read().split("Function Name: ")[1:]:
    name = block.split()[0]
    facts[name] = {k: int(re.search(p, block).group(1)) for k, p in KEYS}
asm = open(work + "/shade.s").read()
for name in facts:
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), asm, re.S | re.M)
    body = m.group(1)
    facts[name]["VALU"] = len(re.findall(r"^\s+v_\w+", body, re.M))
    facts[name]["instructions"] = len(re.findall(r"^\s+[a-z]\w+", body, re.M))
    for op in OPS:
        facts[name][op] = len(re.findall(r"^\s+%s" % op, body, re.M))
names = sorted(facts)
plain = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()))
short = {n: plain[n].split("(")[0].replace("void ", "").replace("rspt::", "") for n in names}
by_short = {short[n]: n for n in names}
cols = [k for k, _ in KEYS] + ["VALU", "instructions"] + list(OPS)
out = ["Static figures of the fast-math shade kernels beside their exact twins: the compiler's resource remarks and the gfx950 assembly of the shade units, no GPU",
       "(tools/static_kernel_facts.sh fast).  VALU / instructions / the per-opcode counts are static counts over the kernel's own body; the exact kernels also",
       "call the out-of-line restatements of logf / expf / acosf / atan2f (glibc_libm.h GL_FN_COLD), which are not counted under the kernel, the fast kernels call nothing.",
       "The generic set's fast kernels (<4282384383u>) are built with RSPT_FAST_MATH but keep the correctly rounded division and square root (DESIGN section 5.3a).",
       "The template argument is the feature set's bit mask (tu_decl.h SV_*); _w / _mw: the build for W waves per SIMD; _m / _mw: the MOVE forms.", "",
       "columns: " + "  ".join(cols), ""]
n_pairs = ieee = n_kept = 0
for s in sorted(by_short):
    if "k_shade_fast" not in s:
        continue
    twin = s.replace("k_shade_fast", "k_shade")
    f, e = facts[by_short[s]], facts[by_short[twin]]
    n_pairs += 1
    if "<4282384383u" in s:   # SV_GENERIC: built with the macro but without the division flags (csrc/Makefile FAST_DIV_TUS)
        n_kept += 1
    else:
        ieee += f["v_div_scale_f32"] + f["v_div_fmas_f32"] + f["v_div_fixup_f32"]
    out += [s, "    fast   " + "  ".join("%5d" % f[c] for c in cols), "    exact  " + "  ".join("%5d" % e[c] for c in cols), ""]
out += ["%d fast kernels; %d of them, the generic set's (<4282384383u>), keep the correctly rounded division on purpose; v_div_scale_f32 + v_div_fmas_f32 + v_div_fixup_f32 over the other %d: %d"
        % (n_pairs, n_kept, n_pairs - n_kept, ieee)]
open(repo + "/profiles/fast_shade_static.txt", "w").write("\n".join(out) + "\n")
print("\n".join(out))
