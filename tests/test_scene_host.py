"""CPU: the host side of rspt_scene_create — scene_validate.h, scene_materials.h and scene_records.h — as a stand-alone program
(tests/scene_host_main.hip) built with the library's arithmetic flags plus AddressSanitizer and UBSan on the host side.  It makes no HIP
runtime call, so every refusal that keeps a bad scene off the GPU, and every record builder, runs here without one.
Not reached from here: the refusals that stay in librspt.hip — allocation and HIP errors, rspt_init missing, and "moving object instances together
with alpha-masked meshes in a scene whose records outgrow the four-box kernel", which takes more than 2^25 records."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs_pbrt_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# csrc/Makefile's FLAGS (what decides the arithmetic), without -fPIC
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result"]
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_host") / "scene_host")
    subprocess.check_call([HIPCC] + FLAGS + SANITIZE + ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "scene_host_main.hip"),
                                                        os.path.join(CSRC, "bvh_build.cpp")])
    # (the leak check needs ptrace, which not every container grants; addresses and undefined behaviour are what the records can get wrong)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    out, err = r.stdout.decode(), r.stderr.decode()
    print(out)
    assert r.returncode == 0, "scene_host failed (%d):\n%s\n%s" % (r.returncode, out[-2000:], err[-4000:])
    assert "runtime error" not in err and "AddressSanitizer" not in err and "LeakSanitizer" not in err, err[-4000:]
    return out


def test_every_case_passes(program_output):
    lines = program_output.splitlines()
    assert not [l for l in lines if l.startswith("FAIL")]
    n = int(re.fullmatch(r"(\d+) cases passed", lines[-1]).group(1))
    assert n == len([l for l in lines if l.startswith("ok ")]) and n > 150


def test_refusal_table_covers_every_text_of_the_headers(program_output):
    """every refusal text of scene_validate.h and of the slot step appears, as a pattern, among the refusals the program provoked"""
    seen = [l.split(") ", 1)[1] for l in program_output.splitlines() if l.startswith("ok refuses (")]
    src = open(os.path.join(CSRC, "scene_validate.h")).read() + open(os.path.join(CSRC, "scene_materials.h")).read()
    formats = re.findall(r'refuse\(\s*[^,]+,\s*"((?:[^"\\]|\\.)*)"', src)
    assert len(formats) >= 80   # (the pattern still finds the call sites: 85 when this was written)
    bvh_texts = ["BVH is not a tree", "BVH deeper than the 64-entry traversal stack", ": leaf range out of bounds", ": bad children"]   # assembled in bvh_tree_depth
    missing = []
    for f in formats:
        if f == "%s":
            continue
        pat = re.escape(f)
        for spec in ("%llu", "%u", "%d", "%s"):
            pat = pat.replace(re.escape(spec), ".*")
        if not any(re.fullmatch(pat, s) for s in seen):
            missing.append(f)
    missing += [t for t in bvh_texts if not any(t in s for s in seen)]
    assert not missing, missing


def test_records_past_the_prefix_were_built(program_output):
    m = re.search(r"ok records of (\d+) random triangles \(the smallest count past 512 records\): (\d+) four-box records", program_output)
    assert m and int(m.group(2)) > 512
