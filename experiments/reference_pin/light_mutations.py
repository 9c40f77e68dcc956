#!/usr/bin/env python3
"""What tests/golden/light_functions.npz can see (sixth batch): one-token mutations of tests/maplight_restated.cpp, each compiled into a temporary
directory and run against the committed fixture by the very comparison of tests/test_reference_light_functions.py.  Prints, per mutation, the number of differing map,
sample_li and power cases and of differing table arrays.  Needs no reference tree and no GPU.  usage: python experiments/reference_pin/light_mutations.py"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from oracle import pyoracle  # noqa: E402
import tests.test_reference_light_functions as T  # noqa: E402

SRC = open(os.path.join(ROOT, "tests", "maplight_restated.cpp")).read()
PHI = "const Float phi = spherical_phi(wp);               // :237"
MUT = [
    ("hither `<` -> `<=`", "if (wl.z < lt.p[16]) return", "if (wl.z <= lt.p[16]) return"),
    ("`>=` -> `>` at the edge p_min.x", "p.x >= x0 &&", "p.x > x0 &&"),
    ("`<=` -> `<` at the edge p_max.y", "p.y <= y1))", "p.y < y1))"),
    ("the wp == 1 arm dropped", "if (wp == 1.0f) return V3{xp, yp, zp};   // :503-508", ""),
    ("`inv * xp` -> `xp / wp`", "return V3{inv * xp, inv * yp, inv * zp};", "return V3{xp / wp, yp / wp, zp / wp};"),
    ("the offset guard removed (y)", "if (y1 > y0) st.y /= y1 - y0;", "st.y /= y1 - y0;"),
    ("y / z swap omitted", "std::swap(wp.y, wp.z);                             // :235", ""),
    ("`phi < 0` -> `phi <= 0`", PHI, "Float phi = std::atan2(wp.y, wp.x); phi = phi <= 0.0f ? phi + 2.0f * PI : phi;"),
    ("INV_2_PI <-> INV_PI", "P2{phi * INV_2_PI, theta * INV_PI}", "P2{phi * INV_PI, theta * INV_2_PI}"),
    ("lookup width 0.5 -> 0 in power", "P2{0.5f, 0.5f}, 0.5f);", "P2{0.5f, 0.5f}, 0.0f);"),
    ("4 pi -> 2 pi", "return m * S3(lt.L) * 4.0f * PI;", "return m * S3(lt.L) * 2.0f * PI;"),
    ("(1 - cos_total_width) dropped", "* 2.0f * PI * (1.0f - lt.p[17]);", "* 2.0f * PI;"),
    ("`/ d2` -> `* (1 / d2)`", "m / distance_squared(pl, iref.p);", "m * (1.0f / distance_squared(pl, iref.p));"),
    ("a dropped `+ 0` term of transform_point (m[0][3])", "m[0][0] * x + m[0][1] * y + m[0][2] * z + m[0][3];", "m[0][0] * x + m[0][1] * y + m[0][2] * z;"),
]
g = dict(np.load(T.FIXTURE))
pyoracle.build()
for name, a, b in [("unmutated", "", "")] + MUT:
    assert a in SRC and (not a or SRC.count(a) == 1), name
    td = tempfile.mkdtemp()
    cpp = os.path.join(td, "m.cpp")
    open(cpp, "w").write(SRC.replace(a, b) if a else SRC)
    so = os.path.join(td, "m.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", ROOT + "/oracle", "-I", ROOT + "/include", "-I", ROOT + "/tests", "-o", so, cpp])
    L = C.CDLL(so)
    L.ml_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.ml_map.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.ml_sample_li.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.ml_light_distribution.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ml_map_n.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.ml_sample_li_n.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    # count differing cases per function
    n = len(g["lights"])
    sc = T.lights_scene(pyoracle.bvh_build, g, range(n))
    nm = ns = 0
    for r in range(n):
        sel = g["map_rec"] == r
        if sel.any():
            nm += int((~T.same_bits(T.restated_map(L, sc, r, g["map_w"][sel]), g["map_out"][sel]).all(axis=1)).sum())
        sel = g["sli_rec"] == r
        if sel.any():
            ns += int((~T.same_bits(T.restated_sample_li(L, sc, r, g["sli_p"][sel]), g["sli_out"][sel]).all(axis=1)).sum())
    f, c, _, _ = T.restated_distribution(L, sc, T.abi.LIGHTS_POWER, (0, 0, 0))
    npw = int((~T.same_bits(f, g["power_y"])).sum())
    bad = T.hold_restatement(L, pyoracle.bvh_build, g)
    ntab = sum(1 for m in bad if m.startswith("ml_light_distribution"))
    print("%-62s | map %5d of %d | sample_li %4d of %d | power %2d of %d | table arrays %2d of 12 | %s" % (name, nm, len(g["map_w"]), ns, len(g["sli_p"]), npw, n, ntab, "CAUGHT" if bad else "not caught"), flush=True)
