"""Sphere, disk and cylinder intersection held to the REFERENCE'S OWN TEXT (the route of tests/test_reference_geom_functions.py, fourth batch).

oracle/make_shape_fixtures.py compiles — syntax rewritten by committed rules, no hand-edited body — Sphere::intersect / intersect_p (shapes/sphere.rs:103-351),
Disk::intersect / intersect_p (shapes/disk.rs:92-197), Cylinder::intersect / intersect_p (shapes/cylinder.rs:95-321) over EFloat and quadratic_efloat
(core/efloat.rs), transform_ray_with_error / transform_vector_with_error, SurfaceInteraction::new and transform_surface_interaction from the Rust text where it
lies; tests/golden/shape_functions.npz holds at least 2^11 seeded cases per shape, in the element layout of rspt_quadric_intersect, with that code's outputs.

The hand restatement tests/quadric_restated.cpp (quad_hook) must give the same BITS in all 64 output words, for all three shapes.  Its sphere is
tests/sphere_restated.cpp's sphere_intersect, which it includes; tests/sphere_render_restated.cpp and tests/quadric_render_restated.cpp carry no intersection of
their own either — they include that same file and call that same function — so holding quad_hook holds every copy there is.  Where /root/reference exists the
fixture is regenerated and compared, and 2^17 fresh cases per shape run through the text and the restatement side by side."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_quadric_host import SHAPES, build_quadric_restated

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HAVE_REF = os.path.exists("/root/reference/src/shapes/sphere.rs")
FIXTURE = os.path.join(HERE, "golden", "shape_functions.npz")
SHAPE_NAMES = ("sphere", "disk", "cylinder")
OUT_COLS = np.r_[0:40, 43]      # the output words in use; the fixture stores these, the others are zero
_V3 = lambda name: [name + "." + a for a in "xyz"]      # noqa: E731
COLUMNS = (["intersect", "t"] + _V3("p") + _V3("p_error") + _V3("n") + ["uv.x", "uv.y"] + _V3("dpdu") + _V3("dpdv") + _V3("dndu") + _V3("dndv") + _V3("shading.n") + _V3("shading.dpdu")
           + _V3("shading.dpdv") + _V3("shading.dndu") + _V3("shading.dndv") + ["unused[%d]" % k for k in (40, 41, 42)] + ["intersect_p"] + ["unused[%d]" % k for k in range(44, 64)])
assert len(COLUMNS) == 64 and COLUMNS[43] == "intersect_p" and COLUMNS[25] == "shading.n.x" and COLUMNS[39] == "shading.dndv.z"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))      # (a NaN has many encodings)


def describe(got, want):
    """None when all 64 words of every case are the same bits; else the first differing column by its meaning and the number of differing cases"""
    ok = same_bits(got, want)
    if ok.all():
        return None
    col = int(np.nonzero(~ok.all(axis=0))[0][0])
    row = int(np.nonzero(~ok[:, col])[0][0])
    return "%d of %d cases differ; first differing column: %s (case %d: %r against the text's %r)" % (int((~ok.all(axis=1)).sum()), len(got), COLUMNS[col], row, got[row, col], want[row, col])


def fixture_elements(g, shape):
    """the fixture's cases of one shape as (n, 64) inputs and (n, 64) expected outputs of rspt_quadric_intersect"""
    rec, idx, ray = g[shape + "_rec"], g[shape + "_idx"], g[shape + "_ray"]
    x = np.zeros((len(idx), 64), np.float32)
    x[:, :rec.shape[1]] = rec[idx]
    x[:, rec.shape[1]:rec.shape[1] + 7] = ray
    want = np.zeros_like(x)
    want[:, OUT_COLS] = g[shape + "_out"]
    return x, want


def restated(L, shape, x):
    out = np.zeros_like(x)
    assert L.quad_hook(SHAPES[shape], x.ctypes.data, len(x), out.ctypes.data) == 0
    return out


def generator():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import make_shape_fixtures
    return make_shape_fixtures


@pytest.fixture(scope="module")
def ref():
    return build_quadric_restated()


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_restatement_equals_the_references_text_on_the_committed_fixture(ref, shape):
    g = np.load(FIXTURE)
    x, want = fixture_elements(g, shape)
    n, hits = len(x), int(want[:, 0].sum())
    assert n >= 1 << 11 and hits * 4 >= n and (n - hits) * 4 >= n, (shape, n, hits)
    assert np.array_equal(want[:, 0], want[:, 43])                                     # intersect and intersect_p agree by the text
    cat = g[shape + "_cat"]
    assert all((cat == c).sum() * 20 >= n for c in np.unique(cat)) and len(np.unique(cat)) >= 8      # every category holds at least 5 % of the cases
    msg = describe(restated(ref, shape, x), want)
    assert msg is None, "%s: tests/quadric_restated.cpp differs from the reference's text: %s" % (shape, msg)


def test_describe_names_a_column_by_its_meaning():
    a = np.zeros((3, 64), np.float32)
    b = a.copy()
    b[1, 6] = 1.0
    b[2, 19] = np.nan
    assert describe(a, a) is None and describe(np.full((1, 64), np.nan, np.float32), np.full((1, 64), -np.nan, np.float32)) is None
    assert "2 of 3 cases differ; first differing column: p_error.y (case 1:" in describe(a, b)
    b[1, 6] = 0.0
    assert "1 of 3 cases differ; first differing column: dndu.x (case 2:" in describe(a, b)


@pytest.mark.skipif(not HAVE_REF, reason="the reference tree is not on this machine: the committed fixture is what travels")
def test_committed_fixture_is_what_the_references_text_gives():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "make_shape_fixtures.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(l[len("compiled from "):].rsplit(" ", 1) for l in r.stdout.splitlines() if l.startswith("compiled from "))
    assert lines["Sphere::intersect"] == "shapes/sphere.rs:103-268" and lines["Sphere::intersect_p"] == "shapes/sphere.rs:269-351"
    assert lines["Disk::intersect"] == "shapes/disk.rs:92-162" and lines["Disk::intersect_p"] == "shapes/disk.rs:163-197"
    assert lines["Cylinder::intersect"] == "shapes/cylinder.rs:95-245" and lines["Cylinder::intersect_p"] == "shapes/cylinder.rs:246-321"
    assert lines["quadratic_efloat"] == "core/efloat.rs:16-37" and lines["efloat_div"] == "core/efloat.rs:125-148" and lines["EFloat::new_"] == "core/efloat.rs:49-59"
    assert lines["transform_ray_with_error"] == "core/transform.rs:793-814" and lines["transform_vector_with_error"] == "core/transform.rs:770-792"
    assert lines["surface_interaction_new"] == "core/interaction.rs:249-331" and lines["Transform::transform_surface_interaction"] == "core/transform.rs:815-860"


@pytest.mark.skipif(not HAVE_REF, reason="needs /root/reference to compile the reference's text")
def test_restatement_equals_the_compiled_reference_text_on_131072_fresh_cases_per_shape(ref):
    mk = generator()
    L, _ = mk.convert()
    d, stats = mk.reference(L, per_cat=(1 << 17) // 8, seed=0x5EED9)
    for shape in SHAPE_NAMES:
        x, want = fixture_elements(d, shape)
        assert len(x) >= 1 << 17 and stats[shape]["hits"] * 4 >= len(x) and stats[shape]["misses"] * 4 >= len(x)
        msg = describe(restated(ref, shape, x), want)
        assert msg is None, "%s: tests/quadric_restated.cpp differs from the reference's text: %s" % (shape, msg)
