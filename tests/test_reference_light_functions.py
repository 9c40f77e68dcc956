"""The projection and goniometric lights held to the REFERENCE'S OWN TEXT (the route of tests/test_reference_camera_functions.py, sixth batch).

oracle/make_light_fixtures.py compiles — syntax rewritten by committed rules, no hand-edited body — ProjectionLight::{projection, sample_li, power} with the block of
new_hdr from p_light to cos_total_width (lights/projection.rs), GonioPhotometricLight::{scale, sample_li, power} with the p_light / world_to_light lines of new_hdr
(lights/goniometric.rs) and Bounds2f::offset from the Rust text where it lies; tests/golden/light_functions.npz holds seeded inputs with that code's outputs:
  lights    every light as the text's own fields (p_light, i, world_to_light, light_projection, hither, yon, screen_bounds, cos_total_width) and its map's pyramid;
  map       projection(w) / scale(w) per light and category (CATS below): the hither plane to the ulp, wp == 1, the four inclusive edges to 2 ulps, st on 0 / 1 /
            texel centres / texel borders, the poles, the axes, the phi seam with its -0, st rounding to 1;
  sample_li the ten output words at generic points, at distances 1e-20 and 1e18 and exactly at p_light;  power per light;
  ctor      the constructor blocks over (from, to, up, fov, resolution) tuples and light_to_world matrices;
  tables    func, cdf, nvox and voxel of two small scenes under the three strategies at 256 points (tests/test_gpu_reference_lights.py holds the device to them).

The tests here read the committed file alone, except the two marked as needing the reference.  tests/maplight_restated.cpp (ml_map, ml_sample_li, ml_light_distribution)
must give the same BITS in every output word; so must the records scenes.SceneBuilder.add_projection_light / add_goniometric_light build.  Where /root/reference exists the
fixture is regenerated and compared, and 2^17 fresh cases per function run through the text and the restatement side by side."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.test_maplight_host import build_restated, restated_distribution

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HAVE_REF = os.path.exists("/root/reference/src/lights/projection.rs")
FIXTURE = os.path.join(HERE, "golden", "light_functions.npz")
F32 = np.float32
NF = 77      # the text's fields of one light as floats: p_light 0, i 3, world_to_light.m 6, .m_inv 22, light_projection.m 38, .m_inv 54, hither 70, yon 71, screen_bounds 72, cos_total_width 76
STRATEGIES = (("uniform", abi.LIGHTS_UNIFORM), ("power", abi.LIGHTS_POWER), ("spatial", abi.LIGHTS_SPATIAL))
N_SCENES = 2
SLI = ["li.r", "li.g", "li.b", "wi.x", "wi.y", "wi.z", "pdf", "light_intr.p.x", "light_intr.p.y", "light_intr.p.z"]
# the categories of the map cases; the generator asserts MIN_PER_CAT of each per light, except where EXEMPT says why the light does not admit it
CATS = {
    # projection(w): named by the text's own wl.z and p
    1: "wl.z negative", 2: "wl.z == 0", 3: "wl.z == hither - 1 ulp", 4: "wl.z == hither", 5: "wl.z == hither + 1 ulp", 6: "wl.z == 1 - 1 ulp", 7: "wl.z == 1 (the wp == 1 arm)", 8: "wl.z == 1 + 1 ulp",
    9: "p.x == p_min.x (st.x == 0)", 10: "p.x == p_max.x (st.x == 1)", 11: "p.y == p_min.y (st.y == 0)", 12: "p.y == p_max.y (st.y == 1)",
    13: "p.x within 2 ulps of p_min.x", 14: "p.x within 2 ulps of p_max.x", 15: "p.y within 2 ulps of p_min.y", 16: "p.y within 2 ulps of p_max.y",
    17: "st on a texel centre of level 0", 18: "st on a texel border of level 0", 19: "interior",
    # scale(w): named by the text's own wp (after the swap), phi, theta and st
    32: "the pole wp.z == 1", 33: "the pole wp.z == -1", 34: "within 2 ulps of a pole", 35: "on +x or -x", 36: "on +z or -z (wp.y after the swap)", 37: "within 2 ulps of an axis",
    38: "wp.y == -0 with wp.x > 0 (phi == -0)", 39: "wp.y == -0 with wp.x < 0", 40: "phi the largest below 2 pi or 2 pi itself", 41: "st.x or st.y rounds to exactly 1", 42: "interior",
}
MIN_PER_CAT = 64


def lightref_dt():
    return np.dtype([("kind", "<i4"), ("map", "<i4"), ("f", "<f4", NF)])


def record_words(kind, f):
    """p[0..21] of the rspt_light record of a light given as the text's fields.  What the record leaves out of light_projection.m must be what Transform::perspective leaves
    trivial: +0 (the sign too) and m[3][2] == 1"""
    f = np.asarray(f, F32)
    p = np.zeros(22, F32)
    p[:3] = f[0:3]
    p[3:12] = f[6:22].reshape(4, 4)[:3, :3].reshape(-1)
    if kind == abi.LIGHT_PROJECTION:
        m = f[38:54].reshape(4, 4)
        p[12:16], p[16], p[17] = f[72:76], f[70], f[76]
        p[18:22] = [m[0, 0], m[1, 1], m[2, 2], m[2, 3]]
        rest = m.copy()
        rest[0, 0] = rest[1, 1] = rest[2, 2] = rest[2, 3] = rest[3, 2] = 0
        assert m[3, 2] == 1 and not rest.view(np.uint32).any(), m
    return p


def map_image(g, k):
    """level 0 of map k as (h, w, 3), and its whole pyramid"""
    w, h, _ = (int(v) for v in g["map_shapes"][k])
    lo, hi = int(g["map_offsets"][k]), int(g["map_offsets"][k + 1])
    pyr = g["map_texels"][lo:hi]
    return pyr[:3 * w * h].reshape(h, w, 3), pyr


def add_fixture_light(sb, g, row):
    """light `row` of the fixture into a SceneBuilder: the builder's own entry point makes the record and the map, then the record's words are the fixture's"""
    kind, k, f = int(g["light_kind"][row]), int(g["light_map"][row]), g["lights"][row]
    img = None if k < 0 else map_image(g, k)[0]
    if kind == abi.LIGHT_PROJECTION:
        sb.add_projection_light((0, 0, 0), (0, 0, 1), (1, 1, 1), image=img)
    else:
        sb.add_goniometric_light(np.eye(4, dtype=F32), (1, 1, 1), image=img)
    lt = sb.delta_lights[-1]
    assert lt["kind"] == kind and (int(lt["prim"]) == 0xFFFFFFFF) == (k < 0)
    lt["p"][:] = 0
    lt["p"][:22] = record_words(kind, f)
    lt["L"] = f[3:6]
    if k >= 0:
        assert np.array_equal(sb.envmaps[int(lt["prim"])]["texels"], map_image(g, k)[1])      # the host's pyramid of that image is the fixture's


def lights_scene(builder, g, rows):
    """a floor under the listed fixture lights, in that order"""
    sb = scenes.SceneBuilder()
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], sb.add_material(scenes.matte((0.5, 0.5, 0.5))))
    for r in rows:
        add_fixture_light(sb, g, int(r))
    return sb.finish(builder)


def table_scene(builder, g, k):
    """the two scenes of the device tables: 0 a floor with two walls, 1 a room (a box seen from inside) around a smaller box; one triangle area light, the fixture's map
    lights of that scene, one point light.  Every light lies inside the world bound"""
    sb = scenes.SceneBuilder()
    grey = sb.add_material(scenes.matte((0.6, 0.6, 0.6)))
    if k == 0:
        sb.add_quad([(-4, 0, -4), (4, 0, -4), (4, 0, 4), (-4, 0, 4)], grey)
        sb.add_quad([(-4, 0, 4), (4, 0, 4), (4, 5, 4), (-4, 5, 4)], grey)
        sb.add_quad([(-4, 0, -4), (-4, 0, 4), (-4, 5, 4), (-4, 5, -4)], grey)
        sb.add_mesh(np.array([(-0.5, 4.5, -0.5), (0.5, 4.5, -0.5), (0.0, 4.5, 0.6)], F32), [[0, 1, 2]], grey, emit=(9, 9, 9))
    else:
        sb.add_box((-3, 0, -2), (3, 4, 5), grey)
        sb.add_box((-1.0, 0.0, 1.0), (0.5, 1.5, 2.5), sb.add_material(scenes.matte((0.7, 0.3, 0.2))))
        sb.add_mesh(np.array([(-0.4, 3.9, 1.0), (0.4, 3.9, 1.0), (0.0, 3.9, 1.8)], F32), [[0, 1, 2]], grey, emit=(7, 8, 9), two_sided=True)
    for r in g["tab%d_rows" % k]:
        add_fixture_light(sb, g, int(r))
    sb.add_point_light((1.5, 2.0, -1.0) if k == 0 else (2.0, 1.0, 0.0), (6, 5, 4))
    return sb.finish(builder)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))      # (a NaN has many encodings: tests/test_reference_shape_functions.py compares them so)


def describe(got, want, columns):
    """None when every word of every case is the same bits; else the first differing column by its meaning and the number of differing cases"""
    ok = same_bits(got, want)
    if ok.all():
        return None
    col = int(np.nonzero(~ok.all(axis=0))[0][0])
    row = int(np.nonzero(~ok[:, col])[0][0])
    return "%d of %d cases differ; first differing column: %s (case %d: %r against the text's %r)" % (int((~ok.all(axis=1)).sum()), len(got), columns[col], row, got[row, col], want[row, col])


def restated_lib():
    R = build_restated()
    R.ml_map_n.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    R.ml_sample_li_n.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    return R


def restated_map(R, sc, index, w):
    w = np.ascontiguousarray(w, F32).reshape(-1, 3)
    out = np.zeros((len(w), 3), F32)
    assert R.ml_map_n(C.addressof(sc.desc), index, w.ctypes.data, len(w), out.ctypes.data) == 0
    return out


def restated_sample_li(R, sc, index, p):
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    out = np.zeros((len(p), 10), F32)
    assert R.ml_sample_li_n(C.addressof(sc.desc), index, p.ctypes.data, len(p), out.ctypes.data) == 0
    return out


def restated_tables(R, sc, strategy, pts):
    """ml_light_distribution point by point: func (n, n_lights), cdf (n, n_lights + 1), nvox (3), voxel (n, 3)"""
    rows = [restated_distribution(R, sc, strategy, p) for p in pts]
    assert all(list(r[2]) == list(rows[0][2]) for r in rows)
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), rows[0][2], np.stack([r[3] for r in rows])


def hold_restatement(R, builder, d, tables=True):
    """tests/maplight_restated.cpp against the arrays of a fixture (the committed one, or a fresh one): a list of what differs, with the number of differing cases"""
    bad = []
    n = len(d["lights"])
    sc = lights_scene(builder, d, range(n))
    assert int(sc.desc.n_lights) == n
    for r in range(n):
        sel = d["map_rec"] == r
        if sel.any():
            msg = describe(restated_map(R, sc, r, d["map_w"][sel]), d["map_out"][sel], ["r", "g", "b"])
            if msg:
                bad.append("ml_map, light %d: %s" % (r, msg))
        sel = d["sli_rec"] == r
        if sel.any():
            msg = describe(restated_sample_li(R, sc, r, d["sli_p"][sel]), d["sli_out"][sel], SLI)
            if msg:
                bad.append("ml_sample_li, light %d: %s" % (r, msg))
    f, c, _, _ = restated_distribution(R, sc, abi.LIGHTS_POWER, (0, 0, 0))      # Light::power().y() of every light: the power table of the scene that holds them all
    if not same_bits(f, d["power_y"]).all():
        bad.append("map_power: %d of %d lights differ" % (int((~same_bits(f, d["power_y"])).sum()), n))
    for k in range(N_SCENES if tables else 0):
        sc = table_scene(builder, d, k)
        for name, strategy in STRATEGIES:
            key = "tab%d_%s" % (k, name)
            pts = d["tab%d_pts" % k] if strategy == abi.LIGHTS_SPATIAL else d["tab%d_pts" % k][:1]
            func, cdf, nvox, voxel = restated_tables(R, sc, strategy, pts)
            if list(nvox) != list(d[key + "_nvox"]) or not np.array_equal(voxel, d[key + "_voxel"][:len(pts)]):
                bad.append("ml_light_distribution, %s: the grid or a voxel differs" % key)
            for what, got, want in (("func", func, d[key + "_func"][:len(pts)]), ("cdf", cdf, d[key + "_cdf"][:len(pts)])):
                msg = describe(got, want, ["light %d" % j for j in range(want.shape[1])])
                if msg:
                    bad.append("ml_light_distribution, %s %s: %s" % (key, what, msg))
    return bad


# ---- the edge rooms of tests/test_gpu_reference_lights.py: one floor under (a) a projector whose image rectangle lies wholly inside the frame, (b) a goniometric light whose
# pole and seam fall on the floor.  Chosen here, on the CPU: the restatement alone (now held to the text) says that every class is in the frame ----
EDGE_LOOK = ((0.0, 6.0, -9.0), (0.0, 0.0, 0.0), (0, 1, 0))
EDGE_CLASSES = {"projector": ("lit", "beyond p_min.x", "beyond p_max.x", "beyond p_min.y", "beyond p_max.y"), "goniometric": ("phi quadrant 0", "phi quadrant 1", "phi quadrant 2", "phi quadrant 3")}


def edge_room(builder, which):
    from tests.util import light_maps, tilted
    sb = scenes.SceneBuilder()
    sb.add_quad([(-10, 0, -10), (10, 0, -10), (10, 0, 10), (-10, 0, 10)], sb.add_material(scenes.matte((0.6, 0.6, 0.6))))
    proj, gonio = light_maps()
    if which == "projector":
        sb.add_projection_light((0.25, 4.0, 0.5), (0.5, 0.0, 0.75), (300, 280, 260), fov=40.0, image=proj, up=(0.1, 0, 1))
    else:
        sb.add_goniometric_light(tilted((0.0, 3.0, 0.0), y=(0.2, -0.9, 0.3), x=(1.0, 0.1, 0.2)), (30, 32, 34), image=gonio)
    return sb.finish(builder)


def edge_rd(sampler):
    return scenes.make_render_desc(48, 36, 4, EDGE_LOOK, 60, max_depth=1, sampler=sampler)


def edge_classes(R, oracle, sc, rd, which):
    """the class of the oracle's first hit under four camera rays of every pixel (the perspective camera's own matrices; the sub-pixel positions are a fixed 2 x 2 grid, the
    renders' own samples fall into the same pixels): counts per class of EDGE_CLASSES[which], from the restatement's ml_sample_li and the record's own numbers"""
    r2c, c2w = np.array(rd.raster_to_camera[:], np.float64).reshape(4, 4), np.array(rd.camera_to_world[:], np.float64).reshape(4, 4)
    px, py, sx, sy = (v.reshape(-1) for v in np.meshgrid(np.arange(48), np.arange(36), (0.25, 0.75), (0.25, 0.75), indexing="ij"))
    pc = np.stack([px + sx, py + sy, np.zeros(len(px)), np.ones(len(px))]) 
    pc = r2c @ pc
    d = (c2w[:3, :3] @ (pc[:3] / pc[3])).T
    rays = np.zeros(len(d), abi.RAY_DT)
    rays["o"], rays["d"], rays["t_max"] = c2w[:3, 3].astype(F32), (d / np.linalg.norm(d, axis=1)[:, None]).astype(F32), np.inf
    hits = oracle.trace(sc, rays)
    ok = hits["prim"] != 0xFFFFFFFF
    p = (rays["o"].astype(np.float64) + rays["d"].astype(np.float64) * hits["t"][:, None].astype(np.float64))[ok].astype(F32)
    li = restated_sample_li(R, sc, 0, p)[:, :3]
    lt = sc.lights[0]
    wl = (lt["p"][3:12].reshape(3, 3).astype(np.float64) @ (p.astype(np.float64) - lt["p"][:3].astype(np.float64)).T).T
    if which == "projector":
        assert (wl[:, 2] > 0.1).all()      # the floor lies in front of the projector: what is dark is beyond an edge
        x, y = lt["p"][18] * wl[:, 0] / wl[:, 2], lt["p"][19] * wl[:, 1] / wl[:, 2]
        x0, y0, x1, y1 = (float(v) for v in lt["p"][12:16])
        lit = li.max(axis=1) > 0
        inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
        assert (lit == inside).mean() > 0.999      # (f64 here against f32 there: they part only within an ulp of an edge)
        return int(ok.sum()), [int(lit.sum()), int((~lit & (x < x0)).sum()), int((~lit & (x > x1)).sum()), int((~lit & (y < y0) & (x >= x0) & (x <= x1)).sum()), int((~lit & (y > y1) & (x >= x0) & (x <= x1)).sum())]
    assert (li.min(axis=1) > 0).all()
    phi = np.mod(np.arctan2(wl[:, 2], wl[:, 0]), 2 * np.pi)      # (after the swap wp.y is the light's z)
    return int(ok.sum()), [int(((phi >= q * np.pi / 2) & (phi < (q + 1) * np.pi / 2)).sum()) for q in range(4)]


@pytest.mark.parametrize("which", ["projector", "goniometric"])
def test_the_edge_rooms_hold_what_they_say(oracle, which):
    """at least 32 first hits in every class (lit and dark beyond each of the four edges; each phi quadrant, which is both sides of the seam, around a pole on the floor)"""
    sc = edge_room(oracle.bvh_build, which)
    n, counts = edge_classes(restated_lib(), oracle, sc, edge_rd("sobol"), which)
    assert n >= 48 * 36 * 4 // 2 and all(c >= 32 for c in counts), dict(zip(EDGE_CLASSES[which], counts))      # (the frame's upper rows look past the floor)
    print(which, n, dict(zip(EDGE_CLASSES[which], counts)))
    if which == "goniometric":      # the pole (the light's +y) meets the floor inside the frame's middle
        lt = sc.lights[0]
        l2w = np.linalg.inv(lt["p"][3:12].reshape(3, 3).astype(np.float64))
        pole = lt["p"][:3] + l2w[:, 1] * (-lt["p"][1] / l2w[1, 1])
        assert l2w[1, 1] < 0 and abs(pole[0]) < 3 and abs(pole[2]) < 3


def generator():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import make_light_fixtures
    return make_light_fixtures


@pytest.fixture(scope="module")
def g():
    return dict(np.load(FIXTURE))


def test_the_fixture_holds_what_it_is_there_for(g):
    """the counts the generator asserted, read back from the committed file"""
    kind = g["light_kind"]
    n_proj, n_gonio = int((kind == abi.LIGHT_PROJECTION).sum()), int((kind == abi.LIGHT_GONIOMETRIC).sum())
    assert n_proj >= 9 and n_gonio >= 6 and (g["light_map"][kind == abi.LIGHT_PROJECTION] < 0).any() and (g["light_map"][kind == abi.LIGHT_GONIOMETRIC] < 0).any()
    sbs = g["lights"][kind == abi.LIGHT_PROJECTION][:, 72:76]
    assert ((sbs[:, 0] == sbs[:, 2]) | (sbs[:, 1] == sbs[:, 3])).sum() == 1      # the one record whose screen_bounds have no extent on one axis
    levels = set(int(v) for v in g["map_shapes"][:, 2])
    assert {1, 2} <= levels and max(levels) >= 3 and (g["map_shapes"][:, 0] > g["map_shapes"][:, 1]).any() and (g["map_shapes"][:, 0] < g["map_shapes"][:, 1]).any()
    exempt = set((int(r), int(c)) for r, c in g["map_exempt"])
    for r in np.unique(g["map_rec"]):
        cats = [c for c in CATS if (c < 32) == (kind[r] == abi.LIGHT_PROJECTION)]
        for c in cats:
            n = int(((g["map_rec"] == r) & (g["map_cat"] == c)).sum())
            assert n >= MIN_PER_CAT or (int(r), c) in exempt, (int(r), CATS[c], n)
    for c in CATS:
        assert (g["map_cat"] == c).sum() >= MIN_PER_CAT, CATS[c]
    for r in np.unique(g["sli_rec"]):
        p = g["sli_p"][g["sli_rec"] == r]
        d = np.linalg.norm(p.astype(np.float64) - g["lights"][r, :3], axis=1)
        assert (d == 0).any() and (d < 1e-19).sum() >= 2 and (d > 1e17).any() and ((d > 0.1) & (d < 100)).sum() >= 16, r
    assert len(g["ctor_proj_in"]) >= 32 and len(g["ctor_gonio_in"]) >= 16
    aspect = g["ctor_proj_in"][:, 10] / g["ctor_proj_in"][:, 11]
    assert (aspect > 1).any() and (aspect < 1).any() and (aspect == 1).any()
    for k in range(N_SCENES):
        rows = g["tab%d_rows" % k]
        assert len(rows) >= 6 and {abi.LIGHT_PROJECTION, abi.LIGHT_GONIOMETRIC} == set(int(v) for v in kind[rows]) and (g["light_map"][rows] < 0).any() and (g["light_map"][rows] >= 0).any()
        assert len(g["tab%d_pts" % k]) == 256
        counts = g["tab%d_counts" % k]
        assert counts[15] == 0 and all(counts[c] >= 64 for c in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11)), counts
        for name, _ in STRATEGIES:
            assert np.isfinite(g["tab%d_%s_func" % (k, name)]).all() and np.isfinite(g["tab%d_%s_cdf" % (k, name)]).all()
    assert os.path.getsize(FIXTURE) <= 1 << 20


def test_restatement_equals_the_references_text_on_the_committed_fixture(g, oracle):
    bad = hold_restatement(restated_lib(), oracle.bvh_build, g)
    assert not bad, "tests/maplight_restated.cpp differs from the reference's text:\n" + "\n".join(bad)


def test_record_builders_equal_the_constructor_blocks(g):
    """scenes.SceneBuilder.add_projection_light / add_goniometric_light: every word of the record (p[0..21] and the two p leaves unused, prim, L) against the text of
    ProjectionLight::new_hdr / GonioPhotometricLight::new_hdr on the committed tuples"""
    bad = []
    for i, (row, want) in enumerate(zip(g["ctor_proj_in"], g["ctor_proj_out"])):
        sb = scenes.SceneBuilder()
        w, h = int(row[10]), int(row[11])
        img = np.full((h, w, 3), 0.5, F32)
        sb.add_projection_light(tuple(row[0:3]), tuple(row[3:6]), (3, 2, 1), fov=float(row[9]), image=img, up=tuple(row[6:9]))
        lt = sb.delta_lights[0]
        p = np.zeros(24, F32)
        p[:22] = record_words(abi.LIGHT_PROJECTION, want)
        if not (same_bits(lt["p"], p).all() and lt["prim"] == 0 and np.array_equal(lt["L"], np.array([3, 2, 1], F32)) and lt["kind"] == abi.LIGHT_PROJECTION):
            bad.append("add_projection_light, tuple %d: words %s differ" % (i, np.nonzero(~same_bits(lt["p"], p))[0].tolist()))
    for i, (m, want) in enumerate(zip(g["ctor_gonio_in"], g["ctor_gonio_out"])):
        sb = scenes.SceneBuilder()
        sb.add_goniometric_light(m.reshape(4, 4), (1, 2, 3))
        lt = sb.delta_lights[0]
        p = np.zeros(24, F32)
        p[:22] = record_words(abi.LIGHT_GONIOMETRIC, want)
        if not (same_bits(lt["p"], p).all() and lt["prim"] == 0xFFFFFFFF and np.array_equal(lt["L"], np.array([1, 2, 3], F32)) and lt["kind"] == abi.LIGHT_GONIOMETRIC):
            bad.append("add_goniometric_light, matrix %d: words %s differ" % (i, np.nonzero(~same_bits(lt["p"], p))[0].tolist()))
    assert not bad, "\n".join(bad)


@pytest.mark.skipif(not HAVE_REF, reason="the reference tree is not on this machine: the committed fixture is what travels")
def test_committed_fixture_is_what_the_references_text_gives():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "make_light_fixtures.py"), "--check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(l[len("compiled from "):].rsplit(" ", 1) for l in r.stdout.splitlines() if l.startswith("compiled from "))
    assert lines["ProjectionLight::projection"] == "lights/projection.rs:339-360" and lines["ProjectionLight::sample_li"] == "lights/projection.rs:362-378"
    assert lines["ProjectionLight::power"] == "lights/projection.rs:379-398" and lines["GonioPhotometricLight::scale"] == "lights/goniometric.rs:233-247"
    assert lines["GonioPhotometricLight::sample_li"] == "lights/goniometric.rs:249-265" and lines["GonioPhotometricLight::power"] == "lights/goniometric.rs:266-280"
    assert lines["Bounds2f::offset"] == "core/geometry.rs:1891-1900"
    assert lines["ProjectionLight::new_hdr (p_light .. cos_total_width, world_to_light)"] == "lights/projection.rs:265-301,315"
    assert lines["GonioPhotometricLight::new_hdr (p_light, world_to_light)"] == "lights/goniometric.rs:205-205,214"


@pytest.mark.skipif(not HAVE_REF, reason="needs /root/reference to compile the reference's text")
def test_restatement_equals_the_compiled_reference_text_on_fresh_cases(oracle):
    """2^17 fresh seeded cases per function (projection / scale, sample_li), the chosen categories among them"""
    mk = generator()
    L, _ = mk.convert()
    d = mk.reference(L, n_fresh=1 << 17, seed=0x5EEDC, tables=False)
    for kind in (abi.LIGHT_PROJECTION, abi.LIGHT_GONIOMETRIC):
        assert (d["light_kind"][d["map_rec"]] == kind).sum() >= 1 << 17 and (d["light_kind"][d["sli_rec"]] == kind).sum() >= 1 << 17
    bad = hold_restatement(restated_lib(), oracle.bvh_build, d, tables=False)
    assert not bad, "tests/maplight_restated.cpp differs from the reference's text:\n" + "\n".join(bad)
