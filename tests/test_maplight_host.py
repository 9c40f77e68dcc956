"""Projection and goniometric lights (ABI 24) on the host.  The restatement tests/maplight_restated.cpp, which tests/test_gpu_maplights.py holds
the GPU to, must be the oracle's own path where neither light is present: every camera sample's radiance and the film equal
oracle.render(..., want_li=True) bit for bit (the gallery with all three strategies under Sobol' and Halton, Cornell past the roulette threshold) —
with the restated light distributions, not the oracle's.  Known answers cover each branch of ProjectionLight::projection and
GonioPhotometricLight::scale, and scenes.py's two builders are held to the reference's formulas evaluated here in f32.  No GPU."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.util import DYNAMIC_LOOK_AT, GALLERY_LOOK_AT, MAPLIGHT_LOOK_AT, dynamic_maplight_room, gallery, maplight_feature_room, moving_maplight_room

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NO_MAP = 0xFFFFFFFF


def build_restated():
    td = tempfile.mkdtemp()
    so = os.path.join(td, "libmaplight.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"), "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests"), "-o", so, os.path.join(ROOT, "tests", "maplight_restated.cpp")])
    L = C.CDLL(so)
    L.ml_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.ml_map.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.ml_sample_li.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.ml_light_distribution.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def restated_render(L, sc, rd, threads=4):
    """(film (npix, 4), li (npix, spp, 3)) of the restated li through the oracle's tile loop"""
    npix = scenes.n_pixels(rd)
    film = np.zeros((npix, 4), F32)
    li = np.zeros((npix, int(rd.spp), 3), F32)
    assert L.ml_render(C.addressof(sc.desc), C.addressof(rd), threads, film.ctypes.data, li.ctypes.data) == 0
    return film, li


def restated_distribution(L, sc, strategy, p):
    n = int(sc.desc.n_lights)
    func, cdf, nv, vx = np.zeros(n, F32), np.zeros(n + 1, F32), np.zeros(3, np.int32), np.zeros(3, np.int32)
    pp = np.ascontiguousarray(p, F32)
    assert L.ml_light_distribution(C.addressof(sc.desc), int(strategy), pp.ctypes.data, func.ctypes.data, cdf.ctypes.data, nv.ctypes.data, vx.ctypes.data) == 0
    return func, cdf, nv, vx


def assert_same_li(got, want):
    a, b = got.view(np.uint32), want.view(np.uint32)
    nan = np.isnan(got) & np.isnan(want)
    bad = ((a != b) & ~nan).any(axis=-1)
    assert not bad.any(), "%d of %d camera samples differ" % (int(bad.sum()), bad.size)


@pytest.fixture(scope="module")
def restated():
    return build_restated()


def check(restated, oracle, sc, rd):
    film, li = restated_render(restated, sc, rd)
    ref = oracle.render(sc, rd, threads=4, want_li=True)
    assert_same_li(li, ref["li"].reshape(li.shape))
    assert np.array_equal(film.view(np.uint32), ref["film"].view(np.uint32))
    return li


# ---- the restatement is the oracle's path where the new lights are absent ----
@pytest.mark.parametrize("strategy", [abi.LIGHTS_SPATIAL, abi.LIGHTS_POWER, abi.LIGHTS_UNIFORM])
@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_restated_li_equals_the_oracles_on_the_gallery(restated, oracle, strategy, sampler):
    sc = gallery(oracle.bvh_build, "all")
    rd = scenes.make_render_desc(48, 36, 4, GALLERY_LOOK_AT, 60, max_depth=7, light_strategy=strategy, sampler=sampler)
    assert check(restated, oracle, sc, rd).mean() > 0.0


def test_restated_li_equals_the_oracles_past_roulette(restated, oracle):
    sc = scenes.cornell_box(oracle.bvh_build)
    rd = scenes.cornell_render_desc(res=32, spp=8, max_depth=12)
    check(restated, oracle, sc, rd)


# ---- known answers, one per branch ----
def gradient(h, w):
    """texel (t, s) = (s + 1, t + 1, 100 * t + s): a bilinear lookup names the texels it read"""
    t, s = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([s + 1, t + 1, 100 * t + s], -1).astype(F32)


def one_light_scene(builder, add):
    sb = scenes.SceneBuilder()
    m = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], m)
    add(sb)
    return sb.finish(builder)


def ml_map(L, sc, index, w):
    out = np.zeros(3, F32)
    ww = np.ascontiguousarray(w, F32)
    assert L.ml_map(C.addressof(sc.desc), index, ww.ctypes.data, out.ctypes.data) == 0
    return out


def test_projection_branches(restated, oracle):
    """light at the origin of its own frame looking down +z (LookAt (0 0 0) (0 0 1) up y: world_to_light is the identity up to LookAt's x flip),
    fov 90 so that the screen point of a direction (x, y, z) is (x / z, y / z); a 4 x 2 map: screen_bounds (-2, -1, 2, 1)"""
    sc = one_light_scene(oracle.bvh_build, lambda sb: sb.add_projection_light((0, 0, 0), (0, 0, 1), (2, 3, 4), fov=90.0, image=gradient(2, 4)))
    lt = sc.lights[0]
    assert lt["kind"] == abi.LIGHT_PROJECTION and lt["prim"] == 0
    x0, y0, x1, y1 = (float(v) for v in lt["p"][12:16])
    assert (x0, y0, x1, y1) == (-2.0, -1.0, 2.0, 1.0)
    w2l = lt["p"][3:12].reshape(3, 3).astype(np.float64)
    s = float(lt["p"][18])      # 1 / tan(45 deg) in f32: within an ulp of 1
    assert abs(s - 1.0) < 1e-6
    to_world = lambda v: np.linalg.solve(w2l, np.asarray(v, np.float64))      # noqa: E731  the world direction whose light-space image is v
    # behind the hither plane (wl.z < 1e-3): black, also for z = 0 and z < 0
    for z in (-1.0, 0.0, 0.5e-3):
        assert np.array_equal(ml_map(restated, sc, 0, to_world((0.1, 0.1, z))), np.zeros(3, F32))
    assert ml_map(restated, sc, 0, to_world((0.0, 0.0, 2e-3))).min() > 0      # just past it
    # just outside / just inside each of the four screen-bound edges
    eps = 1e-3
    for (x, y), inside in [((x0 - eps, 0), False), ((x0 + eps, 0), True), ((x1 + eps, 0), False), ((x1 - eps, 0), True),
                           ((0, y0 - eps), False), ((0, y0 + eps), True), ((0, y1 + eps), False), ((0, y1 - eps), True)]:
        v = ml_map(restated, sc, 0, to_world((x / s, y / s, 1.0)))
        assert (v.min() > 0) == inside and (inside or np.array_equal(v, np.zeros(3, F32))), (x, y, v)
    # the centre of texel (t, s) = (1, 2): st = ((2 + 0.5) / 4, (1 + 0.5) / 2) -> screen (0.5, 0.5): the texel itself
    v = ml_map(restated, sc, 0, to_world((0.5 / s, 0.5 / s, 1.0)))
    assert np.allclose(v, gradient(2, 4)[1, 2], rtol=1e-5)
    # sample_li = i * projection / d^2 with wi towards the light, pdf 1
    out = np.zeros(10, F32)
    p = np.array(to_world((0.5 / s, 0.5 / s, 1.0)) * 2.0, F32)
    assert restated.ml_sample_li(C.addressof(sc.desc), 0, p.ctypes.data, out.ctypes.data) == 0
    d2 = float((p.astype(np.float64) ** 2).sum())
    assert np.allclose(out[:3], np.array([2, 3, 4]) * gradient(2, 4)[1, 2] / d2, rtol=1e-5) and out[6] == 1.0
    # and to the bit: i * projection(-wi) / d^2 in f32, over the very direction sample_li hands to projection (the text's value of each piece: tests/test_reference_light_functions.py)
    m = ml_map(restated, sc, 0, -out[3:6])
    d = (lt["p"][:3] - p).astype(F32)
    d2f = F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))
    assert np.array_equal(out[:3], ((np.array([2, 3, 4], F32) * m).astype(F32) / d2f).astype(F32)) and m.min() > 0
    assert np.allclose(out[3:6], -p / math.sqrt(d2), atol=1e-6) and np.array_equal(out[7:10], lt["p"][:3])


def test_goniometric_branches(restated, oracle):
    """identity light_to_world: scale() swaps y and z, so the map's poles (theta = 0, pi) are the world's +y / -y and phi runs from +x towards +z"""
    img = gradient(4, 8)
    sc = one_light_scene(oracle.bvh_build, lambda sb: sb.add_goniometric_light(np.eye(4, dtype=F32), (1, 1, 1), image=img))
    assert sc.lights[0]["kind"] == abi.LIGHT_GONIOMETRIC and sc.lights[0]["prim"] == 0
    # the poles: wp.z = +-1 -> theta = 0 | pi, t = 0 | 1, phi = atan2(0, 0) = 0: rows 0 | 3 blended with the row across the (Repeat) edge
    top, bottom = ml_map(restated, sc, 0, (0, 1, 0)), ml_map(restated, sc, 0, (0, -1, 0))
    assert np.allclose(top[1], 0.5 * (img[0, 0, 1] + img[3, 0, 1])) and np.allclose(bottom[1], 0.5 * (img[0, 0, 1] + img[3, 0, 1]))
    # the equator at phi = pi / 2 (+z in the world: wp.y = 1) and the wrap: atan2 < 0 for world -z -> phi = 3 pi / 2
    v1, v2 = ml_map(restated, sc, 0, (0, 0, 1)), ml_map(restated, sc, 0, (0, 0, -1))
    assert np.allclose(v1[0], 0.25 * 8 + 0.5, atol=1e-4) and np.allclose(v2[0], 0.75 * 8 + 0.5, atol=1e-4)      # channel 0 = s + 1 at texel centre s + 0.5
    # just below the seam: phi slightly under 2 pi -> the last column blended with the first
    v3 = ml_map(restated, sc, 0, (1, 0, -1e-4))
    assert 1.0 < v3[0] < 8.0 and v3[0] > 4.0


def test_mapless_lights_are_exactly_i_over_d2(restated, oracle):
    def add(sb):
        sb.add_goniometric_light(scenes.Transform.translate((1, 2, 3)), (5, 6, 7))
        sb.add_projection_light((1, 2, 3), (1, 0, 3), (5, 6, 7), fov=60.0, up=(0, 0, 1))
    sc = one_light_scene(oracle.bvh_build, add)
    assert list(sc.lights["prim"]) == [NO_MAP, NO_MAP] and len(sc.envmaps) == 0
    for index, p in [(0, (0.3, 0.1, -2.0)), (0, (4.0, 5.0, 6.0)), (1, (1.2, 0.0, 3.1))]:      # (the projector looks straight down: the third point is inside its frustum)
        pp = np.array(p, F32)
        out = np.zeros(10, F32)
        assert restated.ml_sample_li(C.addressof(sc.desc), index, pp.ctypes.data, out.ctypes.data) == 0
        d = (np.array([1, 2, 3], F32) - pp).astype(F32)
        d2 = F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))
        assert np.array_equal(out[:3], (np.array([5, 6, 7], F32) / d2).astype(F32)) and out[6] == 1.0


def test_restated_power_distribution(restated, oracle):
    """power: func = Light::power().y() — 4 pi i (goniometric), 2 pi i (1 - cos_total_width) (projection), times the map's coarsest texel"""
    img = np.full((2, 4, 3), 0.5, F32)

    def add(sb):
        sb.add_goniometric_light(np.eye(4, dtype=F32), (1, 1, 1))
        sb.add_goniometric_light(np.eye(4, dtype=F32), (1, 1, 1), image=img)
        sb.add_projection_light((0, 3, 0), (0, 0, 0), (1, 1, 1), fov=45.0, up=(0, 0, 1))
    sc = one_light_scene(oracle.bvh_build, add)
    f, c, _, _ = restated_distribution(restated, sc, abi.LIGHTS_POWER, (0, 0, 0))
    cos_w = float(sc.lights[2]["p"][17])
    assert np.allclose(f, [4 * math.pi, 2 * math.pi, 2 * math.pi * (1 - cos_w)], rtol=1e-5) and c[0] == 0 and abs(c[-1] - 1) < 1e-6
    # and to the bit, term by term in f32: ((map * i) * k) * PI [* (1 - cos_total_width)], then RGBSpectrum::y
    y = lambda r: F32(F32(F32(F32(0.212671) * r) + F32(F32(0.715160) * r)) + F32(F32(0.072169) * r))      # noqa: E731
    pi = F32(math.pi)
    want = [y(F32(F32(4) * pi)), y(F32(F32(F32(0.5) * F32(4)) * pi)), y(F32(F32(F32(2) * pi) * F32(F32(1) - sc.lights[2]["p"][17])))]
    assert np.array_equal(f, np.array(want, F32))


# ---- scenes.py's builders against the reference's formulas, evaluated here in f32 ----
def f32_dot_row(m, i, p):
    return F32(F32(F32(F32(m[i, 0] * p[0]) + F32(m[i, 1] * p[1])) + F32(m[i, 2] * p[2])) + m[i, 3])


def f32_transform_point(m, p):      # transform.rs:490-517
    p = [F32(v) for v in p]
    xp, yp, zp, wp = (f32_dot_row(m, i, p) for i in range(4))
    if wp == F32(1):
        return xp, yp, zp
    inv = F32(F32(1) / wp)
    return F32(inv * xp), F32(inv * yp), F32(inv * zp)


@pytest.mark.parametrize("p_from,p_to,shape,fov", [((0, 5, 0), (1, 0, 2), (2, 8), 45.0), ((-3, 2, 1), (0, 1, 0), (8, 2), 30.0), ((2.5, 4, -2), (2.5, 0, 1), (4, 4), 70.0)])
def test_projection_builder_record(p_from, p_to, shape, fov):
    """wide, tall and square maps at three positions: ProjectionLight::new_hdr (projection.rs:258-317)"""
    h, w = shape
    img = np.random.default_rng(h * 16 + w).uniform(0.1, 1.0, (h, w, 3)).astype(F32)
    sb = scenes.SceneBuilder()
    sb.add_projection_light(p_from, p_to, (3, 2, 1), fov=fov, image=img)
    lt = sb.delta_lights[0]
    l2w = scenes.Transform.look_at(p_from, p_to, (0, 1, 0)).inverse()      # the CTM of `LookAt`: light_to_world
    assert lt["kind"] == abi.LIGHT_PROJECTION and lt["prim"] == 0 and np.array_equal(lt["L"], np.array([3, 2, 1], F32))
    assert np.array_equal(lt["p"][:3], np.array(f32_transform_point(l2w.m, (0, 0, 0)), F32)) and np.allclose(lt["p"][:3], p_from, atol=1e-6)
    assert np.array_equal(lt["p"][3:12], l2w.m_inv[:3, :3].reshape(-1))      # world_to_light = Transform::inverse(light_to_world)
    aspect = F32(F32(w) / F32(h))      # :266-289
    sb_want = (-aspect, F32(-1), aspect, F32(1)) if aspect > 1 else (F32(-1), F32(F32(-1) / aspect), F32(1), F32(F32(1) / aspect))
    assert np.array_equal(lt["p"][12:16], np.array(sb_want, F32))
    proj = scenes.Transform.perspective(fov, 1e-3, 1e30)      # :290-292
    assert lt["p"][16] == F32(1e-3)
    corner = f32_transform_point(proj.m_inv, (sb_want[2], sb_want[3], 0.0))      # :293-301
    inv_len = F32(F32(1) / F32(np.sqrt(F32(F32(F32(corner[0] * corner[0]) + F32(corner[1] * corner[1])) + F32(corner[2] * corner[2])))))
    assert lt["p"][17] == F32(corner[2] * inv_len) and 0.0 < lt["p"][17] < 1.0
    assert np.array_equal(lt["p"][18:22], np.array([proj.m[0, 0], proj.m[1, 1], proj.m[2, 2], proj.m[2, 3]], F32))
    # what the record leaves out of light_projection.m is what Transform::perspective leaves trivial: +0 (the sign too) and m[3][2] = 1
    rest = proj.m.copy()
    rest[0, 0] = rest[1, 1] = rest[2, 2] = rest[2, 3] = rest[3, 2] = 0
    assert proj.m[3, 2] == 1 and not rest.any() and not np.signbit(rest).any()
    # the half angle of the cone through the corner: tan = |corner| * tan(fov / 2)
    t = math.tan(math.radians(fov) / 2) * math.hypot(float(sb_want[2]), float(sb_want[3]))
    assert abs(float(lt["p"][17]) - 1 / math.sqrt(1 + t * t)) < 1e-5
    # the map: the builder's pyramid (mipmap.rs:154-185), no distribution
    env = sb.envmaps[0]
    assert (env["width"], env["height"], env["n_levels"]) == (w, h, 1 + int(math.log2(max(w, h)))) and env["dist_func"] is None and env["dist_nu"] == env["dist_nv"] == 0
    want = scenes.build_envmap(img)
    assert np.array_equal(env["texels"], want["texels"])


@pytest.mark.parametrize("t,deg,shape", [((0, 4, 0), 0.0, (4, 8)), ((1, 2, -3), 35.0, (8, 2)), ((-2, 1, 2), 110.0, (4, 4))])
def test_goniometric_builder_record(t, deg, shape):
    l2w = scenes.Transform.translate(t) * scenes.Transform.rotate_y(deg)
    img = np.random.default_rng(7).uniform(0.1, 1.0, shape + (3,)).astype(F32)
    sb = scenes.SceneBuilder()
    sb.add_goniometric_light(l2w, (1, 2, 3), image=img)
    sb.add_goniometric_light(l2w.m, (1, 2, 3))
    lt, bare = sb.delta_lights
    assert lt["kind"] == bare["kind"] == abi.LIGHT_GONIOMETRIC and lt["prim"] == 0 and bare["prim"] == NO_MAP and len(sb.envmaps) == 1
    assert np.array_equal(lt["p"][:3], np.array(f32_transform_point(l2w.m, (0, 0, 0)), F32)) and np.array_equal(lt["p"][:3], np.array(t, F32))
    assert np.array_equal(lt["p"][3:12], l2w.m_inv[:3, :3].reshape(-1))
    assert np.allclose(bare["p"][3:12], lt["p"][3:12], atol=1e-6)      # (Matrix4x4::inverse of the product against the product of the inverses)
    assert not lt["p"][12:].any() and sb.envmaps[0]["dist_func"] is None


# ---- the rooms that reach the all-features map-light instantiation, and what the generic one's gallery lacks (tests/test_gpu_maplights.py) ----
def changed(a, b):
    """the fraction of camera samples whose radiance differs in any bit"""
    return float((a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).mean())


def dynamic_rd(sampler="sobol", strategy=abi.LIGHTS_SPATIAL, depth=5):
    return scenes.make_render_desc(48, 36, 4, DYNAMIC_LOOK_AT, 75.0, max_depth=depth, sampler=sampler, light_strategy=strategy)


def moving_rd(sampler="sobol"):
    from tests.test_instancing import LOOK
    return scenes.make_render_desc(48, 36, 4, LOOK, 40.0, shutter=(0.0, 1.0), sampler=sampler)


def feature_rd(sampler="sobol"):
    return scenes.make_render_desc(48, 36, 4, MAPLIGHT_LOOK_AT, 60, max_depth=5, sampler=sampler)


@pytest.mark.parametrize("sampler,strategy,depth", [("sobol", abi.LIGHTS_SPATIAL, 5), ("halton", abi.LIGHTS_POWER, 7)])
def test_restated_li_equals_the_oracles_over_dynamic_materials(restated, oracle, sampler, strategy, depth):
    """the room of dynamic slabs without its map lights: lobe lists built per hit pass through the restatement unchanged"""
    from rs_pbrt_amd import lib
    sc = dynamic_maplight_room(oracle.bvh_build, maplights=False)
    assert sum(lib.material_lobes(sc, i)[2] is None for i in range(int(sc.desc.n_materials))) >= 8
    assert check(restated, oracle, sc, dynamic_rd(sampler, strategy, depth)).mean() > 0.0


def test_map_lights_reach_the_dynamic_slabs(restated, oracle):
    """what the GPU case is worth: removing the three map lights changes at least half of the camera samples"""
    rd = dynamic_rd()
    lit = dynamic_maplight_room(oracle.bvh_build)
    kinds = list(lit.lights["kind"])
    assert kinds.count(abi.LIGHT_PROJECTION) == 1 and kinds.count(abi.LIGHT_GONIOMETRIC) == 2 and kinds.count(abi.LIGHT_DIFFUSE_AREA) == 1
    with_lights = restated_render(restated, lit, rd)[1]
    without = restated_render(restated, dynamic_maplight_room(oracle.bvh_build, maplights=False), rd)[1]
    assert not np.isnan(with_lights).any() and changed(with_lights, without) >= 0.5


@pytest.mark.parametrize("mode,dynamic", [("fixed", False), ("reference", False), ("fixed", True)])
def test_restated_li_equals_the_oracles_over_moving_instances(restated, oracle, mode, dynamic):
    """the room of moving instances without its map lights, and what they add: at least half of the camera samples"""
    rd = moving_rd()
    sc = moving_maplight_room(oracle.bvh_build, mode, dynamic, maplights=False)
    assert int(sc.instances["animated"].sum()) >= 5
    without = check(restated, oracle, sc, rd)
    with_lights = restated_render(restated, moving_maplight_room(oracle.bvh_build, mode, dynamic), rd)[1]
    assert not np.isnan(with_lights).any() and changed(with_lights, without) >= 0.5


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_restated_li_equals_the_oracles_in_the_feature_room(restated, oracle, sampler):
    """textures and bump, static instances, a null surface, alpha and shadow-alpha masks, a medium interface and an image-mapped infinite light, without the
    map lights"""
    sc = maplight_feature_room(oracle.bvh_build, maplights=False)
    assert len(sc.instances) == 2 and not sc.instances["animated"].any() and len(sc.media) == 1 and ((sc.prims["material"] == abi.NO_MATERIAL) & (sc.prims["mesh"] != abi.MESH_INSTANCE)).sum() == 2
    assert (np.asarray(sc.meshes["alpha_tex"]) != 0).sum() == 1 and (np.asarray(sc.meshes["shadow_alpha_tex"]) != 0).sum() == 1
    assert check(restated, oracle, sc, feature_rd(sampler)).mean() > 0.0


def test_the_feature_room_holds_what_it_says(restated, oracle):
    """the map lights' maps come after the infinite light's (prim >= 1; only that one carries a distribution), no material is dynamic (the generic set serves
    the room), and the two masks shape what the camera sees: making them opaque changes at least 5 % of the camera samples"""
    from rs_pbrt_amd import lib
    rd = feature_rd()
    sc = maplight_feature_room(oracle.bvh_build)
    by_kind = {int(k): int(p) for k, p in zip(sc.lights["kind"], sc.lights["prim"])}
    assert by_kind[abi.LIGHT_INFINITE] == 0 and by_kind[abi.LIGHT_PROJECTION] == 1 and by_kind[abi.LIGHT_GONIOMETRIC] == 2
    assert [e["dist_func"] is not None for e in sc.envmaps] == [True, False, False]
    assert all(lib.material_lobes(sc, i)[2] is not None for i in range(int(sc.desc.n_materials)))
    masked = restated_render(restated, sc, rd)[1]
    opaque = restated_render(restated, maplight_feature_room(oracle.bvh_build, masks=False), rd)[1]
    assert not np.isnan(masked).any() and changed(masked, opaque) >= 0.05
