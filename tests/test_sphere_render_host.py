"""The restatement of PathIntegrator::li / AOIntegrator::li over a scene view with spheres (tests/sphere_render_restated.cpp, which
tests/test_gpu_sphere_render.py holds the GPU render of sphere scenes to) must be the oracle's own li where there are no spheres: on
triangle-only scenes every camera sample's radiance equals oracle.render(..., want_li=True) bit for bit — every material recipe, textures
and bump maps, null surfaces, an infinite light, alpha masks, depths past the roulette threshold, Sobol' and Halton, all three light
strategies.  No GPU: the helper is compiled here with g++."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.util import GALLERY_LOOK_AT, SPHERE_LOOK_AT, TEXTURED_LOOK_AT, dynamic_sphere_room, gallery, random_scene, sky_scene, textured_room
from tests.test_alpha_masks import masked_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_restated():
    td = tempfile.mkdtemp()
    so = os.path.join(td, "libsphrender.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"), "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests"), "-o", so, os.path.join(ROOT, "tests", "sphere_render_restated.cpp")])
    L = C.CDLL(so)
    L.sr_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L


def restated_render(L, sc, rd, threads=4):
    """(film (npix, 4), li (npix, spp, 3)) of the restated li through the oracle's tile loop"""
    npix = scenes.n_pixels(rd)
    film = np.zeros((npix, 4), np.float32)
    li = np.zeros((npix, int(rd.spp), 3), np.float32)
    assert L.sr_render(C.addressof(sc.desc), C.addressof(rd), threads, film.ctypes.data, li.ctypes.data) == 0
    return film, li


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


def test_restated_li_equals_the_oracles_with_textures_null_surfaces_and_sky(restated, oracle):
    check(restated, oracle, textured_room(oracle.bvh_build), scenes.make_render_desc(40, 30, 4, TEXTURED_LOOK_AT, 60, max_depth=4))
    cb = scenes.cornell_box(oracle.bvh_build)
    cb.prims["material"][cb.prims["material"] == 1] = abi.NO_MATERIAL
    check(restated, oracle, cb, scenes.cornell_render_desc(res=32, spp=4, max_depth=3))
    for kind in ("constant", "image"):
        check(restated, oracle, sky_scene(oracle.bvh_build, kind, with_area=True), scenes.make_render_desc(40, 30, 4, GALLERY_LOOK_AT, 60, max_depth=5, sampler="halton"))


@pytest.mark.parametrize("shadow_only", [False, True])
def test_restated_li_equals_the_oracles_with_alpha_masks(restated, oracle, shadow_only):
    sc = masked_scene(oracle.bvh_build, shadow_only=shadow_only)
    rd = scenes.make_render_desc(40, 30, 4, ((0, 1.5, -4), (0, 1, 0), (0, 1, 0)), 60, max_depth=4)
    check(restated, oracle, sc, rd)


@pytest.mark.parametrize("seed", [101, 104, 110])
def test_restated_li_equals_the_oracles_on_random_scenes(restated, oracle, seed):
    sc = random_scene(oracle.bvh_build, seed)
    rd = scenes.make_render_desc(40, 30, 4, GALLERY_LOOK_AT, 55, max_depth=2 + seed % 9, sampler="halton" if seed % 2 else "sobol",
                                 light_strategy=[abi.LIGHTS_SPATIAL, abi.LIGHTS_POWER, abi.LIGHTS_UNIFORM][seed % 3])
    check(restated, oracle, sc, rd)


@pytest.mark.parametrize("cos_sample", [False, True])
def test_restated_ao_li_equals_the_oracles(restated, oracle, cos_sample):
    sc = scenes.cornell_box(oracle.bvh_build)
    for sampler in ("sobol", "halton"):
        rd = scenes.cornell_render_desc(res=32, spp=4, integrator="ao", ao_samples=4, ao_cos_sample=cos_sample, sampler=sampler)
        check(restated, oracle, sc, rd)


# ---- the room that reaches the dynamic sphere instantiation (tests/test_gpu_sphere_render.py) ----
def dynamic_sphere_rd(sampler="sobol", strategy=abi.LIGHTS_SPATIAL, depth=6):
    return scenes.make_render_desc(48, 36, 4, SPHERE_LOOK_AT, 60, max_depth=depth, sampler=sampler, light_strategy=strategy)


@pytest.mark.parametrize("sampler,strategy,depth", [("sobol", abi.LIGHTS_SPATIAL, 6), ("halton", abi.LIGHTS_POWER, 5)])
def test_restated_li_equals_the_oracles_on_the_dynamic_rooms_triangle_twin(restated, oracle, sampler, strategy, depth):
    """the oracle has no spheres: the same dynamic materials (lobe lists built per hit, UV and spherical mappings) on slabs pass through the restatement unchanged"""
    from rs_pbrt_amd import lib
    sc = dynamic_sphere_room(oracle.bvh_build, shapes="slabs")
    assert len(sc.spheres) == 0 and sum(lib.material_lobes(sc, i)[2] is None for i in range(int(sc.desc.n_materials))) >= 7
    assert check(restated, oracle, sc, dynamic_sphere_rd(sampler, strategy, depth)).mean() > 0.0


def test_dynamic_materials_fill_the_sphere_room(restated):
    """what the GPU case is worth: at least seven materials are dynamic, seven spheres (full, z-clipped, phi-clipped, mirror-scaled) and a slab carry them, and a
    constant matte in their place changes at least 20 % of the camera samples"""
    from rs_pbrt_amd import lib
    rd = dynamic_sphere_rd()
    sc = dynamic_sphere_room(lib.bvh_build)
    dyn = [i for i in range(int(sc.desc.n_materials)) if lib.material_lobes(sc, i)[2] is None]
    assert len(dyn) >= 7
    on_spheres = set(int(m) for m in sc.prims["material"][sc.prims["mesh"] == abi.MESH_SPHERE])
    on_tris = set(int(m) for m in sc.prims["material"][sc.prims["mesh"] != abi.MESH_SPHERE])
    assert len(sc.spheres) == 7 and len(on_spheres & set(dyn)) == 7 and on_tris & set(dyn)
    assert int(sc.spheres["transform_swaps_handedness"].sum()) == 1 and (sc.spheres["phi_max"] < 6.0).sum() == 2 and (sc.spheres["z_max"] < sc.spheres["radius"]).sum() == 2
    li = restated_render(restated, sc, rd)[1]
    plain = restated_render(restated, dynamic_sphere_room(lib.bvh_build, dynamic=False), rd)[1]
    assert not np.isnan(li).any()
    assert float((li.view(np.uint32) != plain.view(np.uint32)).any(axis=-1).mean()) >= 0.2
