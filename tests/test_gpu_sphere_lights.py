"""-m gpu: sphere area lights behind the sphere-light gate (include/rspt.h rspt_set_sphere_lights; off by default).  (a) the stage hook rspt_sphere_light equals the
hand restatement of Sphere::area / sample / sample_with_ref_point / pdf_with_ref_point and DiffuseAreaLight::sample_li (tests/spherelight_restated.cpp, held to
closed forms by tests/test_spherelight_host.py) word for word; (b) with the gate on, every camera sample of a sphere-light scene equals the restated
PathIntegrator::li (tests/spherelight_render_restated.cpp) bit for bit, by the shade instantiation RSPT_VERBOSE names; (c) rspt_light_distribution equals the
restated tables; (d) the gate: off gives today's refusal again, on still refuses what is out of scope by name, ao is served.
Every test that sets the gate restores it in a `finally`: the refusal tests of the other files must find it off."""
import contextlib

import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.test_sphere_render_host import assert_same_li
from tests.test_spherelight_host import (ROOM_LOOK, build_restated, hook, hook_cases, restated_light_distribution, restated_render, sphere_light_room)
from tests.util import film_rmse, shade_instantiation, xf

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def restated():
    return build_restated()


@contextlib.contextmanager
def gate_on(gpu):
    gpu.set_sphere_lights(True)
    try:
        yield
    finally:
        gpu.set_sphere_lights(False)


def room_rd(spp=8, **kw):
    return scenes.make_render_desc(32, 24, spp, ROOM_LOOK, 60, max_depth=5, **kw)


# ---- (a) the hook ----
def test_hook_equals_the_restatement_word_for_word(gpu, restated):
    """all 64 output words of a few thousand elements (tests/test_spherelight_host.py hook_cases says what they cover), compared as uint32 words; the hook
    works with the gate off.  No exemption for NaN: the restatement yields none on these cases (tests/test_spherelight_host.py asserts it), so none may come back."""
    assert not gpu.get_sphere_lights()
    x = hook_cases()
    want = hook(restated, x)
    got = np.empty_like(x)
    gpu._check(gpu.lib().rspt_sphere_light(x.ctypes.data, len(x), got.ctypes.data))
    bad = got.view(np.uint32) != want.view(np.uint32)
    rows = np.nonzero(bad.any(axis=1))[0]
    assert len(rows) == 0, "%d of %d elements differ; first: element %d, words %s, got %s, want %s" % (
        len(rows), len(x), rows[0], np.nonzero(bad[rows[0]])[0], got[rows[0], bad[rows[0]]], want[rows[0], bad[rows[0]]])
    assert np.all(got[:, 29:] == 0.0)


# ---- (b) renders ----
def parity(gpu, restated, sc, rd, monkeypatch, capfd, kernel, rmse=1e-5):
    """the render with the gate on, by the shade instantiation named `kernel`: every camera sample's radiance equals the restatement's, and so does the film"""
    def run():
        with gate_on(gpu), gpu.DeviceScene(sc) as ds:
            li, _ = gpu.render_samples(ds, rd)
            film, _ = gpu.render(ds, rd)
        return li, film
    (li, film), name = shade_instantiation(monkeypatch, capfd, run)
    assert name == kernel
    want_film, want = restated_render(restated, sc, rd)
    assert_same_li(li, want)
    assert film_rmse(film, want_film) < rmse
    assert np.nanmean(li) > 0.0
    return li


@pytest.mark.parametrize("sampler,strategy", [("sobol", abi.LIGHTS_SPATIAL), ("halton", abi.LIGHTS_SPATIAL), ("sobol", abi.LIGHTS_POWER), ("halton", abi.LIGHTS_UNIFORM)])
def test_room_under_a_sphere_light_beside_other_lights(gpu, restated, monkeypatch, capfd, sampler, strategy):
    """a sphere light beside a triangle light, a point light and an infinite light: both samplers, all three light strategies"""
    sc = sphere_light_room(gpu.bvh_build, "mixed")
    parity(gpu, restated, sc, room_rd(sampler=sampler, light_strategy=strategy), monkeypatch, capfd, "generic-spherelight")


@pytest.mark.parametrize("kind,spp", [("inside", 8), ("on_light", 16), ("clipped", 8)])
def test_inside_branch_lights_on_lights_and_clipped_two_sided_lights(gpu, restated, monkeypatch, capfd, kind, spp):
    """the camera and the room inside a large inward-emitting sphere (the inside branch at every vertex); a matte emissive sphere lit by a second sphere light
    (reference points ON a light); a two-sided z- and phi-clipped light under a mirrored, non-uniformly scaled transform"""
    sc = sphere_light_room(gpu.bvh_build, kind)
    parity(gpu, restated, sc, room_rd(spp=spp), monkeypatch, capfd, "generic-spherelight")


def test_room_with_a_dynamic_material(gpu, restated, monkeypatch, capfd):
    sc = sphere_light_room(gpu.bvh_build, "dynamic")
    parity(gpu, restated, sc, room_rd(), monkeypatch, capfd, "dynamic-spherelight")


# ---- (c) the light tables ----
@pytest.mark.parametrize("kind", ["mixed", "on_light"])
def test_light_distribution_equals_the_restated_tables(gpu, restated, kind):
    sc = sphere_light_room(gpu.bvh_build, kind)
    lo, hi = sc.nodes["bmin"][0], sc.nodes["bmax"][0]
    pts = np.random.default_rng(6).uniform(lo - 0.3, hi + 0.3, (34, 3)).astype(F32)
    # ... and points inside every sphere light (its centre and two more)
    sph_of_prim = sc.prims["v"][:, 0][(sc.prims["mesh"] == abi.MESH_SPHERE) & (sc.prims["area_light"] >= 0)]
    inside = [sc.spheres["object_to_world"][k].reshape(4, 4)[:3, 3] + np.array(o, F32) for k in sph_of_prim for o in ((0, 0, 0), (0.1, -0.2, 0.1), (0, 0.3, 0))]
    pts = np.concatenate([pts, np.array(inside, F32)])
    assert len(pts) >= 37
    with gate_on(gpu), gpu.DeviceScene(sc) as ds:
        for strategy in (abi.LIGHTS_SPATIAL, abi.LIGHTS_POWER, abi.LIGHTS_UNIFORM):
            for p in pts if strategy == abi.LIGHTS_SPATIAL else pts[:3]:
                f, c, nv, vx = gpu.light_distribution(ds, strategy, p)
                wf, wc, wnv, wvx = restated_light_distribution(restated, sc, strategy, p)
                assert list(nv) == list(wnv) and list(vx) == list(wvx), (strategy, p)
                assert np.array_equal(f.view(np.uint32), wf.view(np.uint32)) and np.array_equal(c.view(np.uint32), wc.view(np.uint32)), (strategy, p, f, wf)


# ---- (d) the gate ----
def _plain_room(gpu, emit=(1.0, 1.0, 1.0), disk=False, maplight=False):
    sb = scenes.SceneBuilder()
    mat = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], mat)
    sb.add_quad([(-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1)], mat, emit=(5, 5, 5))
    sb.add_point_light((2, 3, -2), (4, 4, 4))
    sb.add_sphere(1.0, object_to_world=xf((0, 1, 0)), material=mat, emit=emit)
    if disk:
        sb.add_disk(0.0, 0.8, object_to_world=xf((2.5, 1.0, 0.0), (1, 0, 0), 90), material=mat)
    if maplight:
        sb.add_projection_light((0, 4, -4), (0, 1, 0), (30, 30, 30), fov=50.0)
    return sb.finish(gpu.bvh_build)


LOOK = ((0, 2.2, -6.5), (0, 1.0, 0), (0, 1, 0))


def _refused(gpu, call, words):
    with pytest.raises(gpu.RsptError) as e:
        call()
    assert e.value.code == abi.E_UNSUPPORTED
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    return str(e.value)


def test_gate_on_then_off_gives_todays_refusal_again(gpu, restated):
    sc = _plain_room(gpu)
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0)
    off_text = "scene with an emissive sphere: sphere area lights are not served on the device yet (path)"
    off_ld_text = "scene with an emissive sphere: the light distributions are not built for sphere area lights yet"
    with gpu.DeviceScene(sc) as ds:
        assert _refused(gpu, lambda: gpu.render(ds, rd), []).endswith(off_text)
        assert _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0)), []).endswith(off_ld_text)
        with gate_on(gpu):
            li, _ = gpu.render_samples(ds, rd)
            gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0))
        assert not gpu.get_sphere_lights()
        assert _refused(gpu, lambda: gpu.render(ds, rd), []).endswith(off_text)
        assert _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0)), []).endswith(off_ld_text)
    assert_same_li(li, restated_render(restated, sc, rd)[1])


def test_the_environment_overrides_the_call(gpu, monkeypatch):
    sc = _plain_room(gpu)
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0)
    with gpu.DeviceScene(sc) as ds:
        monkeypatch.setenv("RSPT_SPHERE_LIGHTS", "1")
        assert not gpu.get_sphere_lights()
        assert gpu.render(ds, rd)[0][:, 3].sum() > 0
        monkeypatch.setenv("RSPT_SPHERE_LIGHTS", "0")
        with gate_on(gpu):
            _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area light"])
        monkeypatch.setenv("RSPT_SPHERE_LIGHTS", "yes")
        with pytest.raises(gpu.RsptError) as e:
            gpu.render(ds, rd)
        assert e.value.code == abi.E_INVALID and "RSPT_SPHERE_LIGHTS" in str(e.value)
        monkeypatch.delenv("RSPT_SPHERE_LIGHTS")
        _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area light"])


@pytest.mark.parametrize("integrator,sampler,word", [("directlighting", "sobol", "directlighting"), ("whitted", "halton", "whitted"), ("volpath", "sobol", "volpath"),
                                                     ("path", "random", "random"), ("path", "02sequence", "02sequence"), ("ao", "stratified", "stratified"),
                                                     ("path", "maxmindist", "maxmindist")])
def test_gate_on_out_of_scope_renders_refused_by_name(gpu, integrator, sampler, word):
    sc = _plain_room(gpu)
    rd = scenes.make_render_desc(16, 16, 16, LOOK, 45.0, integrator=integrator, sampler=sampler, strat=(4, 4))
    with gate_on(gpu), gpu.DeviceScene(sc) as ds:
        _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area light", word])


def test_gate_on_other_shapes_map_lights_on_demand_table_and_counters_refused(gpu, monkeypatch):
    """(the refusal of a scene with more four-box records than a reference holds, 2^25, needs a scene no quick test can build)"""
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0, light_strategy=abi.LIGHTS_SPATIAL)
    with gate_on(gpu):
        with gpu.DeviceScene(_plain_room(gpu, disk=True)) as ds:
            _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area light", "disk"])
            _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, (0, 0.5, 0)), ["sphere area light", "disk"])
        with gpu.DeviceScene(_plain_room(gpu, maplight=True)) as ds:
            _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area light", "projection"])
            _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, (0, 0.5, 0)), ["sphere area light", "projection"])
        with gpu.DeviceScene(_plain_room(gpu)) as ds:
            monkeypatch.setenv("RSPT_LIGHT_TABLE_EAGER_BYTES", "0")
            _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area light", "on-demand"])
            _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, (0, 0.5, 0)), ["sphere area light", "on-demand"])
            monkeypatch.delenv("RSPT_LIGHT_TABLE_EAGER_BYTES")
            monkeypatch.setenv("RSPT_COUNTERS", "1")
            _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area light", "RSPT_COUNTERS"])
            monkeypatch.delenv("RSPT_COUNTERS")
            assert gpu.render(ds, rd)[0][:, 3].sum() > 0      # (the refused table was never kept: the same scene renders)


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_ao_on_an_emissive_sphere_scene_is_served(gpu, restated, sampler):
    """ao reads no lights: with the gate on, a scene with an emissive sphere is served and equals the restatement"""
    sc = sphere_light_room(gpu.bvh_build, "mixed")
    rd = scenes.make_render_desc(32, 24, 4, ROOM_LOOK, 60, integrator="ao", ao_samples=4, sampler=sampler)
    with gate_on(gpu), gpu.DeviceScene(sc) as ds:
        li, _ = gpu.render_samples(ds, rd)
    assert_same_li(li, restated_render(restated, sc, rd)[1])
    assert li.mean() > 0.0
