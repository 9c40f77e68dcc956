"""-m gpu: disk and cylinder area lights behind the quadric-light gate (include/rspt.h rspt_set_quadric_lights; off by default).  (a) the stage hook
rspt_quadric_light equals the hand restatement of Disk / Cylinder area, sample, sample_with_ref_point, pdf_with_ref_point and DiffuseAreaLight::sample_li / power
(tests/quadriclight_restated.cpp, held to closed forms and a Monte-Carlo check by tests/test_quadriclight_host.py) word for word; (b) with the gate on, every
camera sample of a scene lit by a disk or a cylinder equals the restated PathIntegrator::li (tests/quadriclight_render_restated.cpp) bit for bit, by the shade
instantiation RSPT_VERBOSE names; (c) rspt_light_distribution equals the restated tables; (d) the gate: off gives the parent's refusal again, on still refuses
what is out of scope by name, an emissive sphere beside a disk needs both gates, ao is served.
Every test that sets a gate restores it in a `finally`: the refusal tests of the other files must find both off."""
import contextlib

import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.test_quadriclight_host import (ROOM_LOOK, build_restated, emissive_quadrics, hook, hook_cases, quadric_light_room, restated_light_distribution,
                                          restated_render, to_world)
from tests.test_sphere_render_host import assert_same_li
from tests.util import film_rmse, shade_instantiation, xf

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def restated():
    return build_restated()


@contextlib.contextmanager
def gates(gpu, quadric=True, sphere=False):
    gpu.set_quadric_lights(quadric)
    gpu.set_sphere_lights(sphere)
    try:
        yield
    finally:
        gpu.set_quadric_lights(False)
        gpu.set_sphere_lights(False)


def room_rd(spp=8, **kw):
    return scenes.make_render_desc(32, 24, spp, ROOM_LOOK, 60, max_depth=5, **kw)


# ---- (a) the hook ----
def test_hook_equals_the_restatement_word_for_word(gpu, restated):
    """all 64 output words of a few thousand elements (tests/test_quadriclight_host.py hook_cases says what they cover), compared as uint32 words; the hook works
    with the gate off.  No exemption for NaN: the restatement yields none on these cases (tests/test_quadriclight_host.py asserts it), so none may come back."""
    assert not gpu.get_quadric_lights()
    x = hook_cases(restated)
    want = hook(restated, x)
    got = np.empty_like(x)
    gpu._check(gpu.lib().rspt_quadric_light(x.ctypes.data, len(x), got.ctypes.data))
    bad = got.view(np.uint32) != want.view(np.uint32)
    rows = np.nonzero(bad.any(axis=1))[0]
    assert len(rows) == 0, "%d of %d elements differ; first: element %d, words %s, got %s, want %s" % (
        len(rows), len(x), rows[0], np.nonzero(bad[rows[0]])[0], got[rows[0], bad[rows[0]]], want[rows[0], bad[rows[0]]])
    assert np.all(got[:, 32:] == 0.0)
    # a kind that is neither a disk nor a cylinder: all words 0
    y = x[:3].copy()
    y.view(np.uint32)[:, 40] = [abi.MESH_SPHERE, 0, 7]
    gpu._check(gpu.lib().rspt_quadric_light(y.ctypes.data, len(y), got.ctypes.data))
    assert np.all(got[:3].view(np.uint32) == 0)


# ---- (b) renders ----
def parity(gpu, restated, sc, rd, monkeypatch, capfd, kernel, sphere=False, rmse=1e-5):
    """the render with the gate(s) on, by the shade instantiation named `kernel`: every camera sample's radiance equals the restatement's, and so does the film"""
    def run():
        with gates(gpu, True, sphere), gpu.DeviceScene(sc) as ds:
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


@pytest.mark.parametrize("sampler,strategy", [("sobol", abi.LIGHTS_SPATIAL), ("halton", abi.LIGHTS_SPATIAL), ("sobol", abi.LIGHTS_POWER), ("halton", abi.LIGHTS_POWER),
                                              ("sobol", abi.LIGHTS_UNIFORM), ("halton", abi.LIGHTS_UNIFORM)])
def test_room_under_a_disk_lamp_beside_other_lights(gpu, restated, monkeypatch, capfd, sampler, strategy):
    """a disk lamp beside a triangle light, a point light and an infinite light: both samplers, all three light strategies"""
    sc = quadric_light_room(gpu.bvh_build, "mixed")
    parity(gpu, restated, sc, room_rd(sampler=sampler, light_strategy=strategy), monkeypatch, capfd, "generic-quadriclight")


def test_partial_annulus_clipped_cylinder_lamp_and_a_light_on_a_light(gpu, restated, monkeypatch, capfd):
    """a two-sided partial annulus under a mirrored, non-uniformly scaled transform (its samples land in the cut-away part too); a clipped two-sided cylinder
    lamp with a sphere inside it (reference points inside and outside); a matte emissive cylinder lit by a disk light (reference points ON a light)"""
    sc = quadric_light_room(gpu.bvh_build, "shapes")
    parity(gpu, restated, sc, room_rd(), monkeypatch, capfd, "generic-quadriclight")


def test_room_with_a_dynamic_material(gpu, restated, monkeypatch, capfd):
    sc = quadric_light_room(gpu.bvh_build, "dynamic")
    parity(gpu, restated, sc, room_rd(), monkeypatch, capfd, "dynamic-quadriclight")


def test_emissive_sphere_disk_and_cylinder_together_under_both_gates(gpu, restated, monkeypatch, capfd):
    sc = quadric_light_room(gpu.bvh_build, "all_three")
    assert sorted(sc.prims["mesh"][emissive_quadrics(sc)].tolist()) == sorted([abi.MESH_SPHERE, abi.MESH_DISK, abi.MESH_CYLINDER])
    parity(gpu, restated, sc, room_rd(), monkeypatch, capfd, "generic-quadriclight", sphere=True)


def test_shade_variant_naming_another_set_is_refused(gpu, monkeypatch):
    sc = quadric_light_room(gpu.bvh_build, "mixed")
    monkeypatch.setenv("RSPT_SHADE_VARIANT", "generic-quadric")
    with gates(gpu), gpu.DeviceScene(sc) as ds:
        _refused(gpu, lambda: gpu.render(ds, room_rd(spp=1)), ["RSPT_SHADE_VARIANT", "generic-quadriclight", "dynamic-quadriclight"])


# ---- (c) the light tables ----
@pytest.mark.parametrize("kind", ["mixed", "shapes"])
def test_light_distribution_equals_the_restated_tables(gpu, restated, kind):
    sc = quadric_light_room(gpu.bvh_build, kind)
    lo, hi = sc.nodes["bmin"][0], sc.nodes["bmax"][0]
    pts = np.random.default_rng(6).uniform(lo - 0.3, hi + 0.3, (30, 3)).astype(F32)
    # ... and points in every emissive disk's plane and on every emissive cylinder's axis
    special = []
    for i in emissive_quadrics(sc):
        mesh, k = sc.prims["mesh"][i], sc.prims["v"][i, 0]
        if mesh == abi.MESH_DISK:
            rec = sc.disks[k]
            special += [to_world(rec, (a, b, float(rec["height"]))) for a, b in ((0.0, 0.0), (1.7, -0.4), (-0.3, 2.5))]
        elif mesh == abi.MESH_CYLINDER:
            rec = sc.cylinders[k]
            special += [to_world(rec, (0.0, 0.0, z)) for z in (float(rec["z_min"]), 0.5 * float(rec["z_min"] + rec["z_max"]), float(rec["z_max"]) + 0.4)]
    pts = np.concatenate([pts, np.array(special, F32)])
    assert len(pts) >= (33 if kind == "mixed" else 40)
    with gates(gpu), gpu.DeviceScene(sc) as ds:
        for strategy in (abi.LIGHTS_SPATIAL, abi.LIGHTS_POWER, abi.LIGHTS_UNIFORM):
            for p in pts if strategy == abi.LIGHTS_SPATIAL else pts[:3]:
                f, c, nv, vx = gpu.light_distribution(ds, strategy, p)
                wf, wc, wnv, wvx = restated_light_distribution(restated, sc, strategy, p)
                assert list(nv) == list(wnv) and list(vx) == list(wvx), (strategy, p)
                assert np.array_equal(f.view(np.uint32), wf.view(np.uint32)) and np.array_equal(c.view(np.uint32), wc.view(np.uint32)), (strategy, p, f, wf)


# ---- (d) the gate ----
DOWN = ((1, 0, 0), 90)


def _plain_room(gpu, shapes=("disk",), sphere_emit=None, maplight=False, emit=(6.0, 6.0, 6.0)):
    sb = scenes.SceneBuilder()
    mat = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], mat)
    sb.add_quad([(-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1)], mat, emit=(5, 5, 5))
    sb.add_point_light((2, 3, -2), (4, 4, 4))
    sb.add_sphere(1.0, object_to_world=xf((0, 1, 0)), material=mat, emit=sphere_emit)
    if "disk" in shapes:
        sb.add_disk(0.0, 0.8, object_to_world=xf((2.5, 2.5, 0.0), *DOWN), material=mat, emit=emit)
    if "cylinder" in shapes:
        sb.add_cylinder(0.3, -0.6, 0.6, object_to_world=xf((-2.5, 2.0, 0.0)), material=mat, emit=emit)
    if "plain_disk" in shapes:
        sb.add_disk(0.0, 0.8, object_to_world=xf((2.5, 1.0, 0.0), *DOWN), material=mat)
    if maplight:
        sb.add_projection_light((0, 4, -4), (0, 1, 0), (30, 30, 30), fov=50.0)
    return sb.finish(gpu.bvh_build)


LOOK = ((0, 2.2, -6.5), (0, 1.0, 0), (0, 1, 0))


def _refused(gpu, call, words, code=abi.E_UNSUPPORTED):
    with pytest.raises(gpu.RsptError) as e:
        call()
    assert e.value.code == code
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    return str(e.value)


def _lights(shapes):
    return [s + " area light" for s in shapes]


@pytest.mark.parametrize("shapes", [("disk",), ("cylinder",), ("disk", "cylinder")])
def test_gate_on_then_off_gives_the_parents_refusal_again(gpu, restated, shapes):
    sc = _plain_room(gpu, shapes)
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0)
    names, what = " and ".join(shapes), " and ".join(s + " area lights" for s in shapes)
    off_text = "scene with an emissive %s: %s are not served on the device yet (path)" % (names, what)
    off_ld_text = "scene with an emissive %s: the light distributions are not built for %s yet" % (names, what)
    with gpu.DeviceScene(sc) as ds:
        assert _refused(gpu, lambda: gpu.render(ds, rd), []).endswith(off_text)
        assert _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0)), []).endswith(off_ld_text)
        with gates(gpu):
            li, _ = gpu.render_samples(ds, rd)
            gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0))
        assert not gpu.get_quadric_lights()
        assert _refused(gpu, lambda: gpu.render(ds, rd), []).endswith(off_text)
        assert _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0)), []).endswith(off_ld_text)
        with gates(gpu, quadric=False, sphere=True):      # the sphere-light gate serves no disk or cylinder
            assert _refused(gpu, lambda: gpu.render(ds, rd), []).endswith(off_text)
    assert_same_li(li, restated_render(restated, sc, rd)[1])


def test_the_environment_overrides_the_call(gpu, monkeypatch):
    sc = _plain_room(gpu)
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0)
    with gpu.DeviceScene(sc) as ds:
        monkeypatch.setenv("RSPT_QUADRIC_LIGHTS", "1")
        assert not gpu.get_quadric_lights()
        assert gpu.render(ds, rd)[0][:, 3].sum() > 0
        gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0))
        monkeypatch.setenv("RSPT_QUADRIC_LIGHTS", "0")
        with gates(gpu):
            _refused(gpu, lambda: gpu.render(ds, rd), ["disk area light", "not served on the device yet"])
            _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0)), ["disk area light"])
        monkeypatch.setenv("RSPT_QUADRIC_LIGHTS", "yes")
        _refused(gpu, lambda: gpu.render(ds, rd), ["RSPT_QUADRIC_LIGHTS"], abi.E_INVALID)
        _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0)), ["RSPT_QUADRIC_LIGHTS"], abi.E_INVALID)
        monkeypatch.delenv("RSPT_QUADRIC_LIGHTS")
        _refused(gpu, lambda: gpu.render(ds, rd), ["disk area light"])


@pytest.mark.parametrize("integrator,sampler,word", [("directlighting", "sobol", "directlighting"), ("whitted", "halton", "whitted"), ("volpath", "sobol", "volpath"),
                                                     ("path", "random", "random"), ("path", "02sequence", "02sequence"), ("ao", "stratified", "stratified"),
                                                     ("path", "maxmindist", "maxmindist")])
@pytest.mark.parametrize("shapes", [("disk",), ("cylinder",)])
def test_gate_on_out_of_scope_renders_refused_by_name(gpu, shapes, integrator, sampler, word):
    sc = _plain_room(gpu, shapes)
    rd = scenes.make_render_desc(16, 16, 16, LOOK, 45.0, integrator=integrator, sampler=sampler, strat=(4, 4))
    with gates(gpu), gpu.DeviceScene(sc) as ds:
        _refused(gpu, lambda: gpu.render(ds, rd), _lights(shapes) + [word])


@pytest.mark.parametrize("shapes", [("disk",), ("disk", "cylinder")])
def test_gate_on_map_lights_on_demand_table_and_counters_refused(gpu, shapes, monkeypatch):
    """(the refusal of a scene with more four-box records than a reference holds, 2^25, needs a scene no quick test can build: tests/test_quadriclight_host.py
    pins its text from the source)"""
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0, light_strategy=abi.LIGHTS_SPATIAL)
    with gates(gpu):
        with gpu.DeviceScene(_plain_room(gpu, shapes, maplight=True)) as ds:
            _refused(gpu, lambda: gpu.render(ds, rd), _lights(shapes) + ["projection"])
            _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, (0, 0.5, 0)), _lights(shapes) + ["projection"])
        with gpu.DeviceScene(_plain_room(gpu, shapes)) as ds:
            monkeypatch.setenv("RSPT_LIGHT_TABLE_EAGER_BYTES", "0")
            _refused(gpu, lambda: gpu.render(ds, rd), _lights(shapes) + ["on-demand"])
            _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, (0, 0.5, 0)), _lights(shapes) + ["on-demand"])
            monkeypatch.delenv("RSPT_LIGHT_TABLE_EAGER_BYTES")
            monkeypatch.setenv("RSPT_COUNTERS", "1")
            _refused(gpu, lambda: gpu.render(ds, rd), _lights(shapes) + ["RSPT_COUNTERS"])
            monkeypatch.delenv("RSPT_COUNTERS")
            assert gpu.render(ds, rd)[0][:, 3].sum() > 0      # (the refused table was never kept: the same scene renders)


def test_an_emissive_sphere_beside_a_disk_needs_both_gates(gpu, restated):
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0)
    served_only_without = "sphere area lights are served in scenes without a disk or a cylinder only"
    # an emissive sphere beside a plain disk
    sc = _plain_room(gpu, ("plain_disk",), sphere_emit=(1.0, 1.0, 1.0))
    with gpu.DeviceScene(sc) as ds:
        _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area lights are not served on the device yet"])
        with gates(gpu, quadric=False, sphere=True):
            _refused(gpu, lambda: gpu.render(ds, rd), [served_only_without])
            _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0)), ["sphere area light", "disk"])
        with gates(gpu, quadric=True, sphere=False):
            _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area light", "rspt_set_sphere_lights"])
            _refused(gpu, lambda: gpu.light_distribution(ds, abi.LIGHTS_POWER, (0, 0.5, 0)), ["sphere area light", "rspt_set_sphere_lights"])
        with gates(gpu, quadric=True, sphere=True):
            li, _ = gpu.render_samples(ds, rd)
            gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, (0, 0.5, 0))
            rd_dl = scenes.make_render_desc(16, 16, 4, LOOK, 45.0, integrator="directlighting")
            _refused(gpu, lambda: gpu.render(ds, rd_dl), ["sphere area light", "directlighting"])
    assert_same_li(li, restated_render(restated, sc, rd)[1])
    # an emissive sphere beside an emissive disk: the quadric gate alone serves the disk and still refuses the sphere
    sc = _plain_room(gpu, ("disk",), sphere_emit=(1.0, 1.0, 1.0))
    with gpu.DeviceScene(sc) as ds:
        with gates(gpu, quadric=False, sphere=True):
            _refused(gpu, lambda: gpu.render(ds, rd), ["disk area light", "not served on the device yet"])
        with gates(gpu, quadric=True, sphere=False):
            _refused(gpu, lambda: gpu.render(ds, rd), ["sphere area light", "rspt_set_sphere_lights"])
        with gates(gpu, quadric=True, sphere=True):
            li, _ = gpu.render_samples(ds, rd)
    assert_same_li(li, restated_render(restated, sc, rd)[1])


def test_a_pure_sphere_light_scene_keeps_its_kernels_whatever_the_quadric_gate_says(gpu, monkeypatch, capfd):
    from tests.test_spherelight_host import sphere_light_room
    sc = sphere_light_room(gpu.bvh_build, "mixed")

    def run():
        with gates(gpu, quadric=True, sphere=True), gpu.DeviceScene(sc) as ds:
            return gpu.render_samples(ds, room_rd(spp=2))[0]
    li, name = shade_instantiation(monkeypatch, capfd, run)
    assert name == "generic-spherelight" and np.nanmean(li) > 0.0
    with gates(gpu, quadric=True, sphere=False), gpu.DeviceScene(sc) as ds:
        _refused(gpu, lambda: gpu.render(ds, room_rd(spp=2)), ["scene with an emissive sphere: sphere area lights are not served on the device yet (path)"])


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_ao_on_a_scene_with_quadric_lights_is_served(gpu, restated, sampler):
    """ao reads no lights: with the gate on, a scene with an emissive disk and cylinder is served and equals the restatement"""
    sc = quadric_light_room(gpu.bvh_build, "shapes")
    rd = scenes.make_render_desc(32, 24, 4, ROOM_LOOK, 60, integrator="ao", ao_samples=4, sampler=sampler)
    with gates(gpu), gpu.DeviceScene(sc) as ds:
        li, _ = gpu.render_samples(ds, rd)
    assert_same_li(li, restated_render(restated, sc, rd)[1])
    assert li.mean() > 0.0
