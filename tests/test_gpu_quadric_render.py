"""-m gpu: disks and cylinders as surfaces in rspt_render (ABI 27) — the path and AO integrators under Sobol' and Halton.  Every camera sample's
radiance equals the hand restatement of PathIntegrator::li / AOIntegrator::li over a scene view that intersects all four primitive kinds
(tests/quadric_render_restated.cpp; tests/test_quadric_render_host.py holds it to the oracle's li and to the sphere restatement, tests/test_quadric_host.py
holds the two shapes' intersect to closed-form answers) bit for bit; a disk no ray reaches changes nothing; a disk casts its closed-form shadow; and what
stays out of scope is refused by name.  Both quadric instantiations of the shade stage are launched and named (RSPT_VERBOSE)."""
import ctypes as C
import math

import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.test_quadric_render_host import QUADRIC_LOOK, build_quadric_render_restated, dynamic_quadric_room, quadric_gallery, restated_render
from tests.test_sphere_render_host import assert_same_li
from tests.util import film_rmse, shade_instantiation, xf

pytestmark = pytest.mark.gpu
F32 = np.float32
LOOK = QUADRIC_LOOK


@pytest.fixture(scope="module")
def restated():
    return build_quadric_render_restated()


@pytest.fixture(scope="module")
def gallery_scene(gpu):
    return quadric_gallery(gpu.bvh_build)


def parity(gpu, restated, sc, rd, rmse=1e-5):
    with gpu.DeviceScene(sc) as ds:
        li, _ = gpu.render_samples(ds, rd)
        film, _ = gpu.render(ds, rd)
    want_film, want = restated_render(restated, sc, rd)
    assert_same_li(li, want)
    assert film_rmse(film, want_film) < rmse
    return li


def parity_on(gpu, restated, sc, rd, monkeypatch, capfd, kernel):
    """parity() by the shade instantiation named `kernel`: a scene that quietly takes another one fails"""
    li, name = shade_instantiation(monkeypatch, capfd, lambda: parity(gpu, restated, sc, rd))
    assert name == kernel
    return li


@pytest.mark.parametrize("depth", [1, 5])
@pytest.mark.parametrize("strategy", [abi.LIGHTS_SPATIAL, abi.LIGHTS_POWER, abi.LIGHTS_UNIFORM])
@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("integrator", ["path", "ao"])
def test_gallery_li_equals_restated_li(gpu, restated, gallery_scene, monkeypatch, capfd, integrator, sampler, strategy, depth):
    rd = scenes.make_render_desc(32, 24, 4, LOOK, 60, max_depth=depth, sampler=sampler, integrator=integrator, light_strategy=strategy, ao_samples=4)
    if integrator == "path":
        li = parity_on(gpu, restated, gallery_scene, rd, monkeypatch, capfd, "generic-quadric")
    else:   # (ao has its own kernels: the shade stage does not run)
        li = parity(gpu, restated, gallery_scene, rd)
    assert np.nanmean(li) > 0.0


@pytest.mark.parametrize("lights,sampler", [("delta", "sobol"), ("area", "halton"), ("sky", "sobol")])
def test_gallery_under_each_kind_of_light(gpu, restated, monkeypatch, capfd, lights, sampler):
    sc = quadric_gallery(gpu.bvh_build, lights)
    rd = scenes.make_render_desc(32, 24, 4, LOOK, 60, max_depth=6, sampler=sampler)
    assert np.nanmean(parity_on(gpu, restated, sc, rd, monkeypatch, capfd, "generic-quadric")) > 0.0


@pytest.mark.parametrize("sampler,strategy,depth,batch", [("sobol", abi.LIGHTS_SPATIAL, 5, None), ("halton", abi.LIGHTS_POWER, 4, 512)])
def test_dynamic_materials_on_disks_and_cylinders(gpu, restated, monkeypatch, capfd, sampler, strategy, depth, batch):
    """dynamic recipes (a lobe list built per hit) and image textures through the uv of cylinders and disks: dynamic-quadric, over several batches too"""
    if batch:
        monkeypatch.setenv("RSPT_BATCH", str(batch))
    sc = dynamic_quadric_room(gpu.bvh_build)
    assert len(sc.disks) == 2 and len(sc.cylinders) == 4
    rd = scenes.make_render_desc(32, 24, 4, ((0, 2.2, -6.5), (0, 1.0, 0), (0, 1, 0)), 60, max_depth=depth, sampler=sampler, light_strategy=strategy)
    assert np.nanmean(parity_on(gpu, restated, sc, rd, monkeypatch, capfd, "dynamic-quadric")) > 0.0


def test_dynamic_quadric_forced_on_the_gallery(gpu, restated, gallery_scene, monkeypatch, capfd):
    """RSPT_SHADE_VARIANT=dynamic-quadric on a scene the generic quadric set serves: the same bits"""
    rd = scenes.make_render_desc(32, 24, 4, LOOK, 60, max_depth=5)
    default = parity_on(gpu, restated, gallery_scene, rd, monkeypatch, capfd, "generic-quadric")
    monkeypatch.setenv("RSPT_SHADE_VARIANT", "dynamic-quadric")
    forced = parity_on(gpu, restated, gallery_scene, rd, monkeypatch, capfd, "dynamic-quadric")
    assert_same_li(forced, default)


def test_camera_inside_a_cylinder(gpu, restated):
    sc = quadric_gallery(gpu.bvh_build, "all", camera_inside=True)
    rd = scenes.make_render_desc(32, 24, 4, LOOK, 70, max_depth=5)
    li = parity(gpu, restated, sc, rd)
    plain = restated_render(restated, quadric_gallery(gpu.bvh_build, "all"), rd)[1]
    assert float((li.view(np.uint32) != plain.view(np.uint32)).any(axis=-1).mean()) > 0.3      # the wall around the camera fills much of the frame


def test_null_material_disk_lets_rays_through(gpu, restated, gallery_scene):
    """the gallery's disk without a material stands between the camera and the room (tests/test_quadric_render_host.py counts the camera rays that meet it):
    the pass-through spends no bounce, so with max_depth 1 the room behind it is still lit, and the frame is the frame of the gallery without that disk up to
    the differentials the re-spawned rays lost (texture filtering only)"""
    sc = gallery_scene
    assert ((sc.prims["mesh"] == abi.MESH_DISK) & (sc.prims["material"] == abi.NO_MATERIAL)).sum() == 1
    rd = scenes.make_render_desc(32, 24, 4, LOOK, 60, max_depth=1)
    li = parity(gpu, restated, sc, rd)
    without = parity(gpu, restated, quadric_gallery(gpu.bvh_build, null_disk=False), rd)
    assert np.nanmean(li) > 0.0 and np.nanmean(np.abs(li - without)) < 0.05 * np.nanmean(without)


@pytest.mark.parametrize("streams", ["1", "2"])
def test_batches_and_trace_streams(gpu, restated, gallery_scene, monkeypatch, streams):
    """a batch too small for the frame (two batches), with the shadow-ray launch on the main stream (1) or on its own (2)"""
    rd = scenes.make_render_desc(32, 24, 8, LOOK, 60, max_depth=5)
    monkeypatch.setenv("RSPT_BATCH", str(32 * 24 * 4))
    monkeypatch.setenv("RSPT_TRACE_STREAMS", streams)
    parity(gpu, restated, gallery_scene, rd)


def test_crop_shard_and_sample_range(gpu, restated, gallery_scene, monkeypatch, capfd):
    rd = scenes.make_render_desc(32, 24, 4, LOOK, 60, max_depth=5, crop=(0.1, 0.85, 0.2, 0.95), shard=(1, 3, 2), sample_range=(1, 2))
    assert np.nanmean(parity_on(gpu, restated, gallery_scene, rd, monkeypatch, capfd, "generic-quadric")) > 0.0


# ---- behaviour ----
@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_a_disk_no_ray_reaches_changes_nothing(gpu, sampler):
    """a disk inside the closed capped cylinder: every sample equals the same scene's without it, bit for bit.  The scene without it keeps the very same
    tree: the disk's primitive becomes a degenerate triangle, which no ray can hit (its record stays in disks[], unnamed)."""
    rd = scenes.make_render_desc(32, 24, 8, LOOK, 60, max_depth=5, sampler=sampler)
    with_disk = quadric_gallery(gpu.bvh_build, hidden_disk=True)
    without = quadric_gallery(gpu.bvh_build, hidden_disk=True)
    assert len(with_disk.disks) == len(quadric_gallery(gpu.bvh_build).disks) + 1
    k = np.nonzero((without.prims["mesh"] == abi.MESH_DISK) & (without.prims["v"][:, 0] == 2))[0]      # (declared third: behind the two caps)
    assert len(k) == 1 and without.disks["radius"][2] == F32(0.4)
    without.prims["mesh"][k[0]] = 0
    without.prims["v"][k[0]] = 0
    out = []
    for sc in (without, with_disk):
        with gpu.DeviceScene(sc) as ds:
            out.append(gpu.render_samples(ds, rd)[0])
    assert out[0].mean() > 0.01
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))


def test_analytic_shadow_of_a_disk(gpu):
    """path, max_depth 1, a matte plane lit by a point light straight above a horizontal disk, seen from straight above, one sample per pixel.
    The disk's shadow on the plane is the disk of radius R h / (h - cy) around the light's foot; the part of the plane it hides from the camera is the disk of
    radius R H / (H - cy).  Every pixel whose point lies inside the shadow and outside the hidden part gets exactly 0; every pixel outside the shadow equals
    the disk-free render bit for bit; every pixel inside the hidden part sees the disk's lit top.  Only samples within one pixel footprint of either edge are left out."""
    h, R, cy, H, W, HT, fov = 6.0, 1.0, 4.5, 12.0, 32, 24, 50.0

    def scene(with_disk):
        sb = scenes.SceneBuilder()
        g = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
        sb.add_quad([(-9, 0, -9), (9, 0, -9), (9, 0, 9), (-9, 0, 9)], g)
        sb.add_point_light((0.0, h, 0.0), (40, 40, 40))
        if with_disk:
            sb.add_disk(radius=R, object_to_world=xf((0.0, cy, 0.0), (1, 0, 0), -90), material=g)
        return sb.finish(gpu.bvh_build)

    rd = scenes.make_render_desc(W, HT, 1, ((0, H, 0), (0, 0, 0), (0, 0, 1)), fov, max_depth=1, sample_at_pixel_center=True)
    free, occ = [], []
    for with_disk, out in ((False, free), (True, occ)):
        with gpu.DeviceScene(scene(with_disk)) as ds:
            out.append(gpu.render_samples(ds, rd)[0][:, 0, :])
    free, occ = free[0], occ[0]
    # a point light over a Lambertian plane: radiance ~ h / r^3, so the horizontal distance of a sample's shading point from the light's foot follows from its
    # radiance relative to the brightest sample's (as tests/test_gpu_sphere_render.py places its pixels); the camera stands over the same foot, so the same
    # distance places the sample's view ray.  The brightest sample lies within a pixel of the foot, r0 <= foot: the recovered distance is short of the true one
    # by at most r0^2 / rho, a small part of the one-footprint margin below for every rho the masks keep.
    foot = 2.0 * H * math.tan(math.radians(fov) / 2) / HT      # a pixel's footprint on the plane (the field of view spans the frame's shorter side)
    y = free.astype(np.float64).sum(-1)
    assert y.min() > 0
    rho = np.sqrt(np.maximum(h * h * ((y.max() / y) ** (2.0 / 3.0) - 1.0), 0.0))
    assert 5.0 < rho.max() < 9.0 * math.sqrt(2)                # the frame's corners lie on the plane
    rho_shadow = h * R / (h - cy)
    rho_hidden = H * R / (H - cy)
    ring = (rho > rho_hidden + foot) & (rho < rho_shadow - foot)
    outer = rho > rho_shadow + foot
    inner = rho < rho_hidden - foot
    assert ring.sum() > 40 and outer.sum() > 300 and inner.sum() >= 4
    assert np.all(occ[ring] == 0.0) and np.all(free[ring] > 0.0)
    assert np.array_equal(occ[outer].view(np.uint32), free[outer].view(np.uint32))
    assert np.all(occ[inner].sum(-1) > free[inner].sum(-1))       # the disk's top is nearer the light than the plane behind it


def test_light_distribution_served_on_the_gallery(gpu, oracle, gallery_scene):
    """no disk or cylinder is a light: the hook serves the scene, and its voxel tables equal the oracle's, which needs only bounds and lights there (the
    world bound is the BVH root's, every shape included)"""
    sc = gallery_scene
    rd = scenes.make_render_desc(32, 24, 1, LOOK, 60)
    nl = int(sc.desc.n_lights)
    lo, hi = sc.nodes["bmin"][0], sc.nodes["bmax"][0]
    pts = np.random.default_rng(4).uniform(lo - 0.5, hi + 0.5, (40, 3)).astype(F32)
    with gpu.DeviceScene(sc) as ds:
        for p in pts:
            f, c, nv, vx = gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, p)
            of, oc, onv = np.zeros(nl, F32), np.zeros(nl + 1, F32), (C.c_int32 * 3)()
            oracle.lib().orc_spatial_voxel(C.addressof(sc.desc), C.addressof(rd), (C.c_int32 * 3)(*map(int, vx)), of.ctypes.data, oc.ctypes.data, onv)
            assert list(nv) == list(onv) and np.array_equal(f, of) and np.array_equal(c, oc)
        f, c, _, _ = gpu.light_distribution(ds, abi.LIGHTS_POWER, pts[0])
        assert f.min() > 0 and c[0] == 0 and abs(c[-1] - 1) < 1e-6


# ---- refusals ----
def _room(gpu, shapes, emit=None, maplight=False):
    sb = scenes.SceneBuilder()
    mat = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], mat)
    sb.add_quad([(-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1)], mat, emit=(5, 5, 5))
    sb.add_point_light((2, 3, -2), (4, 4, 4))
    if "disk" in shapes:
        sb.add_disk(radius=1.0, object_to_world=xf((-1.5, 1, 0), (1, 0, 0), -90), material=mat, emit=emit)
    if "cylinder" in shapes:
        sb.add_cylinder(radius=0.5, zmin=0.0, zmax=1.0, object_to_world=xf((1.5, 0, 0), (1, 0, 0), -90), material=mat, emit=emit)
    if maplight:
        sb.add_projection_light((0, 4, -3), (0, 0, 0), (30, 30, 30), fov=40.0)
    return sb.finish(gpu.bvh_build)


def _names(shapes):
    return [s for s in ("disk", "cylinder") if s in shapes]


def _refused(gpu, call, words):
    with pytest.raises(gpu.RsptError) as e:
        call()
    assert e.value.code == abi.E_UNSUPPORTED, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.parametrize("shapes", ["disk", "cylinder", "disk cylinder"])
@pytest.mark.parametrize("integrator", ["path", "ao", "directlighting", "whitted", "volpath"])
def test_emissive_ones_refused_everywhere(gpu, shapes, integrator):
    sc = _room(gpu, shapes, emit=(1.0, 1.0, 1.0))
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0, integrator=integrator)
    with gpu.DeviceScene(sc) as ds:
        _refused(gpu, lambda: gpu.render(ds, rd), ["%s area light" % n for n in _names(shapes)])
        if integrator == "path":
            for strategy in (abi.LIGHTS_POWER, abi.LIGHTS_SPATIAL, abi.LIGHTS_UNIFORM):
                _refused(gpu, lambda: gpu.light_distribution(ds, strategy, (0.0, 0.5, 0.0)), ["%s area light" % n for n in _names(shapes)])


@pytest.mark.parametrize("shapes", ["disk", "cylinder", "disk cylinder"])
@pytest.mark.parametrize("integrator,sampler,word", [("directlighting", "sobol", "directlighting"), ("whitted", "halton", "whitted"), ("volpath", "sobol", "volpath"),
                                                     ("path", "random", "random"), ("path", "02sequence", "02sequence"), ("ao", "stratified", "stratified"),
                                                     ("path", "maxmindist", "maxmindist")])
def test_out_of_scope_renders_refused(gpu, shapes, integrator, sampler, word):
    sc = _room(gpu, shapes)
    rd = scenes.make_render_desc(16, 16, 16, LOOK, 45.0, integrator=integrator, sampler=sampler, strat=(4, 4))
    with gpu.DeviceScene(sc) as ds:
        _refused(gpu, lambda: gpu.render(ds, rd), _names(shapes) + [word])


@pytest.mark.parametrize("shapes", ["disk", "cylinder"])
def test_maplight_on_demand_table_and_counters_refused(gpu, shapes, monkeypatch):
    """a projection light beside them; a spatial light table that would be built on demand; RSPT_COUNTERS.  (The fourth refusal of this kind — more four-box
    records than a reference holds, 2^25 — needs a scene no quick test can build; spheres have none either.)"""
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0, light_strategy=abi.LIGHTS_SPATIAL)
    with gpu.DeviceScene(_room(gpu, shapes, maplight=True)) as ds:
        _refused(gpu, lambda: gpu.render(ds, rd), [shapes, "projection"])
    with gpu.DeviceScene(_room(gpu, shapes)) as ds:
        monkeypatch.setenv("RSPT_LIGHT_TABLE_EAGER_BYTES", "0")
        _refused(gpu, lambda: gpu.render(ds, rd), [shapes, "on-demand"])
        monkeypatch.delenv("RSPT_LIGHT_TABLE_EAGER_BYTES")
        monkeypatch.setenv("RSPT_COUNTERS", "1")
        _refused(gpu, lambda: gpu.render(ds, rd), [shapes, "RSPT_COUNTERS"])
        monkeypatch.delenv("RSPT_COUNTERS")
    with gpu.DeviceScene(_room(gpu, shapes)) as ds:      # (a fresh scene: the one above keeps the on-demand table it was refused with)
        film, _ = gpu.render(ds, rd)
    assert film[:, 3].sum() > 0


def test_sphere_only_scene_keeps_its_wording(gpu):
    """a scene with spheres and no disk or cylinder is answered as before: the sphere refusal, the sphere instantiation's name"""
    sb = scenes.SceneBuilder()
    mat = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], mat)
    sb.add_point_light((2, 3, -2), (4, 4, 4))
    sb.add_sphere(1.0, object_to_world=xf((0, 1, 0)), material=mat)
    sc = sb.finish(gpu.bvh_build)
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0, integrator="whitted")
    with gpu.DeviceScene(sc) as ds:
        with pytest.raises(gpu.RsptError) as e:
            gpu.render(ds, rd)
    assert str(e.value).endswith("scene with spheres under the whitted integrator: spheres are served by path and ao only") and "disk" not in str(e.value)
