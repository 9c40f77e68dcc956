"""-m gpu: projection and goniometric lights (ABI 24) in rspt_render under the path integrator, and in rspt_light_distribution.  Every camera
sample's radiance equals the hand restatement tests/maplight_restated.cpp (held to the oracle's own li on scenes without these lights by
tests/test_maplight_host.py) bit for bit; a map-less goniometric light is a point light; the power and spatial tables equal the restated ones;
ao does not see the lights; and what stays out of scope is refused by name.  Both shade instantiations these scenes can take are launched and named
(RSPT_VERBOSE): generic-maplight over the gallery, over textures, static instances, masks, a null surface and an infinite light, and under a lens, a moving camera,
a crop window with a shard and a sample range; all-maplight over dynamic materials and moving instances, and forced onto the gallery."""
import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.test_maplight_host import assert_same_li, build_restated, dynamic_rd, feature_rd, moving_rd, restated_distribution, restated_render
from tests.util import dynamic_maplight_room, film_rmse, light_maps, maplight_feature_room, moving_maplight_room, shade_instantiation

pytestmark = pytest.mark.gpu
F32 = np.float32
LOOK = ((0, 3.0, -6.5), (0, 1.4, 0), (0, 1, 0))
GONIO_AT = (-1.5, 1.8, 0.5)


def gonio_to_world():
    """tilted so that the map's poles (the light's +-y) point at the floor and the back wall's top, and the phi seam (the light's +x, z = 0+-) runs down the back wall"""
    y = np.array([0.1, 0.5, 0.86]); y /= np.linalg.norm(y)
    x = np.array([1.0, -0.3, 0.2]); x -= x.dot(y) * y; x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = x, y, np.cross(x, y)
    return scenes.Transform.translate(GONIO_AT) * scenes.Transform(m.astype(F32))


def maplight_gallery(builder, which="all", point_for_gonio=False):
    """floor, back wall, three boxes (matte, plastic, glass).  which: "all" = a mapped and a map-less light of each kind + one triangle area light;
    "none" = the area light alone; "projection" / "goniometric" / "bare-goniometric" = that light alone"""
    sb = scenes.SceneBuilder()
    grey = sb.add_material(scenes.matte((0.6, 0.6, 0.6)))
    sb.add_quad([(-6, 0, -6), (6, 0, -6), (6, 0, 5), (-6, 0, 5)], grey)
    sb.add_quad([(-6, 0, 5), (6, 0, 5), (6, 7, 5), (-6, 7, 5)], grey)
    sb.add_box((-3.2, 0.0, 0.5), (-1.8, 1.6, 1.9), sb.add_material(scenes.matte((0.7, 0.3, 0.2), sigma=20.0)))
    sb.add_box((-0.7, 0.0, 1.2), (0.7, 2.2, 2.6), sb.add_material(scenes.plastic((0.2, 0.3, 0.6), (0.4, 0.4, 0.4), 0.1)))
    sb.add_box((1.8, 0.0, 0.2), (3.0, 1.3, 1.4), sb.add_material(scenes.glass((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.5)))
    proj, gonio = light_maps()
    if which in ("all", "none"):
        sb.add_mesh(np.array([(-0.8, 6.0, -0.5), (0.8, 6.0, -0.5), (0.0, 6.0, 0.9)], F32), [[0, 1, 2]], grey, emit=(12, 12, 12))      # one triangle: delta and area estimates mix
    if which in ("all", "projection"):
        # in front of the camera, aimed at the foot of the back wall: the frustum's edge crosses the floor, the boxes and the wall, and the floor
        # between camera and projector lies in its back half-space
        sb.add_projection_light((0.5, 2.5, -1.0), (0.0, 1.0, 4.0), (300, 280, 260), fov=35.0, image=proj)
    if which in ("all", "goniometric"):
        sb.add_goniometric_light(gonio_to_world(), (30, 32, 34), image=gonio)
    if which == "all":
        sb.add_projection_light((4.0, 3.0, -1.0), (0.0, 0.5, 2.0), (60, 60, 80), fov=50.0)
    if which in ("all", "bare-goniometric"):
        if point_for_gonio:
            sb.add_point_light((2.5, 3.5, -3.0), (20, 18, 16))
        else:
            sb.add_goniometric_light(scenes.Transform.translate((2.5, 3.5, -3.0)), (20, 18, 16))
    return sb.finish(builder)


@pytest.fixture(scope="module")
def restated():
    return build_restated()


@pytest.fixture(scope="module")
def gallery_scene(gpu):
    return maplight_gallery(gpu.bvh_build)


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


def test_the_gallery_holds_what_it_says(gallery_scene, restated):
    """the geometry the parity cases rely on, from the restated light functions: the projector's frustum edge and back half-space, the goniometric
    light's poles and seam all fall on surfaces the camera sees"""
    sc = gallery_scene
    kinds = list(sc.lights["kind"])
    assert kinds.count(abi.LIGHT_PROJECTION) == 2 and kinds.count(abi.LIGHT_GONIOMETRIC) == 2 and kinds.count(abi.LIGHT_DIFFUSE_AREA) == 1
    assert sorted(int(p) for k, p in zip(kinds, sc.lights["prim"]) if k != abi.LIGHT_DIFFUSE_AREA) == [0, 1, 0xFFFFFFFF, 0xFFFFFFFF]
    import ctypes as C
    ip = kinds.index(abi.LIGHT_PROJECTION)
    pl = sc.lights[ip]["p"][:3].astype(np.float64)
    xs, zs = np.meshgrid(np.linspace(-5.5, 5.5, 45), np.linspace(-5.5, 4.5, 41))
    lit = np.zeros(xs.shape, bool)
    behind = np.zeros(xs.shape, bool)
    w2l = sc.lights[ip]["p"][3:12].reshape(3, 3).astype(np.float64)
    out = np.zeros(3, F32)
    for i in np.ndindex(xs.shape):
        w = np.array([xs[i], 0.0, zs[i]]) - pl
        ww = w.astype(F32)
        assert restated.ml_map(C.addressof(sc.desc), ip, ww.ctypes.data, out.ctypes.data) == 0
        lit[i] = out.max() > 0
        behind[i] = (w2l @ w)[2] < 0
    assert 0.03 < lit.mean() < 0.6 and behind.any() and not (lit & behind).any()
    # the goniometric light's +-y axis (the poles) and +x axis (the seam) meet the floor / the back wall inside the room
    m = gonio_to_world().m[:3, :3].astype(np.float64)
    o = np.array(GONIO_AT)
    for axis, sign in ((1, 1), (1, -1), (0, 1)):
        d = sign * m[:, axis]
        ts = [t for t in ((0.0 - o[1]) / d[1] if d[1] else -1, (5.0 - o[2]) / d[2] if d[2] else -1) if t > 0]
        p = o + min(ts) * d
        assert -6 < p[0] < 6 and -0.01 < p[1] < 7 and -6 < p[2] < 5.01, (axis, sign, p)


@pytest.mark.parametrize("sampler,strategy,depth,batch", [("sobol", abi.LIGHTS_SPATIAL, 7, None), ("halton", abi.LIGHTS_POWER, 5, None),
                                                          ("sobol", abi.LIGHTS_UNIFORM, 3, None), ("sobol", abi.LIGHTS_SPATIAL, 7, 2048)])
def test_gallery_li_equals_restated_li(gpu, restated, gallery_scene, monkeypatch, capfd, sampler, strategy, depth, batch):
    if batch:
        monkeypatch.setenv("RSPT_BATCH", str(batch))      # 48 x 36 x 4 samples in several batches
    rd = scenes.make_render_desc(48, 36, 4, LOOK, 60, max_depth=depth, sampler=sampler, light_strategy=strategy)
    li = parity_on(gpu, restated, gallery_scene, rd, monkeypatch, capfd, "generic-maplight")
    assert np.nanmean(li) > 0.0


# ---- the all-features instantiation (256 VGPRs, one wave per SIMD): a map light next to a dynamic material or a moving instance ----
@pytest.mark.parametrize("sampler,strategy,depth,batch", [("sobol", abi.LIGHTS_SPATIAL, 5, None), ("halton", abi.LIGHTS_POWER, 7, None),      # (depth 7: past the roulette threshold)
                                                          ("sobol", abi.LIGHTS_SPATIAL, 5, 2048)])
def test_dynamic_materials_under_map_lights(gpu, restated, monkeypatch, capfd, sampler, strategy, depth, batch):
    """eight materials whose lobe lists are built per hit under a mapped projection light, a mapped and a map-less goniometric light and an area light; with
    RSPT_BATCH the one-wave kernel runs over several batches"""
    if batch:
        monkeypatch.setenv("RSPT_BATCH", str(batch))
    sc = dynamic_maplight_room(gpu.bvh_build)
    li = parity_on(gpu, restated, sc, dynamic_rd(sampler, strategy, depth), monkeypatch, capfd, "all-maplight")
    assert np.nanmean(li) > 0.0


@pytest.mark.parametrize("mode,dynamic", [("fixed", False), ("reference", False), ("fixed", True)])
def test_moving_instances_under_map_lights(gpu, restated, monkeypatch, capfd, mode, dynamic):
    """moving, turning and static instances of a textured pyramid (shutter 0 .. 1), both instancing behaviours; and next to a dynamic material, which Sobol' serves"""
    sc = moving_maplight_room(gpu.bvh_build, mode, dynamic)
    assert int(sc.instances["animated"].sum()) >= 5
    li = parity_on(gpu, restated, sc, moving_rd(), monkeypatch, capfd, "all-maplight")
    assert np.nanmean(li) > 0.0


def test_all_maplight_forced_on_the_gallery(gpu, restated, gallery_scene, monkeypatch, capfd):
    """RSPT_SHADE_VARIANT=all-maplight on a scene the generic set serves: the same bits as the default render, and as the restated li — the big instantiation
    computes nothing else, whatever a new scene does"""
    rd = scenes.make_render_desc(48, 36, 4, LOOK, 60, max_depth=6)
    default = parity_on(gpu, restated, gallery_scene, rd, monkeypatch, capfd, "generic-maplight")
    monkeypatch.setenv("RSPT_SHADE_VARIANT", "all-maplight")
    forced = parity_on(gpu, restated, gallery_scene, rd, monkeypatch, capfd, "all-maplight")
    assert_same_li(forced, default)


# ---- the generic map-light instantiation over what its gallery lacks ----
@pytest.fixture(scope="module")
def feature_scene(gpu):
    return maplight_feature_room(gpu.bvh_build)


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_feature_room_li_equals_restated_li(gpu, restated, feature_scene, monkeypatch, capfd, sampler):
    """the texture stage, bump, static instances, a null surface in the beam, alpha and shadow-alpha masks, a medium interface, and the map lights' maps behind
    an infinite light's in the pool (envmap indices 1 and 2)"""
    li = parity_on(gpu, restated, feature_scene, feature_rd(sampler), monkeypatch, capfd, "generic-maplight")
    assert np.nanmean(li) > 0.0


def test_feature_room_light_distributions_equal_the_restated_tables(gpu, restated, feature_scene):
    """the map-light table kernels over an infinite light's power and sample_li too"""
    sc = feature_scene
    lo, hi = sc.nodes["bmin"][0], sc.nodes["bmax"][0]
    pts = np.random.default_rng(6).uniform(lo - 0.5, hi + 0.5, (20, 3)).astype(F32)
    with gpu.DeviceScene(sc) as ds:
        f, c, _, _ = gpu.light_distribution(ds, abi.LIGHTS_POWER, pts[0])
        wf, wc, _, _ = restated_distribution(restated, sc, abi.LIGHTS_POWER, pts[0])
        assert np.array_equal(f.view(np.uint32), wf.view(np.uint32)) and np.array_equal(c.view(np.uint32), wc.view(np.uint32)) and f.min() > 0
        for p in pts:
            f, c, nv, vx = gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, p)
            wf, wc, wnv, wvx = restated_distribution(restated, sc, abi.LIGHTS_SPATIAL, p)
            assert list(nv) == list(wnv) and list(vx) == list(wvx)
            assert np.array_equal(f.view(np.uint32), wf.view(np.uint32)) and np.array_equal(c.view(np.uint32), wc.view(np.uint32)), p


# ---- the render description's features over map lights ----
@pytest.mark.parametrize("kw", [dict(lens_radius=0.05, focal_distance=6.0), dict(look_at_end=((0.6, 3.2, -6.2), (0.2, 1.4, 0), (0, 1, 0))),
                                dict(crop=(0.1, 0.85, 0.2, 0.95), shard=(1, 3, 2), sample_range=(1, 2))], ids=["lens", "moving-camera", "crop-shard-range"])
def test_gallery_under_render_features(gpu, restated, gallery_scene, monkeypatch, capfd, kw):
    rd = scenes.make_render_desc(48, 36, 4, LOOK, 60, max_depth=5, **kw)
    li = parity_on(gpu, restated, gallery_scene, rd, monkeypatch, capfd, "generic-maplight")
    assert np.nanmean(li) > 0.0


def test_mapless_goniometric_light_is_a_point_light(gpu):
    """Spectrum(1) * i is i: the same scene with RSPT_LIGHT_POINT at that position and intensity renders the same bits (no restated code involved)"""
    rd = scenes.make_render_desc(48, 36, 4, LOOK, 60, max_depth=5)
    got = []
    for point in (False, True):
        sc = maplight_gallery(gpu.bvh_build, "all", point_for_gonio=point)
        assert (abi.LIGHT_POINT in list(sc.lights["kind"])) == point
        with gpu.DeviceScene(sc) as ds:
            got.append(gpu.render_samples(ds, rd)[0])
    assert_same_li(got[0], got[1])
    assert np.nanmean(got[0]) > 0.0


def test_light_distributions_equal_the_restated_tables(gpu, restated, gallery_scene):
    sc = gallery_scene
    lo, hi = sc.nodes["bmin"][0], sc.nodes["bmax"][0]
    pts = np.random.default_rng(5).uniform(lo - 0.5, hi + 0.5, (40, 3)).astype(F32)
    with gpu.DeviceScene(sc) as ds:
        f, c, _, _ = gpu.light_distribution(ds, abi.LIGHTS_POWER, pts[0])
        wf, wc, _, _ = restated_distribution(restated, sc, abi.LIGHTS_POWER, pts[0])
        assert np.array_equal(f.view(np.uint32), wf.view(np.uint32)) and np.array_equal(c.view(np.uint32), wc.view(np.uint32)) and f.min() > 0
        for p in pts:
            f, c, nv, vx = gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, p)
            wf, wc, wnv, wvx = restated_distribution(restated, sc, abi.LIGHTS_SPATIAL, p)
            assert list(nv) == list(wnv) and list(vx) == list(wvx)
            assert np.array_equal(f.view(np.uint32), wf.view(np.uint32)) and np.array_equal(c.view(np.uint32), wc.view(np.uint32)), p
        f, c, nv, _ = gpu.light_distribution(ds, abi.LIGHTS_UNIFORM, pts[0])
        assert np.array_equal(f, np.ones(5, F32)) and list(nv) == [1, 1, 1]


@pytest.mark.parametrize("which", ["projection", "goniometric"])
def test_only_such_a_light_in_the_scene(gpu, restated, which):
    """n_lights = 1: the strategy is forced to uniform (lightdistrib.rs:397)"""
    sc = maplight_gallery(gpu.bvh_build, which)
    assert int(sc.desc.n_lights) == 1
    rd = scenes.make_render_desc(48, 36, 4, LOOK, 60, max_depth=4, light_strategy=abi.LIGHTS_SPATIAL)
    li = parity(gpu, restated, sc, rd)
    assert np.nanmean(li) > 0.0


@pytest.mark.parametrize("which,integrator,sampler,word", [("projection", "directlighting", "sobol", "directlighting"), ("goniometric", "whitted", "halton", "whitted"),
                                                           ("projection", "volpath", "sobol", "volpath"), ("goniometric", "path", "random", "random")])
def test_out_of_scope_renders_refused(gpu, which, integrator, sampler, word):
    sc = maplight_gallery(gpu.bvh_build, which)
    rd = scenes.make_render_desc(16, 16, 16, LOOK, 45.0, integrator=integrator, sampler=sampler, strat=(4, 4))
    with gpu.DeviceScene(sc) as ds:
        with pytest.raises(gpu.RsptError) as e:
            gpu.render(ds, rd)
        assert e.value.code == abi.E_UNSUPPORTED and which in str(e.value) and word in str(e.value)


def test_on_demand_light_table_refused(gpu, monkeypatch):
    monkeypatch.setenv("RSPT_LIGHT_TABLE_EAGER_BYTES", "0")
    sc = maplight_gallery(gpu.bvh_build, "all")
    rd = scenes.make_render_desc(16, 16, 4, LOOK, 45.0, light_strategy=abi.LIGHTS_SPATIAL)
    with gpu.DeviceScene(sc) as ds:
        with pytest.raises(gpu.RsptError) as e:
            gpu.render(ds, rd)
        assert e.value.code == abi.E_UNSUPPORTED and "projection" in str(e.value) and "goniometric" in str(e.value) and "on-demand" in str(e.value)
        with pytest.raises(gpu.RsptError) as e:
            gpu.light_distribution(ds, abi.LIGHTS_SPATIAL, (0.0, 1.0, 0.0))
        assert e.value.code == abi.E_UNSUPPORTED and "on-demand" in str(e.value)


@pytest.mark.parametrize("kind", [abi.LIGHT_PROJECTION, abi.LIGHT_GONIOMETRIC])
def test_bad_records_are_invalid(gpu, kind):
    name = "projection" if kind == abi.LIGHT_PROJECTION else "goniometric"

    def create(edit):
        sc = maplight_gallery(gpu.bvh_build, name)
        edit(sc.lights[0])
        with pytest.raises(gpu.RsptError) as e:
            gpu.DeviceScene(sc)
        assert e.value.code == abi.E_INVALID and "light 0" in str(e.value) and name in str(e.value)

    def nan_param(lt): lt["p"][4] = np.nan
    def inf_intensity(lt): lt["L"][1] = np.inf
    def prim_out_of_range(lt): lt["prim"] = 1
    create(nan_param)
    create(inf_intensity)
    create(prim_out_of_range)
    if kind == abi.LIGHT_PROJECTION:
        def flipped_bounds(lt): lt["p"][12], lt["p"][14] = lt["p"][14], lt["p"][12]
        create(flipped_bounds)


def test_infinite_light_still_needs_its_distribution(gpu):
    """a map without a distribution is accepted only when nothing but projection / goniometric lights name it"""
    sb = scenes.SceneBuilder()
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], sb.add_material(scenes.matte((0.5, 0.5, 0.5))))
    sb.add_infinite_light((1, 1, 1))
    sc = sb.finish(gpu.bvh_build)
    env = sc._env_structs[0]      # the rspt_envmap the description points at: the same scene, its distribution taken away
    env.dist_func = None
    env.dist_nu = env.dist_nv = 0
    with pytest.raises(gpu.RsptError) as e:
        gpu.DeviceScene(sc)
    assert e.value.code == abi.E_INVALID and "envmap 0" in str(e.value)


def test_ao_does_not_see_the_lights(gpu):
    rd = scenes.make_render_desc(48, 36, 4, LOOK, 60, integrator="ao", ao_samples=4)
    got = []
    for which in ("all", "none"):
        with gpu.DeviceScene(maplight_gallery(gpu.bvh_build, which)) as ds:
            got.append(gpu.render_samples(ds, rd)[0])
    assert_same_li(got[0], got[1])
    assert np.nanmean(got[0]) > 0.0
