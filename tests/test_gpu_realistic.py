"""-m gpu: the realistic camera (ABI 26, camera_kind = 3) in rspt_render under path and ao.  The yardstick is tests/realistic_restated.cpp (held to the
oracle's tile loop, to the library's own setup and to known answers by tests/test_realistic_host.py).  rspt_camera_rays — the device function the raygen
kernel calls — equals the restatement's generate_ray_differential on all 22 floats bit for bit for samples of every arm the CPU scan finds; every camera
sample's radiance from rspt_render_samples equals the yardstick's li bit for bit, the film lies within the project's RMSE bar of 1e-5, no path is cut.
Every frame is 48 x 36 x 4 or smaller; about a quarter of its samples have weight 0 (tests/test_realistic_host.py::test_frame_conditions)."""
import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from rs_pbrt_amd.lib import RsptError
from tests.test_camera_host import LOOK_END, assert_same_li
from tests.test_realistic_host import ARMS, LENSES, build_realistic_restated, lens_desc, real_rays, real_render, scan_samples
from tests.util import GALLERY_LOOK_AT, SKY_LOOK_AT, SPHERE_LOOK_AT, TEXTURED_LOOK_AT, film_rmse, gallery, sky_scene, textured_room

pytestmark = pytest.mark.gpu
LENS_NAMES = sorted(LENSES)


@pytest.fixture(scope="module")
def restated():
    return build_realistic_restated()


@pytest.fixture(scope="module")
def restated_spheres():
    return build_realistic_restated("spheres")


@pytest.fixture(scope="module")
def gallery_scene(gpu):
    return gallery(gpu.bvh_build, "all")


def parity(gpu, restated, sc, rd):
    with gpu.DeviceScene(sc) as ds:
        li, _ = gpu.render_samples(ds, rd)
        film, st = gpu.render(ds, rd)
    want_film, want, w = real_render(restated, sc, rd)
    assert_same_li(li, want)
    assert film_rmse(film, want_film) < 1e-5
    if rd.filter_radius[0] <= 0.5:      # (a wider filter's weights are summed in another order than the tiles')
        assert np.array_equal(film[:, 3], want_film[:, 3])      # a sample of weight 0 still counts with its filter weight
    assert st["truncated_paths"] == 0
    return li, w


# ---- the hook: the device's generate_ray_differential ----
@pytest.mark.parametrize("name", LENS_NAMES)
@pytest.mark.parametrize("mode", ["simple-still", "physical-moving"])
def test_camera_rays_hook(gpu, restated, name, mode):
    """up to 4096 samples of each arm from a 2^20-sample CPU scan (the rare arms: all the scan finds; tests/test_realistic_host.py::test_every_arm_occurs says
    which arms a lens can reach), dead-by-shift samples included; a moving camera with the physical weighting and a shutter of 0 - 0.5, and the still camera
    with the simple weighting"""
    kw = {} if mode == "simple-still" else dict(simple_weighting=False, shutter=(0.0, 0.5), look_at_end=LOOK_END, camera_times=(0.1, 0.45))
    rd = lens_desc(name, **kw)
    smp, _, arms = scan_samples(restated, rd)
    pick = np.concatenate([np.flatnonzero(arms == a)[:4096] for a in range(len(ARMS))])
    assert len(pick) >= 2 * 4096
    want, want_arms = real_rays(restated, rd, smp[pick])
    assert np.array_equal(want_arms, arms[pick])
    got = gpu.camera_rays(rd, smp[pick])
    a, b = got.view(np.uint32), want.view(np.uint32)
    bad = ((a != b) & ~(np.isnan(got) & np.isnan(want))).any(axis=1)
    assert not bad.any(), "%d of %d camera samples differ (arms %s)" % (int(bad.sum()), len(pick), sorted(set(want_arms[bad].tolist())))
    assert (np.isnan(got) == np.isnan(want)).all()
    if mode == "physical-moving":
        assert len(np.unique(got[got[:, 0] > 0, 8])) > 1000 and got[:, 8].max() <= 0.5      # the ray's time: lerp over the shutter


def test_camera_rays_hook_refusals(gpu):
    rd = lens_desc("singlet")
    smp = np.full((4, 5), 0.5, np.float32)
    assert gpu.camera_rays(rd, smp).shape == (4, 22)
    rd.n_exit_pupil_bounds = 0
    with pytest.raises(RsptError) as e:
        gpu.camera_rays(rd, smp)
    assert e.value.code == abi.E_INVALID and "camera_kind" in str(e.value)
    with pytest.raises(RsptError) as e:
        gpu.camera_rays(scenes.make_render_desc(16, 16, 4, GALLERY_LOOK_AT, 60.0), smp)
    assert e.value.code == abi.E_UNSUPPORTED


# ---- renders ----
@pytest.mark.parametrize("name", LENS_NAMES)
@pytest.mark.parametrize("sampler,env", [("sobol", {}), ("halton", {}), ("sobol", {"RSPT_BATCH": "2048"}), ("halton", {"RSPT_BATCH": "2048"}),
                                         ("sobol", {"RSPT_CAMERA_PACKET": "1"}), ("sobol", {"RSPT_CAMERA_PACKET": "0"})],
                         ids=["sobol", "halton", "sobol-batches", "halton-batches", "sobol-packet", "sobol-per-lane"])
def test_path_on_the_gallery(gpu, restated, gallery_scene, monkeypatch, name, sampler, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    li, w = parity(gpu, restated, gallery_scene, lens_desc(name, max_depth=5, sampler=sampler))
    assert np.nanmean(li) > 0.0 and (li[w == 0] == 0).all() and 0.1 < (w == 0).mean() < 0.5


@pytest.mark.parametrize("name", LENS_NAMES)
@pytest.mark.parametrize("schedule", ["move-from-0", "slots"])
def test_path_schedules(gpu, restated, gallery_scene, monkeypatch, name, schedule):
    """a dead slot under the MOVE schedule from the first iteration on (its radiance goes to L_final at once) and under slots for life without the fresh flag"""
    for k, v in ({"RSPT_MOVE_FROM": "0"} if schedule == "move-from-0" else {"RSPT_MOVE": "0", "RSPT_FRESH": "0"}).items():
        monkeypatch.setenv(k, v)
    parity(gpu, restated, gallery_scene, lens_desc(name, max_depth=5))


@pytest.mark.parametrize("name", LENS_NAMES)
@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_ao(gpu, restated, gallery_scene, name, sampler):
    li, w = parity(gpu, restated, gallery_scene, lens_desc(name, integrator="ao", ao_samples=16, sampler=sampler))
    assert 0.0 < np.nanmean(li) < 1.0 and (li[w == 0] == 0).all()


@pytest.mark.parametrize("name", LENS_NAMES)
def test_sky(gpu, restated, name):
    """an infinite light: a vignetted sample that ran li anyway would pick the sky up at bounce 0"""
    sc = sky_scene(gpu.bvh_build)
    li, w = parity(gpu, restated, sc, lens_desc(name, look=SKY_LOOK_AT, max_depth=3))
    assert (li[w == 0] == 0).all() and (li[w > 0].max(axis=-1) > 0).mean() > 0.5


@pytest.mark.parametrize("name", LENS_NAMES)
@pytest.mark.parametrize("trilinear", [False, True], ids=["ewa", "trilinear"])
def test_textured_room(gpu, restated, name, trilinear):
    """image textures under EWA and trilinear filtering, bump maps: the differentials k_raygen_lens stored pick the MIP levels.  The case can tell: the frame
    differs from the yardstick's frame with the differentials dropped in more than 5 % of the samples.  The trilinear cases render 24 x 18: at 48 x 36 the
    singlet's narrow view magnifies every texture, trilinear filtering clamps to level 0 with or without differentials and the case could not tell."""
    sc = textured_room(gpu.bvh_build, trilinear=trilinear)
    rd = lens_desc(name, *((24, 18) if trilinear else (48, 36)), look=TEXTURED_LOOK_AT, max_depth=4)
    li, _ = parity(gpu, restated, sc, rd)
    _, flat, _ = real_render(restated, sc, rd, zero_diff=True)
    differs = (li.reshape(-1, 3).view(np.uint32) != flat.reshape(-1, 3).view(np.uint32)).any(axis=-1).mean()
    assert differs > 0.05, "dropping the differentials changes %.1f %% of the samples only" % (100 * differs)


@pytest.mark.parametrize("name", LENS_NAMES)
@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_moving_camera(gpu, restated, gallery_scene, name, sampler):
    rd = lens_desc(name, max_depth=3, sampler=sampler, look_at_end=LOOK_END, camera_times=(0.2, 0.85), shutter=(0.0, 1.0))
    li, _ = parity(gpu, restated, gallery_scene, rd)
    with gpu.DeviceScene(gallery_scene) as ds:
        still, _ = gpu.render_samples(ds, lens_desc(name, max_depth=3, sampler=sampler))
    assert not np.array_equal(li, still)


@pytest.mark.parametrize("name", LENS_NAMES)
def test_moving_camera_over_textures(gpu, restated, name):
    sc = textured_room(gpu.bvh_build, trilinear=False)
    parity(gpu, restated, sc, lens_desc(name, look=TEXTURED_LOOK_AT, max_depth=3, look_at_end=((0.4, 2.8, -4.4), (0.2, 1.5, 2), (0.05, 1, 0)), camera_times=(0.2, 0.85)))


@pytest.mark.parametrize("name", LENS_NAMES)
def test_crop_shard_and_sample_range(gpu, restated, gallery_scene, name):
    rd = lens_desc(name, max_depth=3, crop=(0.1, 0.85, 0.2, 0.95), shard=(1, 2, 1), sample_range=(1, 2))
    li, _ = parity(gpu, restated, gallery_scene, rd)
    assert np.nanmean(li) > 0.0 and (li[:, 0] == 0).all() and (li[:, 3] == 0).all()      # samples outside the range stay unwritten


@pytest.mark.parametrize("name", LENS_NAMES)
@pytest.mark.parametrize("integrator", ["path", "ao"])
def test_gaussian_filter(gpu, restated, gallery_scene, name, integrator):
    """radius 2: k_film_gather, where the ray weight is folded into the staged radiance"""
    rd = lens_desc(name, max_depth=3, integrator=integrator, ao_samples=8, filter_radius=(2.0, 2.0), filter_table=scenes.gaussian_filter_table((2.0, 2.0), 2.0))
    parity(gpu, restated, gallery_scene, rd)


@pytest.mark.parametrize("name", LENS_NAMES)
def test_physical_weighting(gpu, restated, gallery_scene, name):
    """simple_weighting off with a shutter of 0 - 0.5: the weight carries (shutter_close - shutter_open) / lens_rear_z^2"""
    rd = lens_desc(name, max_depth=3, simple_weighting=False, shutter=(0.0, 0.5))
    _, w = parity(gpu, restated, gallery_scene, rd)
    _, _, w_simple = real_render(restated, gallery_scene, lens_desc(name, max_depth=3))
    assert ((w > 0) == (w_simple > 0)).all() and not np.array_equal(w, w_simple)


@pytest.mark.parametrize("name", LENS_NAMES)
def test_analytic_spheres(gpu, restated_spheres, name):
    from tests.test_gpu_sphere_render import sphere_gallery
    sc = sphere_gallery(gpu.bvh_build)
    li, _ = parity(gpu, restated_spheres, sc, lens_desc(name, look=SPHERE_LOOK_AT, max_depth=5))
    assert np.nanmean(li) > 0.0


# ---- independent of the yardstick's li ----
@pytest.mark.parametrize("name", LENS_NAMES)
@pytest.mark.parametrize("integrator", ["path"])
def test_furnace(gpu, restated, name, integrator):
    """a closed box whose walls all emit L, max_depth = 0: every sample's li is exactly L or exactly 0, and the zeros are the samples the restatement gives weight 0"""
    L = (0.75, 1.5, 3.0)
    sc = furnace_box(gpu.bvh_build, L)
    look = ((0.2, -0.1, 0.3), (1.0, 0.4, 2.0), (0.1, 1.0, 0.0))
    rd = lens_desc(name, look=look, max_depth=0, integrator=integrator)
    with gpu.DeviceScene(sc) as ds:
        li, st = gpu.render_samples(ds, rd)
    assert st["nan_samples"] == 0
    _, _, w = real_render(restated, sc, rd)
    lit, black = (li == np.array(L, np.float32)).all(axis=-1), (li == 0).all(axis=-1)
    assert (lit | black).all()
    assert np.array_equal(black, w == 0) and 0.1 < black.mean() < 0.5


def furnace_box(builder, L, lo=(-2.0, -1.5, -3.0), hi=(2.5, 1.0, 2.0)):
    sb = scenes.SceneBuilder()
    m = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    for quad in ([(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)], [(x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)],
                 [(x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)], [(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)],
                 [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)], [(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]):
        sb.add_quad(quad, m, emit=L, two_sided=True)
    return sb.finish(builder)


# ---- refusals ----
@pytest.mark.parametrize("what,kw", [("volpath", dict(integrator="volpath")), ("directlighting", dict(integrator="directlighting", max_depth=3)),
                                     ("whitted", dict(integrator="whitted", max_depth=3)), ("02sequence", dict(sampler="02sequence"))])
def test_refused_by_name(gpu, gallery_scene, what, kw):
    rd = lens_desc("dgauss50", 32, 32, **kw)
    good = lens_desc("dgauss50", 32, 32)
    with gpu.DeviceScene(gallery_scene) as ds:
        for call in (lambda: gpu.render(ds, rd), lambda: gpu.render_samples(ds, rd)):
            with pytest.raises(RsptError) as e:
                call()
            assert e.value.code == abi.E_UNSUPPORTED and "realistic camera" in str(e.value) and what in str(e.value)
        film, _ = gpu.render(ds, good)      # and a correct render works right after
        assert film[:, 3].min() > 0


@pytest.mark.parametrize("what", ["no-elements", "no-bounds", "too-many-elements", "full-res", "film-diagonal"])
def test_bad_tables_are_refused_by_name(gpu, gallery_scene, what):
    rd = lens_desc("singlet", 16, 16)
    if what == "no-elements":
        rd.n_lens_elements = 0
    elif what == "no-bounds":
        rd.exit_pupil_bounds = None
    elif what == "too-many-elements":
        rd.n_lens_elements = abi.MAX_LENS_ELEMENTS + 1
    elif what == "full-res":
        rd.full_res[0] = 0
    else:
        rd.film_diagonal = 0.0
    with gpu.DeviceScene(gallery_scene) as ds:
        for call in (lambda: gpu.render(ds, rd), lambda: gpu.render_samples(ds, rd)):
            with pytest.raises(RsptError) as e:
                call()
            assert e.value.code == abi.E_INVALID and "camera_kind" in str(e.value)
        buf = gpu.DeviceBuffer(scenes.n_pixels(rd) * 16)
        try:
            with pytest.raises(RsptError) as e:
                gpu.render_device(ds, rd, buf.ptr)
            assert e.value.code == abi.E_INVALID and "camera_kind" in str(e.value)
        finally:
            buf.free()
        gpu.render(ds, lens_desc("singlet", 16, 16))
    rd4 = lens_desc("singlet", 16, 16)
    rd4.camera_kind = 4
    with gpu.DeviceScene(gallery_scene) as ds:
        with pytest.raises(RsptError) as e:
            gpu.render(ds, rd4)
        assert e.value.code == abi.E_INVALID and "camera_kind" in str(e.value)


# ---- the other cameras keep their bits ----
def test_perspective_camera_keeps_its_bits(gpu, oracle):
    """camera_kind = 0 after the film kernels learnt the ray weight and PathBuf grew two pointers: a lens, a moving camera and textures against the ORACLE,
    bit for bit, under the box filter and under a wider one (k_film_gather)"""
    sc = textured_room(gpu.bvh_build, trilinear=False)
    for fr in ((0.5, 0.5), (1.5, 1.5)):
        rd = scenes.make_render_desc(48, 36, 4, TEXTURED_LOOK_AT, 55.0, max_depth=4, lens_radius=0.05, focal_distance=6.0, filter_radius=fr,
                                     look_at_end=((0.4, 2.8, -4.4), (0.2, 1.5, 2), (0.05, 1, 0)), camera_times=(0.2, 0.85), shutter=(0.0, 1.0))
        assert rd.camera_kind == abi.CAMERA_PERSPECTIVE
        with gpu.DeviceScene(sc) as ds:
            li, _ = gpu.render_samples(ds, rd)
            film, _ = gpu.render(ds, rd)
        ref = oracle.render(sc, rd, threads=4, want_li=True)
        assert_same_li(li, ref["li"])
        assert film_rmse(film, ref["film"]) < 1e-5
