"""-m gpu: WhittedIntegrator on the GPU (src/integrators/whitted.rs) against the oracle's restatement (oracle/orc_render.hpp recursive_li,
whitted branch; pyoracle.render_integrator(.., "whitted")).  The wavefront form (direct.h, WH instantiations) and the per-lane forms
(dl_serial.h DlSerial<.., WH> under lane_serial.h and tile_serial.h) both.

The oracle computes the light term as (f * li) * Spectrum(|cos| / pdf); whitted.rs:93 reads ((f * li) * |cos|) / pdf, which the device
follows.  Where every light has pdf == 1 (point / spot / distant lights) the two are the same bits and the device must equal the oracle
exactly; with area and infinite lights they differ in the last bit of some terms, and the bound below is what is asked."""
import os

import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.util import GALLERY_LOOK_AT, SKY_LOOK_AT, TEXTURED_LOOK_AT, gallery, sky_scene, textured_room

pytestmark = pytest.mark.gpu

REL = 2.0 ** -20
CORNELL_LOOK_AT = ((278, 273, -800), (278, 273, 0), (0, 1, 0))


def render_pair(gpu, oracle, sc, rd):
    with gpu.DeviceScene(sc) as ds:
        film, st = gpu.render(ds, rd)
        li, _ = gpu.render_samples(ds, rd)
    ref = oracle.render_integrator(sc, rd, "whitted", threads=8, want_li=True)
    assert st["samples"] == ref["counters"]["samples"] and st["nan_samples"] == 0
    assert np.array_equal(film[:, 3], ref["film"][:, 3])   # filter-weight sums
    return film, li, ref


def check_exact(gpu, oracle, sc, rd):
    film, li, ref = render_pair(gpu, oracle, sc, rd)
    assert np.array_equal(li, ref["li"])   # every camera sample's radiance, bit for bit
    return li


def check_bounded(gpu, oracle, sc, rd):
    film, li, ref = render_pair(gpu, oracle, sc, rd)
    assert np.isfinite(li).all()
    assert (np.abs(li.astype(np.float64) - ref["li"]) <= REL * np.abs(ref["li"].astype(np.float64))).all()
    return li, ref


def point_lit_glass_cornell(builder, area=False):
    """Cornell box whose blocks are a mirror and a two-lobe glass (reflection AND transmission children), lit by a point light only
    (area=True: and by the ceiling's area light)"""
    sb = scenes.SceneBuilder()
    white = sb.add_material(scenes.matte((0.725, 0.71, 0.68)))
    red = sb.add_material(scenes.matte((0.63, 0.065, 0.05)))
    mir = sb.add_material(scenes.mirror())
    gls = sb.add_material(scenes.glass(multiple_lobes=False))
    q = sb.add_quad
    q([(552.8, 0, 0), (0, 0, 0), (0, 0, 559.2), (549.6, 0, 559.2)], white)
    q([(556, 548.8, 0), (556, 548.8, 559.2), (0, 548.8, 559.2), (0, 548.8, 0)], white)
    q([(549.6, 0, 559.2), (0, 0, 559.2), (0, 548.8, 559.2), (556, 548.8, 559.2)], white)
    q([(0, 0, 559.2), (0, 0, 0), (0, 548.8, 0), (0, 548.8, 559.2)], red)
    q([(552.8, 0, 0), (549.6, 0, 559.2), (556, 548.8, 559.2), (556, 548.8, 0)], red)
    if area:
        q([(343, 548.7, 227), (343, 548.7, 332), (213, 548.7, 332), (213, 548.7, 227)], white, emit=(17, 12, 4))
    for quads, m in (([[(130, 165, 65), (82, 165, 225), (240, 165, 272), (290, 165, 114)], [(290, 0, 114), (290, 165, 114), (240, 165, 272), (240, 0, 272)],
                       [(130, 0, 65), (130, 165, 65), (290, 165, 114), (290, 0, 114)], [(82, 0, 225), (82, 165, 225), (130, 165, 65), (130, 0, 65)],
                       [(240, 0, 272), (240, 165, 272), (82, 165, 225), (82, 0, 225)]], gls),
                     ([[(423, 330, 247), (265, 330, 296), (314, 330, 456), (472, 330, 406)], [(423, 0, 247), (423, 330, 247), (472, 330, 406), (472, 0, 406)],
                       [(472, 0, 406), (472, 330, 406), (314, 330, 456), (314, 0, 456)], [(314, 0, 456), (314, 330, 456), (265, 330, 296), (265, 0, 296)],
                       [(265, 0, 296), (265, 330, 296), (423, 330, 247), (423, 0, 247)]], mir)):
        for p in quads:
            q(p, m)
    sb.add_point_light((278, 400, 100), (60000, 60000, 50000))
    return sb.finish(builder)


def whitted_desc(xres, yres, spp, look_at, fov, sc, **kw):
    return scenes.make_render_desc(xres, yres, spp, look_at, fov, integrator="whitted", light_samples=[1] * sc.desc.n_lights, **kw)


@pytest.mark.parametrize("form", ["wavefront", "lane"])
@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("depth", [1, 3, 5])
def test_delta_lights_bit_exact(gpu, oracle, form, sampler, depth, monkeypatch):
    """point, spot and distant lights have pdf == 1: the text's association and the oracle's give the same bits"""
    if form == "lane":
        monkeypatch.setenv("RSPT_DL_FORM", "lane")
    sc = gallery(gpu.bvh_build, "delta")
    check_exact(gpu, oracle, sc, whitted_desc(32, 24, 4, GALLERY_LOOK_AT, 60.0, sc, max_depth=depth, sampler=sampler))
    sc = point_lit_glass_cornell(gpu.bvh_build)
    li = check_exact(gpu, oracle, sc, whitted_desc(32, 32, 4, CORNELL_LOOK_AT, 40.0, sc, max_depth=depth, sampler=sampler))
    assert li[..., 1].mean() > 0.001


def test_area_and_infinite_lights(gpu, oracle, monkeypatch):
    """within 2^-20 of the oracle per sample and channel; the two device forms agree bit for bit.  On the Cornell box NOT every sample equals
    the oracle's: the device computes ((f * li) * |cos|) / pdf as whitted.rs:93 reads, the oracle (f * li) * (|cos| / pdf)
    (orc_render.hpp:1385), and with an area light's pdf != 1 the two round apart — this is what shows the device follows the text."""
    cases = []
    sc = scenes.cornell_box(gpu.bvh_build)
    cases.append(("cornell", sc, whitted_desc(40, 40, 8, CORNELL_LOOK_AT, 40.0, sc)))
    for kind in ("constant", "map"):
        sc = sky_scene(gpu.bvh_build, kind)
        cases.append((kind, sc, whitted_desc(40, 30, 4, SKY_LOOK_AT, 50.0, sc, max_depth=4)))
    sc = gallery(gpu.bvh_build, "all")
    cases.append(("gallery", sc, whitted_desc(32, 24, 4, GALLERY_LOOK_AT, 60.0, sc, max_depth=3)))
    sc = point_lit_glass_cornell(gpu.bvh_build, area=True)
    cases.append(("glass", sc, whitted_desc(32, 32, 4, CORNELL_LOOK_AT, 40.0, sc, sampler="halton")))
    for name, sc, rd in cases:
        monkeypatch.delenv("RSPT_DL_FORM", raising=False)
        li, ref = check_bounded(gpu, oracle, sc, rd)
        if name == "cornell":
            assert not np.array_equal(li, ref["li"]), "every sample equals the oracle's association"
        monkeypatch.setenv("RSPT_DL_FORM", "lane")
        with gpu.DeviceScene(sc) as ds:
            li_lane, _ = gpu.render_samples(ds, rd)
        assert np.array_equal(li, li_lane), name


@pytest.mark.parametrize("specular", [False, True])
def test_pre_bump_normal(gpu, oracle, specular):
    """whitted.rs:58 reads isect.shading.n before the bump map moves it; the light term's cosine uses that normal.  specular=False: the
    wavefront form's texture stage; True: the per-lane form with reflected / refracted differentials"""
    sc = textured_room(gpu.bvh_build, bump=True, specular=specular)
    check_bounded(gpu, oracle, sc, whitted_desc(40, 30, 4, TEXTURED_LOOK_AT, 55.0, sc, max_depth=3))


@pytest.mark.parametrize("sampler", ["random", "02sequence", "stratified", "maxmindist"])
def test_pixel_samplers(gpu, oracle, sampler):
    sc = gallery(gpu.bvh_build, "delta")
    check_exact(gpu, oracle, sc, whitted_desc(32, 24, 4, GALLERY_LOOK_AT, 60.0, sc, max_depth=3, sampler=sampler, strat=(2, 2), allow_slow_paths=True))
    sc = point_lit_glass_cornell(gpu.bvh_build, area=True)
    check_bounded(gpu, oracle, sc, whitted_desc(24, 24, 4, CORNELL_LOOK_AT, 40.0, sc, max_depth=4, sampler=sampler, strat=(2, 2), allow_slow_paths=True))


def test_scene_features(gpu, oracle):
    """object instances in both instancing modes (REFERENCE mode's null surfaces), moving instances, a moving camera with a thin lens,
    alpha masks"""
    from tests.test_alpha_masks import LOOK as MASK_LOOK, masked_scene
    from tests.test_instancing import moving_scene, rd_small, small_scene
    for mode in ("reference", "fixed"):
        sc = small_scene(gpu.bvh_build, mode=mode)
        check_bounded(gpu, oracle, sc, rd_small(spp=4, res=(48, 36), integrator="whitted", light_samples=[1] * sc.desc.n_lights, max_depth=3))
    sc = moving_scene(gpu.bvh_build)
    check_bounded(gpu, oracle, sc, rd_small(spp=4, res=(48, 36), integrator="whitted", light_samples=[1] * sc.desc.n_lights, shutter=(0.0, 1.0)))
    sc = point_lit_glass_cornell(gpu.bvh_build)
    la1 = ((300, 290, -780), (270, 260, 0), (0.05, 1, 0))
    check_exact(gpu, oracle, sc, whitted_desc(32, 32, 4, CORNELL_LOOK_AT, 40.0, sc, look_at_end=la1, camera_times=(0.2, 0.85), shutter=(0.0, 1.0),
                                              lens_radius=8.0, focal_distance=700.0))
    sc = masked_scene(gpu.bvh_build)
    check_bounded(gpu, oracle, sc, whitted_desc(48, 36, 4, MASK_LOOK, 45.0, sc))


def test_limits_and_ranges(gpu, oracle):
    from rs_pbrt_amd.lib import RsptError
    sc = point_lit_glass_cornell(gpu.bvh_build)
    with gpu.DeviceScene(sc) as ds:
        li0, _ = gpu.render_samples(ds, whitted_desc(24, 24, 4, CORNELL_LOOK_AT, 40.0, sc, max_depth=0))
        li1, _ = gpu.render_samples(ds, whitted_desc(24, 24, 4, CORNELL_LOOK_AT, 40.0, sc, max_depth=1))
        assert np.array_equal(li0, li1)   # whitted.rs:103: depth + 1 < max_depth is false for both
        with pytest.raises(RsptError) as e:
            gpu.render(ds, whitted_desc(24, 24, 4, CORNELL_LOOK_AT, 40.0, sc, max_depth=33))
        assert e.value.code == abi.E_UNSUPPORTED and "whitted" in str(e.value)
        gpu.render(ds, whitted_desc(24, 24, 4, CORNELL_LOOK_AT, 40.0, sc, max_depth=2))   # the device is still usable
        full = whitted_desc(24, 24, 8, CORNELL_LOOK_AT, 40.0, sc)
        film, _ = gpu.render(ds, full)
        a, _ = gpu.render(ds, whitted_desc(24, 24, 8, CORNELL_LOOK_AT, 40.0, sc, sample_range=(0, 3)))
        b, _ = gpu.render(ds, whitted_desc(24, 24, 8, CORNELL_LOOK_AT, 40.0, sc, sample_range=(3, 5)))
        assert np.array_equal(a[:, 3] + b[:, 3], film[:, 3])
    # max_depth 9 .. 32: the per-lane form
    for depth in (9, 32):
        check_exact(gpu, oracle, sc, whitted_desc(16, 16, 2, CORNELL_LOOK_AT, 40.0, sc, max_depth=depth))
    # a stream beyond the 1024 Sobol' dimensions: 520 point lights draw 1040 at the first hit
    sb = scenes.SceneBuilder()
    m = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-5, 0, -5), (-5, 0, 5), (5, 0, 5), (5, 0, -5)], m)
    for k in range(520):
        sb.add_point_light((-4 + 8 * (k % 26) / 25.0, 3.0, -4 + 8 * (k // 26) / 19.0), (0.05, 0.05, 0.05))
    many = sb.finish(gpu.bvh_build)
    look = ((0, 4, -6), (0, 0, 0), (0, 1, 0))
    for form in (None, "lane"):
        with gpu.DeviceScene(many) as ds:
            if form:
                os.environ["RSPT_DL_FORM"] = form
            try:
                with pytest.raises(RsptError) as e:
                    gpu.render(ds, scenes.make_render_desc(16, 16, 2, look, 50.0, integrator="whitted"))
            finally:
                os.environ.pop("RSPT_DL_FORM", None)
            assert e.value.code == abi.E_UNSUPPORTED and "whitted" in str(e.value) and "dimensions" in str(e.value)
            film, _ = gpu.render(ds, scenes.make_render_desc(16, 16, 2, look, 50.0, integrator="path"))   # and the device renders right after
            assert np.isfinite(film).all()


def test_python_mirror(gpu):
    from rs_pbrt_amd.integrator import WhittedIntegrator
    sc = scenes.cornell_box(gpu.bvh_build)
    film = WhittedIntegrator(camera=scenes.cornell_render_desc(res=24, spp=2)).render(sc)
    assert film.pixels.shape == (24, 24, 4) and (film.pixels[..., 3] >= 2).all() and np.isfinite(film.pixels).all()
