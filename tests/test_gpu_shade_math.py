"""-m gpu: the fast shade-math mode (include/rspt.h rspt_set_shade_math) against the oracle and against the exact mode.

The bounds, for every fast render below:
  * a camera sample DEVIATES when a channel has |got - want| > 1e-3 * max(1, |want|) (1e-3: BASELINE.md section 3's tolerance), want = the oracle's radiance
    of that sample; at most 1e-3 of a render's samples may deviate (a cap on decision flips: a roulette draw or an edge hit decided the other way changes a
    whole path);
  * film RMSE against the oracle's film < 1e-3;
  * the film's filter-weight channel is bit-identical to the oracle's, no NaN sample, no truncated path.
Every figure is printed before it is asserted (pytest -s shows them; DESIGN section 5.3a records them)."""
import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from rs_pbrt_amd.lib import RsptError
from tests.util import DYNAMIC_LOOK_AT, GALLERY_LOOK_AT, TEXTURED_LOOK_AT, dynamic_gallery, film_rmse, gallery, shade_instantiation, textured_room

pytestmark = pytest.mark.gpu
TOL, CAP, RMSE = 1e-3, 1e-3, 1e-3


@pytest.fixture(autouse=True)
def exact_afterwards(gpu):
    """whatever a test did, the process is back in the exact mode for the rest of the suite"""
    yield
    gpu.lib().rspt_set_shade_math(abi.SHADE_MATH_EXACT)


def textured_statue(builder):
    """the textured C3 stand-in (plastic with an image Kd over a matte ground) at a few thousand triangles: a scene the `textured` set serves"""
    return scenes.statue_standin(builder, grid=40, textured=True)


# case -> (scene, render desc for a sampler, the shade set that has to serve it; None: not pinned)
CASES = {
    "cornell": (lambda b: scenes.cornell_box(b), lambda **kw: scenes.cornell_render_desc(res=64, spp=16, max_depth=5, **kw), "diffuse"),
    "plastic": (lambda b: scenes.statue_standin(b, grid=48), lambda **kw: scenes.statue_render_desc(xres=48, yres=36, spp=16, **kw), "plastic"),
    "textured": (textured_statue, lambda **kw: scenes.statue_render_desc(xres=48, yres=36, spp=16, **kw), "textured"),
    "textured-room": (lambda b: textured_room(b), lambda **kw: scenes.make_render_desc(48, 36, 16, TEXTURED_LOOK_AT, 45, max_depth=4, **kw), None),   # (whichever set serves its substrate and uber slabs)
    "gallery": (lambda b: gallery(b), lambda **kw: scenes.make_render_desc(48, 36, 16, GALLERY_LOOK_AT, 55, max_depth=5, **kw), "generic"),
}
_scenes, _refs, _exact = {}, {}, {}


def scene_of(gpu, case):
    if case not in _scenes:
        _scenes[case] = CASES[case][0](gpu.bvh_build)
    return _scenes[case]


def reference(oracle, gpu, case, sampler):
    """the oracle's render of a case, computed once and shared"""
    if (case, sampler) not in _refs:
        _refs[case, sampler] = oracle.render(scene_of(gpu, case), CASES[case][1](sampler=sampler), threads=8, want_li=True)
    return _refs[case, sampler]


def exact_li(gpu, case, sampler, monkeypatch, capfd):
    """(the exact mode's radiance of every sample of a case, the instantiation that served it), rendered once and shared"""
    if (case, sampler) not in _exact:
        assert gpu.get_shade_math() == "exact"
        with gpu.DeviceScene(scene_of(gpu, case)) as ds:
            _exact[case, sampler] = shade_instantiation(monkeypatch, capfd, lambda: gpu.render_samples(ds, CASES[case][1](sampler=sampler))[0])
    return _exact[case, sampler]


def figures(li, want):
    """(share of deviating samples, 99.9th percentile and maximum of the per-sample relative deviation max_c |got - want| / max(1, |want|))"""
    rel = (np.abs(li.astype(np.float64) - want) / np.maximum(1.0, np.abs(want.astype(np.float64)))).max(axis=-1).ravel()
    rel = np.where(np.isfinite(rel), rel, np.inf)
    return float((rel > TOL).mean()), float(np.percentile(rel, 99.9)), float(rel.max())


def render_both(gpu, ds, rd):
    film, st = gpu.render(ds, rd)
    li, _ = gpu.render_samples(ds, rd)
    return film, li, st


def check_bounds(label, film, li, st, ref):
    share, p999, worst = figures(li, ref["li"])
    rmse = film_rmse(film, ref["film"])
    print("\nfast %-28s deviating %.3e (%d of %d)  p99.9 %.3e  max %.3e  film rmse %.3e" % (label, share, round(share * li.shape[0] * li.shape[1]), li.shape[0] * li.shape[1], p999, worst, rmse))
    assert np.array_equal(film[:, 3], ref["film"][:, 3]), "filter weight sums differ from the oracle's"
    assert st["nan_samples"] == 0 and st["truncated_paths"] == 0
    assert share <= CAP, "%.3e of the samples deviate" % share
    assert rmse < RMSE, "film rmse %.3e" % rmse


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("case", list(CASES))
def test_fast_parity_per_set(gpu, oracle, monkeypatch, capfd, case, sampler):
    """each fast set serves its scene under the name <set>-fast, within the bounds, and is not the exact render.

    The generic set's fast build keeps the correctly rounded division and square root (csrc/Makefile FAST_DIV_TUS) because of the textured room here: with the
    approximate ones 32 of its 27 648 samples deviated under halton (1.157e-3 against the cap of 1e-3; 19 under sobol), with the division exact and only the libm
    functions fast 7 (4 under sobol).  DESIGN section 5.3a has the substitution-by-substitution figures and the mechanism (the room's bump maps)."""
    ref = reference(oracle, gpu, case, sampler)
    before, exact_name = exact_li(gpu, case, sampler, monkeypatch, capfd)
    if CASES[case][2]:
        assert exact_name == CASES[case][2] + ("-halton" if sampler == "halton" and CASES[case][2] != "generic" else "")
    assert np.array_equal(before, ref["li"]), "the exact mode no longer equals the oracle"
    gpu.set_shade_math("fast")
    rd = CASES[case][1](sampler=sampler)
    with gpu.DeviceScene(scene_of(gpu, case)) as ds:
        (film, li, st), name = shade_instantiation(monkeypatch, capfd, lambda: render_both(gpu, ds, rd))
    assert name == exact_name + "-fast"
    check_bounds("%s/%s '%s'" % (case, sampler, name), film, li, st, ref)
    differing = int((li.view(np.uint32) != before.view(np.uint32)).any(axis=-1).sum())
    print("     samples whose bits differ from the exact render: %d" % differing)
    assert differing > 0, "the fast render is the exact render: the switch changed nothing"


@pytest.mark.parametrize("env", [("RSPT_MOVE", "0"), ("RSPT_MOVE", "1"), ("RSPT_SHADE_WAVES", "3"), ("RSPT_SHADE_WAVES", "4"), ("RSPT_SHADE_WAVES", "0"), ("RSPT_MOVE_FROM", "0")])
def test_fast_schedules_and_wave_builds(gpu, oracle, monkeypatch, capfd, env):
    """the schedule and build switches pick among the fast kernels as they do among the exact ones; each choice meets the bounds"""
    ref = reference(oracle, gpu, "cornell", "sobol")
    rd = CASES["cornell"][1](sampler="sobol")
    gpu.set_shade_math("fast")
    with gpu.DeviceScene(scene_of(gpu, "cornell")) as ds:
        base = gpu.render_samples(ds, rd)[0]
        monkeypatch.setenv(*env)
        (film, li, st), name = shade_instantiation(monkeypatch, capfd, lambda: render_both(gpu, ds, rd))
    assert name == "diffuse-fast"
    check_bounds("cornell %s=%s" % env, film, li, st, ref)
    print("     bit-identical to the default fast schedule: %s" % np.array_equal(li, base))   # reported, not asserted


def test_fast_is_deterministic_over_runs_sample_ranges_and_batches(gpu, monkeypatch):
    gpu.set_shade_math("fast")
    mk = CASES["gallery"][1]
    with gpu.DeviceScene(scene_of(gpu, "gallery")) as ds:
        film_a, li_a, _ = render_both(gpu, ds, mk(sampler="sobol"))
        film_b, li_b, _ = render_both(gpu, ds, mk(sampler="sobol"))
        assert np.array_equal(li_a, li_b) and np.array_equal(film_a[:, 3], film_b[:, 3])   # (a film's xyz is summed by atomics: its order is free in either mode)
        assert film_rmse(film_a, film_b) < 1e-6
        for begin, count in ((0, 8), (8, 8)):
            part = gpu.render_samples(ds, mk(sampler="sobol", sample_range=(begin, count)))[0]
            assert np.array_equal(part[:, begin:begin + count], li_a[:, begin:begin + count]), "samples [%d, %d)" % (begin, begin + count)
        monkeypatch.setenv("RSPT_BATCH", str(48 * 36 * 8))   # 16 spp: two batches of 8 samples per pixel
        film_c, li_c, _ = render_both(gpu, ds, mk(sampler="sobol"))
        assert np.array_equal(li_c, li_a) and np.array_equal(film_c[:, 3], film_a[:, 3]) and film_rmse(film_c, film_a) < 1e-6


@pytest.mark.parametrize("case", ["directlighting", "ao", "random", "dynamic", "quadric"])
def test_renders_fast_does_not_cover_stay_exact(gpu, oracle, monkeypatch, capfd, case):
    """fast mode, a render without fast kernels: served under the plain name, bit-identical to the oracle"""
    from tests.test_quadric_render_host import QUADRIC_LOOK, build_quadric_render_restated, dynamic_quadric_room, restated_render
    from tests.test_sphere_render_host import assert_same_li
    b = gpu.bvh_build
    if case == "dynamic":
        sc, rd, want_name = dynamic_gallery(b), scenes.make_render_desc(48, 20, 8, DYNAMIC_LOOK_AT, 75.0, max_depth=4), "dynamic"
    elif case == "quadric":
        sc, rd, want_name = dynamic_quadric_room(b, dynamic=True), scenes.make_render_desc(32, 24, 4, QUADRIC_LOOK, 60, max_depth=5), "dynamic-quadric"
    else:
        kw = {"directlighting": dict(integrator="directlighting"), "ao": dict(integrator="ao", ao_samples=8), "random": dict(sampler="random", allow_slow_paths=True)}[case]
        sc, rd, want_name = scenes.cornell_box(b), scenes.cornell_render_desc(res=48, spp=8, **kw), "diffuse"
    if case == "quadric":
        want = restated_render(build_quadric_render_restated(), sc, rd)[1]   # (the quadric restatement: the oracle holds no disk or cylinder)
    elif case == "directlighting":
        want = oracle.render_integrator(sc, rd, "direct", threads=8, want_li=True)["li"]
    else:
        want = oracle.render(sc, rd, threads=8, want_li=True)["li"]
    gpu.set_shade_math("fast")
    with gpu.DeviceScene(sc) as ds:
        li, name = shade_instantiation(monkeypatch, capfd, lambda: gpu.render_samples(ds, rd)[0])
    assert name == want_name and not name.endswith("-fast")
    assert_same_li(li, want)


def test_back_to_exact(gpu, oracle, monkeypatch, capfd):
    ref = reference(oracle, gpu, "cornell", "sobol")
    rd = CASES["cornell"][1](sampler="sobol")
    with gpu.DeviceScene(scene_of(gpu, "cornell")) as ds:
        gpu.set_shade_math("fast")
        _, name = shade_instantiation(monkeypatch, capfd, lambda: gpu.render(ds, rd))
        assert name == "diffuse-fast"
        gpu.set_shade_math("exact")
        li, name = shade_instantiation(monkeypatch, capfd, lambda: gpu.render_samples(ds, rd)[0])
    assert name == "diffuse" and np.array_equal(li, ref["li"])


def test_python_mirror_sets_the_mode_for_its_render_and_restores_it(gpu, monkeypatch, capfd):
    from rs_pbrt_amd import integrator
    rd = CASES["cornell"][1](sampler="sobol")
    with gpu.DeviceScene(scene_of(gpu, "cornell")) as ds:
        _, name = shade_instantiation(monkeypatch, capfd, lambda: integrator.PathIntegrator(max_depth=5, camera=rd, shade_math="fast").render(ds))
        assert name == "diffuse-fast" and gpu.get_shade_math() == "exact"
        gpu.set_shade_math("fast")
        _, name = shade_instantiation(monkeypatch, capfd, lambda: integrator.PathIntegrator(max_depth=5, camera=rd, shade_math="exact").render(ds))
        assert name == "diffuse" and gpu.get_shade_math() == "fast"


def test_environment_overrides_the_call(gpu, oracle, monkeypatch, capfd):
    ref = reference(oracle, gpu, "cornell", "sobol")
    rd = CASES["cornell"][1](sampler="sobol")
    with gpu.DeviceScene(scene_of(gpu, "cornell")) as ds:
        monkeypatch.setenv("RSPT_SHADE_MATH", "fast")       # the call never made
        assert gpu.get_shade_math() == "exact"
        _, name = shade_instantiation(monkeypatch, capfd, lambda: gpu.render(ds, rd))
        assert name == "diffuse-fast"
        monkeypatch.setenv("RSPT_SHADE_MATH", "exact")      # over the call
        gpu.set_shade_math("fast")
        li, name = shade_instantiation(monkeypatch, capfd, lambda: gpu.render_samples(ds, rd)[0])
        assert name == "diffuse" and np.array_equal(li, ref["li"])
        monkeypatch.setenv("RSPT_SHADE_MATH", "")           # set and empty: the call holds
        _, name = shade_instantiation(monkeypatch, capfd, lambda: gpu.render(ds, rd))
        assert name == "diffuse-fast"
        monkeypatch.setenv("RSPT_SHADE_MATH", "quick")
        with pytest.raises(RsptError) as e:
            gpu.render(ds, rd)
        assert e.value.code == abi.E_INVALID and "RSPT_SHADE_MATH" in str(e.value)
