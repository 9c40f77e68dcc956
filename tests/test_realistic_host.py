"""The CPU yardstick of the realistic camera (ABI 26): tests/realistic_restated.cpp.  Its tile loop is first held to the oracle's own (camera_kind = 0: film
and every sample's li bit for bit, the cases of tests/test_camera_host.py); rspt_realistic_camera_setup is held to the restatement's setup bit for bit; the
restatement is held to known answers that depend on neither (a thick lens' focal length, where a paraxial ray crosses the axis, a bare stop, Snell's law);
every arm of generate_ray_differential is shown to occur; and the frames tests/test_gpu_realistic.py renders are shown to hold both live and dead samples.
tests/test_gpu_realistic.py holds rspt_camera_rays and rspt_render to this yardstick."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rs_pbrt_amd import abi, lib, scenes
from tests.test_camera_host import LOOK_END, assert_same_li, loop_cases
from tests.util import GALLERY_LOOK_AT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LENS_DIR = os.path.join(ROOT, "tests", "golden", "lenses")
# lens file, film diagonal (mm), aperture diameter (mm), focus distance: the two cameras of the GPU tests
LENSES = {"dgauss50": (os.path.join(LENS_DIR, "dgauss50.dat"), 35.0, 8.0, 6.0), "singlet": (os.path.join(LENS_DIR, "singlet.dat"), 24.0, 10.0, 2.0)}
ARMS = ("primary vignetted", "clean", "x retried", "y retried", "dead by x shifts", "dead by y shifts")


def build_realistic_restated(with_li=None):
    """with_li: None | "spheres" — link tests/sphere_render_restated.cpp in and let real_render install its li"""
    td = tempfile.mkdtemp()
    so = os.path.join(td, "librealistic.so")
    src = [os.path.join(ROOT, "tests", "realistic_restated.cpp")]
    defs = []
    if with_li:
        src.append(os.path.join(ROOT, "tests", {"spheres": "sphere_render_restated.cpp"}[with_li]))
        defs = ["-DCAM_LI_" + with_li.upper()]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "oracle"), "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests")] + defs + ["-o", so] + src)
    L = C.CDLL(so)
    vp, f, u32 = C.c_void_p, C.c_float, C.c_uint32
    L.real_render.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int]
    L.real_rays.restype = None
    L.real_rays.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.real_setup.argtypes = [vp, u32, f, f, f, u32, vp, vp, C.c_int]
    L.real_trace_from_film.argtypes = [vp, u32, vp, vp, vp]
    L.real_trace_from_scene.argtypes = [vp, u32, vp, vp, vp]
    L.real_cardinal_points.argtypes = [vp, u32, f, vp, vp]
    L.real_t_neg_count.restype = C.c_uint64
    L.real_sample.restype = None
    L.real_sample.argtypes = [vp, C.c_int32, C.c_int32, C.c_int64, vp]
    return L


def real_render(L, sc, rd, kind=None, strategy="all", light_samples=None, zero_diff=False, threads=4):
    """(film (npix, 4), li (npix, spp, 3), ray weights (npix, spp))"""
    npix = scenes.n_pixels(rd)
    film, li, w = np.zeros((npix, 4), F32), np.zeros((npix, int(rd.spp), 3), F32), np.zeros((npix, int(rd.spp)), F32)
    ns = None if light_samples is None else np.ascontiguousarray(light_samples, np.int32)
    rc = L.real_render(C.addressof(sc.desc), C.addressof(rd), threads, film.ctypes.data, li.ctypes.data, w.ctypes.data, {None: 0, "direct": 2, "whitted": 3}[kind],
                       {"all": 0, "one": 1}[strategy], None if ns is None else ns.ctypes.data, int(zero_diff))
    assert rc == 0
    return film, li, w


def real_rays(L, rd, samples):
    """generate_ray_differential of the restatement: ((n, 22) f32 in rspt_camera_rays' layout, arms (n,) i32)"""
    smp = np.ascontiguousarray(samples, F32).reshape(-1, 5)
    out, arms = np.zeros((len(smp), 22), F32), np.zeros(len(smp), np.int32)
    L.real_rays(C.addressof(rd), smp.ctypes.data, len(smp), out.ctypes.data, arms.ctypes.data)
    return out, arms


def lens_desc(name, xres=48, yres=36, spp=4, look=GALLERY_LOOK_AT, **kw):
    path, diag, ap, focus = LENSES[name]
    return scenes.make_render_desc(xres, yres, spp, look, 60.0, camera="realistic", lens=path, aperture_diameter=ap, focus_distance=focus, film_diagonal=diag, **kw)


def raw_elements(name, aperture=None):
    """the lens file in metres, unfocused: RealisticCamera::new's table before focus_thick_lens"""
    data = scenes.read_lens_file(LENSES[name][0])
    el = np.zeros(len(data), abi.LENS_ELEMENT_DT)
    el["curvature_radius"], el["thickness"], el["eta"] = data[:, 0] * F32(0.001), data[:, 1] * F32(0.001), data[:, 2]
    diam = data[:, 3].copy()
    if aperture is not None:
        stop = data[:, 0] == 0
        diam[stop] = np.where(aperture > diam[stop], diam[stop], F32(aperture))
    el["aperture_radius"] = diam * F32(0.001) / F32(2)
    return el


def trace_from_film(L, el, o, d):
    el = np.ascontiguousarray(el, abi.LENS_ELEMENT_DT)
    o, d, out = np.array(o, F32), np.array(d, F32), np.zeros(7, F32)
    ok = L.real_trace_from_film(el.ctypes.data, len(el), o.ctypes.data, d.ctypes.data, out.ctypes.data)
    return (out[:3].astype(np.float64), out[3:6].astype(np.float64)) if ok else None


def scan_samples(L, rd, n=1 << 20, seed=17):
    """n pseudo-random CameraSamples over the frame -> (samples (n, 5), rays (n, 22), arms (n,))"""
    rng = np.random.default_rng(seed)
    smp = rng.random((n, 5), dtype=F32)
    smp[:, 0] *= F32(rd.full_res[0]); smp[:, 1] *= F32(rd.full_res[1])
    out, arms = real_rays(L, rd, smp)
    return smp, out, arms


@pytest.fixture(scope="module")
def restated():
    return build_realistic_restated()


# ---- 1. the loop copy is the oracle's loop ----
def test_the_loop_copy_is_the_oracles_loop(restated, oracle):
    for name, sc, rd, (kind, strategy, ls) in loop_cases(oracle.bvh_build):
        assert rd.camera_kind == abi.CAMERA_PERSPECTIVE
        film, li, w = real_render(restated, sc, rd, kind, strategy, ls)
        ref = oracle.render(sc, rd, threads=4, want_li=True) if kind is None else oracle.render_integrator(sc, rd, kind, strategy=strategy, light_samples=ls, threads=4, want_li=True)
        assert_same_li(li, ref["li"])
        assert np.array_equal(film.view(np.uint32), ref["film"].view(np.uint32)), name
        assert (w == 1.0).all() and np.nanmean(li) > 0.0, name


# ---- 2. rspt_realistic_camera_setup is the restatement's setup ----
@pytest.mark.parametrize("name", sorted(LENSES))
def test_setup_equals_the_restatement(restated, name):
    path, diag, ap, focus = LENSES[name]
    data = scenes.read_lens_file(path)
    el, bounds = lib.realistic_camera_setup(data, ap, focus, diag, 64)
    want_el, want_b = np.zeros(len(data), abi.LENS_ELEMENT_DT), np.zeros((64, 4), F32)
    assert restated.real_setup(data.ctypes.data, len(data), ap, focus, diag, 64, want_el.ctypes.data, want_b.ctypes.data, 4) == 0
    assert el.tobytes() == want_el.tobytes()
    assert bounds.tobytes() == want_b.tobytes()
    assert restated.real_t_neg_count() == 0
    # the split over threads cannot show
    el1, b1 = lib.realistic_camera_setup(data, ap, focus, diag, 64, threads=1)
    assert el1.tobytes() == el.tobytes() and b1.tobytes() == bounds.tobytes()
    # mm -> m, the stop takes the given aperture, only the last thickness changes
    raw = raw_elements(name, ap)
    assert el[:-1].tobytes() == raw[:-1].tobytes() and el[-1]["thickness"] != raw[-1]["thickness"]
    assert (bounds[:, 2] > bounds[:, 0]).all() and (bounds[:, 3] > bounds[:, 1]).all()


def test_setup_error_paths(restated):
    path, diag, ap, _ = LENSES["dgauss50"]
    data = scenes.read_lens_file(path)
    el, b = np.zeros(len(data), abi.LENS_ELEMENT_DT), np.zeros((64, 4), F32)
    with pytest.raises(lib.RsptError) as e:      # a focus distance inside the lens' own focal range: assert!(c > 0)
        lib.realistic_camera_setup(data, ap, 0.05, diag)
    assert e.value.code == abi.E_INVALID and "Coefficient must be positive" in str(e.value) and "too short" in str(e.value)
    assert restated.real_setup(data.ctypes.data, len(data), ap, 0.05, diag, 64, el.ctypes.data, b.ctypes.data, 4) == 3
    # an aperture larger than the stop's own diameter keeps the file's value ("Clamping it.")
    stop = int(np.flatnonzero(data[:, 0] == 0)[0])
    big, _ = lib.realistic_camera_setup(data, 40.0, 6.0, diag, 2)
    assert big[stop]["aperture_radius"] == data[stop, 3] * F32(0.001) / F32(2)
    small, _ = lib.realistic_camera_setup(data, 8.0, 6.0, diag, 2)
    assert small[stop]["aperture_radius"] == F32(8.0) * F32(0.001) / F32(2)
    # a stop no ray passes: "Unable to trace ray from scene to film for thick lens approximation"
    with pytest.raises(lib.RsptError) as e:
        lib.realistic_camera_setup(data, 1e-4, 6.0, diag, 2)
    assert e.value.code == abi.E_INVALID and "thick lens approximation" in str(e.value)
    L = lib.lib()
    assert L.rspt_realistic_camera_setup(None, 3, 1.0, 1.0, 35.0, 64, el.ctypes.data, b.ctypes.data, 0) == abi.E_INVALID
    assert L.rspt_realistic_camera_setup(data.ctypes.data, abi.MAX_LENS_ELEMENTS + 1, 1.0, 1.0, 35.0, 64, el.ctypes.data, b.ctypes.data, 0) == abi.E_INVALID


def test_make_render_desc_caches_the_tables():
    a, b = lens_desc("singlet"), lens_desc("singlet", xres=32, yres=32)
    assert a.camera_kind == abi.CAMERA_REALISTIC and a.lens_elements == b.lens_elements and a.exit_pupil_bounds == b.exit_pupil_bounds
    assert a.n_lens_elements == 3 and a.n_exit_pupil_bounds == 64 and a.lens_simple_weighting == 1
    assert a.film_diagonal == F32(24.0) * F32(0.001)
    c = lens_desc("singlet", simple_weighting=False, shutter=(0.0, 0.5))
    assert c.lens_simple_weighting == 0 and c.lens_elements == a.lens_elements


# ---- 3. known answers, independent of the library and of the restatement's structure ----
def test_singlet_focal_length(restated):
    """1 / f = (n - 1) (1 / R1 - 1 / R2 + (n - 1) d / (n R1 R2)) with n = 1.5, R1 = 60, R2 = -60, d = 6 mm: 61.017 mm.  The ray of the thick-lens
    approximation runs 0.001 x the film diagonal above the axis, so the paraxial formula applies."""
    n, r1, r2, d = 1.5, 60.0, -60.0, 6.0
    f_mm = 1.0 / ((n - 1.0) * (1.0 / r1 - 1.0 / r2 + (n - 1.0) * d / (n * r1 * r2)))
    assert abs(f_mm - 61.017) < 1e-3
    el = raw_elements("singlet")
    pz, fz = np.zeros(2, F32), np.zeros(2, F32)
    assert restated.real_cardinal_points(el.ctypes.data, len(el), 0.024, pz.ctypes.data, fz.ctypes.data) == 0
    for side in (0, 1):      # a lens in air: the same focal length from both sides
        assert abs(abs(float(fz[side]) - float(pz[side])) * 1000.0 - f_mm) < 1e-3 * f_mm


@pytest.mark.parametrize("name", sorted(LENSES))
@pytest.mark.parametrize("focus", [2.0, 3.0])
def test_a_paraxial_ray_from_the_film_centre_crosses_the_axis_at_the_focus_distance(restated, name, focus):
    """a ray from the film centre through (0.5 mm, 0, lens_rear_z).  The bound is 1 % of the focus distance.  What the ray misses the paraxial focus by is
    the lens' longitudinal spherical aberration, which grows with the square of the ray height and, seen from the object side, in proportion to the focus
    distance: the uncorrected singlet shows 0.17 % per metre at this height (0.35 % at its own 2 m), the double Gauss a fifth of that, so both focus
    distances stay well inside the bound; at 6 m the singlet's aberration alone would exceed it."""
    path, diag, ap, _ = LENSES[name]
    el, _ = lib.realistic_camera_setup(scenes.read_lens_file(path), ap, focus, diag, 1)
    rear_z, lu = float(el[-1]["thickness"]), 0.0005
    r = trace_from_film(restated, el, (0.0, 0.0, 0.0), (lu, 0.0, rear_z))
    assert r is not None
    o, d = r
    t = -o[0] / d[0]
    z = o[2] + t * d[2]
    assert abs(z - focus) < 0.01 * focus, z


def test_a_bare_stop(restated):
    """one interface, the stop, 40 mm in front of the film, 5 mm radius: no refraction, so the ray leaves along p_rear - p_film from the stop plane, and the
    simple weight is cos^4 theta x area / area_0"""
    el = np.zeros(1, abi.LENS_ELEMENT_DT)
    el[0] = (0.0, 0.04, 0.0, 0.005)
    p_film, p_rear = np.array((0.002, -0.001, 0.0)), np.array((-0.003, 0.002, 0.04))
    o, d = trace_from_film(restated, el, p_film, p_rear - p_film)
    want = (p_rear - p_film) / np.linalg.norm(p_rear - p_film)
    assert np.abs(d / np.linalg.norm(d) - want).max() < 1e-6
    assert abs(o[2] - 0.04) < 1e-7 and np.abs(o[:2] - p_rear[:2]).max() < 1e-7
    assert trace_from_film(restated, el, p_film, np.array((0.006, 0.0, 0.04)) - p_film) is None      # outside the 5 mm radius
    # the weight, through generate_ray_differential: one exit-pupil box for the whole film, the lens sample picks p_rear inside it
    rd = scenes.make_render_desc(40, 30, 4, GALLERY_LOOK_AT, 60.0)
    bounds = np.array([[-0.006, -0.006, 0.006, 0.006]], F32)
    rd.camera_kind = abi.CAMERA_REALISTIC
    rd.lens_elements, rd.n_lens_elements = el.ctypes.data, 1
    rd.exit_pupil_bounds, rd.n_exit_pupil_bounds = bounds.ctypes.data, 1
    rd.film_diagonal, rd.lens_simple_weighting = 0.03, 1
    rng = np.random.default_rng(3)
    smp = rng.random((4096, 5), dtype=F32)
    smp[:, 0] = 2 + 36 * smp[:, 0]; smp[:, 1] = 2 + 26 * smp[:, 1]
    out, arms = real_rays(restated, rd, smp)
    ex = np.sqrt(0.03 ** 2 / (1 + 0.75 ** 2)); ey = 0.75 * ex      # Film::get_physical_extent
    s = smp.astype(np.float64)
    pf = np.stack([-(-ex / 2 + ex * s[:, 0] / 40), -ey / 2 + ey * s[:, 1] / 30, np.zeros(len(s))], 1)
    rf = np.hypot(pf[:, 0], pf[:, 1])
    pl = np.stack([-0.006 + 0.012 * s[:, 3], -0.006 + 0.012 * s[:, 4]], 1)
    c, sn = pf[:, 0] / rf, pf[:, 1] / rf
    pr = np.stack([c * pl[:, 0] - sn * pl[:, 1], sn * pl[:, 0] + c * pl[:, 1], np.full(len(s), 0.04)], 1)
    inside = np.hypot(pr[:, 0], pr[:, 1]) <= 0.005
    cos = 0.04 / np.linalg.norm(pr - pf, axis=1)
    clean = arms == 1
    assert clean.sum() > 1000 and (arms == 0).sum() > 500
    edge = np.abs(np.hypot(pr[:, 0], pr[:, 1]) - 0.005) < 1e-6
    assert ((out[:, 0] > 0) == inside)[~edge & (clean | (arms == 0))].all()
    assert np.abs(out[clean, 0] - cos[clean] ** 4).max() < 1e-5      # area / area_0 = 1: one box


def test_snells_law_at_the_singlets_first_surface(restated):
    """the singlet's first surface alone (R = 60 mm, n = 1.5), 50 mm in front of the film: a ray from the film travels inside the glass (eta_i = the
    element's eta) and leaves into air (no interface in front of it: eta_t = 1), so n_i sin(theta_i) = n_t sin(theta_t) about the sphere's normal at the
    hit point, which numpy finds in float64"""
    el = np.zeros(1, abi.LENS_ELEMENT_DT)
    el[0] = (0.06, 0.05, 1.5, 0.015)
    o, d = np.array((0.001, 0.0005, 0.0)), np.array((0.004, -0.002, 0.05))
    r = trace_from_film(restated, el, o, d)
    assert r is not None
    p, w = r
    d_n = d / np.linalg.norm(d)
    centre = np.array((0.0, 0.0, 0.05 - 0.06))      # camera space (the lens looks along +z): the vertex at z = 0.05, the centre one radius behind it
    # intersection of the film ray with the sphere, in float64
    oc = o - centre
    b, c = 2 * np.dot(d_n, oc), np.dot(oc, oc) - 0.06 ** 2
    ts = np.roots([1.0, b, c]).real
    hit = [o + t * d_n for t in ts if t > 0 and abs((o + t * d_n)[2] - 0.05) < 0.01][0]
    assert np.abs(p - hit).max() < 1e-6
    n = (hit - centre) / 0.06
    sin_i = np.linalg.norm(np.cross(d_n, n))
    sin_t = np.linalg.norm(np.cross(w / np.linalg.norm(w), n))
    assert abs(1.5 * sin_i - 1.0 * sin_t) < 1e-6
    assert abs(np.dot(np.cross(d_n, n), w)) < 1e-6      # the refracted ray stays in the plane of incidence


# ---- 4. every arm of generate_ray_differential occurs ----
@pytest.mark.parametrize("name", sorted(LENSES))
def test_every_arm_occurs(restated, name):
    """2^20 pseudo-random CameraSamples per lens.  Under dgauss50 every arm is met at least 100 times.  Under the singlet the two retry arms CANNOT occur,
    and the test holds it to that instead: its stop is the rearmost interface and all its exit-pupil boxes are equal, so whether a sample passes is decided
    by |p_lens| against the stop's radius alone (p_rear is p_lens rotated about the axis; the 15 mm glass behind the 5 mm stop clips nothing) — a shift of
    p_film cannot vignette a ray whose unshifted twin passed.  Dead-by-shift samples are reported and kept for the GPU test, none is required."""
    rd = lens_desc(name)
    smp, out, arms = scan_samples(restated, rd)
    counts = np.bincount(arms, minlength=6)
    print("%s: %s" % (name, ", ".join("%s %d" % (a, c) for a, c in zip(ARMS, counts))))
    for a in ((0, 1, 2, 3) if name == "dgauss50" else (0, 1)):
        assert counts[a] >= 100, (ARMS[a], counts[a])
    if name == "singlet":
        assert (counts[2:] == 0).all()
    assert restated.real_t_neg_count() == 0
    dead = (arms == 0) | (arms >= 4)
    assert (out[dead, 0] == 0).all() and (out[~dead, 0] > 0).all()
    assert (out[dead, 9:] == 0).all() and (out[~dead, 21] == 1).all()      # no differentials where the weight is 0
    assert (out[arms == 0, 1:9] == 0).all()      # a vignetted primary ray leaves Ray::default()
    assert np.isfinite(np.delete(out, 7, axis=1)).all() and (out[~dead, 7] == np.inf).all()      # t_max: inf less two error-bound terms


# ---- 5. the frames of the GPU tests hold both kinds of sample ----
@pytest.mark.parametrize("name", sorted(LENSES))
@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_frame_conditions(restated, name, sampler):
    rd = lens_desc(name, sampler=sampler)
    smp = np.zeros((48 * 36 * 4, 5), F32)
    k = 0
    for py in range(36):
        for px in range(48):
            for s in range(4):
                restated.real_sample(C.addressof(rd), px, py, s, smp[k:].ctypes.data)
                k += 1
    out, _ = real_rays(restated, rd, smp)
    dead, live = float((out[:, 0] == 0).mean()), float((out[:, 0] > 0).mean())
    print("%s / %s: weight 0 in %.1f %%, > 0 in %.1f %% of the samples" % (name, sampler, 100 * dead, 100 * live))
    assert dead >= 0.10 and live >= 0.50
