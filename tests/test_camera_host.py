"""The CPU yardstick of the orthographic and environment cameras (ABI 25): tests/camera_restated.cpp.  Its tile loop is first held to the oracle's own
(camera_kind = 0: film and every sample's li bit for bit, over all five integrators, both global samplers, a lens with a moving camera and a pixel
sampler); only then are the two new cameras held to known answers that follow from the reference's text (orthographic.rs:150-235,
environment.rs:92-116), and the orthographic camera's depth invariance is shown through a whole render, with the perspective camera as the control.
tests/test_gpu_cameras.py holds rspt_render to this yardstick."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.util import GALLERY_LOOK_AT, gallery

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LOOK_END = ((0.6, 3.3, -4.6), (0.3, 1.8, 2), (0.1, 1, 0))      # the second key of the moving camera: a translation and a rotation away from GALLERY_LOOK_AT


def build_camera_restated(with_li=None):
    """with_li: None | "spheres" — link tests/sphere_render_restated.cpp in and let cam_render install its li"""
    td = tempfile.mkdtemp()
    so = os.path.join(td, "libcamera.so")
    src = [os.path.join(ROOT, "tests", "camera_restated.cpp")]
    defs = []
    if with_li:
        src.append(os.path.join(ROOT, "tests", {"spheres": "sphere_render_restated.cpp"}[with_li]))
        defs = ["-DCAM_LI_" + with_li.upper()]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "oracle"), "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests")] + defs + ["-o", so] + src)
    L = C.CDLL(so)
    L.cam_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.cam_ray.restype = None
    L.cam_ray.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    L.cam_ray_camera_space.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    L.cam_sample.restype = None
    L.cam_sample.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p]
    return L


def cam_render(L, sc, rd, kind=None, strategy="all", light_samples=None, zero_diff=False, threads=4):
    """(film (npix, 4), li (npix, spp, 3)); kind: None = the desc's path / ao / volpath, "direct" | "whitted" as pyoracle.render_integrator takes them"""
    npix = scenes.n_pixels(rd)
    film = np.zeros((npix, 4), F32)
    li = np.zeros((npix, int(rd.spp), 3), F32)
    ns = None if light_samples is None else np.ascontiguousarray(light_samples, np.int32)
    rc = L.cam_render(C.addressof(sc.desc), C.addressof(rd), threads, film.ctypes.data, li.ctypes.data, {None: 0, "direct": 2, "whitted": 3}[kind],
                      {"all": 0, "one": 1}[strategy], None if ns is None else ns.ctypes.data, int(zero_diff))
    assert rc == 0
    return film, li


RAY_FIELDS = (("o", 0, 3), ("d", 3, 6), ("t_max", 6, 7), ("time", 7, 8), ("has_diff", 8, 9), ("rx_o", 9, 12), ("rx_d", 12, 15), ("ry_o", 15, 18), ("ry_d", 18, 21))


def cam_ray(L, rd, p_film, time=0.0, p_lens=(0.0, 0.0), camera_space=False):
    pf, pl, out = np.array(p_film, F32), np.array(p_lens, F32), np.zeros(21, F32)
    if camera_space:
        assert L.cam_ray_camera_space(C.addressof(rd), pf.ctypes.data, float(time), pl.ctypes.data, out.ctypes.data) == 0
    else:
        L.cam_ray(C.addressof(rd), pf.ctypes.data, float(time), pl.ctypes.data, out.ctypes.data)
    return {k: (out[a:b].copy() if b - a > 1 else out[a]) for k, a, b in RAY_FIELDS}


def cam_sample(L, rd, px, py, s):
    out = np.zeros(5, F32)
    L.cam_sample(C.addressof(rd), px, py, s, out.ctypes.data)
    return out


def assert_same_li(got, want):
    a, b = np.ascontiguousarray(got, F32).reshape(-1, 3).view(np.uint32), np.ascontiguousarray(want, F32).reshape(-1, 3).view(np.uint32)
    nan = np.isnan(np.asarray(got, F32).reshape(-1, 3)) & np.isnan(np.asarray(want, F32).reshape(-1, 3))
    bad = ((a != b) & ~nan).any(axis=-1)
    assert not bad.any(), "%d of %d camera samples differ" % (int(bad.sum()), bad.size)


@pytest.fixture(scope="module")
def restated():
    return build_camera_restated()


# ---- 1. the loop copy is the oracle's loop ----
def loop_cases(builder):
    """(name, scene, desc, oracle call) — each 24 x 24 at 4 - 16 spp, camera_kind = 0"""
    from tests.test_gpu_volpath import LOOK as FOG_LOOK, fog_room
    g_all, g_delta = gallery(builder, "all"), gallery(builder, "delta")
    ls = [2] * g_all.desc.n_lights
    mk = scenes.make_render_desc
    return [
        ("path-sobol", g_all, mk(24, 24, 4, GALLERY_LOOK_AT, 60, max_depth=5), (None, "all", None)),
        ("path-halton-lens-moving", g_all, mk(24, 24, 6, GALLERY_LOOK_AT, 60, max_depth=5, sampler="halton", lens_radius=0.05, focal_distance=6.0, look_at_end=LOOK_END,
                                           camera_times=(0.2, 0.85), shutter=(0.0, 1.0)), (None, "all", None)),
        ("ao", g_all, mk(24, 24, 4, GALLERY_LOOK_AT, 60, integrator="ao", ao_samples=16), (None, "all", None)),
        ("direct-all", g_all, mk(24, 24, 4, GALLERY_LOOK_AT, 60, max_depth=3, integrator="directlighting", light_samples=ls), ("direct", "all", ls)),
        ("direct-one", g_all, mk(24, 24, 8, GALLERY_LOOK_AT, 60, max_depth=3, integrator="directlighting", direct_strategy="one"), ("direct", "one", None)),
        ("whitted", g_delta, mk(24, 24, 4, GALLERY_LOOK_AT, 60, max_depth=3, integrator="whitted", light_samples=[1] * g_delta.desc.n_lights), ("whitted", "all", None)),
        ("volpath", fog_room(builder), mk(24, 24, 16, FOG_LOOK, 55.0, integrator="volpath", max_depth=5), (None, "all", None)),
        ("path-02sequence", g_all, mk(24, 24, 4, GALLERY_LOOK_AT, 60, max_depth=3, sampler="02sequence"), (None, "all", None)),
    ]


def test_the_loop_copy_is_the_oracles_loop(restated, oracle):
    for name, sc, rd, (kind, strategy, ls) in loop_cases(oracle.bvh_build):
        assert rd.camera_kind == abi.CAMERA_PERSPECTIVE
        film, li = cam_render(restated, sc, rd, kind, strategy, ls)
        ref = oracle.render(sc, rd, threads=4, want_li=True) if kind is None else oracle.render_integrator(sc, rd, kind, strategy=strategy, light_samples=ls, threads=4, want_li=True)
        assert_same_li(li, ref["li"])
        assert np.array_equal(film.view(np.uint32), ref["film"].view(np.uint32)), name
        assert np.nanmean(li) > 0.0, name


# ---- 2. orthographic known answers ----
ORTHO_LOOK = ((1.0, 2.0, -6.0), (0.5, 1.0, 0.0), (0.1, 1.0, 0.0))
WINDOW = (-3.0, 5.0, -2.0, 1.5)      # not centred, not the frame's aspect ratio


def xf_vec(m16, v):
    m = np.array(m16, np.float64).reshape(4, 4)
    return m[:3, :3] @ np.asarray(v, np.float64)


def xf_pnt(m16, p):
    m = np.array(m16, np.float64).reshape(4, 4)
    return m[:3, :3] @ np.asarray(p, np.float64) + m[:3, 3]


def test_orthographic_rays_without_a_lens(restated):
    res = (20, 14)
    rd = scenes.make_render_desc(res[0], res[1], 4, ORTHO_LOOK, 33.0, camera="orthographic", screen_window=WINDOW)
    assert rd.camera_kind == abi.CAMERA_ORTHOGRAPHIC
    c2w, r2c = rd.camera_to_world[:], rd.raster_to_camera[:]
    m = np.array(c2w, F32).reshape(4, 4)
    want_d = np.array([m[i, 0] * F32(0) + m[i, 1] * F32(0) + m[i, 2] * F32(1) for i in range(3)], F32)      # Transform::transform_vector of (0, 0, 1), not renormalised
    dx_w, dy_w = xf_vec(c2w, xf_vec(r2c, (1, 0, 0))), xf_vec(c2w, xf_vec(r2c, (0, 1, 0)))
    rng = np.random.default_rng(3)
    for px in range(res[0]):
        for py in range(res[1]):
            r = cam_ray(restated, rd, (px + rng.random(), py + rng.random()), time=rng.random(), p_lens=rng.random(2))
            assert r["has_diff"] == 1.0 and r["time"] >= 0.0
            for k in ("d", "rx_d", "ry_d"):
                assert r[k].tobytes() == want_d.tobytes()
            # the offsets: equal to the world transform of dx_camera / dy_camera up to the rounding of the two points and their difference
            # (the origin also carries transform_ray's shift along d: up to gamma(3) * |o| ~ 2e-6 here)
            tol = 8 * np.finfo(F32).eps * np.abs(r["o"]).max() + 4e-6
            assert np.abs((r["rx_o"].astype(np.float64) - r["o"]) - dx_w).max() < tol and np.abs((r["ry_o"].astype(np.float64) - r["o"]) - dy_w).max() < tol
    # the four corners of the frame map back to the screen window's corners (camera space: x = screen x, y = screen y, z = 0)
    for (fx, fy), (sx, sy) in (((0, 0), (WINDOW[0], WINDOW[3])), ((res[0], 0), (WINDOW[1], WINDOW[3])), ((0, res[1]), (WINDOW[0], WINDOW[2])), ((res[0], res[1]), (WINDOW[1], WINDOW[2]))):
        r = cam_ray(restated, rd, (fx, fy), camera_space=True)
        assert np.allclose(r["o"], (sx, sy, 0.0), atol=1e-5) and r["d"].tolist() == [0.0, 0.0, 1.0]
        w = cam_ray(restated, rd, (fx, fy))
        assert np.allclose(w["o"], xf_pnt(c2w, (sx, sy, 0.0)), atol=2e-5)


def test_orthographic_rays_with_a_lens(restated, oracle):
    """the two traps of orthographic.rs:172-217: the lens point REPLACES the origin (the film position survives in the direction only), and both
    offset rays aim at the one p_focus (dy_camera unused)"""
    res, radius = (20, 14), 0.25
    rd = scenes.make_render_desc(res[0], res[1], 4, ORTHO_LOOK, 33.0, camera="orthographic", screen_window=WINDOW, lens_radius=radius, focal_distance=4.0)
    u = (0.3, 0.8)
    disk = np.zeros(2, F32)
    oracle.lib().orc_concentric_sample_disk(u[0], u[1], disk.ctypes.data)
    want_o = np.array([disk[0] * F32(radius), disk[1] * F32(radius), 0.0], F32)
    dirs = set()
    for px in range(0, res[0], 3):
        for py in range(0, res[1], 3):
            r = cam_ray(restated, rd, (px + 0.5, py + 0.5), p_lens=u, camera_space=True)
            assert r["o"].tobytes() == want_o.tobytes()
            assert r["rx_o"].tobytes() == want_o.tobytes() and r["ry_o"].tobytes() == want_o.tobytes()
            assert r["rx_d"].tobytes() == r["ry_d"].tobytes() and r["rx_d"].tobytes() != r["d"].tobytes()
            assert abs(float(np.linalg.norm(r["d"].astype(np.float64))) - 1.0) < 2e-7
            # the lens ray passes through the film position's point on the focal plane
            t = 4.0 / r["d"][2]
            p_film_cam = cam_ray(restated, scenes.make_render_desc(res[0], res[1], 4, ORTHO_LOOK, 33.0, camera="orthographic", screen_window=WINDOW), (px + 0.5, py + 0.5), camera_space=True)["o"]
            assert np.allclose(r["o"] + t * r["d"], (p_film_cam[0], p_film_cam[1], 4.0), atol=1e-5)
            dirs.add(r["d"].tobytes())
            w = cam_ray(restated, rd, (px + 0.5, py + 0.5), p_lens=u)
            assert w["rx_o"].tobytes() == w["ry_o"].tobytes() and w["rx_d"].tobytes() == w["ry_d"].tobytes()
    assert len(dirs) > 1


# ---- 3. environment known answers ----
def libm32(name, x):
    return scenes._libm_f32(name, F32(x))


def test_environment_rays(restated):
    res = (64, 32)
    ident = ((0, 0, 0), (0, 0, 1), (0, 1, 0))      # camera_to_world = identity: world space is camera space
    rd = scenes.make_render_desc(res[0], res[1], 4, ident, 50.0, camera="environment")
    assert rd.camera_kind == abi.CAMERA_ENVIRONMENT and np.array_equal(np.array(rd.camera_to_world[:]).reshape(4, 4), np.eye(4))
    for px in range(res[0]):
        for py in range(res[1]):
            r = cam_ray(restated, rd, (px + 0.5, py + 0.25))
            assert r["has_diff"] == 0.0 and r["o"].tolist() == [0.0, 0.0, 0.0] and np.isinf(r["t_max"])
            # |d|^2 = sin^2 (cos^2 phi + sin^2 phi) + cos^2: each of sinf / cosf is within 1 ulp, so the length is within a few 1e-7 of 1
            assert abs(float(np.linalg.norm(r["d"].astype(np.float64))) - 1.0) < 2e-6
    # the row p_film.y = 0 looks along +y whatever x: theta = 0, sin = 0, cos = 1
    for x in (0.0, 0.5, 13.25, 63.99):
        assert cam_ray(restated, rd, (x, 0.0))["d"].tolist() == [0.0, 1.0, 0.0]
    # p_film = (0, res.y / 2): theta = PI * 16 / 32 in f32 steps, phi = 0 -> (sinf(theta) * cosf(0), cosf(theta), sinf(theta) * sinf(0)) with the host's sinf / cosf
    theta = F32(F32(F32(math.pi) * F32(res[1] / 2)) / F32(res[1]))
    st, ct = libm32("sinf", theta), libm32("cosf", theta)
    want = np.array([F32(st * libm32("cosf", 0.0)), ct, F32(st * libm32("sinf", 0.0))], F32)
    got = cam_ray(restated, rd, (0.0, res[1] / 2))["d"]
    assert got.tobytes() == want.tobytes() and got[0] == 1.0 and abs(got[1]) < 1e-7 and got[2] == 0.0
    # and a general film position, operation for operation (environment.rs:93-99)
    pf = (F32(41.375), F32(9.8125))
    theta = F32(F32(F32(math.pi) * pf[1]) / F32(res[1])); phi = F32(F32(F32(F32(2) * F32(math.pi)) * pf[0]) / F32(res[0]))
    want = np.array([F32(libm32("sinf", theta) * libm32("cosf", phi)), libm32("cosf", theta), F32(libm32("sinf", theta) * libm32("sinf", phi))], F32)
    assert cam_ray(restated, rd, pf)["d"].tobytes() == want.tobytes()
    # lens_radius, focal_distance and raster_to_camera do not reach the ray
    a = cam_ray(restated, rd, (20.5, 7.25), time=0.3, p_lens=(0.2, 0.9))
    rd.lens_radius, rd.focal_distance = 0.7, 3.0
    for i in range(16):
        rd.raster_to_camera[i] = 0.37 * (i + 1)
    b = cam_ray(restated, rd, (20.5, 7.25), time=0.3, p_lens=(0.2, 0.9))
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k, _, _ in RAY_FIELDS)


def test_moving_camera_transforms_the_new_cameras_rays(restated, oracle):
    """camera_to_world with its animation is shared: at a time inside the interval the world ray is the camera-space ray under the oracle's interpolated matrix"""
    for camera in ("orthographic", "environment"):
        rd = scenes.make_render_desc(32, 24, 4, GALLERY_LOOK_AT, 60, camera=camera, screen_window=(-4, 4, -3, 3), look_at_end=LOOK_END, camera_times=(0.2, 0.85), shutter=(0.0, 1.0))
        cs, w = cam_ray(restated, rd, (10.5, 7.5), time=0.5, camera_space=True), cam_ray(restated, rd, (10.5, 7.5), time=0.5)
        m = oracle.interpolate_transform(np.array(rd.camera_to_world[:]), 0.2, np.array(rd.camera_to_world_end[:]), 0.85, 0.5)
        assert np.allclose(w["d"], xf_vec(m.reshape(-1), cs["d"]), atol=1e-6) and np.allclose(w["o"], xf_pnt(m.reshape(-1), cs["o"]), atol=1e-4)
        assert not np.allclose(w["d"], xf_vec(rd.camera_to_world[:], cs["d"]), atol=1e-3)


# ---- 4. orthographic depth invariance through cam_render ----
EDGE_X, EDGE_Y = (4.25 + 1 / 128, 11.25 + 1 / 128), (5.25 + 1 / 128, 12.25 + 1 / 128)


def quad_scene(builder, z):
    """an emissive quad facing the camera (which looks along +z from the origin's side), its edges between the sample lattice's lines: the 1024 Sobol' samples of
    a 16 x 16 x 4 frame lie on multiples of 1 / 64 px (a (0, 2)-net over the frame), x.25 included, so the edges sit at x.25 + 1 / 128 px, half a step from any sample"""
    sb = scenes.SceneBuilder()
    m = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    # window (-2, 2) x (-2, 2) over 16 pixels: 4 pixels per unit; raster x = (X + 2) * 4, raster y = (2 - Y) * 4.  Edges at raster EDGE_X and EDGE_Y.
    x0, x1, y0, y1 = EDGE_X[0] / 4 - 2, EDGE_X[1] / 4 - 2, 2 - EDGE_Y[1] / 4, 2 - EDGE_Y[0] / 4      # (exact in binary)
    sb.add_quad([(x0, y0, z), (x0, y1, z), (x1, y1, z), (x1, y0, z)], m, emit=(3, 3, 3), two_sided=True)
    return sb.finish(builder)


def test_orthographic_depth_invariance(restated, oracle):
    look = ((0, 0, 0), (0, 0, 1), (0, 1, 0))
    mk = lambda camera: scenes.make_render_desc(16, 16, 4, look, 53.13010235, max_depth=0, camera=camera, screen_window=(-2, 2, -2, 2))      # noqa: E731
    rd = mk("orthographic")
    # no Sobol' sample of the frame falls within 1e-3 px of an edge
    for px in range(16):
        for py in range(16):
            for s in range(4):
                cs = cam_sample(restated, rd, px, py, s)
                assert min(abs(cs[0] - e) for e in EDGE_X) > 1e-3 and min(abs(cs[1] - e) for e in EDGE_Y) > 1e-3
    lit = {}
    for camera in ("orthographic", "perspective"):
        for z in (2.0, 5.0):
            _, li = cam_render(restated, quad_scene(oracle.bvh_build, z), mk(camera))
            assert set(np.unique(li)) <= {0.0, 3.0}
            lit[camera, z] = li[..., 0] > 0
    assert lit["orthographic", 2.0].any() and np.array_equal(lit["orthographic", 2.0], lit["orthographic", 5.0])
    # exactly the samples whose film position lies inside the quad's raster rectangle
    inside = np.zeros((16, 16, 4), bool)
    for px in range(16):
        for py in range(16):
            for s in range(4):
                cs = cam_sample(restated, rd, px, py, s)
                inside[py, px, s] = EDGE_X[0] < cs[0] < EDGE_X[1] and EDGE_Y[0] < cs[1] < EDGE_Y[1]
    assert np.array_equal(lit["orthographic", 2.0], inside.reshape(256, 4))
    # the control: the perspective camera sees the quad shrink with distance
    assert lit["perspective", 2.0].sum() > lit["perspective", 5.0].sum() > 0
