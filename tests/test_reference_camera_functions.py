"""The realistic, orthographic and environment cameras held to the REFERENCE'S OWN TEXT (the route of tests/test_reference_shape_functions.py, fifth batch).

oracle/make_camera_fixtures.py compiles — syntax rewritten by committed rules, no hand-edited body — RealisticCamera's generate_ray, generate_ray_differential,
trace_lenses_from_film / _from_scene, intersect_spherical_element, the thick-lens focus, bound_exit_pupil and sample_exit_pupil with two blocks of its constructor
(cameras/realistic.rs), OrthographicCamera and EnvironmentCamera::generate_ray_differential, quadratic, Film::get_physical_extent and the Bounds2f helpers from the
Rust text where it lies; tests/golden/camera_functions.npz holds seeded inputs with that code's outputs:
  setup     both committed prescriptions at LENSES' parameters (the focused element table, all 64 exit-pupil boxes, the cardinal points), each once more with an aperture
            larger than its stop and once at a second focus distance (bands 0, 1, 31, 62, 63), and three refusals as their status codes;
  tracing   2^12 rays per lens and direction, between a quarter and three quarters of which pass;
  rays      per lens and mode the 22 floats of rspt_camera_rays for samples of every arm the lens reaches, 256 at the film centre (r_film == 0), 256 within 2 ulps of
            a band border, 256 on the frame's last row and column; 2^12 samples over six orthographic and 2^12 over two environment cameras.

The first three tests read the committed file alone.  The hand restatements (tests/realistic_restated.cpp part (a), tests/camera_restated.cpp part (a)) must give the
same BITS in every output word; so must rspt_realistic_camera_setup (host code, no device) and the tables scenes.make_render_desc puts into a descriptor.
cam_ray_camera_space has no counterpart in the text (the function's last statement is the transform to world space): it emits the value cam_ray hands to
transform_ray, in the same source, and is held in the two words that transform leaves alone.  Where /root/reference exists the fixture is regenerated and compared, and
2^17 fresh samples per camera kind and 2^15 fresh rays per lens and direction run through the text and the restatements side by side."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rs_pbrt_amd import abi, lib, scenes
from tests.test_camera_host import build_camera_restated
from tests.test_realistic_host import build_realistic_restated, real_rays

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HAVE_REF = os.path.exists("/root/reference/src/cameras/realistic.rs")
FIXTURE = os.path.join(HERE, "golden", "camera_functions.npz")
LENS_DIR = os.path.join(HERE, "golden", "lenses")
F32 = np.float32
NAMES = ("dgauss50", "singlet")
MODES = ("simple-still", "physical-moving")
PART_BANDS = (0, 1, 31, 62, 63)
N_ORTHO, N_ENV = 6, 2
RAY22 = ["weight"] + [a + "." + c for a in ("o", "d") for c in "xyz"] + ["t_max", "time"] + [a + "." + c for a in ("rx_o", "rx_d", "ry_o", "ry_d") for c in "xyz"] + ["has_diff"]
RAY21 = RAY22[1:9] + ["has_diff"] + RAY22[9:21]
RAY8 = ["pass"] + RAY22[1:8]
REFUSAL_WORDS = {1: "Unable to trace ray from scene to film for thick lens approximation", 2: "Unable to trace ray from film to scene for thick lens approximation",
                 3: "Coefficient must be positive"}      # the reference's assert! messages (realistic.rs:466, :480, :495)


def camera_desc(cam, el=None, bounds=None):
    """the render descriptor of one fixture camera: `cam` holds kind, xres, yres, r2c (16), c2w (16), c2w_end (16), animated, times (2), shutter (2), lens_radius,
    focal_distance, film_diagonal (metres), simple_weighting; el (n, 4) / bounds (m, 4): the realistic camera's tables (kept alive by the desc object)"""
    from rs_pbrt_amd import abi, scenes
    from tests.util import GALLERY_LOOK_AT
    rd = scenes.make_render_desc(int(cam["xres"]), int(cam["yres"]), 4, GALLERY_LOOK_AT, 60.0)
    rd.camera_kind = int(cam["kind"])
    rd.raster_to_camera[:] = [float(v) for v in cam["r2c"]]
    rd.camera_to_world[:] = [float(v) for v in cam["c2w"]]
    rd.camera_to_world_end[:] = [float(v) for v in cam["c2w_end"]]
    rd.camera_animated = int(cam["animated"])
    rd.camera_time[:] = [float(v) for v in cam["times"]]
    rd.shutter_open, rd.shutter_close = float(cam["shutter"][0]), float(cam["shutter"][1])
    rd.lens_radius, rd.focal_distance = float(cam["lens_radius"]), float(cam["focal_distance"])
    if el is not None:
        rd._lens_elements = np.frombuffer(np.ascontiguousarray(el, F32).tobytes(), abi.LENS_ELEMENT_DT).copy()
        rd._exit_pupil_bounds = np.ascontiguousarray(bounds, F32).copy()
        rd.lens_elements, rd.n_lens_elements = rd._lens_elements.ctypes.data, len(rd._lens_elements)
        rd.exit_pupil_bounds, rd.n_exit_pupil_bounds = rd._exit_pupil_bounds.ctypes.data, len(rd._exit_pupil_bounds)
        rd.film_diagonal, rd.lens_simple_weighting = float(cam["film_diagonal"]), int(cam["simple_weighting"])
    return rd


def camera_of_desc(rd):
    """the inverse of camera_desc: what the fixture stores of a descriptor, as (17, 16) f32 rows — r2c, c2w, c2w_end, and a row of scalars"""
    return {"kind": int(rd.camera_kind), "xres": int(rd.full_res[0]), "yres": int(rd.full_res[1]), "r2c": np.array(rd.raster_to_camera[:], F32), "c2w": np.array(rd.camera_to_world[:], F32),
            "c2w_end": np.array(rd.camera_to_world_end[:], F32), "animated": int(rd.camera_animated), "times": np.array(rd.camera_time[:], F32), "shutter": np.array([rd.shutter_open, rd.shutter_close], F32),
            "lens_radius": F32(rd.lens_radius), "focal_distance": F32(rd.focal_distance), "film_diagonal": F32(rd.film_diagonal), "simple_weighting": int(rd.lens_simple_weighting)}


def pack_camera(cam):
    """a camera as one (4, 16) f32 array: rows r2c, c2w, c2w_end, scalars"""
    sc = np.zeros(16, F32)
    sc[:13] = [cam["kind"], cam["xres"], cam["yres"], cam["animated"], cam["times"][0], cam["times"][1], cam["shutter"][0], cam["shutter"][1], cam["lens_radius"], cam["focal_distance"],
               cam["film_diagonal"], cam["simple_weighting"], 0]
    return np.stack([cam["r2c"], cam["c2w"], cam["c2w_end"], sc]).astype(F32)


def unpack_camera(a):
    sc = a[3]
    return {"kind": int(sc[0]), "xres": int(sc[1]), "yres": int(sc[2]), "animated": int(sc[3]), "times": sc[4:6], "shutter": sc[6:8], "lens_radius": sc[8], "focal_distance": sc[9], "film_diagonal": sc[10],
            "simple_weighting": int(sc[11]), "r2c": a[0], "c2w": a[1], "c2w_end": a[2]}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))      # (a NaN has many encodings)


def describe(got, want, columns):
    """None when every word of every case is the same bits; else the first differing column by its meaning and the number of differing cases"""
    ok = same_bits(got, want)
    if ok.all():
        return None
    col = int(np.nonzero(~ok.all(axis=0))[0][0])
    row = int(np.nonzero(~ok[:, col])[0][0])
    return "%d of %d cases differ; first differing column: %s (case %d: %r against the text's %r)" % (int((~ok.all(axis=1)).sum()), len(got), columns[col], row, got[row, col], want[row, col])


def lens_data(name):
    return scenes.read_lens_file(os.path.join(LENS_DIR, name + ".dat"))


def setups(g):
    """the fixture's setup cases: (label, lens, (aperture, focus, diagonal), bands or None for all 64, elements, boxes)"""
    for name in NAMES:
        yield name, name, g[name + "_params"], None, g[name + "_el"], g[name + "_bounds"]
        for tag in ("clamp", "refocus"):
            key = "%s_%s" % (name, tag)
            yield key, name, g[key + "_params"], list(PART_BANDS), g[key + "_el"], g[key + "_bounds"]


def restated_trace(R, el, from_scene, rays):
    """real_trace_from_film / real_trace_from_scene ray by ray, in camref_trace's layout: (n, 8) pass, o, d, t_max (zeros where it fails)"""
    el = np.frombuffer(np.ascontiguousarray(el, F32).tobytes(), abi.LENS_ELEMENT_DT).copy()
    rays, out = np.ascontiguousarray(rays, F32), np.zeros((len(rays), 8), F32)
    fn = R.real_trace_from_scene if from_scene else R.real_trace_from_film
    for i in range(len(rays)):
        out[i, 0] = fn(el.ctypes.data, len(el), rays[i, :3].ctypes.data, rays[i, 3:].ctypes.data, out[i, 1:].ctypes.data)
        if out[i, 0] == 0:
            out[i] = 0
    return out


def restated_cam_rays(K, rd, samples, camera_space=False):
    """cam_ray (or cam_ray_camera_space) sample by sample: (n, 21)"""
    smp, out = np.ascontiguousarray(samples, F32), np.zeros((len(samples), 21), F32)
    for i in range(len(smp)):
        if camera_space:
            assert K.cam_ray_camera_space(C.addressof(rd), smp[i, :2].ctypes.data, float(smp[i, 2]), smp[i, 3:].ctypes.data, out[i].ctypes.data) == 0
        else:
            K.cam_ray(C.addressof(rd), smp[i, :2].ctypes.data, float(smp[i, 2]), smp[i, 3:].ctypes.data, out[i].ctypes.data)
    return out


def hold_restatements(R, K, d, full_setup=True):
    """every restatement against the arrays of a fixture (the committed one, or a fresh one): a list of what differs"""
    bad = []
    for label, name, (ap, focus, diag), bands, el, box in setups(d) if full_setup else [(n, n, d[n + "_params"], list(PART_BANDS), d[n + "_el"], d[n + "_bounds"]) for n in NAMES]:
        data = lens_data(name)
        got_el, got_b = np.zeros(len(data), abi.LENS_ELEMENT_DT), np.zeros((64, 4), F32)
        st = R.real_setup(data.ctypes.data, len(data), ap, focus, diag, 64, got_el.ctypes.data, got_b.ctypes.data, 8)
        if st != 0 or got_el.tobytes() != el.tobytes() or got_b[bands if bands is not None else slice(None)].tobytes() != box.tobytes():
            bad.append("real_setup, %s" % label)
    for name in NAMES:
        el = d[name + "_el"]
        for direction in ("film", "scene"):
            msg = describe(restated_trace(R, el, direction == "scene", d["%s_%s_rays" % (name, direction)]), d["%s_%s_out" % (name, direction)], RAY8)
            if msg:
                bad.append("real_trace_from_%s, %s: %s" % (direction, name, msg))
        if name + "_cardinal" in d:
            e = np.frombuffer(el.tobytes(), abi.LENS_ELEMENT_DT).copy()
            pz, fz = np.zeros(2, F32), np.zeros(2, F32)
            st = R.real_cardinal_points(e.ctypes.data, len(e), float(F32(d[name + "_params"][2]) * F32(0.001)), pz.ctypes.data, fz.ctypes.data)
            if st != 0 or not same_bits(np.concatenate([pz, fz]), d[name + "_cardinal"]).all():
                bad.append("real_cardinal_points, %s" % name)
        for mode in MODES:
            key = "%s_%s" % (name, mode)
            rd = camera_desc(unpack_camera(d[key + "_camera"]), el, d[name + "_bounds"] if len(d[name + "_bounds"]) == 64 else d[name + "_all_bounds"])
            got, arm = real_rays(R, rd, d[name + "_samples"])
            msg = describe(got, d[key + "_rays"], RAY22)
            if msg or not np.array_equal(arm, d[name + "_arm"]):
                bad.append("real_rays, %s: %s" % (key, msg or "the arms differ"))
    if "refusals" in d:
        for lens, ap, focus, diag, want in d["refusals"]:
            data = lens_data(NAMES[int(lens)])
            e, b = np.zeros(len(data), abi.LENS_ELEMENT_DT), np.zeros((64, 4), F32)
            if R.real_setup(data.ctypes.data, len(data), ap, focus, diag, 64, e.ctypes.data, b.ctypes.data, 4) != int(want):
                bad.append("real_setup's refusal %d" % int(want))
    if R.real_t_neg_count() != 0:
        bad.append("real_t_neg_count")
    for kind, n in (("ortho", N_ORTHO), ("env", N_ENV)):
        for i in range(n):
            key = "%s%d" % (kind, i)
            rd = camera_desc(unpack_camera(d[key + "_camera"]))
            msg = describe(restated_cam_rays(K, rd, d[key + "_samples"]), d[key + "_rays"], RAY21)
            if msg:
                bad.append("cam_ray, %s: %s" % (key, msg))
            cs = restated_cam_rays(K, rd, d[key + "_samples"][:256], camera_space=True)
            if not same_bits(cs[:, 7:9], d[key + "_rays"][:256, 7:9]).all():
                bad.append("cam_ray_camera_space, %s" % key)
    return bad


def generator():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import make_camera_fixtures
    return make_camera_fixtures


@pytest.fixture(scope="module")
def g():
    return dict(np.load(FIXTURE))


def test_the_fixture_holds_what_it_is_there_for(g):
    """the counts the generator asserted, read back from the committed file"""
    for name in NAMES:
        assert g[name + "_bounds"].shape == (64, 4) and g[name + "_clamp_bounds"].shape == (5, 4) and g[name + "_refocus_bounds"].shape == (5, 4)
        for direction in ("film", "scene"):
            out = g["%s_%s_out" % (name, direction)]
            assert len(out) >= 1 << 12 and len(out) // 4 <= out[:, 0].sum() <= 3 * len(out) // 4
        arm, cat = g[name + "_arm"], g[name + "_cat"]
        for a in ((0, 1, 2, 3) if name == "dgauss50" else (0, 1)):
            assert (arm[cat == 0] == a).sum() >= 100
        assert all((cat == c).sum() >= 256 for c in (1, 2, 3))
        for mode in MODES:
            rays = g["%s_%s_rays" % (name, mode)]
            dead = (arm == 0) | (arm >= 4)
            assert (rays[dead, 0] == 0).all() and (rays[~dead, 0] > 0).all() and (rays[:, 21] == (rays[:, 0] > 0)).all()
    assert sorted(g["refusals"][:, 4].tolist()) == [1.0, 2.0, 3.0]
    assert sum(len(g["ortho%d_samples" % i]) for i in range(N_ORTHO)) >= 1 << 12 and sum(len(g["env%d_samples" % i]) for i in range(N_ENV)) >= 1 << 12
    lens = [float(unpack_camera(g["ortho%d_camera" % i])["lens_radius"]) > 0 for i in range(N_ORTHO)]
    moving = [unpack_camera(g["ortho%d_camera" % i])["animated"] for i in range(N_ORTHO)]
    assert any(lens) and not all(lens) and any(moving) and not all(moving) and len({g["ortho%d_camera" % i][0].tobytes() for i in range(N_ORTHO)}) == 2      # two screen windows
    for i in range(N_ENV):
        s = g["env%d_samples" % i]
        assert (s[:, 1] == 0).any() and (s[:, 1] == 36).any() and (s[:, 0] == 0).any() and (s[:, 0] == 48).any()
    assert os.path.getsize(FIXTURE) <= 1 << 20


def test_restatements_equal_the_references_text_on_the_committed_fixture(g):
    bad = hold_restatements(build_realistic_restated(), build_camera_restated(), g)
    assert not bad, "the restatements differ from the reference's text:\n" + "\n".join(bad)


def test_library_setup_and_make_render_desc_equal_the_references_text(g):
    """rspt_realistic_camera_setup (host only) on every setup case byte for byte, the refusals with the reference's wording, and the tables scenes.make_render_desc puts
    into a realistic descriptor"""
    for label, name, (ap, focus, diag), bands, el, box in setups(g):
        got_el, got_b = lib.realistic_camera_setup(lens_data(name), ap, focus, diag, 64)
        assert got_el.tobytes() == el.tobytes(), label
        assert got_b[bands if bands is not None else slice(None)].tobytes() == box.tobytes(), label
    for lens, ap, focus, diag, want in g["refusals"]:
        with pytest.raises(lib.RsptError) as e:
            lib.realistic_camera_setup(lens_data(NAMES[int(lens)]), ap, focus, diag, 2)
        assert e.value.code == abi.E_INVALID and REFUSAL_WORDS[int(want)] in str(e.value), (int(want), str(e.value))
    for name in NAMES:
        ap, focus, diag = (float(v) for v in g[name + "_params"])
        rd = scenes.make_render_desc(48, 36, 4, ((0, 0, 5), (0, 0, 0), (0, 1, 0)), 60.0, camera="realistic", lens=os.path.join(LENS_DIR, name + ".dat"), aperture_diameter=ap,
                                     focus_distance=focus, film_diagonal=diag)
        assert rd.n_lens_elements == len(g[name + "_el"]) and rd.n_exit_pupil_bounds == 64
        assert C.string_at(rd.lens_elements, 16 * rd.n_lens_elements) == g[name + "_el"].tobytes()
        assert C.string_at(rd.exit_pupil_bounds, 16 * 64) == g[name + "_bounds"].tobytes()
        assert F32(rd.film_diagonal) == unpack_camera(g[name + "_simple-still_camera"])["film_diagonal"]


@pytest.mark.skipif(not HAVE_REF, reason="the reference tree is not on this machine: the committed fixture is what travels")
def test_committed_fixture_is_what_the_references_text_gives():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "make_camera_fixtures.py"), "--check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(l[len("compiled from "):].rsplit(" ", 1) for l in r.stdout.splitlines() if l.startswith("compiled from "))
    assert lines["RealisticCamera::generate_ray"] == "cameras/realistic.rs:198-251" and lines["RealisticCamera::generate_ray_differential"] == "cameras/realistic.rs:693-735"
    assert lines["RealisticCamera::trace_lenses_from_film"] == "cameras/realistic.rs:266-327" and lines["RealisticCamera::trace_lenses_from_scene"] == "cameras/realistic.rs:366-421"
    assert lines["RealisticCamera::intersect_spherical_element"] == "cameras/realistic.rs:328-365" and lines["quadratic"] == "core/pbrt.rs:248-268"
    assert lines["RealisticCamera::bound_exit_pupil"] == "cameras/realistic.rs:573-652" and lines["RealisticCamera::sample_exit_pupil"] == "cameras/realistic.rs:656-688"
    assert lines["RealisticCamera::focus_thick_lens"] == "cameras/realistic.rs:483-499" and lines["RealisticCamera::new (interface loop)"] == "cameras/realistic.rs:61-80"
    assert lines["OrthographicCamera::generate_ray_differential"] == "cameras/orthographic.rs:150-235" and lines["EnvironmentCamera::generate_ray_differential"] == "cameras/environment.rs:92-116"
    assert lines["Film::get_physical_extent"] == "core/film.rs:293-307" and lines["bnd2_expand"] == "core/geometry.rs:1010-1015"


@pytest.mark.skipif(not HAVE_REF, reason="needs /root/reference to compile the reference's text")
def test_restatements_equal_the_compiled_reference_text_on_fresh_cases():
    """2^17 fresh samples per camera kind (realistic: 2^15 from a scan per lens and mode, besides the chosen cases) and 2^15 fresh lens-trace rays per lens and direction"""
    mk = generator()
    L, _ = mk.convert()
    R, K = build_realistic_restated(), build_camera_restated()
    d, _ = mk.reference(L, R, per_arm=1024, n_special=512, n_trace=1 << 15, n_other=1 << 17, seed=0x5EEDA, full_setup=False)
    rng = np.random.default_rng(0x5EEDB)
    for name in NAMES:      # the chosen cases hold a few thousand samples: the rest of the 2^17 comes straight from a scan
        extra = rng.random((1 << 15, 5), dtype=F32) * np.array([48, 36, 1, 1, 1], F32)
        d[name + "_samples"] = np.concatenate([d[name + "_samples"], extra])
        d[name + "_arm"] = np.concatenate([d[name + "_arm"], np.zeros(len(extra), np.uint8)])
        for mode in MODES:
            key = "%s_%s" % (name, mode)
            rd = camera_desc(unpack_camera(d[key + "_camera"]), d[name + "_el"], d[name + "_all_bounds"])
            tail, neg = mk.realistic_rays(L, rd, extra)
            assert neg == 0
            d[key + "_rays"] = np.concatenate([d[key + "_rays"], tail])
            d[name + "_arm"][-len(extra):] = real_rays(R, rd, extra)[1]
    assert sum(len(d[n + "_samples"]) for n in NAMES) * len(MODES) >= 1 << 17
    bad = hold_restatements(R, K, d, full_setup=False)
    assert not bad, "the restatements differ from the reference's text:\n" + "\n".join(bad)
