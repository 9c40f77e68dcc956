#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — fifth batch pinned by the reference's OWN TEXT: the realistic, orthographic and environment cameras.  From cameras/realistic.rs:
generate_ray, generate_ray_differential, lens_rear_z, lens_front_z, rear_element_radius, trace_lenses_from_film, intersect_spherical_element,
trace_lenses_from_scene, compute_cardinal_points, compute_thick_lens_approximation, focus_thick_lens, bound_exit_pupil, sample_exit_pupil, and two blocks of
RealisticCamera::new (the interface loop with its aperture clamping, the r0 / r1 lines of the band loop; the crossbeam scaffolding around them is scheduling and
focus_binary_search's result is discarded there: both left out).  From cameras/orthographic.rs: generate_ray_differential and the dx_camera / dy_camera lines of
new.  From cameras/environment.rs: generate_ray_differential.  And what these reach that no earlier batch compiled: quadratic (core/pbrt.rs),
Film::get_physical_extent (core/film.rs), Bounds2f::{diagonal, area, lerp}, pnt2_inside_bnd2f, bnd2_union_pnt2, bnd2_expand (core/geometry.rs).  Compiled by
the earlier batches and reused here, not repeated: refract, radical_inverse, lerp, concentric_sample_disk, nrm_faceforward_vec3, Transform::scale,
Transform::transform_ray / _point / _vector, AnimatedTransform::transform_ray over interpolate, Ray::position, the vector helpers.

Same route as oracle/make_{leaf,geom,flow,shape}_fixtures.py, whose prelude, carriers, rules and compiled functions this script builds on (it imports them): the
Rust text is read from /root/reference where it lies, its SYNTAX is rewritten by the committed rules below (C1 .. C10), the result is compiled as C++ into
oracle/_ref/libcameraref.so (git-ignored, never committed) with g++ -O2 -ffp-contract=off and the platform libm, and tests/golden/camera_functions.npz holds
seeded inputs with that code's outputs.  No function body is edited or typed in by hand.

Hand-written here: the CARRIERS (LensElementInterface; RealisticCamera / OrthographicCamera / EnvironmentCamera with the reference's field names; a Film holding
full_resolution and diagonal; a Bounds2f with the three methods' names; CameraSample and RayDifferential are the flow batch's), and the C wrapper, which moves
values in and out and strings RealisticCamera::new's compiled pieces together in the constructor's order.  The reference's assert!s become a status code by rule
(C3): 1 / 2 the two thick-lens assertions, 3 `c > 0`; `assert!(t >= 0.0)` becomes a counter.

tests/test_reference_camera_functions.py holds tests/realistic_restated.cpp, tests/camera_restated.cpp, rspt_realistic_camera_setup and scenes.make_render_desc to
the fixture, tests/test_gpu_reference_cameras.py the device.  usage: python oracle/make_camera_fixtures.py [--build-only | --check]
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import make_leaf_fixtures as base  # noqa: E402
import make_geom_fixtures as geom  # noqa: E402
import make_flow_fixtures as flow  # noqa: E402
import make_shape_fixtures as shape  # noqa: E402

REF = geom.REF
OUT_DIR = base.OUT_DIR
FIXTURE = os.path.join(ROOT, "tests", "golden", "camera_functions.npz")

CARRIERS = r"""
// ---- carriers of the camera batch (oracle/make_camera_fixtures.py): fields and method names; every body is the reference's text, compiled below ----
namespace camb {
struct Bounds2f {                                      // geometry.rs:1865-1869; #[derive(Default)]: zeros
    Point2f p_min, p_max;
    Vector2f diagonal() const; Float area() const; Point2f lerp(Point2f t) const;
    static Bounds2f default_() { return Bounds2f{Point2f{Float(0.0f), Float(0.0f)}, Point2f{Float(0.0f), Float(0.0f)}}; }
};
struct Film { Point2i full_resolution; Float diagonal; Bounds2f get_physical_extent() const; };      // film.rs:150-176: the two fields the cameras read
struct LensElementInterface { Float curvature_radius, thickness, eta, aperture_radius; };            // realistic.rs:28-33
struct Status { int code = 0; uint64_t t_neg = 0; };                                                 // what the assert!s become (rule C3)
struct FloatSlice { const float* p; size_t n; size_t len() const { return n; } Float operator[](size_t i) const { return Float(p[i]); } };   // `&[Float]`
static inline RayDifferential ray_differential_some(RayDifferential d) { d.some = true; return d; }   // Some(rd)
struct RealisticCamera {                               // realistic.rs:36-47
    AnimatedTransform camera_to_world; Float shutter_open, shutter_close; Film film; MediumRef medium; bool simple_weighting;
    Vec<LensElementInterface> element_interfaces; Vec<Bounds2f> exit_pupil_bounds; Status* status;
    Float generate_ray(const CameraSample& sample, Ray& ray) const; Float generate_ray_differential(const CameraSample& sample, Ray& ray) const;
    Float lens_rear_z() const; Float lens_front_z() const; Float rear_element_radius() const;
    bool trace_lenses_from_film(const Ray& r_camera, Ray* r_out) const; bool trace_lenses_from_scene(const Ray& r_camera, Ray* r_out) const;
    bool intersect_spherical_element(Float radius, Float z_center, const Ray& ray, Float* t, Normal3f* n) const;
    void compute_cardinal_points(const Ray& r_in, const Ray& r_out, size_t idx, Float* pz, Float* fz) const;
    void compute_thick_lens_approximation(Float* pz, Float* fz) const; Float focus_thick_lens(Float focus_distance) const;
    Bounds2f bound_exit_pupil(Float p_film_x0, Float p_film_x1) const; Point3f sample_exit_pupil(Point2f p_film, Point2f lens_sample, Float* sample_bounds_area) const;
};
struct OrthographicCamera {                            // orthographic.rs:19-36 (the fields generate_ray_differential reads)
    AnimatedTransform camera_to_world; Float shutter_open, shutter_close; MediumRef medium; Transform raster_to_camera; Float lens_radius, focal_distance; Vector3f dx_camera, dy_camera;
    Float generate_ray_differential(const CameraSample& sample, Ray& ray) const;
};
struct EnvironmentCamera {                             // environment.rs:20-28
    AnimatedTransform camera_to_world; Float shutter_open, shutter_close; Film film; MediumRef medium;
    Float generate_ray_differential(const CameraSample& sample, Ray& ray) const;
};
bool quadratic(Float a, Float b, Float c, Float* t0, Float* t1);
Bounds2f bnd2_union_pnt2(const Bounds2f& b, Point2f p); bool pnt2_inside_bnd2f(Point2f pt, const Bounds2f& b); Bounds2f bnd2_expand(const Bounds2f& b, Float delta);
}
"""

# (file, search-from regex or None, first-line regex, name, class)
RC = r"^impl RealisticCamera \{"
SOURCES = [
    ("core/pbrt.rs", None, r"^pub fn quadratic\(", "quadratic", None),
    ("core/geometry.rs", r"^impl Bounds2f \{", r"^    pub fn diagonal\(&self\) -> Vector2f \{", "diagonal", "Bounds2f"),
    ("core/geometry.rs", r"^impl Bounds2f \{", r"^    pub fn area\(&self\) -> Float \{", "area", "Bounds2f"),
    ("core/geometry.rs", r"^impl Bounds2f \{", r"^    pub fn lerp\(&self, t: Point2f\) -> Point2f \{", "lerp", "Bounds2f"),
    ("core/geometry.rs", None, r"^pub fn bnd2_union_pnt2\(", "bnd2_union_pnt2", None),
    ("core/geometry.rs", None, r"^pub fn pnt2_inside_bnd2f\(", "pnt2_inside_bnd2f", None),
    ("core/geometry.rs", None, r"^pub fn bnd2_expand\(", "bnd2_expand", None),
    ("core/film.rs", r"^impl Film \{", r"^    pub fn get_physical_extent\(&self\) -> Bounds2f \{", "get_physical_extent", "Film"),
    ("cameras/realistic.rs", RC, r"^    pub fn lens_rear_z\(&self\)", "lens_rear_z", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn lens_front_z\(&self\)", "lens_front_z", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn rear_element_radius\(&self\)", "rear_element_radius", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn intersect_spherical_element\($", "intersect_spherical_element", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn trace_lenses_from_film\(", "trace_lenses_from_film", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn trace_lenses_from_scene\(", "trace_lenses_from_scene", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn compute_cardinal_points\($", "compute_cardinal_points", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn compute_thick_lens_approximation\(", "compute_thick_lens_approximation", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn focus_thick_lens\(", "focus_thick_lens", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn bound_exit_pupil\(", "bound_exit_pupil", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn sample_exit_pupil\($", "sample_exit_pupil", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn generate_ray\(", "generate_ray", "RealisticCamera"),
    ("cameras/realistic.rs", RC, r"^    pub fn generate_ray_differential\(", "generate_ray_differential", "RealisticCamera"),
    ("cameras/orthographic.rs", r"^impl OrthographicCamera \{", r"^    pub fn generate_ray_differential\(", "generate_ray_differential", "OrthographicCamera"),
    ("cameras/environment.rs", r"^impl EnvironmentCamera \{", r"^    pub fn generate_ray_differential\(", "generate_ray_differential", "EnvironmentCamera"),
]
TYPES_EXTRA = {"Option<&mut Ray>": "Ray*", "&mut Normal3f": "Normal3f*", "&mut [Float; 2]": "Float*", "Bounds2f": "Bounds2f", "&Bounds2f": "const Bounds2f&", "Ray": "Ray", "&Ray": "const Ray&",
               "&mut Ray": "Ray&", "&CameraSample": "const CameraSample&", "CameraSample": "CameraSample", "Transform": "Transform", "Normal3f": "Normal3f", "Point3f": "Point3f",
               "Vector2f": "Vector2f", "Point2f": "Point2f", "RayDifferential": "RayDifferential", "LensElementInterface": "LensElementInterface", "f64": "double", "usize": "size_t",
               "i32": "int32_t", "bool": "bool", "&mut Float": "Float*", "Vector3f": "Vector3f"}
LITERALS = ("Point3f", "Vector3f", "Point2f", "Vector2f", "Bounds2f", "LensElementInterface")      # C1: their fields are written in the carrier's declared order

RULES_CAMERA = [
    # C2  the Ray / RayDifferential literals of the three cameras (the flow batch's F13 knows the others), Ray's derived Default (zeros, t_max included), the optional
    #     differential a camera fills field by field
    (r"(medium: |\.medium = )None", r"\1MediumRef{0}", 0),
    (r"Ray \{\s*o: ([^;]*?),\s*d: ([^;]*?),\s*t_max: ([^;]*?),\s*time: ([^;]*?),\s*\.\.Default::default\(\),?\s*\}", r"Ray{\1, \2, \3, \4, RayDifferential{}, MediumRef{0}}", re.S),
    (r"Ray \{\s*o: ([^;]*?),\s*d: ([^;]*?),\s*t_max: ([^;]*?),\s*time: ([^;]*?),\s*medium: MediumRef\{0\},\s*differential: None,?\s*\}", r"Ray{\1, \2, \3, \4, RayDifferential{}, MediumRef{0}}", re.S),
    (r"RayDifferential \{\s*rx_origin,\s*rx_direction: (.*?),\s*ry_origin,\s*ry_direction: (.*?),\s*\}", r"RayDifferential{true, rx_origin, ry_origin, \1, \2}", re.S),
    (r"Ray::default\(\)", "Ray{}", 0), (r"RayDifferential::default\(\)", "RayDifferential{}", 0), (r"Some\(rd\)", "ray_differential_some(rd)", 0),
    # C3  the assert!s: the two thick-lens assertions and `c > 0` set a status code and leave (the caller leaves too); `assert!(t >= 0.0)` counts
    (r"assert!\(\s*(this->trace_lenses_from_(scene|film)\([^;]*?\)),\s*\"[^\"]*\"\s*\);", lambda m: "if (!(%s)) { this->status->code = %d; return; }" % (m.group(1), 1 if m.group(2) == "scene" else 2), re.S),
    (r"(this->compute_thick_lens_approximation\(&mut pz, &mut fz\);)", r"\1 if (this->status->code != 0) { return Float(0.0f); }", 0),
    (r"assert!\(\s*c > 0\.0 as Float,\s*\"[^\"]*\",\s*focus_distance\s*\);", "if (!(c > 0.0 as Float)) { this->status->code = 3; return Float(0.0f); }", re.S),
    (r"assert!\(t >= 0\.0 as Float\);", "if (!(t >= 0.0 as Float)) { this->status->t_neg += 1; }", 0),
    # C4  `Option<&mut Ray>`: a pointer.  Some(&mut x) / Some(ray) -> the address, None -> the null pointer, `if let Some(r_out) = r_out {` -> the test
    (r"Some\(&mut (\w+)\)", r"&mut \1", 0), (r"Some\(ray\)", "&mut ray", 0), (r"if let Some\(r_out\) = r_out \{", "if (r_out != nullptr) {", 0), (r"\bNone\b", "nullptr", 0),
    (r"generate_ray\(&sshift, &mut (\w+)\)", r"generate_ray(sshift, \1)", 0),      # (a `&mut Ray` parameter is a C++ reference: F13)
    # C5  Vec: `.last().unwrap()`, `Vec::new()` under a typed let, `(a.len() - 1).min(i)` on usize, the stepped range over a slice
    (r"\.last\(\)\.unwrap\(\)", ".back()", 0),
    (r"let mut (\w+): Vec<(\w+)> = Vec::new\(\);", r"Vec<\2> \1;", 0),
    (r"\((this->\w+\.len\(\) - 1)\)\.min\((\w+)\)", r"std::min<size_t>(\1, \2)", 0),
    (r"for (\w+) in \(0\.\.(\w+)\.len\(\)\)\.step_by\((\d+)\) \{", r"for (size_t \1 = 0; \1 < \2.len(); \1 += \3) {", 0),
    # C6  the fixed arrays: `for eps in eps_values.iter() {` (eps a pointer to the element, as F17's items), `x += eps`, `&mut pz` of a `[Float; 2]` -> the array
    (r"for (\w+) in (\w+)\.iter\(\) \{", r"for (const Float& \1__v : \2) { const Float* \1 = &\1__v;", 0),
    (r"\+= eps;", "+= *eps;", 0), (r"&mut (pz|fz)\b", r"\1", 0),
    # C7  an untyped `let mut z = 0.0;` whose uses make it a Float; a compound assignment or a swap that ends a block without `;`
    (r"let mut (\w+) = (\d+\.\d+);", r"let mut \1: Float = \2 as Float;", 0),
    (r"^(\s*\w+ \+= [\w.]+)\n(\s*\})", r"\1;\n\2", re.M),
    (r"(std::mem::swap\(&mut \(\*\w+\), &mut \(\*\w+\)\))\n", r"\1;\n", 0),
    # C8  (the first half is applied in rewrite()) Transform's associated functions; `0_u16`
    (r"Transform::(scale|translate|inverse)\(", r"transform_\1(", 0),
    (r"\b(\d+)_u16\b", r"(uint16_t)\1", 0),
    # C9  a borrow of a negated field at a call site: `&-ray.d`
    (r"&-ray\.d", "-ray.d", 0),
]
TYPED_LET = r"\blet (?:mut )?(\w+): (Ray|Transform|Normal3f|Point3f|Point2f|Vector2f|Vector3f|Bounds2f|CameraSample|RayDifferential|LensElementInterface|Float|bool|i32|usize|f64) = "


def rewrite(body, cls, name, sig, params, fn_names):
    """a body through the rules, in order: C1 (struct literals), C2 .. C9, the earlier batches' rules, the typed declarations, shadowing, the block's value"""
    body = flow.join_multiline_if(body)
    body = re.sub(r"\)\n\s*\.floor\(\)", ").floor()", body)      # C8: rustfmt's break in front of a method of a parenthesised expression, then `( .. ).floor() as usize` (G1, ahead of G15)
    body = geom.cast_after_parens(body, "usize", "(size_t)(%s)")
    for lit in LITERALS:
        body = shape.struct_literal(body, lit, lit)
    if cls and name == "lerp":                  # (Rust's free function `lerp` inside a method of the same name: C++ needs the scope spelled out; the flow batch does the same)
        body = re.sub(r"(?<![\w.>:])lerp\(", "::lerp(", body)
    for nm in re.findall(r"Ray& (\w+)", sig):              # C10: a `&mut Ray` is a C++ reference: `*ray = ..` assigns through it
        body = re.sub(r"(?<![\w)\]])\*%s\b" % nm, nm, body)
    for nm in re.findall(r"Normal3f\* (\w+)", sig):        # (F9 of the flow batch) a method call through a `&mut Normal3f` auto-dereferences
        body = re.sub(r"(?<![\w>.*])%s\.(?=\w)" % nm, nm + "->", body)
    for pat, rep, flags in RULES_CAMERA + shape.RULES_SHAPE + flow.RULES_CAM + flow.RULES_FLOW + geom.RULES_INT + geom.RULES_LIGHT + geom.RULES_PRE:
        body = re.sub(pat, rep, body, flags=flags)
    body = geom.cast_after_parens(body, "Float", "Float(%s)")
    body = geom.cast_after_parens(body, "usize", "(size_t)(%s)")
    for pat, rep, flags in base.RULES:
        body = re.sub(pat, rep, body, flags=flags)
    body = re.sub(TYPED_LET, lambda m: "%s %s = " % (base.TYPES.get(m.group(2), m.group(2)), m.group(1)), body)
    body = base.shadowing(body, set(params) | fn_names)
    return body


def new_blocks():
    """the two blocks of RealisticCamera::new and the dx_camera / dy_camera lines of OrthographicCamera::new, each as a function over the carriers (as the flow batch compiles blocks)"""
    out = []
    lines = open(REF + "cameras/realistic.rs").read().split("\n")
    i0 = next(k for k, l in enumerate(lines) if l.strip() == "let mut element_interfaces: Vec<LensElementInterface> = Vec::new();")
    i1 = next(k for k in range(i0, len(lines)) if lines[k].strip() == "let mut camera = RealisticCamera {")
    j0 = next(k for k, l in enumerate(lines) if l.strip() == "let r0: Float =")
    j1 = next(k for k in range(j0, len(lines)) if lines[k].strip() == "*bound = camera.bound_exit_pupil(r0, r1);")
    olines = open(REF + "cameras/orthographic.rs").read().split("\n")
    k0 = next(k for k, l in enumerate(olines) if l.strip() == "let dx_camera: Vector3f = raster_to_camera.transform_vector(&Vector3f {")
    k1 = next(k for k in range(k0, len(olines)) if olines[k].strip() == "OrthographicCamera {")
    for src, fname, a, b, sig, tail, params, label in (
            (lines, "cameras/realistic.rs", i0, i1, "static Vec<LensElementInterface> new_interfaces(FloatSlice lens_data, Float aperture_diameter) {\n",
             "    return element_interfaces;      // (hand-written: the table the constructor stores)\n}\n", {"lens_data", "aperture_diameter"}, "RealisticCamera::new (interface loop)"),
            (lines, "cameras/realistic.rs", j0, j1, "static void new_band(size_t i, size_t n_samples, const Film& film, Float* r0_out, Float* r1_out) {\n",
             "    *r0_out = r0; *r1_out = r1;      // (hand-written: the two radii bound_exit_pupil receives)\n}\n", {"i", "n_samples", "film"}, "RealisticCamera::new (band radii)"),
            (olines, "cameras/orthographic.rs", k0, k1, "static void ortho_new_block(const Transform& raster_to_camera, Vector3f* dx_out, Vector3f* dy_out) {\n",
             "    *dx_out = dx_camera; *dy_out = dy_camera;      // (hand-written: the two vectors the constructor stores)\n}\n", {"raster_to_camera"}, "OrthographicCamera::new (dx_camera, dy_camera)")):
        indent = len(src[a]) - len(src[a].lstrip())
        text = "\n".join(("    " + l[indent:]) if l.strip() else "" for l in src[a:b])
        body = re.sub(r"^\s*//.*\n", "", text, flags=re.M) + "\n}\n"
        body = rewrite(body, None, label, sig, set(params), set(geom.FN_NAMES))
        out.append(("// %s%s:%d-%d\n%s%s" % (REF, fname, a + 1, b, sig, body.rstrip()[:-1].rstrip() + "\n" + tail), "%s %s:%d-%d" % (label, fname, a + 1, b)))
    return out


def convert_parts():
    saved = (dict(geom.TYPES), dict(base.TYPES), dict(flow.TYPES))
    try:
        return _convert_parts()
    finally:
        geom.TYPES.clear(); geom.TYPES.update(saved[0]); base.TYPES.clear(); base.TYPES.update(saved[1]); flow.TYPES.clear(); flow.TYPES.update(saved[2])


def _convert_parts():
    parts, where = shape.convert_parts()       # the four earlier batches: prelude, carriers and every function they compile (their spans come first in `where`)
    where = list(where)
    parts.append(CARRIERS)
    types = dict(geom.TYPES)
    types.update(TYPES_EXTRA)
    fn_names = set(geom.FN_NAMES) | {s[3] for s in SOURCES}
    code = []
    for fname, after_re, first_re, name, cls in SOURCES:
        for tab in (geom.TYPES, base.TYPES):
            tab.clear(); tab.update(types)
            tab["Self"] = cls or "Float"
        text, l0, l1 = geom.extract(fname, after_re, first_re, None)
        text = re.sub(r"^\s*//.*\n", "", text, flags=re.M)                      # comment lines
        sig, body, params = geom.signature(text, name, cls)
        body = rewrite(body, cls, name, sig, params, fn_names)
        if not sig.startswith("void"):
            body = geom.tail_value(body)
        code.append("// %s%s:%d-%d\n%s%s" % (REF, fname, l0, l1, sig, body))
        where.append("%s%s %s:%d-%d" % ((cls + "::") if cls else "", name, fname, l0, l1))
    for tab in (geom.TYPES, base.TYPES):
        tab.clear(); tab.update(types)
    for text, label in new_blocks():
        code.append(text)
        where.append(label)
    parts.append("namespace camb {\n" + "\n".join(code) + "}\n")
    return parts, where


WRAPPERS = r"""
// ---- the C wrapper: values are moved, RealisticCamera::new's compiled pieces run in the constructor's order; nothing is computed here ----
namespace camb {
static inline Matrix4x4 mat_of(const float* m) { Matrix4x4 r; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.m[i][j] = Float(m[4 * i + j]); return r; }
static AnimatedTransform animated_of(const rspt_render_desc& rd) {      // AnimatedTransform::new (transform.rs:911-932) over the compiled decompose, as the flow batch's hooks build it
    AnimatedTransform at{};
    const float* end = rd.camera_animated ? rd.camera_to_world_end : rd.camera_to_world;
    at.start_transform = Transform{mat_of(rd.camera_to_world), matrix4x4_inverse(mat_of(rd.camera_to_world))};
    at.end_transform = Transform{mat_of(end), matrix4x4_inverse(mat_of(end))};
    at.start_time = Float(rd.camera_animated ? rd.camera_time[0] : 0.0f); at.end_time = Float(rd.camera_animated ? rd.camera_time[1] : 1.0f);
    at.actually_animated = std::memcmp(rd.camera_to_world, end, 64) != 0;
    AnimatedTransform::decompose(at.start_transform.m, &at.t[0], &at.r[0], &at.s[0]);
    AnimatedTransform::decompose(at.end_transform.m, &at.t[1], &at.r[1], &at.s[1]);
    if (quat_dot_quat(at.r[0], at.r[1]) < Float(0.0f)) at.r[1] = -at.r[1];
    at.has_rotation = quat_dot_quat(at.r[0], at.r[1]) < Float(0.9995f);
    return at;
}
static RealisticCamera table_camera(const rspt_lens_element* el, uint32_t n, Float diagonal, Status* st) {
    RealisticCamera cam{};
    cam.status = st; cam.film = Film{Point2i{1, 1}, diagonal}; cam.shutter_open = Float(0.0f); cam.shutter_close = Float(1.0f); cam.simple_weighting = true; cam.medium = MediumRef{0};
    for (uint32_t i = 0; i < n; i++) cam.element_interfaces.push(LensElementInterface{Float(el[i].curvature_radius), Float(el[i].thickness), Float(el[i].eta), Float(el[i].aperture_radius)});
    return cam;
}
static inline void put_ray22(Float w, const Ray& ray, float* o) {      // rspt_camera_rays' layout
    o[0] = w.v; o[1] = ray.o.x.v; o[2] = ray.o.y.v; o[3] = ray.o.z.v; o[4] = ray.d.x.v; o[5] = ray.d.y.v; o[6] = ray.d.z.v; o[7] = ray.t_max.get().v; o[8] = ray.time.v;
    const RayDifferential& d = ray.differential;
    const Float v[12] = {d.rx_origin.x, d.rx_origin.y, d.rx_origin.z, d.rx_direction.x, d.rx_direction.y, d.rx_direction.z, d.ry_origin.x, d.ry_origin.y, d.ry_origin.z, d.ry_direction.x, d.ry_direction.y, d.ry_direction.z};
    for (int k = 0; k < 12; k++) o[9 + k] = d.some ? v[k].v : 0.0f;
    o[21] = d.some ? 1.0f : 0.0f;
}
extern "C" {
// RealisticCamera::new (realistic.rs:50-144): the interface loop, focus_thick_lens into the last thickness, then bound_exit_pupil for the listed bands of n_bounds.
// 0 and the element table / the listed bands' boxes (p_min.x, p_min.y, p_max.x, p_max.y), or 1 / 2 / 3: the assertion that fails.  *t_neg: how often assert!(t >= 0) would fire.
int camref_setup(const float* lens_data, uint32_t n_elements, float aperture_diameter_mm, float focus_distance, float film_diagonal_mm, uint32_t n_bounds, const uint32_t* bands, uint32_t n_bands,
                 rspt_lens_element* elements_out, float* bounds_out, uint64_t* t_neg, int threads) {
    Status st;
    RealisticCamera camera{};
    camera.status = &st; camera.shutter_open = Float(0.0f); camera.shutter_close = Float(1.0f); camera.simple_weighting = true; camera.medium = MediumRef{0};
    camera.film = Film{Point2i{1, 1}, Float(film_diagonal_mm) * Float(0.001f)};                               // Film::new, film.rs:214: `diagonal: diagonal * 0.001`
    camera.element_interfaces = new_interfaces(FloatSlice{lens_data, 4 * (size_t)n_elements}, Float(aperture_diameter_mm));      // :61-80
    const Float thickness = camera.focus_thick_lens(Float(focus_distance));                                   // :95-96 (:92, focus_binary_search: its result is discarded)
    if (t_neg) *t_neg = st.t_neg;
    if (st.code != 0) return st.code;
    camera.element_interfaces.back().thickness = thickness;
    for (uint32_t i = 0; i < n_elements; i++) { const LensElementInterface& e = camera.element_interfaces[i]; elements_out[i] = rspt_lens_element{e.curvature_radius.v, e.thickness.v, e.eta.v, e.aperture_radius.v}; }
    std::atomic<uint32_t> next{0};
    std::atomic<uint64_t> negs{0};
    auto worker = [&]() {
        Status mine; RealisticCamera c = camera; c.status = &mine;
        for (;;) {
            const uint32_t k = next.fetch_add(1);
            if (k >= n_bands) break;
            Float r0, r1;
            new_band((size_t)bands[k], (size_t)n_bounds, c.film, &r0, &r1);                                   // :118-121
            const Bounds2f b = c.bound_exit_pupil(r0, r1);                                                    // :122
            bounds_out[4 * k] = b.p_min.x.v; bounds_out[4 * k + 1] = b.p_min.y.v; bounds_out[4 * k + 2] = b.p_max.x.v; bounds_out[4 * k + 3] = b.p_max.y.v;
        }
        negs += mine.t_neg;
    };
    std::vector<std::thread> th;
    for (int t = 1; t < threads; t++) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
    if (t_neg) *t_neg += negs.load();
    return 0;
}
// trace_lenses_from_film (from_scene = 0) / trace_lenses_from_scene (1) over an element table in metres: rays n x 6 (o, d; t_max inf, time 0) -> out n x 8 (pass, o, d, t_max; zeros where it fails)
uint64_t camref_trace(const rspt_lens_element* elements, uint32_t n_elements, int from_scene, const float* rays, uint64_t n, float* out) {
    Status st;
    const RealisticCamera cam = table_camera(elements, n_elements, Float(0.0f), &st);
    for (uint64_t i = 0; i < n; i++) {
        const float* q = rays + 6 * i; float* o = out + 8 * i;
        Ray r{}; r.o = Point3f{Float(q[0]), Float(q[1]), Float(q[2])}; r.d = Vector3f{Float(q[3]), Float(q[4]), Float(q[5])}; r.t_max.v = Float(INFINITY); r.medium = MediumRef{0};
        Ray r_out{};
        const bool ok = from_scene ? cam.trace_lenses_from_scene(r, &r_out) : cam.trace_lenses_from_film(r, &r_out);
        for (int k = 0; k < 8; k++) o[k] = 0.0f;
        if (ok) { o[0] = 1.0f; o[1] = r_out.o.x.v; o[2] = r_out.o.y.v; o[3] = r_out.o.z.v; o[4] = r_out.d.x.v; o[5] = r_out.d.y.v; o[6] = r_out.d.z.v; o[7] = r_out.t_max.get().v; }
    }
    return st.t_neg;
}
// compute_thick_lens_approximation over an element table and a film diagonal in metres: pz[2], fz[2]; 0 or the failing assertion
int camref_cardinal_points(const rspt_lens_element* elements, uint32_t n_elements, float film_diagonal, float pz[2], float fz[2]) {
    Status st;
    const RealisticCamera cam = table_camera(elements, n_elements, Float(film_diagonal), &st);
    Float p[2] = {}, f[2] = {};
    cam.compute_thick_lens_approximation(p, f);
    for (int k = 0; k < 2; k++) { pz[k] = p[k].v; fz[k] = f[k].v; }
    return st.code;
}
// RealisticCamera::generate_ray_differential over the desc's own tables: samples n x 5 (p_film, time, p_lens) -> out n x 22 (rspt_camera_rays' layout).  Returns the t < 0 count.
uint64_t camref_realistic_rays(const rspt_render_desc* rd, const float* samples, uint64_t n, float* out) {
    Status st;
    RealisticCamera cam = table_camera(rd->lens_elements, rd->n_lens_elements, Float(rd->film_diagonal), &st);
    cam.film.full_resolution = Point2i{rd->full_res[0], rd->full_res[1]};
    cam.camera_to_world = animated_of(*rd); cam.shutter_open = Float(rd->shutter_open); cam.shutter_close = Float(rd->shutter_close); cam.simple_weighting = rd->lens_simple_weighting != 0;
    for (uint32_t i = 0; i < rd->n_exit_pupil_bounds; i++) { const float* b = rd->exit_pupil_bounds + 4 * i; cam.exit_pupil_bounds.push(Bounds2f{Point2f{Float(b[0]), Float(b[1])}, Point2f{Float(b[2]), Float(b[3])}}); }
    for (uint64_t i = 0; i < n; i++) {
        const float* s = samples + 5 * i;
        Ray ray{};                                                                                          // Ray::default()
        const Float w = cam.generate_ray_differential(CameraSample{Point2f{Float(s[0]), Float(s[1])}, Float(s[2]), Point2f{Float(s[3]), Float(s[4])}}, ray);
        put_ray22(w, ray, out + 22 * i);
    }
    return st.t_neg;
}
// OrthographicCamera / EnvironmentCamera::generate_ray_differential by rd->camera_kind: samples n x 5 -> out n x 21 (tests/camera_restated.cpp's cam_ray layout: o, d, t_max, time, has_diff,
// rx_o, rx_d, ry_o, ry_d; the differential's words are zero where the camera leaves `differential: None`)
int camref_cam_rays(const rspt_render_desc* rd, const float* samples, uint64_t n, float* out) {
    const AnimatedTransform c2w = animated_of(*rd);
    OrthographicCamera oc{}; EnvironmentCamera ec{};
    if (rd->camera_kind == RSPT_CAMERA_ORTHOGRAPHIC) {
        oc.camera_to_world = c2w; oc.shutter_open = Float(rd->shutter_open); oc.shutter_close = Float(rd->shutter_close); oc.medium = MediumRef{0};
        oc.raster_to_camera = Transform{mat_of(rd->raster_to_camera), matrix4x4_inverse(mat_of(rd->raster_to_camera))}; oc.lens_radius = Float(rd->lens_radius); oc.focal_distance = Float(rd->focal_distance);
        ortho_new_block(oc.raster_to_camera, &oc.dx_camera, &oc.dy_camera);                                 // orthographic.rs:73-82
    } else if (rd->camera_kind == RSPT_CAMERA_ENVIRONMENT) {
        ec.camera_to_world = c2w; ec.shutter_open = Float(rd->shutter_open); ec.shutter_close = Float(rd->shutter_close); ec.medium = MediumRef{0};
        ec.film = Film{Point2i{rd->full_res[0], rd->full_res[1]}, Float(0.0f)};
    } else return -1;
    for (uint64_t i = 0; i < n; i++) {
        const float* s = samples + 5 * i; float* o = out + 21 * i;
        const CameraSample cs{Point2f{Float(s[0]), Float(s[1])}, Float(s[2]), Point2f{Float(s[3]), Float(s[4])}};
        Ray ray{};
        if (rd->camera_kind == RSPT_CAMERA_ORTHOGRAPHIC) oc.generate_ray_differential(cs, ray); else ec.generate_ray_differential(cs, ray);
        const RayDifferential& d = ray.differential;
        const Float v[21] = {ray.o.x, ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z, ray.t_max.get(), ray.time, Float(d.some ? 1.0f : 0.0f), d.rx_origin.x, d.rx_origin.y, d.rx_origin.z,
                             d.rx_direction.x, d.rx_direction.y, d.rx_direction.z, d.ry_origin.x, d.ry_origin.y, d.ry_origin.z, d.ry_direction.x, d.ry_direction.y, d.ry_direction.z};
        for (int k = 0; k < 21; k++) o[k] = (k < 9 || d.some) ? v[k].v : 0.0f;
    }
    return 0;
}
}
}
"""


def convert():
    parts, where = convert_parts()
    parts.append(WRAPPERS)
    os.makedirs(OUT_DIR, exist_ok=True)
    cpp = os.path.join(OUT_DIR, "camera_functions.cpp")
    open(cpp, "w").write("\n".join(parts))
    so = os.path.join(OUT_DIR, "libcameraref.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), "-o", so, cpp])
    L = C.CDLL(so)
    vp, f, u32, u64 = C.c_void_p, C.c_float, C.c_uint32, C.c_uint64
    L.camref_setup.restype = C.c_int
    L.camref_setup.argtypes = [vp, u32, f, f, f, u32, vp, u32, vp, vp, vp, C.c_int]
    L.camref_trace.restype = u64
    L.camref_trace.argtypes = [vp, u32, C.c_int, vp, u64, vp]
    L.camref_cardinal_points.restype = C.c_int
    L.camref_cardinal_points.argtypes = [vp, u32, f, vp, vp]
    L.camref_realistic_rays.restype = u64
    L.camref_realistic_rays.argtypes = [vp, vp, u64, vp]
    L.camref_cam_rays.restype = C.c_int
    L.camref_cam_rays.argtypes = [vp, vp, u64, vp]
    return L, where


# ---------------------------------------------------------------- running the text ----------------------------------------------------------------
F32 = np.float32
NAMES = ("dgauss50", "singlet")
MODES = ("simple-still", "physical-moving")
PART_BANDS = (0, 1, 31, 62, 63)                # the bands of the variant setups (each band costs 2^20 lens traces)
XRES, YRES = 48, 36                            # the frame of tests/test_realistic_host.py's lens_desc
N_BOUNDS = 64


def lens_params(name):
    """(lens data (n, 4), aperture diameter mm, focus distance, film diagonal mm) at the parameters of LENSES in tests/test_realistic_host.py"""
    from rs_pbrt_amd import scenes
    from tests.test_realistic_host import LENSES
    path, diag, ap, focus = LENSES[name]
    return scenes.read_lens_file(path), ap, focus, diag


def setup(L, data, aperture, focus, diagonal, bands=None, n_bounds=N_BOUNDS, threads=16):
    """RealisticCamera::new by the text: (status, elements (n, 4) f32, the listed bands' boxes (len(bands), 4) f32, t < 0 count)"""
    data = np.ascontiguousarray(data, F32).reshape(-1, 4)
    bands = np.arange(n_bounds, dtype=np.uint32) if bands is None else np.ascontiguousarray(bands, np.uint32)
    el, box, neg = np.zeros((len(data), 4), F32), np.zeros((len(bands), 4), F32), C.c_uint64(0)
    st = L.camref_setup(data.ctypes.data, len(data), aperture, focus, diagonal, n_bounds, bands.ctypes.data, len(bands), el.ctypes.data, box.ctypes.data, C.addressof(neg), threads)
    return st, el, box, neg.value


def trace(L, el, from_scene, rays):
    """trace_lenses_from_film / _from_scene by the text: (n, 8) f32 (pass, o, d, t_max), t < 0 count"""
    el, rays = np.ascontiguousarray(el, F32), np.ascontiguousarray(rays, F32).reshape(-1, 6)
    out = np.zeros((len(rays), 8), F32)
    neg = L.camref_trace(el.ctypes.data, len(el), int(from_scene), rays.ctypes.data, len(rays), out.ctypes.data)
    return out, neg


def _helpers():
    import tests.test_reference_camera_functions as t      # the descriptor helpers live with the tests that read the committed file alone (they need no reference tree)
    return t


def camera_desc(cam, el=None, bounds=None):
    return _helpers().camera_desc(cam, el, bounds)


def camera_of_desc(rd):
    return _helpers().camera_of_desc(rd)


def pack_camera(cam):
    return _helpers().pack_camera(cam)


def cardinal_points(L, el, film_diagonal_m):
    """compute_thick_lens_approximation by the text over an element table in metres: (status, [pz[0], pz[1], fz[0], fz[1]] f32)"""
    el, out = np.ascontiguousarray(el, F32), np.zeros(4, F32)
    st = L.camref_cardinal_points(el.ctypes.data, len(el), float(film_diagonal_m), out[:2].ctypes.data, out[2:].ctypes.data)
    return st, out


def realistic_rays(L, rd, samples):
    """RealisticCamera::generate_ray_differential by the text over the desc's tables: (n, 22) f32 in rspt_camera_rays' layout, t < 0 count"""
    smp = np.ascontiguousarray(samples, F32).reshape(-1, 5)
    out = np.zeros((len(smp), 22), F32)
    neg = L.camref_realistic_rays(C.addressof(rd), smp.ctypes.data, len(smp), out.ctypes.data)
    return out, neg


def cam_rays(L, rd, samples):
    """OrthographicCamera / EnvironmentCamera::generate_ray_differential by the text: (n, 21) f32 in cam_ray's layout"""
    smp = np.ascontiguousarray(samples, F32).reshape(-1, 5)
    out = np.zeros((len(smp), 21), F32)
    assert L.camref_cam_rays(C.addressof(rd), smp.ctypes.data, len(smp), out.ctypes.data) == 0
    return out


# ---------------------------------------------------------------- seeded inputs ----------------------------------------------------------------
SEED = 0xCA3E7A
REFUSALS = (("dgauss50", None, 0.05, 3), ("dgauss50", 1e-4, None, 1), ("singlet", 0.046, None, 2))      # (lens, aperture or the lens' own, focus distance or the lens' own, the status the text gives)
ORTHO_CAMERAS = (dict(), dict(lens_radius=0.05, focal_distance=6.0), dict(screen_window=(-0.5, 1.25, -0.75, 0.5), moving=True), dict(screen_window=(-0.5, 1.25, -0.75, 0.5), lens_radius=0.125, focal_distance=3.5, moving=True),
                 dict(moving=True), dict(screen_window=(-0.5, 1.25, -0.75, 0.5), lens_radius=0.05, focal_distance=6.0))


def mode_kw(mode):
    """the two descriptors tests/test_gpu_realistic.py::test_camera_rays_hook builds"""
    from tests.test_camera_host import LOOK_END
    return {} if mode == "simple-still" else dict(simple_weighting=False, shutter=(0.0, 0.5), look_at_end=LOOK_END, camera_times=(0.1, 0.45))


def realistic_camera(name, mode):
    """the camera of lens `name` under `mode`, without its tables: what scenes.make_render_desc puts into the descriptor beside them"""
    from rs_pbrt_amd import abi, scenes
    from tests.util import GALLERY_LOOK_AT
    kw = mode_kw(mode)
    simple = kw.pop("simple_weighting", True)
    cam = camera_of_desc(scenes.make_render_desc(XRES, YRES, 4, GALLERY_LOOK_AT, 60.0, **kw))
    cam.update(kind=abi.CAMERA_REALISTIC, film_diagonal=F32(lens_params(name)[3]) * F32(0.001), simple_weighting=int(simple))      # Film::new (film.rs:214)
    return cam


def other_camera(kind, spec):
    from rs_pbrt_amd import scenes
    from tests.test_camera_host import LOOK_END
    from tests.util import GALLERY_LOOK_AT
    spec = dict(spec)
    kw = dict(look_at_end=LOOK_END, camera_times=(0.1, 0.45), shutter=(0.0, 0.5)) if spec.pop("moving", False) else {}
    return camera_of_desc(scenes.make_render_desc(XRES, YRES, 4, GALLERY_LOOK_AT, 60.0, camera=kind, **kw, **spec))


def grid(rng, shape, bits=12):
    """uniform numbers in [0, 1) on a 2^-bits grid (their f32 words keep the fixture small)"""
    return (rng.integers(0, 1 << bits, shape) / float(1 << bits)).astype(F32)


def film_rays(rng, el, diagonal_m, n):
    """rays as bound_exit_pupil casts them: from a film point on the half diagonal (x in [0, diagonal / 2), y = 0) towards a point of the 1.5 x rear-radius box in the
    plane of the rear element; every other one towards the inner 0.45 x rear-radius part of that box, where most of the exit pupil lies"""
    rear_z, rear_r = F32(el[-1, 1]), F32(el[-1, 3])
    x = F32(diagonal_m) / F32(2) * grid(rng, n)
    f = np.where(np.arange(n) % 2 == 0, F32(1.5), F32(0.45)).astype(F32)[:, None]
    pr = -f * rear_r + F32(2) * f * rear_r * grid(rng, (n, 2))
    z = np.zeros(n, F32)
    rays = np.stack([x, z, z, pr[:, 0] - x, pr[:, 1], np.full(n, rear_z, F32)], 1)
    # the first four: from the film centre to the rear element's rim on the axes.  Where the rear element is the stop (the singlet) t is exactly 1, p_hit is the rim point
    # itself and r2 == aperture_radius^2 exactly: the ray passes by `r2 > ..`, and would not by `>=`
    rays[:4] = [[0, 0, 0, sx * rear_r, sy * rear_r, rear_z] for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1))]
    return rays


def scene_rays(rng, el, n):
    """parallel bundles arriving obliquely (up to 20 degrees off the axis, 17 x 8 directions) at the front element: origins on the plane 1 cm in front of it, within 1.2 x
    (every other one: 0.3 x) the front element's aperture radius"""
    front_z, front_r = el[:, 1].sum(dtype=F32), F32(el[0, 3])
    th, ph = np.radians(20.0) * rng.integers(0, 17, n) / 16, 2 * np.pi * rng.integers(0, 8, n) / 8
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], 1).astype(F32)
    f = np.where(np.arange(n) % 2 == 0, F32(1.2), F32(0.3)).astype(F32)[:, None]
    t = -f * front_r + F32(2) * f * front_r * grid(rng, (n, 2))
    return np.concatenate([t, np.full((n, 1), front_z + F32(0.01), F32), d], 1).astype(F32)


def r_film_of(cam, p_film):
    """sample_exit_pupil's r_film and band index of CameraSample positions, in numpy's f32 arithmetic (IEEE, as the text's): for CHOOSING samples near a band border only"""
    xres, yres, diag = F32(cam["xres"]), F32(cam["yres"]), F32(cam["film_diagonal"])
    aspect = yres / xres
    ex = np.sqrt(diag * diag / (F32(1) + aspect * aspect)); ey = aspect * ex
    s = np.asarray(p_film, F32) / np.array([xres, yres], F32)
    lerp = lambda t, a, b: a * (F32(1) - t) + b * t      # noqa: E731
    px, py = -lerp(s[:, 0], -ex / F32(2), ex / F32(2)), lerp(s[:, 1], -ey / F32(2), ey / F32(2))
    r = np.sqrt(px * px + py * py)
    return r, np.floor(r / (diag / F32(2)) * F32(N_BOUNDS))


def border_samples(rng, cam, n):
    """CameraSamples whose r_film lies within 2 ulps of the smallest r_film of a band, half of them below it and half at or above it: p_film.x walks bit by bit over the place
    where the band index changes, on three rows of the frame"""
    lo_side, hi_side = [], []
    for y in (F32(YRES) / 2, F32(7.25), F32(30.5)):
        for k in range(1, N_BOUNDS):
            a, b = F32(0.0), F32(XRES) / 2      # r_film falls as p_film.x runs from the left edge to the middle
            ia, ib = r_film_of(cam, [[a, y]])[1][0], r_film_of(cam, [[b, y]])[1][0]
            if not (ia >= k > ib):
                continue
            ba, bb = int(a.view(np.uint32)), int(b.view(np.uint32))
            while bb - ba > 1:
                m = (ba + bb) // 2
                if r_film_of(cam, [[np.uint32(m).view(F32), y]])[1][0] >= k:
                    ba = m
                else:
                    bb = m
            xs = np.arange(ba - 3, bb + 4, dtype=np.uint32).view(F32)
            r, idx = r_film_of(cam, np.stack([xs, np.full(len(xs), y, F32)], 1))
            border = r[idx >= k].min()      # the smallest r_film of band k on this row
            ulps = r.view(np.uint32).astype(np.int64) - int(border.view(np.uint32))
            for x, u, i in zip(xs, ulps, idx):
                if abs(u) <= 2:
                    (hi_side if i >= k else lo_side).append((x, y))
    assert len(lo_side) >= n // 2 and len(hi_side) >= n // 2, (len(lo_side), len(hi_side))
    pick = [lo_side[i] for i in rng.choice(len(lo_side), n // 2, replace=False)] + [hi_side[i] for i in rng.choice(len(hi_side), n - n // 2, replace=False)]
    return np.concatenate([np.array(pick, F32), grid(rng, (n, 3))], 1)


def special_samples(rng, cam, n):
    """(samples, category): 1 p_film exactly at the film centre (r_film == 0), 2 r_film within 2 ulps of a band border, 3 the frame's last row and column — a quarter of
    them within 0.05 of the far corner, where the differential's shifted samples leave the film and r_index is clamped"""
    centre = np.concatenate([np.tile(np.array([XRES / 2, YRES / 2], F32), (n, 1)), grid(rng, (n, 3))], 1)
    assert (r_film_of(cam, centre[:, :2])[0] == 0).all()
    border = border_samples(rng, cam, n)
    last = np.concatenate([grid(rng, (n, 2)) * np.array([XRES, YRES], F32), grid(rng, (n, 3))], 1)
    k = np.arange(n) % 4
    last[k == 0, 0] = F32(XRES - 1) + grid(rng, (k == 0).sum())
    last[k == 1, 1] = F32(YRES - 1) + grid(rng, (k == 1).sum())
    last[k == 2, 0] = F32(XRES - 1) + grid(rng, (k == 2).sum()); last[k == 2, 1] = F32(YRES - 1) + grid(rng, (k == 2).sum())
    last[k == 3, 0] = F32(XRES) - F32(0.05) * grid(rng, (k == 3).sum()) - F32(2.0 ** -12); last[k == 3, 1] = F32(YRES) - F32(0.05) * grid(rng, (k == 3).sum()) - F32(2.0 ** -12)
    return np.concatenate([centre, border, last]).astype(F32), np.repeat(np.array([1, 2, 3], np.uint8), n)


def realistic_cases(L, R, name, mode, el, bounds, per_arm, n_special, seed):
    """one lens and mode: the camera, the chosen samples, their category (0: from the scan, by arm) and the restatement's arm (which chooses cases only)"""
    from tests.test_realistic_host import real_rays, scan_samples
    cam = realistic_camera(name, mode)
    rd = camera_desc(cam, el, bounds)
    smp, _, arms = scan_samples(R, rd, seed=seed)
    need = (0, 1, 2, 3) if name == "dgauss50" else (0, 1)
    pick = []
    for a in range(6):
        found = np.flatnonzero(arms == a)
        assert len(found) >= 100 or a not in need, (name, mode, a, len(found))      # (what tests/test_realistic_host.py::test_every_arm_occurs guarantees of such a scan)
        assert len(found) == 0 or name == "dgauss50" or a in need
        pick.append(found[:per_arm if a in need else 1024])
    pick = np.concatenate(pick)
    sp, cat = special_samples(np.random.default_rng(seed ^ 0x5BEC), cam, n_special)
    samples = np.concatenate([smp[pick], sp])
    _, arm = real_rays(R, rd, samples)
    return cam, rd, samples, np.concatenate([np.zeros(len(pick), np.uint8), cat]), arm.astype(np.uint8)


def check_arms(rays, arm, what):
    """the text's weight and has_diff agree with what each arm means"""
    dead = (arm == 0) | (arm >= 4)
    assert (rays[dead, 0] == 0).all() and (rays[dead, 21] == 0).all() and (rays[~dead, 0] > 0).all() and (rays[~dead, 21] == 1).all(), what
    assert (rays[arm == 0, 1:] == 0).all(), what      # a vignetted primary ray leaves Ray::default()


def other_samples(rng, n, edges):
    """CameraSamples on a 2^-12 grid over the frame; with `edges`, the first 64 sit on the frame's four edges (p_film.y at 0 and full_res.y: the environment camera's poles)"""
    s = np.concatenate([grid(rng, (n, 2)) * np.array([XRES, YRES], F32), grid(rng, (n, 3))], 1)
    if edges:
        k = np.arange(64) % 4
        s[:64][k == 0, 1] = 0; s[:64][k == 1, 1] = YRES; s[:64][k == 2, 0] = 0; s[:64][k == 3, 0] = XRES
    return s.astype(F32)


def reference(L, R, per_arm=104, n_special=256, n_trace=1 << 12, n_other=1 << 12, seed=SEED, full_setup=True):
    """inputs and the text's outputs as the fixture's arrays; the generator's own conditions on them are asserted here.  R: tests/realistic_restated.cpp, built (its arms
    choose cases).  full_setup False: only the two main setups, PART_BANDS of them (the fresh-sample test)"""
    from rs_pbrt_amd import abi
    d, stats = {}, {}
    rng = np.random.default_rng(seed)
    for name in NAMES:
        data, ap, focus, diag = lens_params(name)
        stop_d = float(data[data[:, 0] == 0][0, 3])
        st, el, box, neg = setup(L, data, ap, focus, diag, None if full_setup else PART_BANDS)
        assert st == 0 and neg == 0
        d[name + "_params"], d[name + "_el"], d[name + "_bounds"] = np.array([ap, focus, diag], F32), el, box
        st, d[name + "_cardinal"] = cardinal_points(L, el, F32(diag) * F32(0.001))      # (of the focused table)
        assert st == 0
        if full_setup:
            for tag, (a2, f2) in (("clamp", (2.0 * stop_d, focus)), ("refocus", (ap, 1.5 * focus))):      # an aperture larger than the stop's own diameter; a second focus distance
                st, el2, box2, neg = setup(L, data, a2, f2, diag, PART_BANDS)
                assert st == 0 and neg == 0
                d["%s_%s_params" % (name, tag)], d["%s_%s_el" % (name, tag)], d["%s_%s_bounds" % (name, tag)] = np.array([a2, f2, diag], F32), el2, box2
            stop = int(np.flatnonzero(data[:, 0] == 0)[0])
            assert d[name + "_clamp_el"][stop, 3] == data[stop, 3] * F32(0.001) / F32(2) and d[name + "_el"][stop, 3] == F32(ap) * F32(0.001) / F32(2)      # the clamping branch, and the other one
            assert d[name + "_refocus_el"][-1, 1] != el[-1, 1] and (d[name + "_refocus_el"][:-1] == el[:-1]).all()
        else:
            box = d[name + "_all_bounds"] = setup(L, data, ap, focus, diag)[2]      # (the ray cases need all 64 boxes)
        for direction, rays in (("film", film_rays(rng, el, diag * 0.001, n_trace)), ("scene", scene_rays(rng, el, n_trace))):
            out, neg = trace(L, el, direction == "scene", rays)
            assert neg == 0 and len(rays) // 4 <= out[:, 0].sum() <= 3 * len(rays) // 4, (name, direction, out[:, 0].mean())      # between a quarter and three quarters pass by the text
            d["%s_%s_rays" % (name, direction)], d["%s_%s_out" % (name, direction)] = rays, out
            stats["%s %s trace" % (name, direction)] = "%d of %d pass" % (int(out[:, 0].sum()), len(rays))
        for mode in MODES:
            cam, rd, samples, cat, arm = realistic_cases(L, R, name, mode, el, box, per_arm, n_special, seed=17 if seed == SEED else seed & 0xFFFF)
            rays, neg = realistic_rays(L, rd, samples)
            assert neg == 0
            check_arms(rays, arm, (name, mode))
            for c in (1, 2, 3):
                assert (cat == c).sum() >= min(256, n_special)
            key = "%s_%s" % (name, mode)
            if mode != MODES[0]:      # (a lens' samples are stored once: the scan and the special cases depend on the lens and its tables, not on the mode)
                assert np.array_equal(d[name + "_samples"].view(np.uint32), samples.view(np.uint32)) and np.array_equal(d[name + "_cat"], cat) and np.array_equal(d[name + "_arm"], arm)
            d[key + "_camera"], d[name + "_samples"], d[name + "_cat"], d[name + "_arm"], d[key + "_rays"] = pack_camera(cam), samples, cat, arm, rays
            stats[key] = "%d samples, arms %s, weight 0 in %d" % (len(samples), np.bincount(arm, minlength=6).tolist(), int((rays[:, 0] == 0).sum()))
    if full_setup:
        codes = []
        for name, a2, f2, want in REFUSALS:
            data, ap, focus, diag = lens_params(name)
            codes.append((NAMES.index(name), ap if a2 is None else a2, focus if f2 is None else f2, diag, setup(L, data, ap if a2 is None else a2, focus if f2 is None else f2, diag, [])[0]))
            assert codes[-1][4] == want, codes[-1]
        d["refusals"] = np.array(codes, F32)      # rows: lens (index into NAMES), aperture diameter, focus distance, film diagonal, the status the text gives
    per = -(-n_other // len(ORTHO_CAMERAS))
    for i, spec in enumerate(ORTHO_CAMERAS):
        cam = other_camera("orthographic", spec)
        s = other_samples(rng, per, False)
        d["ortho%d_camera" % i], d["ortho%d_samples" % i], d["ortho%d_rays" % i] = pack_camera(cam), s, cam_rays(L, camera_desc(cam), s)
        assert cam["kind"] == abi.CAMERA_ORTHOGRAPHIC and (d["ortho%d_rays" % i][:, 8] == 1).all()
    for i, spec in enumerate((dict(), dict(moving=True))):
        cam = other_camera("environment", spec)
        s = other_samples(rng, n_other // 2, True)
        d["env%d_camera" % i], d["env%d_samples" % i], d["env%d_rays" % i] = pack_camera(cam), s, cam_rays(L, camera_desc(cam), s)
        assert cam["kind"] == abi.CAMERA_ENVIRONMENT and (d["env%d_rays" % i][:, 8:] == 0).all()      # the environment camera leaves `differential: None`
        assert (s[:, 1] == 0).sum() >= 8 and (s[:, 1] == YRES).sum() >= 8 and (s[:, 0] == 0).sum() >= 8 and (s[:, 0] == XRES).sum() >= 8
    return d, stats


def restated():
    from tests.test_realistic_host import build_realistic_restated
    return build_realistic_restated()


def main():
    L, where = convert()
    for w in where[-len(SOURCES) - 3:]:
        print("compiled from", w)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-only":
        return 0
    d, stats = reference(L, restated())
    for k, v in stats.items():
        print(k + ":", v)
    if len(sys.argv) > 1 and sys.argv[1] == "--check":
        g = np.load(FIXTURE)
        bad = [k for k in d if k not in g.files or g[k].shape != d[k].shape or not np.array_equal(g[k].view(np.uint8), d[k].view(np.uint8))]
        print("committed fixture %s the reference's text%s" % ("equals" if not bad and set(g.files) == set(d) else "DIFFERS from", "" if not bad else ": " + ", ".join(bad)))
        return 1 if bad or set(g.files) != set(d) else 0
    np.savez_compressed(FIXTURE, **d)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
