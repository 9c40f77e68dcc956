#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — fourth batch pinned by the reference's OWN TEXT: the three analytic shapes.  Sphere::intersect / intersect_p (shapes/sphere.rs),
Disk::intersect / intersect_p (shapes/disk.rs), Cylinder::intersect / intersect_p (shapes/cylinder.rs) with everything they reach: quadratic_efloat and EFloat's
methods and operators (core/efloat.rs), Transform::transform_vector_with_error / transform_ray_with_error (core/transform.rs), SurfaceInteraction::new
(core/interaction.rs), and — compiled by the earlier batches, reused here, not repeated — gamma, next_float_up / _down, clamp_t, the Vector3f / Normal3f helpers,
Ray::position, pnt3_distancef, transform_point_with_error, transform_point_with_abs_error, transform_vector, transform_normal, transform_surface_interaction.

Same route as oracle/make_{leaf,geom,flow}_fixtures.py, whose prelude, carriers, rules and compiled functions this script builds on (it imports them): the Rust
text is read from /root/reference where it lies, its SYNTAX is rewritten by the committed rules below, the result is compiled as C++ into oracle/_ref/libshaperef.so
(git-ignored, never committed) with g++ -O2 -ffp-contract=off and the platform libm, and tests/golden/shape_functions.npz holds seeded inputs with that code's
outputs.  No function body is edited or typed in by hand.

Hand-written here: the CARRIERS (EFloat's three fields; Sphere / Disk / Cylinder with Rust's field names; operators that name the compiled functions), and the C
wrapper, which moves an element of rspt_quadric_intersect's layout (include/rspt.h: 64 floats in — the record's words, o, d, t_max — and 64 out) in and out.
Rules that are specific to one function (S5, S6 below): SurfaceInteraction::new is compiled at `sh = None`, the only value the three shapes pass (sphere.rs:256-258,
disk.rs:150-152, cylinder.rs:233-235) — its `if let Some(shape) = sh` blocks are replaced by their else branch (or dropped where they have none) — and its
struct literal loses the `bssrdf` field the carrier of the geom batch does not hold.

tests/test_reference_shape_functions.py holds tests/quadric_restated.cpp (and through it tests/sphere_restated.cpp) to the fixture, tests/test_gpu_reference_shapes.py
the device.  usage: python oracle/make_shape_fixtures.py [--build-only | --check]
"""
import ctypes as C
import math
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

REF = geom.REF
OUT_DIR = base.OUT_DIR
FIXTURE = os.path.join(ROOT, "tests", "golden", "shape_functions.npz")

CARRIERS = r"""
// ---- carriers of the shape batch (oracle/make_shape_fixtures.py): fields and operator names; every body is the reference's text, compiled below ----
struct EFloat {                                        // efloat.rs:41-46; #[derive(Default)]: zeros
    Float v, low, high;
    static EFloat new_(Float v, Float err); Float lower_bound() const; Float upper_bound() const; bool eq(const EFloat& rhs) const;
    static EFloat default_() { return EFloat{Float(0.0f), Float(0.0f), Float(0.0f)}; }
};
EFloat efloat_add(EFloat self_, EFloat rhs); EFloat efloat_sub(EFloat self_, EFloat rhs); EFloat efloat_mul(EFloat self_, EFloat rhs); EFloat efloat_mul_f32(EFloat self_, Float rhs); EFloat efloat_div(EFloat self_, EFloat rhs);
static inline EFloat operator+(EFloat a, EFloat b) { return efloat_add(a, b); }          // impl Add / Sub / Mul / Mul<f32> / Div / PartialEq for EFloat (efloat.rs:68-149): the text's
static inline EFloat operator-(EFloat a, EFloat b) { return efloat_sub(a, b); }
static inline EFloat operator*(EFloat a, EFloat b) { return efloat_mul(a, b); }
static inline EFloat operator*(EFloat a, Float b) { return efloat_mul_f32(a, b); }
static inline EFloat operator/(EFloat a, EFloat b) { return efloat_div(a, b); }
static inline bool operator==(const EFloat& a, const EFloat& b) { return a.eq(b); }
bool quadratic_efloat(EFloat a, EFloat b, EFloat c, EFloat* t0, EFloat* t1);
Vector3f transform_vector_with_error(const Transform& self_, const Vector3f& v, Vector3f* abs_error);
Ray transform_ray_with_error(const Transform& self_, const Ray& r, Vector3f* o_error, Vector3f* d_error);
FullInteraction surface_interaction_new(const Point3f& p, const Vector3f& p_error, Point2f uv, const Vector3f& wo, const Vector3f& dpdu, const Vector3f& dpdv, const Normal3f& dndu, const Normal3f& dndv, Float time, NoneT sh);
struct Sphere {                                        // sphere.rs:21-35
    Float radius, z_min, z_max, theta_min, theta_max, phi_max; Transform object_to_world, world_to_object; bool reverse_orientation, transform_swaps_handedness;
    bool intersect(const Ray& r, Float* t_hit, FullInteraction& isect) const; bool intersect_p(const Ray& r) const;
};
struct Disk {                                          // disk.rs:17-28
    Float height, radius, inner_radius, phi_max; Transform object_to_world, world_to_object; bool reverse_orientation, transform_swaps_handedness;
    bool intersect(const Ray& r, Float* t_hit, FullInteraction& isect) const; bool intersect_p(const Ray& r) const;
};
struct Cylinder {                                      // cylinder.rs:19-31
    Float radius, z_min, z_max, phi_max; Transform object_to_world, world_to_object; bool reverse_orientation, transform_swaps_handedness;
    bool intersect(const Ray& r, Float* t_hit, FullInteraction& isect) const; bool intersect_p(const Ray& r) const;
};
"""

# (file, search-from regex or None, first-line regex, name, class — `@T`: a method compiled as a free function over the carrier T of another batch, as in the flow batch)
SOURCES = [
    ("core/efloat.rs", r"^impl EFloat \{", r"^    pub fn new\(v: f32, err: f32\) -> Self \{", "new_", "EFloat"),
    ("core/efloat.rs", r"^impl EFloat \{", r"^    pub fn lower_bound\(&self\) -> f32 \{", "lower_bound", "EFloat"),
    ("core/efloat.rs", r"^impl EFloat \{", r"^    pub fn upper_bound\(&self\) -> f32 \{", "upper_bound", "EFloat"),
    ("core/efloat.rs", r"^impl PartialEq for EFloat \{", r"^    fn eq\(&self, rhs: &EFloat\) -> bool \{", "eq", "EFloat"),
    ("core/efloat.rs", r"^impl Add for EFloat \{", r"^    fn add\(self, rhs: EFloat\) -> EFloat \{", "efloat_add", None),
    ("core/efloat.rs", r"^impl Sub for EFloat \{", r"^    fn sub\(self, rhs: EFloat\) -> EFloat \{", "efloat_sub", None),
    ("core/efloat.rs", r"^impl Mul for EFloat \{", r"^    fn mul\(self, rhs: EFloat\) -> EFloat \{", "efloat_mul", None),
    ("core/efloat.rs", r"^impl Mul<f32> for EFloat \{", r"^    fn mul\(self, rhs: f32\) -> EFloat \{", "efloat_mul_f32", None),
    ("core/efloat.rs", r"^impl Div for EFloat \{", r"^    fn div\(self, rhs: EFloat\) -> EFloat \{", "efloat_div", None),
    ("core/efloat.rs", None, r"^pub fn quadratic_efloat\(", "quadratic_efloat", None),
    ("core/transform.rs", r"^impl Transform \{", r"^    pub fn transform_vector_with_error\(", "transform_vector_with_error", "@Transform"),
    ("core/transform.rs", r"^impl Transform \{", r"^    pub fn transform_ray_with_error\($", "transform_ray_with_error", "@Transform"),
    ("core/interaction.rs", r"^impl<'a> SurfaceInteraction<'a> \{", r"^    pub fn new\($", "surface_interaction_new", None),
    ("shapes/sphere.rs", None, r"^    pub fn intersect\(&self, r: &Ray, t_hit: &mut Float, isect: &mut SurfaceInteraction\) -> bool \{", "intersect", "Sphere"),
    ("shapes/sphere.rs", None, r"^    pub fn intersect_p\(&self, r: &Ray\) -> bool \{", "intersect_p", "Sphere"),
    ("shapes/disk.rs", None, r"^    pub fn intersect\(&self, r: &Ray, t_hit: &mut Float, isect: &mut SurfaceInteraction\) -> bool \{", "intersect", "Disk"),
    ("shapes/disk.rs", None, r"^    pub fn intersect_p\(&self, r: &Ray\) -> bool \{", "intersect_p", "Disk"),
    ("shapes/cylinder.rs", None, r"^    pub fn intersect\(&self, r: &Ray, t_hit: &mut Float, isect: &mut SurfaceInteraction\) -> bool \{", "intersect", "Cylinder"),
    ("shapes/cylinder.rs", None, r"^    pub fn intersect_p\(&self, r: &Ray\) -> bool \{", "intersect_p", "Cylinder"),
]
TYPES_EXTRA = {"EFloat": "EFloat", "&EFloat": "const EFloat&", "&mut EFloat": "EFloat*", "f32": "Float", "&Transform": "const Transform&", "Ray": "Ray", "&Ray": "const Ray&",
               "&mut Vector3f": "Vector3f*", "&mut Float": "Float*", "&mut SurfaceInteraction": "FullInteraction&", "Option<&Shape>": "NoneT", "Point2f": "Point2f",
               "&Point3f": "const Point3f&", "&Vector3f": "const Vector3f&", "&Normal3f": "const Normal3f&"}

RULES_SHAPE = [
    # S1  f32 / f64 literals and casts:  `2.0f32`, `-0.5f32`, `1e-5_f32` -> Float(..f);  `4.0f64` -> 4.0;  `x as f32` -> Float(x) (Float's constructor from double rounds once, as the cast does);
    #     `let r: f64 = d.sqrt();` -> the f64 square root
    (r"(?<![\w.])(\d+(?:\.\d+)?(?:e-?\d+)?)_?f32\b", r"Float(\1f)", 0),
    (r"(?<![\w.])(\d+\.\d+)f64\b", r"\1", 0),
    (r"\b(\w+) as f32\b", r"Float(\1)", 0),
    (r"let (\w+): f64 = (\w+)\.sqrt\(\);", r"double \1 = std::sqrt(\2);", 0),
    # S2  `std::mem::swap(&mut (*a), &mut (*b))` over two `&mut EFloat`
    (r"std::mem::swap\(&mut \(\*(\w+)\), &mut \(\*(\w+)\)\)", r"std::swap(*\1, *\2)", 0),
    # S3  the two Transform methods compiled as functions over the flow batch's carrier (`@Transform`): the receiver becomes the first argument
    (r"([\w.>\-]+?)\s*\.transform_(ray|vector)_with_error\(", r"transform_\2_with_error(\1, ", 0),
    # S4  SurfaceInteraction::new is the function surface_interaction_new over the geom batch's FullInteraction
    (r"SurfaceInteraction::new\(", "surface_interaction_new(", 0),
    (r"let (?:mut )?(\w+): (EFloat|Ray|Vector3f|Point3f|Normal3f|Point2f|Float) = ", r"\2 \1 = ", 0),
]


def struct_literal(body, rust_name, cxx_name, skip=()):
    """S6: `NAME {\n f: E,\n g,\n}` -> CXX{.f = E, .g = g} on one line: the fields in their written order (which is the carrier's declared order), the field-init
    shorthand spelled out, the fields in `skip` left out (the carrier does not hold them)."""
    pos = 0
    while True:
        m = re.compile(r"\b%s \{" % rust_name).search(body, pos)
        if not m:
            return body
        j = geom.matching(body, m.end() - 1, "{", "}")
        inner, fields, depth, cur = body[m.end():j], [], 0, ""
        for ch in inner:
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            if ch == "," and depth == 0:
                fields.append(cur); cur = ""
            else:
                cur += ch
        fields.append(cur)
        out = []
        for f in [re.sub(r"\s*\n\s*", " ", re.sub(r"^\s*//.*$", "", f, flags=re.M)).strip() for f in fields]:
            if not f:
                continue
            mm = re.match(r"(\w+): (.*)$", f, re.S)
            name, expr = (mm.group(1), mm.group(2)) if mm else (f, f)
            if name not in skip:
                out.append(".%s = %s" % (name, expr))
        rep = "%s{%s}" % (cxx_name, ", ".join(out))
        body = body[:m.start()] + rep + body[j + 1:]
        pos = m.start() + len(cxx_name)


def none_branch(body, head):
    """S5: `head { A } else { B }` with the Option of `head` None -> B's statements in place; without an else the statement is dropped"""
    while head in body:
        i = body.index(head)
        j = geom.matching(body, body.index("{", i), "{", "}")
        m = re.match(r"\s*else \{", body[j + 1:])
        if not m:
            body = body[:body.rfind("\n", 0, i)] + body[j + 1:]
            continue
        k0 = j + 1 + m.end() - 1
        k1 = geom.matching(body, k0, "{", "}")
        body = body[:i] + body[k0 + 1:k1].strip() + body[k1 + 1:]
    return body


def convert_parts():
    saved = (dict(geom.TYPES), dict(base.TYPES), dict(flow.TYPES))
    try:
        return _convert_parts()
    finally:
        geom.TYPES.clear(); geom.TYPES.update(saved[0]); base.TYPES.clear(); base.TYPES.update(saved[1]); flow.TYPES.clear(); flow.TYPES.update(saved[2])


def _convert_parts():
    parts, where = flow.convert_parts()        # the three earlier batches: prelude, carriers and every function they compile (their spans come first in `where`)
    where = list(where)
    parts.append(CARRIERS)
    types = dict(geom.TYPES)
    types.update(TYPES_EXTRA)
    fn_names = set(geom.FN_NAMES) | {s[3] for s in SOURCES}
    for fname, after_re, first_re, name, cls in SOURCES:
        for tab in (geom.TYPES, base.TYPES):
            tab.clear(); tab.update(types)
            tab["Self"] = "FullInteraction" if name == "surface_interaction_new" else (cls or "EFloat")
        text, l0, l1 = geom.extract(fname, after_re, first_re, None)
        text = re.sub(r"^\s*//.*\n", "", text, flags=re.M)                      # comment lines
        text = re.sub(r"\bself\s*\n\s*\.", "self.", text)                       # rustfmt's break behind `self`
        self_type = None
        if cls and cls.startswith("@"):
            self_type, cls = cls[1:], None
            text = text.replace("&self,", "self_: &%s," % self_type)
        if name.startswith("efloat_"):                                          # `impl Op for EFloat { fn op(self, rhs) }` -> a function of two values (the carrier's operator names it)
            text = re.sub(r"fn \w+\(self, ", "fn %s(self_: EFloat, " % name, text)
        if self_type or name.startswith("efloat_"):
            text = re.sub(r"\bself\b(?!_)", "self_", text)
        sig, body, params = geom.signature(text, name, cls)
        body = flow.join_multiline_if(body)
        for nm in re.findall(r"(?:Vector3f|EFloat)\* (\w+)", sig):             # (F9 of the flow batch) field access through a `&mut T` auto-dereferences
            body = re.sub(r"(?<![\w>.*])%s\.(?=(?:[xyz]|v|low|high)\b)" % nm, nm + "->", body)
        if name == "surface_interaction_new":
            body = none_branch(body, "if let Some(shape) = sh {")
            body = struct_literal(body, "SurfaceInteraction", "FullInteraction", skip=("bssrdf",))
            body = struct_literal(body, "Shading", "Shading")
            body = struct_literal(body, "InteractionCommon", "InteractionCommon")
        body = struct_literal(body, "EFloat", "EFloat")
        for pat, rep, flags in RULES_SHAPE + flow.RULES_CAM + geom.RULES_FULL + geom.RULES_LIGHT + geom.RULES_PRE:
            body = re.sub(pat, rep, body, flags=flags)
        body = geom.cast_after_parens(body, "Float", "Float(%s)")
        for pat, rep, flags in base.RULES:
            body = re.sub(pat, rep, body, flags=flags)
        body = base.shadowing(body, set(params) | fn_names)
        if not sig.startswith("void"):
            body = geom.tail_value(body)
        parts.append("// %s%s:%d-%d\n%s%s" % (REF, fname, l0, l1, sig, body))
        where.append("%s%s %s:%d-%d" % ((cls + "::") if cls else "", name, fname, l0, l1))
    return parts, where


WRAPPERS = r"""
// the element layout of rspt_quadric_intersect (include/rspt.h): 64 floats in (the record's words, o, d, t_max), 64 out (out[0] intersect's result, out[1] t,
// out[2..24] the interaction, out[25..39] the shading frame, out[43] intersect_p's result, zeros elsewhere).  Values are moved, nothing is computed.
static inline Transform shape_xf(const float* m, const float* mi) {
    Transform t;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { t.m.m[r][c] = Float(m[4 * r + c]); t.m_inv.m[r][c] = Float(mi[4 * r + c]); }
    return t;
}
static inline void shape_emit(const FullInteraction& si, Float t, float* r) {
    const Float v[38] = {si.common.p.x, si.common.p.y, si.common.p.z, si.common.p_error.x, si.common.p_error.y, si.common.p_error.z, si.common.n.x, si.common.n.y, si.common.n.z, si.uv.x, si.uv.y,
                         si.dpdu.x, si.dpdu.y, si.dpdu.z, si.dpdv.x, si.dpdv.y, si.dpdv.z, si.dndu.x, si.dndu.y, si.dndu.z, si.dndv.x, si.dndv.y, si.dndv.z,
                         si.shading.n.x, si.shading.n.y, si.shading.n.z, si.shading.dpdu.x, si.shading.dpdu.y, si.shading.dpdu.z, si.shading.dpdv.x, si.shading.dpdv.y, si.shading.dpdv.z,
                         si.shading.dndu.x, si.shading.dndu.y, si.shading.dndu.z, si.shading.dndv.x, si.shading.dndv.y, si.shading.dndv.z};
    r[0] = 1.0f; r[1] = t.v;
    for (int k = 0; k < 38; k++) r[2 + k] = v[k].v;
}
template <class S> static void shape_run(const S& s, const float* q, float* r) {
    for (int k = 0; k < 64; k++) r[k] = 0.0f;
    Ray ray{}; ray.o = Point3f{Float(q[0]), Float(q[1]), Float(q[2])}; ray.d = Vector3f{Float(q[3]), Float(q[4]), Float(q[5])}; ray.t_max.v = Float(q[6]);
    ray.time = Float(0.0f); ray.differential = RayDifferential{}; ray.medium = MediumRef{0};
    Float t(0.0f); FullInteraction si{};
    if (s.intersect(ray, &t, si)) shape_emit(si, t, r);
    r[43] = s.intersect_p(ray) ? 1.0f : 0.0f;
}
extern "C" int shape_hook(uint32_t shape, const float* x, uint64_t n, float* out) {
    if (shape != RSPT_MESH_SPHERE && shape != RSPT_MESH_DISK && shape != RSPT_MESH_CYLINDER) return -1;
    for (uint64_t i = 0; i < n; i++) {
        const float* e = x + 64 * i; float* r = out + 64 * i;
        if (shape == RSPT_MESH_SPHERE) {
            rspt_sphere s; std::memcpy(&s, e, sizeof s);
            shape_run(Sphere{Float(s.radius), Float(s.z_min), Float(s.z_max), Float(s.theta_min), Float(s.theta_max), Float(s.phi_max), shape_xf(s.object_to_world, s.world_to_object),
                             shape_xf(s.world_to_object, s.object_to_world), s.reverse_orientation != 0, s.transform_swaps_handedness != 0}, e + 42, r);
        } else if (shape == RSPT_MESH_DISK) {
            rspt_disk s; std::memcpy(&s, e, sizeof s);
            shape_run(Disk{Float(s.height), Float(s.radius), Float(s.inner_radius), Float(s.phi_max), shape_xf(s.object_to_world, s.world_to_object),
                           shape_xf(s.world_to_object, s.object_to_world), s.reverse_orientation != 0, s.transform_swaps_handedness != 0}, e + 40, r);
        } else {
            rspt_cylinder s; std::memcpy(&s, e, sizeof s);
            shape_run(Cylinder{Float(s.radius), Float(s.z_min), Float(s.z_max), Float(s.phi_max), shape_xf(s.object_to_world, s.world_to_object),
                               shape_xf(s.world_to_object, s.object_to_world), s.reverse_orientation != 0, s.transform_swaps_handedness != 0}, e + 40, r);
        }
    }
    return 0;
}
"""


def convert():
    parts, where = convert_parts()
    parts.append(WRAPPERS)
    os.makedirs(OUT_DIR, exist_ok=True)
    cpp = os.path.join(OUT_DIR, "shape_functions.cpp")
    open(cpp, "w").write("\n".join(parts))
    so = os.path.join(OUT_DIR, "libshaperef.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), "-o", so, cpp])
    L = C.CDLL(so)
    L.shape_hook.restype = C.c_int
    L.shape_hook.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    return L, where


# ---------------------------------------------------------------- seeded inputs ----------------------------------------------------------------
F32 = np.float32
SEEDS = {"sphere": 0x5BE4E, "disk": 0xD15C, "cylinder": 0xC711D}
CATS = ["outside_on", "outside_off", "inside", "clipped_first", "spawned", "tmax_at_hit", "grazing", "parallel", "azimuth_edge", "centre_and_rims", "orientation"]
SHAPE_CATS = {"sphere": [0, 1, 2, 3, 4, 5, 6, 8, 10], "cylinder": [0, 1, 2, 3, 4, 5, 6, 8, 10], "disk": [0, 1, 4, 5, 7, 8, 9, 10]}
OUT_COLS = np.r_[0:40, 43]                     # the columns of the hook's 64 output words that are in use
N_EXACT = 5                                    # records 0 .. 4 of a pool: identity, axis-permuting and axis-mirroring transforms (object space is exact under them)


def shape_code(shape):
    from rs_pbrt_amd import abi
    return {"sphere": abi.MESH_SPHERE, "disk": abi.MESH_DISK, "cylinder": abi.MESH_CYLINDER}[shape]


def record_pool(shape, n_rec=40):
    """the records of one shape's cases, stored once: five exact transforms (identity, identity + partial, an axis permutation, identity + reverse_orientation, an
    axis mirror that swaps handedness), then tests/test_quadric_host.py's random_xf — rotations, non-uniform and mirroring scales, every sixth far away — over full,
    phi-clipped and z-clipped / annular records, every fourth with reverse_orientation set"""
    from rs_pbrt_amd import scenes
    from tests.test_quadric_host import random_xf
    rng = np.random.default_rng(SEEDS[shape] ^ 0xEC)
    perm = np.array([[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F32)
    mirror = np.diag([1.0, -1.0, 1.0, 1.0]).astype(F32)
    exact = [(None, 0, 360.0, 0), (None, 2, 270.0, 0), (scenes.Transform(perm), 2, 200.0, 0), (None, 1, 90.0, 1), (scenes.Transform(mirror), 2, 300.0, 0)]
    recs = []
    for i in range(n_rec):
        if i < N_EXACT:
            xf, partial, phimax, rev = exact[i]
            r = [1.0, 1.5, 0.75, 2.0, 1.25][i]
        else:
            xf, partial, rev = random_xf(rng, far=(i % 6 == 0)), i % 3, int(i % 4 == 1)
            phimax = 360.0 if partial == 0 else float(rng.uniform(30, 330))
            r = float(rng.uniform(0.3, 3.0))
        sb = scenes.SceneBuilder()
        if shape == "sphere":
            sb.add_sphere(r, zmin=None if partial != 2 else -0.5 * r, zmax=None if partial != 2 else 0.625 * r, phimax=phimax, object_to_world=xf)
            rec = sb.spheres[0][0]
        elif shape == "disk":
            sb.add_disk(height=[0.0, 0.5, -0.25, 1.0, 0.0][i] if i < N_EXACT else float(rng.uniform(-1, 1)), radius=r, innerradius=0.0 if partial != 2 else 0.25 * r, phimax=phimax, object_to_world=xf)
            rec = sb.disks[0][0]
        else:
            z0 = -1.0 if i < N_EXACT else float(rng.uniform(-2, 0))
            sb.add_cylinder(radius=r, zmin=z0, zmax=z0 + (2.0 if i < N_EXACT else float(rng.uniform(0.2, 3))), phimax=phimax, object_to_world=xf)
            rec = sb.cylinders[0][0]
        rec = rec.copy()
        rec["reverse_orientation"] = rev
        recs.append(np.frombuffer(rec.tobytes(), F32).copy())
    return np.stack(recs)


class Pool:
    """a record pool's parameters as f64 arrays (what the generator aims with; the text reads the f32 words themselves)"""
    def __init__(self, shape, words):
        from rs_pbrt_amd import abi
        dt = {"sphere": abi.SPHERE_DT, "disk": abi.DISK_DT, "cylinder": abi.CYLINDER_DT}[shape]
        rec = np.frombuffer(np.ascontiguousarray(words).tobytes(), dt)
        self.shape, self.words, self.n = shape, words, len(rec)
        self.m = rec["object_to_world"].astype(np.float64).reshape(-1, 4, 4)
        self.r, self.phimax = rec["radius"].astype(np.float64), rec["phi_max"].astype(np.float64)
        if shape == "disk":
            self.h, self.ri = rec["height"].astype(np.float64), rec["inner_radius"].astype(np.float64)
            self.z_clipped = self.ri > 0                      # ("z" of a disk: its radial extent)
        else:
            self.zlo, self.zhi = rec["z_min"].astype(np.float64), rec["z_max"].astype(np.float64)
            self.z_clipped = (self.zlo > -self.r) | (self.zhi < self.r) if shape == "sphere" else np.ones(self.n, bool)
        self.phi_clipped = self.phimax < 2 * math.pi - 0.05
        self.flagged = (rec["reverse_orientation"] != 0) | (rec["transform_swaps_handedness"] != 0)

    def point(self, k, phi, z):
        """the surface point of record k at azimuth phi and height z (a disk: radius z)"""
        if self.shape == "sphere":
            rho = np.sqrt(np.maximum(self.r[k] ** 2 - z ** 2, 0.0))
            return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
        if self.shape == "cylinder":
            return np.stack([self.r[k] * np.cos(phi), self.r[k] * np.sin(phi), z], 1)
        return np.stack([z * np.cos(phi), z * np.sin(phi), self.h[k]], 1)

    def normal(self, k, p):
        if self.shape == "sphere":
            return p / self.r[k, None]
        if self.shape == "cylinder":
            return np.stack([p[:, 0], p[:, 1], np.zeros(len(p))], 1) / self.r[k, None]
        return np.tile([0.0, 0.0, 1.0], (len(p), 1))

    def inside(self, rng, k):
        """(phi, z) inside the record's clipped region, 2 % off its edges"""
        phi = rng.uniform(0.02, 0.98, len(k)) * self.phimax[k]
        if self.shape == "disk":
            return phi, self.ri[k] + rng.uniform(0.02, 0.98, len(k)) * (self.r[k] - self.ri[k])
        return phi, self.zlo[k] + rng.uniform(0.02, 0.98, len(k)) * (self.zhi[k] - self.zlo[k])

    def outside(self, rng, k):
        """(phi, z) on the unclipped surface (a disk: its plane) but outside the record's region: past phi_max, or past the z clip (a disk: the rim or the hole).
        A full sphere has no such point: it gets an ordinary one."""
        phi, z = self.inside(rng, k)
        use_phi = self.phi_clipped[k] & (~self.z_clipped[k] | (rng.uniform(size=len(k)) < 0.5))
        phi = np.where(use_phi, self.phimax[k] + rng.uniform(0.05, 0.95, len(k)) * (2 * math.pi - self.phimax[k]), phi)
        f, top = rng.uniform(0.05, 0.9, len(k)), rng.uniform(size=len(k)) < 0.5
        if self.shape == "disk":
            zo = np.where(top | (self.ri[k] == 0), self.r[k] * (1.02 + f), self.ri[k] * (0.95 - f))
        elif self.shape == "cylinder":
            zo = np.where(top, self.zhi[k] + 0.05 + 2 * f, self.zlo[k] - 0.05 - 2 * f)
        else:
            can_top, can_bot = self.zhi[k] < self.r[k], self.zlo[k] > -self.r[k]
            top = np.where(can_top & can_bot, top, can_top)
            zo = np.where(top, self.zhi[k] + (0.03 + 0.9 * f) * (self.r[k] - self.zhi[k]), self.zlo[k] - (0.03 + 0.9 * f) * (self.zlo[k] + self.r[k]))
        return phi, np.where(~use_phi & self.z_clipped[k], zo, z)

    def world(self, k, po, pd, t_max):
        """(n, 7) f32 rays o, d, t_max in world space"""
        m = self.m[k]
        wo = np.einsum("nij,nj->ni", m[:, :3, :3], po) + m[:, :3, 3]
        wd = np.einsum("nij,nj->ni", m[:, :3, :3], pd)
        return np.concatenate([wo, wd, np.asarray(t_max, np.float64).reshape(-1, 1)], 1).astype(F32)


def unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1)[:, None]


def elements(words, idx, ray):
    """(n, 64) elements of rspt_quadric_intersect: the record's words, then o, d, t_max"""
    x = np.zeros((len(idx), 64), F32)
    w = words.shape[1]
    x[:, :w] = words[idx]
    x[:, w:w + 7] = ray
    return x


def run_text(L, shape, words, idx, ray):
    x = elements(words, np.asarray(idx), np.asarray(ray, F32))
    out = np.zeros_like(x)
    assert L.shape_hook(shape_code(shape), x.ctypes.data, len(x), out.ctypes.data) == 0
    return out


def aimed(P, rng, k, target_kind, inside_origin=False):
    """rays aimed at a surface point: from outside (the origin on the outer side of the tangent plane, both sides of a disk) or from inside the body"""
    n = len(k)
    phi, z = P.inside(rng, k) if target_kind == "in" else P.outside(rng, k)
    tgt = P.point(k, phi, z)
    nrm = P.normal(k, tgt)
    if inside_origin:
        u = unit(rng, n) * rng.uniform(0, 1, (n, 1)) ** (1 / 3)
        if P.shape == "sphere":
            o = u * 0.9 * P.r[k, None]
        else:
            o = np.stack([u[:, 0] * 0.9 * P.r[k], u[:, 1] * 0.9 * P.r[k], P.zlo[k] - 0.3 + rng.uniform(size=n) * (P.zhi[k] - P.zlo[k] + 0.6)], 1)
    else:
        u = unit(rng, n)
        c = (u * nrm).sum(1)
        u = u - 2 * np.minimum(c, 0)[:, None] * nrm                       # onto the outer side
        u = u + 0.3 * nrm
        u /= np.linalg.norm(u, axis=1)[:, None]
        if P.shape == "disk":
            u[:, 2] *= rng.choice([-1.0, 1.0], n)
        o = tgt + u * (rng.uniform(0.5, 6.0, n) * P.r[k])[:, None]
    s = rng.uniform(0.3, 3.0, n)
    return o, (tgt - o) * s[:, None], s


def cases(L, shape, per_cat=256, seed=None):
    """one shape's cases: (words, idx, ray, cat).  Aiming is done in f64 in object space and taken to world space through the record's matrix; what the text
    answers decides the categories that depend on it (spawned origins, t_max at the text's own t)."""
    rng = np.random.default_rng(SEEDS[shape] if seed is None else seed)
    words = record_pool(shape)
    P = Pool(shape, words)
    every, exact = np.arange(P.n), np.arange(N_EXACT)
    partial = every[P.phi_clipped | P.z_clipped]                  # records with something to clip (every cylinder: its z range is finite)
    flagged = every[P.flagged]
    inf = np.inf
    idx_all, ray_all, cat_all = [], [], []

    def emit(cat, k, ray):
        idx_all.append(np.asarray(k, np.uint16)); ray_all.append(np.asarray(ray, F32)); cat_all.append(np.full(len(k), cat, np.uint8))

    def hits_of(k, ray, need):
        """`need` of the given rays that the text hits (cycled if there are fewer), with the text's outputs"""
        out = run_text(L, shape, words, k, ray)
        h = np.nonzero(out[:, 0] == 1)[0]
        assert len(h) >= need // 4, (shape, len(h), need)
        h = np.resize(h, need)
        return k[h], ray[h], out[h]

    def upper_bound_ulps(k, ray, tb):
        """how many ulps above the text's t (bits tb) its t.upper_bound() lies: the smallest t_max that still hits, found by bisection over the text itself"""
        lo, hi = np.full(len(k), -1, np.int64), np.full(len(k), 1 << 24, np.int64)
        while (hi - lo > 1).any():
            mid = (lo + hi) // 2
            r2 = ray.copy(); r2[:, 6] = (tb + mid).astype(np.uint32).view(F32)
            h = run_text(L, shape, words, k, r2)[:, 0] == 1
            hi = np.where(h, mid, hi); lo = np.where(h, lo, mid)
        return hi

    for cat in SHAPE_CATS[shape]:
        m = per_cat * 3 // 2 if cat == 3 else per_cat
        if cat == 0:      # outside, aimed on
            k = rng.choice(every, m)
            o, d, _ = aimed(P, rng, k, "in")
            emit(cat, k, P.world(k, o, d, np.full(m, inf)))
        elif cat == 1:    # outside, aimed off: at a clipped point of the unclipped surface, or past the silhouette altogether
            k = np.concatenate([rng.choice(partial, m // 2), rng.choice(every, m - m // 2)])
            o, d, _ = aimed(P, rng, k, "out")
            if shape != "disk":
                j = np.arange(m // 2, m)
                phi, z = P.inside(rng, k[j])
                p = P.point(k[j], phi, z)
                nrm = P.normal(k[j], p)
                q = p + nrm * (rng.uniform(0.05, 1.0, len(j)) * P.r[k[j]])[:, None]
                t = unit(rng, len(j))
                t -= (t * nrm).sum(1)[:, None] * nrm
                t /= np.linalg.norm(t, axis=1)[:, None]
                o[j] = q - t * (rng.uniform(1, 4, len(j)) * P.r[k[j]])[:, None]
                d[j] = t * rng.uniform(0.3, 3.0, (len(j), 1))
            emit(cat, k, P.world(k, o, d, np.full(m, inf)))
        elif cat == 2:    # origin inside: t0.lower_bound() <= 0, t1 is taken
            k = rng.choice(every, m)
            o, d, s = aimed(P, rng, k, "in", inside_origin=True)
            o2, d2, s2 = aimed(P, rng, k, "out", inside_origin=True)
            off = rng.uniform(size=m) < 0.3
            o[off], d[off], s[off] = o2[off], d2[off], s2[off]
            t_max = np.where(rng.uniform(size=m) < 0.8, inf, rng.uniform(0.3, 2.0, m) / s)
            emit(cat, k, P.world(k, o, d, t_max))
        elif cat == 3:    # the first root is clipped away by z, theta or phi_max; the retry on t1 decides (half end on the surface, a quarter on a clipped point again, a quarter short of t1)
            k = rng.choice(partial, m)
            p0 = P.point(k, *P.outside(rng, k))
            p1_in, p1_out = P.point(k, *P.inside(rng, k)), P.point(k, *P.outside(rng, k))
            kind = np.arange(m) % 4
            p1 = np.where((kind == 3)[:, None], p1_out, p1_in)
            lead, s = rng.uniform(0.3, 2.0, m), rng.uniform(0.3, 3.0, m)
            o, d = p0 - lead[:, None] * (p1 - p0), (p1 - p0) * s[:, None]
            t_max = np.where(kind == 2, (lead + rng.uniform(0.2, 0.8, m)) / s, inf)
            ray = P.world(k, o, d, t_max)
            j = np.nonzero(kind == 1)[0]      # a quarter: t_max at the retried root's own t, at its upper bound, one ulp either side of that, and half way (t1.upper_bound() > t_max decides, :161 / :151)
            out = run_text(L, shape, words, k[j], ray[j])
            j, out = j[out[:, 0] == 1], out[out[:, 0] == 1]
            tb = out[:, 1].copy().view(np.uint32).astype(np.int64)
            ub = upper_bound_ulps(k[j], ray[j], tb)
            var = np.arange(len(j)) % 5
            ray[j, 6] = (tb + np.select([var == 0, var == 1, var == 2, var == 3], [ub, ub - 1, ub + 1, 0], ub // 2)).astype(np.uint32).view(F32)
            emit(cat, k, ray)
        elif cat == 4:    # spawned on the surface: the origin is a hit point of the text's, times 0.9999 or within a few ulps of it; the error bounds decide
            k = rng.choice(every, 3 * m)
            o, d, _ = aimed(P, rng, k, "in")
            kk, _, out = hits_of(k, P.world(k, o, d, np.full(3 * m, inf)), m)
            nudge = rng.integers(-4, 5, (m, 1)) * 2.0 ** -23       # (every other origin: the hit point itself, or a few ulps off it — t0 straddles 0 and t0.lower_bound() <= 0 decides)
            wo = np.where((np.arange(m) % 2 == 0)[:, None], out[:, 2:5] * F32(0.9999), (out[:, 2:5].astype(np.float64) * (1 + nudge)).astype(F32))
            wd = np.einsum("nij,nj->ni", P.m[kk][:, :3, :3], unit(rng, m) * rng.uniform(0.3, 3.0, (m, 1)))
            emit(cat, kk, np.concatenate([wo, wd.astype(F32), np.full((m, 1), inf, F32)], 1))
        elif cat == 5:    # t_max at the text's own t, one ulp above and below; sphere and cylinder: also at t.upper_bound(), one ulp below and above it, and half way between t.v and it
            k = rng.choice(every, 3 * m)
            o, d, _ = aimed(P, rng, k, "in")
            if shape != "disk":
                o2, d2, _ = aimed(P, rng, k, "in", inside_origin=True)
                ins = rng.uniform(size=3 * m) < 0.4
                o[ins], d[ins] = o2[ins], d2[ins]
            kk, ray, out = hits_of(k, P.world(k, o, d, np.full(3 * m, inf)), m)
            tb = out[:, 1].copy().view(np.uint32).astype(np.int64)      # t > 0: consecutive floats are consecutive integers
            assert (out[:, 1] > 0).all()
            ub = upper_bound_ulps(kk, ray, tb) if shape != "disk" else np.zeros(m, np.int64)
            var = np.arange(m) % (7 if shape != "disk" else 3)
            step = np.select([var == 0, var == 1, var == 2, var == 3, var == 4, var == 5], [0, 1, -1, ub - 1, ub, ub + 1], ub // 2)
            ray = ray.copy(); ray[:, 6] = (tb + step).astype(np.uint32).view(F32)
            emit(cat, kk, ray)
        elif cat == 6:    # grazing the quadratic: tangent rays a little inside, on and a little outside the surface (a discriminant near zero, both signs)
            k = rng.choice(every, m)
            p = P.point(k, *P.inside(rng, k))
            nrm = P.normal(k, p)
            t = unit(rng, m)
            t -= (t * nrm).sum(1)[:, None] * nrm
            t /= np.linalg.norm(t, axis=1)[:, None]
            eps = rng.choice([-1e-5, -1e-6, -1e-7, 0.0, 1e-7, 1e-6, 1e-5], m)
            q = p + nrm * (eps * P.r[k])[:, None]
            emit(cat, k, P.world(k, q - t * (rng.uniform(1, 4, m) * P.r[k])[:, None], t * rng.uniform(0.3, 3.0, (m, 1)), np.full(m, inf)))
        elif cat == 7:    # disk: parallel to the plane — d.z == 0 exactly in object space (exact transforms only) — and all but parallel
            k = rng.choice(exact, m)
            tgt = P.point(k, *P.inside(rng, k))
            d = unit(rng, m)
            dz = np.where(np.arange(m) % 2 == 0, 0.0, rng.choice([1e-38, 1e-30, 1e-12, 1e-6, 1e-3], m) * rng.choice([-1.0, 1.0], m))
            d[:, 2] = dz
            o = tgt - d * rng.uniform(0.5, 2.0, (m, 1))
            o[:, 2] = np.where((np.arange(m) % 4 == 0), P.h[k], np.where(dz == 0, P.h[k] + rng.uniform(-1, 1, m), o[:, 2]))
            emit(cat, k, P.world(k, o, d, np.full(m, inf)))
        elif cat == 8:    # azimuth at the edges: phi within a few ulps of 0, of phi_max and of 2 pi (exact transforms), hit points on the negative-y side included
            k = rng.choice(exact, m)
            base = np.select([np.arange(m) % 4 == 0, np.arange(m) % 4 == 1, np.arange(m) % 4 == 2], [np.zeros(m), P.phimax[k], np.full(m, float(F32(2 * math.pi)))], rng.uniform(math.pi, 2 * math.pi, m))
            ulps = rng.integers(-6, 7, m)
            phi = np.where(base == 0, ulps * 2.0 ** -24, base.astype(F32).astype(np.float64) + ulps * np.spacing(base.astype(F32)).astype(np.float64))
            _, z = P.inside(rng, k)
            p = P.point(k, phi, z).astype(F32).astype(np.float64)
            nrm = P.normal(k, p) if shape != "disk" else np.tile([0.0, 0.0, 1.0], (m, 1)) * rng.choice([-1.0, 1.0], (m, 1))
            if shape == "sphere":      # ... and the pole itself, where x == 0 and y == 0 and the text moves x off the axis (sphere.rs:146-148)
                pole = np.arange(m) % 16 == 15
                p[pole] = np.stack([np.zeros(m), np.zeros(m), P.r[k] * rng.choice([-1.0, 1.0], m)], 1)[pole]
                nrm[pole] = p[pole] / P.r[k[pole], None]
            dist = np.round(rng.uniform(1, 3, m) * 4) / 4
            s = rng.choice([0.5, 1.0, 2.0], m)
            short = (shape == "cylinder") | ((shape == "sphere") & (np.arange(m) % 8 >= 4))       # (the segment ends in front of the far wall: the edge alone decides)
            emit(cat, k, P.world(k, p + nrm * dist[:, None], -nrm * s[:, None], np.where(short, 1.25 * dist / s, inf)))
        elif cat == 9:    # disk: a hit exactly at the centre (r_hit == 0: the text's dpdv is NaN), hits exactly on radius and on inner_radius, and within an ulp of them
            k = rng.choice(exact, m)
            var = np.arange(m) % 4
            rad = np.select([var == 0, var == 1, var == 2], [np.where(P.ri[k] == 0, 0.0, P.ri[k]), P.r[k], np.where(P.ri[k] == 0, P.r[k], P.ri[k])], P.r[k])
            rad = rad * (1 + np.where(np.arange(m) % 16 >= 8, rng.integers(-2, 3, m), 0) * 2.0 ** -23)
            phi = np.where(np.arange(m) % 8 < 4, 0.0, rng.uniform(0, 1, m) * P.phimax[k])
            p = P.point(k, phi, rad).astype(F32).astype(np.float64)
            nz = rng.choice([-1.0, 1.0], m)
            slant = np.where((np.arange(m) % 16 >= 12)[:, None], np.round(unit(rng, m) * 4) / 8, 0.0)
            up = np.stack([slant[:, 0], slant[:, 1], nz * np.round(rng.uniform(1, 3, m) * 4) / 4], 1)
            emit(cat, k, P.world(k, p + up, -up * rng.choice([0.5, 1.0, 2.0], (m, 1)), np.full(m, inf)))
        elif cat == 10:   # orientation flags set: reverse_orientation and / or transform_swaps_handedness (the text passes None for the shape: n is not flipped)
            k = rng.choice(flagged, m)
            o, d, _ = aimed(P, rng, k, "in")
            if shape != "disk":
                o2, d2, _ = aimed(P, rng, k, "out", inside_origin=True)
                sel = rng.uniform(size=m) < 0.4
                o[sel], d[sel] = o2[sel], d2[sel]
            emit(cat, k, P.world(k, o, d, np.full(m, inf)))
    return words, np.concatenate(idx_all), np.concatenate(ray_all), np.concatenate(cat_all)


def reference(L, per_cat=256, seed=None):
    """inputs and the text's outputs of all three shapes, as the fixture's arrays; the generator's own conditions on them are asserted here"""
    d, stats = {}, {}
    for shape in ("sphere", "disk", "cylinder"):
        words, idx, ray, cat = cases(L, shape, per_cat, None if seed is None else seed + len(shape))
        out = run_text(L, shape, words, idx, ray)
        assert (out[:, 40:43] == 0).all() and (out[:, 44:] == 0).all()
        n, hits = len(idx), int(out[:, 0].sum())
        assert n >= 1 << 11 or per_cat < 256
        for c in SHAPE_CATS[shape]:
            assert (cat == c).sum() * 20 >= n, (shape, CATS[c])                      # every category: at least 5 % of the shape's cases
        assert hits * 4 >= n and (n - hits) * 4 >= n, (shape, hits, n)               # a quarter hits, a quarter misses
        st = {"cases": n, "hits": hits, "misses": n - hits}
        if shape != "disk":
            retry = cat == 3
            st["retry_hits"], st["retry_misses"] = int(out[retry, 0].sum()), int(retry.sum() - out[retry, 0].sum())
            assert (st["retry_hits"] >= 100 and st["retry_misses"] >= 100) or per_cat < 256, (shape, st)
        check_categories(shape, words, idx, ray, cat, out)
        stats[shape] = st
        d.update({shape + "_rec": words, shape + "_idx": idx, shape + "_ray": ray, shape + "_cat": cat, shape + "_out": np.ascontiguousarray(out[:, OUT_COLS])})
    return d, stats


def check_categories(shape, words, idx, ray, cat, out):
    """what a category is there for did happen, by the text's own answers"""
    hit = out[:, 0] == 1
    for c in SHAPE_CATS[shape]:
        sel = cat == c
        if c in (0, 2, 5, 8, 10):
            assert hit[sel].sum() >= sel.sum() // 4, (shape, CATS[c], int(hit[sel].sum()))
        if c in (1, 5, 6, 8) or (c == 4 and shape != "disk"):
            assert (~hit[sel]).sum() >= sel.sum() // 8, (shape, CATS[c], int((~hit[sel]).sum()))
    if shape == "disk":
        assert not hit[(cat == 7) & (np.arange(len(cat)) % 2 == 0)].any() and hit[cat == 7].sum() >= 16      # d.z == 0 never hits; all-but-parallel rays do
        nine = out[cat == 9]
        assert np.isnan(nine[nine[:, 0] == 1][:, 16:19]).any(axis=1).sum() >= 16                             # the centre: r_hit == 0, dpdv is NaN
        assert (nine[:, 0] == 1).sum() >= 64 and (nine[:, 0] == 0).sum() >= 16                               # on a rim and an ulp past it
    sel = cat == 8
    if shape == "sphere":      # the pole under the identity: p = (1e-5 r, 0, +-r)
        assert (hit & sel & (idx == 0) & (out[:, 3] == 0) & (out[:, 2] == F32(1e-5))).sum() >= 2
    assert (hit & sel & (out[:, 11] > 0.99)).sum() >= 8 and (hit & sel & (out[:, 11] < 0.01)).sum() >= 8, shape       # u at both ends of [0, 1]


def main():
    L, where = convert()
    for w in where:
        print("compiled from", w)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-only":
        return 0
    d, stats = reference(L)
    for shape, st in stats.items():
        print(shape, " ".join("%s=%d" % kv for kv in st.items()))
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
