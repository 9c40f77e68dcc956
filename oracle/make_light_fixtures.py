#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — sixth batch pinned by the reference's OWN TEXT: the projection and goniometric lights.  From lights/projection.rs: projection, sample_li,
power, and of new_hdr the block from `p_light` to `cos_total_width` with its `world_to_light` initialiser (aspect, both screen_bounds arms, hither / yon,
Transform::perspective and its inverse, p_corner, w_corner), compiled as a function over a resolution and a light_to_world.  From lights/goniometric.rs: scale, sample_li,
power and the p_light / world_to_light lines of new_hdr.  And what these reach that no earlier batch compiled: Bounds2f::offset (core/geometry.rs).  Compiled by the
earlier batches and reused here, not repeated: pnt2_inside_bnd2f, pnt3_distance_squaredf, Transform::{perspective, inverse, transform_point, transform_vector, look_at},
Matrix4x4::inverse, spherical_theta / spherical_phi, MipMap::{lookup_pnt_flt, triangle, texel} in Repeat mode over the MIP carrier, Vector3f::normalize, clamp_t,
Distribution1D::new, PointLight / DiffuseAreaLight::power.  SpatialLightDistribution::compute_distribution (core/lightdistrib.rs) is the flow batch's text and goes
through the flow batch's rules once more, here over a second carrier: a light list whose projection / goniometric entries dispatch to the text compiled below, while point
and area lights keep the flow batch's route (the flow batch's own carrier hands every light to the oracle, which knows neither kind).  RGBSpectrum's operators
are element-wise carriers since the first batch (`Spectrum * Spectrum / Float` is among them).

Same route as oracle/make_{leaf,geom,flow,shape,camera}_fixtures.py, whose prelude, carriers, rules and compiled functions this script builds on (it imports them): the
Rust text is read from /root/reference where it lies, its SYNTAX is rewritten by the committed rules below (L1 .. L7), the result is compiled as C++ into
oracle/_ref/liblightref.so (git-ignored, never committed) with g++ -O2 -ffp-contract=off and the platform libm, and tests/golden/light_functions.npz holds seeded
inputs with that code's outputs.  No function body is edited or typed in by hand.

Hand-written here: the CARRIERS (ProjectionLight / GonioPhotometricLight with the reference's field names, a Bounds2f with `offset`, the optional map) and the C wrapper,
which moves values in and out, names the class of a direction from values the text computed, and takes the grid of SpatialLightDistribution::new and the voxel of
SpatialLightDistribution::lookup from the oracle (orc::light_distrib_init, orc::Bounds3::offset: held to the text by the flow batch).

OUT OF SCOPE, on purpose: the image decoding of new / new_hdr (the OpenEXR and Radiance readers); MipMap::new's resampling of sides that are no power of two (listed as
unpinned in DESIGN.md: every map here has power-of-two sides and the pyramid of scenes.build_light_map); sample_le / pdf_le (not on the device); api.rs' parameter
parsing (scenes.py's builders take `from to up fov` / a matrix and put light_to_world = LookAt's inverse); rust_shim/.

tests/test_reference_light_functions.py holds tests/maplight_restated.cpp and scenes.py's two builders to the fixture, tests/test_gpu_reference_lights.py the device.
usage: python oracle/make_light_fixtures.py [--build-only | --check]
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
import make_camera_fixtures as camera  # noqa: E402

REF = geom.REF
OUT_DIR = base.OUT_DIR
FIXTURE = os.path.join(ROOT, "tests", "golden", "light_functions.npz")

CARRIERS = r"""
// ---- carriers of the light batch (oracle/make_light_fixtures.py): fields and method names; every body is the reference's text, compiled below ----
namespace lightb {
struct Bounds2f {                                      // geometry.rs:1865-1869; pnt2_inside_bnd2f is the camera batch's, over its own carrier of the same two fields
    Point2f p_min, p_max; Vector2f offset(Point2f p) const;
    operator camb::Bounds2f() const { return camb::Bounds2f{p_min, p_max}; }
};
using camb::pnt2_inside_bnd2f;
static inline Point2f Point2f_from(const Vector2f& v) { return Point2f{v.x, v.y}; }                    // impl From<Vector2f> for Point2f (geometry.rs): the two fields
struct MapRef { const MipMapS* m; Spectrum lookup_pnt_flt(Point2f st, Float width) const { return m->lookup_pnt_flt(st, width); } };      // Arc<MipMap<Spectrum>>
typedef flow::Option<MapRef> OptMap;                   // Option<Arc<MipMap<Spectrum>>>
struct ProjectionLight {                               // projection.rs:47-63 (the fields the three methods read)
    OptMap projection_map; Point3f p_light; Spectrum i; Transform light_projection; Float hither, yon; Bounds2f screen_bounds; Float cos_total_width; Transform light_to_world, world_to_light;
    Spectrum projection(const Vector3f& w) const; Spectrum power() const;
    Spectrum sample_li(const InteractionCommon& iref, InteractionCommon& light_intr, Point2f _u, Vector3f* wi, Float* pdf, VisibilityTester& vis) const;
};
struct GonioPhotometricLight {                         // goniometric.rs:48-58
    Point3f p_light; Spectrum i; OptMap mipmap; Transform light_to_world, world_to_light;
    Spectrum scale(const Vector3f& w) const; Spectrum power() const;
    Spectrum sample_li(const InteractionCommon& iref, InteractionCommon& light_intr, Point2f _u, Vector3f* wi, Float* pdf, VisibilityTester& vis) const;
};
}
"""

SPATIAL_CARRIERS = r"""
// ---- SpatialLightDistribution::compute_distribution over a light list that knows the two map lights: the flow batch's carriers (SpatialScene, SpatialLightDistribution) with one
// change, the dispatch in sample_li.  The body is the reference's text, compiled below by the flow batch's rules ----
namespace flow {
typedef bool (*MapLightSampleLi)(uint32_t index, const orc::V3& ref_p, Spectrum* li, Vector3f* wi, Float* pdf, orc::V3* p_light);      // true and the text's values, or false: not a map light
struct MapSpatialScene {
    const Scene* s; MapLightSampleLi map_light;
    Bounds3fL world_bound() const { return SpatialScene{s, {s}}.world_bound(); }
    struct Lights { const Scene* s; MapLightSampleLi map_light; size_t len() const { return s->lights.len(); }
        struct L { const Scene* s; MapLightSampleLi map_light; uint32_t index;
            Spectrum sample_li(const InteractionCommon& iref, InteractionCommon* light_intr, Point2f u, Vector3f* wi, Float* pdf, VisibilityTester* vis) const {
                Spectrum ml; orc::V3 pl{0, 0, 0};
                if (map_light(index, iref.it.p, &ml, wi, pdf, &pl)) { light_intr->it.p = pl; return ml; }
                return SpatialScene::Lights::L{s, index}.sample_li(iref, light_intr, u, wi, pdf, vis);
            } };
        L operator[](size_t j) const { return L{s, map_light, (uint32_t)j}; } } lights;
};
struct MapSpatialLightDistribution { MapSpatialScene scene; int32_t n_voxels[3]; Distribution1D compute_distribution(const Point3i& pi) const; };
}
"""

PL, GL = r"^impl ProjectionLight \{", r"^impl GonioPhotometricLight \{"
SOURCES = [
    ("core/geometry.rs", r"^impl Bounds2f \{", r"^    pub fn offset\(&self, p: Point2f\) -> Vector2f \{", "offset", "Bounds2f"),
    ("lights/projection.rs", PL, r"^    pub fn projection\(&self, w: &Vector3f\) -> Spectrum \{", "projection", "ProjectionLight"),
    ("lights/projection.rs", PL, r"^    pub fn sample_li<'a, 'b>\($", "sample_li", "ProjectionLight"),
    ("lights/projection.rs", PL, r"^    pub fn power\(&self\) -> Spectrum \{", "power", "ProjectionLight"),
    ("lights/goniometric.rs", GL, r"^    pub fn scale\(&self, w: &Vector3f\) -> Spectrum \{", "scale", "GonioPhotometricLight"),
    ("lights/goniometric.rs", GL, r"^    pub fn sample_li<'a, 'b>\($", "sample_li", "GonioPhotometricLight"),
    ("lights/goniometric.rs", GL, r"^    pub fn power\(&self\) -> Spectrum \{", "power", "GonioPhotometricLight"),
]
TYPES_EXTRA = {"Bounds2f": "Bounds2f", "Vector2f": "Vector2f", "Point2f": "Point2f", "Point3f": "Point3f", "Vector3f": "Vector3f", "Transform": "Transform", "Spectrum": "Spectrum",
               "&Vector3f": "const Vector3f&", "&InteractionCommon": "const InteractionCommon&", "&mut InteractionCommon": "InteractionCommon&", "&mut Vector3f": "Vector3f*",
               "&mut Float": "Float*", "&mut VisibilityTester": "VisibilityTester&", "Float": "Float", "bool": "bool"}
LITERALS = ("Point3f", "Point2f", "Bounds2f")      # L1: their fields are written in the carrier's declared order (the shape batch's S6)

RULES_LIGHTB = [
    # L2  the optional map: `if let Some(m) = &self.map {` borrows a field (the flow batch's F3 then tests and unwraps it)
    (r"if let Some\((\w+)\) = &this->(\w+) \{", r"if let Some(\1) = this->\2 {", 0),
    # L3  conversions between the point / vector carriers, whatever the argument
    (r"\bPoint2f::from\(", "Point2f_from(", 0), (r"\bVector3f::from\(", "Vector3f_from(", 0),
    # L4  `std::mem::swap(&mut a.y, &mut a.z)` on two fields
    (r"std::mem::swap\(&mut (\w+\.\w+), &mut (\w+\.\w+)\)", r"std::swap(\1, \2)", 0),
    # L5  `let b = if C {\n Bounds2f{..}\n } else {\n Bounds2f{..}\n };` (after L1): a conditional over the two literals
    (r"let (\w+) = if ([^{}]*?) \{\s*(Bounds2f\{[^;]*?\})\s*\} else \{\s*(Bounds2f\{[^;]*?\})\s*\};", r"Bounds2f \1 = (\2) ? \3 : \4;", re.S),
    # L6  Transform's associated functions (the flow batch's F29 names them so)
    (r"Transform::perspective\(", "transform_perspective(", 0), (r"Transform::inverse\(", "transform_inverse(", 0),
]
TYPED_LET = r"\blet (?:mut )?(\w+): (Transform|Point3f|Point2f|Vector2f|Vector3f|Bounds2f|Spectrum|Float|bool) = "


def rewrite(body, sig, params, fn_names):
    """a body through the rules, in order: L1 (struct literals), L2 .. L6, the earlier batches' rules, the typed declarations, shadowing"""
    body = flow.join_multiline_if(body)
    for lit in LITERALS:
        body = shape.struct_literal(body, lit, lit)
    for pat, rep, flags in RULES_LIGHTB + geom.RULES_LIGHT + flow.RULES_CAM + flow.RULES_FLOW + geom.RULES_INT + geom.RULES_PRE:
        body = re.sub(pat, rep, body, flags=flags)
    body = geom.cast_after_parens(body, "Float", "Float(%s)")
    for pat, rep, flags in base.RULES:
        body = re.sub(pat, rep, body, flags=flags)
    body = re.sub(TYPED_LET, lambda m: "%s %s = " % (m.group(2), m.group(1)), body)
    body = base.shadowing(body, set(params) | fn_names)
    return body


def new_blocks():
    """ProjectionLight::new_hdr from `p_light` to `cos_total_width` and GonioPhotometricLight::new_hdr's p_light line, each with the `world_to_light` initialiser of the
    struct literal behind it (L7: `field: E,` -> `let field: Transform = E;`), as functions over the carriers (as the flow and camera batches compile blocks)"""
    out = []
    for fname, first, last, sig, tail, params, label in (
            ("lights/projection.rs", "let p_light: Point3f = light_to_world.transform_point(&Point3f::default());", "return ProjectionLight {",
             "static void projection_new_block(const Transform& light_to_world, Point2i resolution, Float fov, ProjectionLight* out) {\n",
             "    out->p_light = p_light; out->light_projection = light_projection; out->hither = hither; out->yon = yon; out->screen_bounds = screen_bounds; out->cos_total_width = cos_total_width;\n"
             "    out->light_to_world = light_to_world; out->world_to_light = world_to_light;      // (hand-written: the fields the constructor stores)\n}\n",
             {"light_to_world", "resolution", "fov"}, "ProjectionLight::new_hdr (p_light .. cos_total_width, world_to_light)"),
            ("lights/goniometric.rs", "let p_light: Point3f = light_to_world.transform_point(&Point3f::default());", "return GonioPhotometricLight {",
             "static void goniometric_new_block(const Transform& light_to_world, GonioPhotometricLight* out) {\n",
             "    out->p_light = p_light; out->light_to_world = light_to_world; out->world_to_light = world_to_light;      // (hand-written: the fields the constructor stores)\n}\n",
             {"light_to_world"}, "GonioPhotometricLight::new_hdr (p_light, world_to_light)")):
        lines = open(REF + fname).read().split("\n")
        h0 = next(k for k, l in enumerate(lines) if l.strip() == "pub fn new_hdr(")
        i0 = next(k for k in range(h0, len(lines)) if lines[k].strip() == first)
        i1 = next(k for k in range(i0, len(lines)) if lines[k].strip() == last)
        w = next(k for k in range(i1, len(lines)) if lines[k].strip() == "world_to_light: Transform::inverse(light_to_world),")
        src = lines[i0:i1] + [re.sub(r"^(\s*)(\w+): (.+),$", r"\1let \2: Transform = \3;", lines[w])]
        text = "\n".join("    " + l.strip() if k == len(src) - 1 else (("    " + l[len(lines[i0]) - len(lines[i0].lstrip()):]) if l.strip() else "") for k, l in enumerate(src))
        body = re.sub(r"^\s*//.*\n", "", text, flags=re.M) + "\n}\n"
        body = rewrite(body, sig, set(params), set(geom.FN_NAMES))
        out.append(("// %s%s:%d-%d, %d\n%s%s" % (REF, fname, i0 + 1, i1, w + 1, sig, body.rstrip()[:-1].rstrip() + "\n" + tail), "%s %s:%d-%d,%d" % (label, fname, i0 + 1, i1, w + 1)))
    return out


def convert_parts():
    saved = (dict(geom.TYPES), dict(base.TYPES), dict(flow.TYPES))
    try:
        return _convert_parts()
    finally:
        geom.TYPES.clear(); geom.TYPES.update(saved[0]); base.TYPES.clear(); base.TYPES.update(saved[1]); flow.TYPES.clear(); flow.TYPES.update(saved[2])


def _convert_parts():
    parts, where = camera.convert_parts()       # the five earlier batches: prelude, carriers and every function they compile (their spans come first in `where`)
    where = list(where)
    parts.append(CARRIERS)
    types = dict(geom.TYPES)
    types.update(TYPES_EXTRA)
    fn_names = set(geom.FN_NAMES) | {s[3] for s in SOURCES}
    code = []
    for fname, after_re, first_re, name, cls in SOURCES:
        for tab in (geom.TYPES, base.TYPES):
            tab.clear(); tab.update(types)
            tab["Self"] = cls
        text, l0, l1 = geom.extract(fname, after_re, first_re, None)
        text = re.sub(r"^\s*//.*\n", "", text, flags=re.M)                      # comment lines
        sig, body, params = geom.signature(text, name, cls)
        body = rewrite(body, sig, params, fn_names)
        if not sig.startswith("void"):
            body = geom.tail_value(body)
        code.append("// %s%s:%d-%d\n%s%s" % (REF, fname, l0, l1, sig, body))
        where.append("%s::%s %s:%d-%d" % (cls, name, fname, l0, l1))
    for tab in (geom.TYPES, base.TYPES):
        tab.clear(); tab.update(types)
    for text, label in new_blocks():
        code.append(text)
        where.append(label)
    parts.append("namespace lightb {\n" + "\n".join(code) + "}\n")
    text, label = spatial_part()
    parts.append(SPATIAL_CARRIERS)
    parts.append(text)
    where.append(label)
    return parts, where


def spatial_part():
    """SpatialLightDistribution::compute_distribution through the flow batch's own steps (make_flow_fixtures._convert_parts, a source of its `in_flow` kind: F15, F11, G15 .. G17, the
    base rules), as a method of the carrier above"""
    fname, cls, name = "core/lightdistrib.rs", "MapSpatialLightDistribution", "compute_distribution"
    for tab in (geom.TYPES, base.TYPES):
        tab.update(flow.TYPES)
    text, l0, l1 = geom.extract(fname, None, r"^    pub fn compute_distribution\(&self, pi: &Point3i\) -> Distribution1D \{", None)
    text = re.sub(r"^\s*//.*\n", "", text, flags=re.M)
    sig, body, params = geom.signature(text, name, cls)
    body = flow.join_multiline_if(body)
    for pat, rep_, flags in flow.RULES_FLOW + geom.RULES_INT + geom.RULES_PRE:
        body = re.sub(pat, rep_, body, flags=flags)
    body = geom.cast_after_parens(body, "Float", "Float(%s)")
    body = geom.cast_after_parens(body, "usize", "(size_t)(%s)")
    for pat, rep_, flags in base.RULES:
        body = re.sub(pat, rep_, body, flags=flags)
    body = re.sub(r"\blet (?:mut )?(\w+): (usize|bool|Float|Point3f|Point2f|Spectrum|Vector3f|VisibilityTester|InteractionCommon) = ", lambda m: "%s %s = " % (flow.TYPES.get(m.group(2), m.group(2)), m.group(1)), body)
    body = re.sub(r"\blet (\w+): (usize|Float);", lambda m: "%s %s;" % (flow.TYPES[m.group(2)], m.group(1)), body)
    base.TYPES["T"] = "Float"
    body = base.shadowing(body, set(params) | set(geom.FN_NAMES) | {"li"})
    body = geom.tail_value(body)
    return "namespace flow {\n// %s%s:%d-%d\n%s%s}\n" % (REF, fname, l0, l1, sig, body), "%s::%s %s:%d-%d" % (cls, name, fname, l0, l1)


WRAPPERS = r"""
// ---- the C wrapper: values are moved, the class of a direction is named from values the text computed; nothing else is computed here ----
extern "C" {
struct lightref_light { int32_t kind, map; float p_light[3], i[3], w2l[16], l2w[16], proj[16], proj_inv[16], hither, yon, sb[4], cos_total_width; };      // kind: RSPT_LIGHT_PROJECTION / _GONIOMETRIC, 0: another kind; map: index or -1
struct lightref_pyramid { const float* texels; uint32_t width, height, n_levels; };      // the pyramid, level after level (rspt_envmap's layout)
}
namespace lightb {
static inline Matrix4x4 mat_of(const float* m) { Matrix4x4 r; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.m[i][j] = Float(m[4 * i + j]); return r; }
static inline void mat_out(const Matrix4x4& m, float* o) { for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) o[4 * i + j] = m.m[i][j].v; }
static inline Spectrum spec_of(const float* p) { Spectrum r; for (int k = 0; k < 3; k++) r.c[k] = Float(p[k]); return r; }
struct Maps {
    std::vector<MipMapS> mm;
    Maps(const lightref_pyramid* maps, uint32_t n) : mm(n) {
        for (uint32_t k = 0; k < n; k++) {
            mm[k].wrap_mode = ImageWrap::Repeat;                      // projection.rs:257, goniometric.rs:197
            const float* p = maps[k].texels; size_t w = maps[k].width, h = maps[k].height;
            for (uint32_t l = 0; l < maps[k].n_levels; l++) { mm[k].pyramid.push(MipLevel{p, w, h}); p += 3 * w * h; w = std::max<size_t>(1, w / 2); h = std::max<size_t>(1, h / 2); }
        }
    }
    OptMap of(int32_t k) const { return k < 0 ? OptMap{false, MapRef{nullptr}} : OptMap{true, MapRef{&mm[(size_t)k]}}; }
};
static ProjectionLight projection_of(const lightref_light& l, const Maps& maps) {
    ProjectionLight pl{};
    pl.projection_map = maps.of(l.map); pl.p_light = Point3f{Float(l.p_light[0]), Float(l.p_light[1]), Float(l.p_light[2])}; pl.i = spec_of(l.i);
    pl.light_projection = Transform{mat_of(l.proj), mat_of(l.proj_inv)}; pl.hither = Float(l.hither); pl.yon = Float(l.yon);
    pl.screen_bounds = Bounds2f{Point2f{Float(l.sb[0]), Float(l.sb[1])}, Point2f{Float(l.sb[2]), Float(l.sb[3])}}; pl.cos_total_width = Float(l.cos_total_width);
    pl.light_to_world = Transform{mat_of(l.l2w), mat_of(l.w2l)}; pl.world_to_light = Transform{mat_of(l.w2l), mat_of(l.l2w)};
    return pl;
}
static GonioPhotometricLight gonio_of(const lightref_light& l, const Maps& maps) {
    GonioPhotometricLight gl{};
    gl.p_light = Point3f{Float(l.p_light[0]), Float(l.p_light[1]), Float(l.p_light[2])}; gl.i = spec_of(l.i); gl.mipmap = maps.of(l.map);
    gl.light_to_world = Transform{mat_of(l.l2w), mat_of(l.w2l)}; gl.world_to_light = Transform{mat_of(l.w2l), mat_of(l.l2w)};
    return gl;
}
// the class of a direction, named from the values the text's own functions give for it.  Projection: 0 behind the hither plane, 1 / 2 left of p_min.x / right of p_max.x,
// 3 / 4 below p_min.y / above p_max.y (the first that applies), 5 inside, 6 none (a NaN).  Goniometric: 8 + the quadrant of phi
static uint8_t class_of(const ProjectionLight& pl, const Vector3f& w) {
    const Vector3f wl = pl.world_to_light.transform_vector(w);
    if (wl.z < pl.hither) return 0;
    const Point3f p = pl.light_projection.transform_point(Point3f{wl.x, wl.y, wl.z});
    if (pnt2_inside_bnd2f(Point2f{p.x, p.y}, pl.screen_bounds)) return 5;
    if (p.x < pl.screen_bounds.p_min.x) return 1;
    if (p.x > pl.screen_bounds.p_max.x) return 2;
    if (p.y < pl.screen_bounds.p_min.y) return 3;
    if (p.y > pl.screen_bounds.p_max.y) return 4;
    return 6;
}
static uint8_t class_of(const GonioPhotometricLight& gl, const Vector3f& w) {
    Vector3f wp = gl.world_to_light.transform_vector(w).normalize();
    std::swap(wp.y, wp.z);
    const float phi = spherical_phi(wp).v;
    return (uint8_t)(8 + (phi < 1.5707964f ? 0 : (phi < 3.1415927f ? 1 : (phi < 4.712389f ? 2 : 3))));
}
// the intermediate values a case is CHOSEN and LABELLED by (never compared): wl, p.x, p.y | wp after the swap, phi, theta, st
static void aux_of(const ProjectionLight& pl, const Vector3f& w, float* a) {
    const Vector3f wl = pl.world_to_light.transform_vector(w);
    const Point3f p = pl.light_projection.transform_point(Point3f{wl.x, wl.y, wl.z});
    a[0] = wl.x.v; a[1] = wl.y.v; a[2] = wl.z.v; a[3] = p.x.v; a[4] = p.y.v; a[5] = a[6] = a[7] = 0.0f;
}
static void aux_of(const GonioPhotometricLight& gl, const Vector3f& w, float* a) {
    Vector3f wp = gl.world_to_light.transform_vector(w).normalize();
    std::swap(wp.y, wp.z);
    const Float theta = spherical_theta(wp), phi = spherical_phi(wp);
    a[0] = wp.x.v; a[1] = wp.y.v; a[2] = wp.z.v; a[3] = phi.v; a[4] = theta.v; a[5] = (phi * INV_2_PI).v; a[6] = (theta * INV_PI).v; a[7] = 0.0f;
}
static Spectrum run_sample_li(const lightref_light& l, const Maps& maps, const Point3f& ref, Vector3f* wi, Float* pdf, Point3f* p_out) {
    const InteractionCommon iref{ref, Float(0.25f), Vector3f{Float(0.0f), Float(0.0f), Float(0.0f)}, Vector3f{Float(0.0f), Float(0.0f), Float(0.0f)}, Normal3f{Float(0.0f), Float(0.0f), Float(0.0f)}, None};
    InteractionCommon li = iref; li.time = Float(0.0f); VisibilityTester vis{nullptr, nullptr};
    const Spectrum s = l.kind == RSPT_LIGHT_PROJECTION ? projection_of(l, maps).sample_li(iref, li, Point2f{Float(0.5f), Float(0.5f)}, wi, pdf, vis)
                                                       : gonio_of(l, maps).sample_li(iref, li, Point2f{Float(0.5f), Float(0.5f)}, wi, pdf, vis);
    *p_out = li.p;
    return s;
}
// what the light list's dispatch (flow::MapSpatialScene above) reads while compute_distribution runs
static const lightref_light* g_lights = nullptr; static const rspt_light* g_records = nullptr; static const Maps* g_maps = nullptr; static uint64_t* g_counts = nullptr;
static bool hook(uint32_t index, const orc::V3& ref_p, Spectrum* li, Vector3f* wi, Float* pdf, orc::V3* p_light) {
    const lightref_light& l = g_lights[index];
    if (l.kind != RSPT_LIGHT_PROJECTION && l.kind != RSPT_LIGHT_GONIOMETRIC) {
        if (g_records[index].kind == RSPT_LIGHT_POINT && g_records[index].p[0] == ref_p.x && g_records[index].p[1] == ref_p.y && g_records[index].p[2] == ref_p.z) g_counts[15] += 1;
        return false;
    }
    if (l.p_light[0] == ref_p.x && l.p_light[1] == ref_p.y && l.p_light[2] == ref_p.z) g_counts[15] += 1;      // a voxel sample point AT a light: the table would not be finite
    Point3f pl{};
    *li = run_sample_li(l, *g_maps, Point3f{Float(ref_p.x), Float(ref_p.y), Float(ref_p.z)}, wi, pdf, &pl);
    *p_light = orc::V3{pl.x.v, pl.y.v, pl.z.v};
    g_counts[l.kind == RSPT_LIGHT_PROJECTION ? class_of(projection_of(l, *g_maps), -(*wi)) : class_of(gonio_of(l, *g_maps), -(*wi))] += 1;
    return true;
}
}
extern "C" {
// light_to_world of `LookAt from to up` as scenes.py's builder takes it: Transform::inverse(Transform::look_at(from, to, up)) -> m, m_inv
void lightref_look_at(const float* from, const float* to, const float* up, float* l2w, float* w2l) {
    const Transform t = transform_inverse(transform_look_at(Point3f{Float(from[0]), Float(from[1]), Float(from[2])}, Point3f{Float(to[0]), Float(to[1]), Float(to[2])}, Vector3f{Float(up[0]), Float(up[1]), Float(up[2])}));
    lightb::mat_out(t.m, l2w); lightb::mat_out(t.m_inv, w2l);
}
// Transform::new (transform.rs:264-301): m_inv = Matrix4x4::inverse(m)
void lightref_inverse(const float* m, float* m_inv) { lightb::mat_out(matrix4x4_inverse(lightb::mat_of(m)), m_inv); }
// the constructor blocks: ProjectionLight::new_hdr over (light_to_world, fov, resolution), GonioPhotometricLight::new_hdr over light_to_world
void lightref_projection_new(const float* l2w, const float* w2l, float fov, int32_t resx, int32_t resy, lightref_light* out) {
    lightb::ProjectionLight pl{};
    lightb::projection_new_block(Transform{lightb::mat_of(l2w), lightb::mat_of(w2l)}, Point2i{resx, resy}, Float(fov), &pl);
    out->kind = RSPT_LIGHT_PROJECTION;
    out->p_light[0] = pl.p_light.x.v; out->p_light[1] = pl.p_light.y.v; out->p_light[2] = pl.p_light.z.v;
    lightb::mat_out(pl.world_to_light.m, out->w2l); lightb::mat_out(pl.world_to_light.m_inv, out->l2w); lightb::mat_out(pl.light_projection.m, out->proj); lightb::mat_out(pl.light_projection.m_inv, out->proj_inv);
    out->hither = pl.hither.v; out->yon = pl.yon.v; out->cos_total_width = pl.cos_total_width.v;
    out->sb[0] = pl.screen_bounds.p_min.x.v; out->sb[1] = pl.screen_bounds.p_min.y.v; out->sb[2] = pl.screen_bounds.p_max.x.v; out->sb[3] = pl.screen_bounds.p_max.y.v;
}
void lightref_goniometric_new(const float* l2w, const float* w2l, lightref_light* out) {
    lightb::GonioPhotometricLight gl{};
    lightb::goniometric_new_block(Transform{lightb::mat_of(l2w), lightb::mat_of(w2l)}, &gl);
    out->kind = RSPT_LIGHT_GONIOMETRIC;
    out->p_light[0] = gl.p_light.x.v; out->p_light[1] = gl.p_light.y.v; out->p_light[2] = gl.p_light.z.v;
    lightb::mat_out(gl.world_to_light.m, out->w2l); lightb::mat_out(gl.world_to_light.m_inv, out->l2w);
}
// ProjectionLight::projection(w) / GonioPhotometricLight::scale(w): w n x 3 -> out n x 3, cls n, aux n x 8
void lightref_map(const lightref_light* l, const lightref_pyramid* maps, uint32_t n_maps, const float* w, uint64_t n, float* out, uint8_t* cls, float* aux) {
    const lightb::Maps mm(maps, n_maps);
    const lightb::ProjectionLight pl = lightb::projection_of(*l, mm); const lightb::GonioPhotometricLight gl = lightb::gonio_of(*l, mm);
    for (uint64_t i = 0; i < n; i++) {
        const Vector3f v{Float(w[3 * i]), Float(w[3 * i + 1]), Float(w[3 * i + 2])};
        const Spectrum s = l->kind == RSPT_LIGHT_PROJECTION ? pl.projection(v) : gl.scale(v);
        for (int k = 0; k < 3; k++) out[3 * i + k] = s.c[k].v;
        cls[i] = l->kind == RSPT_LIGHT_PROJECTION ? lightb::class_of(pl, v) : lightb::class_of(gl, v);
        if (l->kind == RSPT_LIGHT_PROJECTION) lightb::aux_of(pl, v, aux + 8 * i); else lightb::aux_of(gl, v, aux + 8 * i);
    }
}
// sample_li at the reference points p (n x 3): out n x 10 = value (3), wi (3), pdf, light_intr.p (3)
void lightref_sample_li(const lightref_light* l, const lightref_pyramid* maps, uint32_t n_maps, const float* p, uint64_t n, float* out) {
    const lightb::Maps mm(maps, n_maps);
    for (uint64_t i = 0; i < n; i++) {
        Vector3f wi{Float(0.0f), Float(0.0f), Float(0.0f)}; Float pdf(0.0f); Point3f pl{};
        const Spectrum s = lightb::run_sample_li(*l, mm, Point3f{Float(p[3 * i]), Float(p[3 * i + 1]), Float(p[3 * i + 2])}, &wi, &pdf, &pl);
        const Float v[10] = {s.c[0], s.c[1], s.c[2], wi.x, wi.y, wi.z, pdf, pl.x, pl.y, pl.z};
        for (int k = 0; k < 10; k++) out[10 * i + k] = v[k].v;
    }
}
void lightref_power(const lightref_light* l, const lightref_pyramid* maps, uint32_t n_maps, float* out) {
    const lightb::Maps mm(maps, n_maps);
    const Spectrum s = l->kind == RSPT_LIGHT_PROJECTION ? lightb::projection_of(*l, mm).power() : lightb::gonio_of(*l, mm).power();
    for (int k = 0; k < 3; k++) out[k] = s.c[k].v;
    out[3] = s.y().v;      // what compute_light_power_distribution takes of it (integrator.rs:573-584)
}
// The light distribution of (scene, strategy) at the points pts (n x 3), as rspt_light_distribution reports it: func (n x n_lights), cdf (n x (n_lights + 1)), the grid, the voxel of each
// point.  lights[i].kind names the map lights of sd->lights (the text compiled above serves them); a point or a triangle area light keeps the flow batch's route.  Uniform:
// Distribution1D::new over ones (lightdistrib.rs:30-37); power: over Light::power().y() (integrator.rs:573-584); spatial: compute_distribution of the point's voxel.
// counts[0..11]: the (voxel sample point, map light) pairs per class over the distinct voxels computed; counts[15]: sample points that equal a light's position.  -1: a light kind without a route
int lightref_tables(const rspt_scene_desc* sd, const lightref_light* lights, const lightref_pyramid* maps, uint32_t n_maps, uint32_t strategy, const float* pts, uint64_t n, float* func, float* cdf,
                    int32_t* nvox, int32_t* voxel, uint64_t* counts) {
    const uint32_t nl = sd->n_lights;
    const lightb::Maps mm(maps, n_maps);
    std::vector<rspt_light> masked(sd->lights, sd->lights + nl);      // the oracle knows neither kind: in its Scene each is a black point light at the same place (as tests/maplight_restated.cpp does)
    for (uint32_t i = 0; i < nl; i++) {
        const bool ml = masked[i].kind == RSPT_LIGHT_PROJECTION || masked[i].kind == RSPT_LIGHT_GONIOMETRIC;
        if (ml != (lights[i].kind != 0)) return -2;
        if (ml) { const float px = masked[i].p[0], py = masked[i].p[1], pz = masked[i].p[2]; masked[i] = rspt_light{}; masked[i].kind = RSPT_LIGHT_POINT; masked[i].p[0] = px; masked[i].p[1] = py; masked[i].p[2] = pz; }
        else if (masked[i].kind != RSPT_LIGHT_POINT && masked[i].kind != RSPT_LIGHT_DIFFUSE_AREA) return -1;
    }
    rspt_scene_desc copy = *sd; copy.lights = masked.data();
    orc::Scene sc{copy};
    sc.prepare_media();
    rspt_render_desc rd{}; rd.light_strategy = strategy;
    orc::RenderCtx cx; cx.scene = &sc; cx.rd = &rd;
    for (uint32_t i = 0; i < nl; i++) cx.n_light_samples.push_back(1);
    orc::light_distrib_init(cx);
    nvox[0] = nvox[1] = nvox[2] = 1;
    auto put = [&](uint64_t i, const flow::Distribution1D& d) { for (uint32_t j = 0; j < nl; j++) func[nl * i + j] = d.func[j].v; for (uint32_t j = 0; j <= nl; j++) cdf[(nl + 1) * i + j] = d.cdf[j].v; };
    if (cx.strategy != RSPT_LIGHTS_SPATIAL) {
        Vec<Float> f;
        static const uint32_t idx[3] = {0, 1, 2};
        for (uint32_t i = 0; i < nl; i++) {
            if (cx.strategy == RSPT_LIGHTS_UNIFORM) { f.push(Float(1.0f)); continue; }
            const rspt_light& l = sd->lights[i];
            Spectrum pw = Spectrum::new_(Float(0.0f));
            if (lights[i].kind == RSPT_LIGHT_PROJECTION) pw = lightb::projection_of(lights[i], mm).power();
            else if (lights[i].kind == RSPT_LIGHT_GONIOMETRIC) pw = lightb::gonio_of(lights[i], mm).power();
            else if (l.kind == RSPT_LIGHT_POINT) pw = PointLight{Point3f{Float(l.p[0]), Float(l.p[1]), Float(l.p[2])}, flow::S3f(l.L)}.power();
            else {      // (as the flow batch's flow_light_power builds it)
                const rspt_prim& pr = sd->prims[l.prim];
                Point3f tp[3]; for (int k = 0; k < 3; k++) { const float* q = sd->P + 3 * (size_t)pr.v[k]; tp[k] = Point3f{Float(q[0]), Float(q[1]), Float(q[2])}; }
                DiffuseAreaLight dl{}; dl.l_emit = flow::S3f(l.L); dl.two_sided = l.two_sided != 0; dl.shape.id = 0; dl.shape.mesh.vertex_indices = idx; dl.shape.mesh.p = tp;
                dl.area = dl.shape.area();
                pw = dl.power();
            }
            f.push(pw.y());
        }
        const flow::Distribution1D d = flow::Distribution1D::new_(f);
        for (uint64_t i = 0; i < n; i++) { put(i, d); voxel[3 * i] = voxel[3 * i + 1] = voxel[3 * i + 2] = 0; }
        return (int)nl;
    }
    for (int k = 0; k < 3; k++) nvox[k] = cx.n_voxels[k];
    flow::Scene scene{&cx, nullptr, {}, {}};
    for (uint32_t i = 0; i < nl; i++) scene.lights.v.push_back(flow::LightRef{&scene, i});
    const flow::MapSpatialLightDistribution sld{flow::MapSpatialScene{&scene, lightb::hook, {&scene, lightb::hook}}, {cx.n_voxels[0], cx.n_voxels[1], cx.n_voxels[2]}};
    std::map<std::array<int32_t, 3>, flow::Distribution1D> done;
    lightb::g_lights = lights; lightb::g_records = sd->lights; lightb::g_maps = &mm; lightb::g_counts = counts;
    for (uint64_t i = 0; i < n; i++) {
        const orc::V3 off = sc.world_bound().offset(orc::V3{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]});      // SpatialLightDistribution::lookup (lightdistrib.rs:276-295), as the oracle states it
        std::array<int32_t, 3> pi;
        for (int k = 0; k < 3; k++) pi[k] = voxel[3 * i + k] = orc::clamp_t(orc::f2i(off[k] * (float)cx.n_voxels[k]), 0, cx.n_voxels[k] - 1);
        auto it = done.find(pi);
        if (it == done.end()) it = done.emplace(pi, sld.compute_distribution(flow::Point3i{pi[0], pi[1], pi[2]})).first;
        put(i, it->second);
    }
    return (int)nl;
}
}
"""


def convert():
    parts, where = convert_parts()
    parts.append(WRAPPERS)
    os.makedirs(OUT_DIR, exist_ok=True)
    cpp = os.path.join(OUT_DIR, "light_functions.cpp")
    open(cpp, "w").write("\n".join(parts))
    so = os.path.join(OUT_DIR, "liblightref.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), "-o", so, cpp])
    L = C.CDLL(so)
    vp, f, u32, u64, i32 = C.c_void_p, C.c_float, C.c_uint32, C.c_uint64, C.c_int32
    for name, args in (("lightref_look_at", [vp] * 5), ("lightref_inverse", [vp, vp]), ("lightref_projection_new", [vp, vp, f, i32, i32, vp]), ("lightref_goniometric_new", [vp, vp, vp]),
                       ("lightref_map", [vp, vp, u32, vp, u64, vp, vp, vp]), ("lightref_sample_li", [vp, vp, u32, vp, u64, vp]), ("lightref_power", [vp, vp, u32, vp])):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = args
    L.lightref_tables.restype = C.c_int
    L.lightref_tables.argtypes = [vp, vp, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    return L, where


# ---------------------------------------------------------------- running the text ----------------------------------------------------------------
F32 = np.float32
SEED = 0x11647
PROJ, GONIO = 6, 7      # RSPT_LIGHT_PROJECTION / RSPT_LIGHT_GONIOMETRIC (checked against rs_pbrt_amd.abi in reference())


class MapC(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("n_levels", C.c_uint32)]


def _helpers():
    import tests.test_reference_light_functions as t      # the record and scene helpers live with the tests that read the committed file alone (they need no reference tree)
    return t


class Maps:
    """the pyramids of the fixture's maps as the wrapper's array"""
    def __init__(self, pyramids):
        self.pyramids = [(w, h, n, np.ascontiguousarray(t, F32)) for w, h, n, t in pyramids]
        self.arr = (MapC * max(1, len(self.pyramids)))()
        for k, (w, h, n, t) in enumerate(self.pyramids):
            self.arr[k] = MapC(t.ctypes.data, w, h, n)

    def __len__(self):
        return len(self.pyramids)


def light_struct(kind, k, f):
    a = np.zeros(1, _helpers().lightref_dt())
    a["kind"], a["map"], a["f"] = kind, k, np.asarray(f, F32)
    return a


def run_map(L, lt, maps, w):
    """projection(w) / scale(w) by the text: out (n, 3), the class of each direction, the intermediate values (n, 8)"""
    w = np.ascontiguousarray(w, F32).reshape(-1, 3)
    out, cls, aux = np.zeros((len(w), 3), F32), np.zeros(len(w), np.uint8), np.zeros((len(w), 8), F32)
    L.lightref_map(lt.ctypes.data, C.addressof(maps.arr), len(maps), w.ctypes.data, len(w), out.ctypes.data, cls.ctypes.data, aux.ctypes.data)
    return out, cls, aux


def run_sample_li(L, lt, maps, p):
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    out = np.zeros((len(p), 10), F32)
    L.lightref_sample_li(lt.ctypes.data, C.addressof(maps.arr), len(maps), p.ctypes.data, len(p), out.ctypes.data)
    return out


def run_power(L, lt, maps):
    out = np.zeros(4, F32)
    L.lightref_power(lt.ctypes.data, C.addressof(maps.arr), len(maps), out.ctypes.data)
    return out


def look_at(L, frm, to, up):
    a, b, c, m, mi = (np.array(v, F32) for v in (frm, to, up, np.zeros(16), np.zeros(16)))
    L.lightref_look_at(a.ctypes.data, b.ctypes.data, c.ctypes.data, m.ctypes.data, mi.ctypes.data)
    return m, mi


def inverse(L, m):
    m, mi = np.ascontiguousarray(m, F32).reshape(16), np.zeros(16, F32)
    L.lightref_inverse(m.ctypes.data, mi.ctypes.data)
    return mi


def projection_new(L, frm, to, up, fov, rx, ry):
    """ProjectionLight::new_hdr's block by the text: the light's fields (i left zero)"""
    l2w, w2l = look_at(L, frm, to, up)
    a = light_struct(0, -1, np.zeros(77))
    L.lightref_projection_new(l2w.ctypes.data, w2l.ctypes.data, float(fov), int(rx), int(ry), a.ctypes.data)
    assert a["kind"][0] == PROJ
    return a["f"][0].copy()


def goniometric_new(L, m):
    m = np.ascontiguousarray(m, F32).reshape(16)
    mi = inverse(L, m)
    a = light_struct(0, -1, np.zeros(77))
    L.lightref_goniometric_new(m.ctypes.data, mi.ctypes.data, a.ctypes.data)
    assert a["kind"][0] == GONIO
    return a["f"][0].copy()


def run_tables(L, sc, lights, maps, strategy, pts):
    """the text's tables of one scene and strategy at pts: func (n, nl), cdf (n, nl + 1), nvox (3), voxel (n, 3), counts (16)"""
    nl, pts = int(sc.desc.n_lights), np.ascontiguousarray(pts, F32).reshape(-1, 3)
    func, cdf, nvox, voxel, counts = np.zeros((len(pts), nl), F32), np.zeros((len(pts), nl + 1), F32), np.zeros(3, np.int32), np.zeros((len(pts), 3), np.int32), np.zeros(16, np.uint64)
    assert len(lights) == nl
    r = L.lightref_tables(C.addressof(sc.desc), lights.ctypes.data, C.addressof(maps.arr), len(maps), int(strategy), pts.ctypes.data, len(pts), func.ctypes.data, cdf.ctypes.data, nvox.ctypes.data,
                          voxel.ctypes.data, counts.ctypes.data)
    assert r == nl, r
    return func, cdf, nvox, voxel, counts


# ---------------------------------------------------------------- seeded inputs ----------------------------------------------------------------
MAP_SHAPES = ((8, 2), (2, 8), (4, 4), (1, 1), (16, 4), (2, 1), (1, 2))      # (w, h): wide, tall, square, 1 x 1 (one level), five levels, two levels wide and tall
AXIS = ((0, 0, 0), (0, 0, 1), (0, 1, 0))      # LookAt down +z from the origin: world_to_light has entries 0 and +-1 only, so a chosen light-space value is reached exactly
PROJ_LIGHTS = (      # (from, to, up), fov, map
    (AXIS, 45.0, 0), (((1, 2, 3), (0.25, -1, 0.5), (0, 1, 0)), 20.0, 1), (AXIS, 90.0, 2), (AXIS, 1.0, 3), (((-2, 1, 0.5), (1, 0, 2), (0, 0, 1)), 150.0, -1), (AXIS, 179.0, 4),
    (AXIS, 45.0, -1), (((0.5, 3, -1), (0, 0, 0), (1, 0, 0)), 90.0, 5), (AXIS, 20.0, 6))
DEGENERATE_OF = 2      # one more projection light: this one's fields with screen_bounds.p_min.y == p_max.y == 0 (Bounds2f::offset must not divide)


def rot(axis, deg):
    a = np.array(axis, np.float64); a /= np.linalg.norm(a)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4); m[:3, :3] = c * np.eye(3) + s * k + (1 - c) * np.outer(a, a)
    return m


def mat(rows3=None, t=(0, 0, 0)):
    m = np.eye(4)
    if rows3 is not None:
        m[:3, :3] = rows3
    m[:3, 3] = t
    return m


GONIO_LIGHTS = (      # light_to_world, map: identity, a rotation, a non-uniform scale, a shear, a translation (which must not matter), a mirror, and no map
    (mat(), 0), (rot((1, 2, 3), 40.0), 2), (mat(np.diag([2.0, 0.5, 3.0])), 1), (mat([[1, 0.5, 0], [0, 1, 0.25], [0, 0, 1]]), 4), (mat(t=(1, 2, 3)), 5), (mat(np.diag([-1.0, 1.0, 1.0])), 6),
    (rot((0, 1, 1), 115.0) @ mat(t=(0.5, -1, 2)), -1))


def grid(rng, shape, bits=10):
    """uniform numbers in [0, 1) on a 2^-bits grid (their f32 words keep the fixture small)"""
    return (rng.integers(0, 1 << bits, shape) / float(1 << bits)).astype(F32)


def step(x, k):
    """the f32 k ulps above x (below for k < 0), elementwise; +-0 are neighbours of the smallest denormals"""
    x = np.asarray(x, F32)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i) + k      # a monotone integer line through the floats
    return np.where(i < 0, (-i) | 0x80000000, i).astype(np.uint32).view(F32)


def ulps(a, b):
    """signed distance in ulps from b to a along that line"""
    def line(x):
        i = np.asarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return line(a) - line(b)


def make_maps(rng):
    from rs_pbrt_amd import scenes
    out = []
    for w, h in MAP_SHAPES:
        img = (F32(0.125) + F32(0.875) * grid(rng, (h, w, 3), 6)).astype(F32)
        m = scenes.build_light_map(img)
        assert (m["width"], m["height"]) == (w, h)
        out.append((w, h, int(m["n_levels"]), m["texels"]))
    return Maps(out)


def make_lights(L, rng, maps):
    """(kind, map, fields) of every light of the map cases: the constructor blocks over PROJ_LIGHTS / GONIO_LIGHTS, and the degenerate one"""
    out = []
    for (frm, to, up), fov, k in PROJ_LIGHTS:
        rx, ry = (1, 1) if k < 0 else maps.pyramids[k][:2]      # (scenes.py's builder gives a map-less light the geometry of a square map)
        f = projection_new(L, frm, to, up, fov, rx, ry)
        f[3:6] = F32(0.5) + F32(8) * grid(rng, 3, 4)
        out.append((PROJ, k, f))
    f = out[DEGENERATE_OF][2].copy()
    f[73] = f[75] = 0.0
    out.append((PROJ, out[DEGENERATE_OF][1], f))
    for m, k in GONIO_LIGHTS:
        f = goniometric_new(L, m.astype(F32))
        f[3:6] = F32(0.5) + F32(8) * grid(rng, 3, 4)
        out.append((GONIO, k, f))
    return out


def world_dirs(f, xl, yl, zl):
    """world directions whose light-space image is (xl, yl, zl) up to rounding: light_to_world's 3 x 3 in f64, then f32"""
    m = f[22:38].reshape(4, 4)[:3, :3].astype(np.float64)
    l = np.stack([np.asarray(v, np.float64) * np.ones(np.broadcast(xl, yl, zl).shape) for v in (xl, yl, zl)], 0)
    if not (m - np.diag(np.diag(m))).any():
        return (l.T * np.diag(m)).astype(F32)      # (a diagonal frame: each product alone, so a signed zero keeps its sign)
    return (m @ l).T.astype(F32)


def projection_candidates(rng, f, shape, n):
    """directions around every place where projection() decides: far more than are kept; the text's own intermediate values choose among them"""
    p18, p19, hither = float(f[38]), float(f[43]), f[70]
    x0, y0, x1, y1 = (float(v) for v in f[72:76])
    zs = np.array([1.0, 2.0, 0.375, 5.5])
    w = []

    def screen(px, py, z):      # the light-space direction of screen point (px, py) at depth z
        return np.asarray(px) * z / p18, np.asarray(py) * z / p19, z
    inx = lambda m: x0 + (x1 - x0) * grid(rng, m).astype(np.float64)      # noqa: E731
    iny = lambda m: y0 + (y1 - y0) * grid(rng, m).astype(np.float64)      # noqa: E731
    z = 0.25 + 8 * grid(rng, n).astype(np.float64)
    w.append(world_dirs(f, *screen(inx(n), iny(n), z)))                                                         # inside, any depth
    w.append(world_dirs(f, *screen(2.5 * (inx(n // 2) - (x0 + x1) / 2) + (x0 + x1) / 2, 2.5 * (iny(n // 2) - (y0 + y1) / 2) + (y0 + y1) / 2, z[:n // 2])))      # around the frame
    w.append(world_dirs(f, inx(160), iny(160), -(0.001 + 4 * grid(rng, 160).astype(np.float64))))            # behind the light
    w.append(world_dirs(f, 0.5 + inx(400), iny(400), 0.0))                                                     # in the light's plane
    for centre in (hither, F32(1.0)):                                                                           # the hither plane and wp == 1, ulp by ulp
        k = np.repeat(np.arange(-3, 4), 192)
        zc = step(np.full(len(k), centre, F32), k).astype(np.float64)
        w.append(world_dirs(f, *screen(np.tile(inx(192), 7), np.tile(iny(192), 7), zc)))
    k = np.arange(-8, 9)
    tx = [x0, x1] + ([x0 + (x1 - x0) * (i + 0.5) / shape[0] for i in range(shape[0])] + [x0 + (x1 - x0) * i / shape[0] for i in range(1, shape[0])] if shape else [])
    ty = [y0, y1] + ([y0 + (y1 - y0) * (j + 0.5) / shape[1] for j in range(shape[1])] + [y0 + (y1 - y0) * j / shape[1] for j in range(1, shape[1])] if shape else [])
    for axis, targets in ((0, tx), (1, ty)):                                                                    # each edge, texel centre and texel border: the light-space coordinate walks 17 ulps over it
        for i, t in enumerate(targets):
            for zz in zs:
                other = (iny if axis == 0 else inx)(48 if i < 2 else 12)
                for o in other:
                    px, py = (t, o) if axis == 0 else (o, t)
                    xl, yl, zl = screen(px, py, zz)
                    xl, yl = (step(np.full(17, xl, F32), k), np.full(17, yl)) if axis == 0 else (np.full(17, xl), step(np.full(17, yl, F32), k))
                    w.append(world_dirs(f, xl, yl, np.full(17, zl)))
    return np.concatenate(w)


def projection_categories(f, shape, cls, aux):
    x0, y0, x1, y1 = f[72:76]
    wlz, px, py = aux[:, 2], aux[:, 3], aux[:, 4]
    cat = np.where(cls == 5, 19, 20).astype(np.uint8)
    front = cls != 0
    if shape:
        sx = ((px - x0) / (x1 - x0) if x1 > x0 else px - x0).astype(F32)      # Bounds2f::offset in numpy's f32 (IEEE, as the text's): for LABELLING only
        sy = ((py - y0) / (y1 - y0) if y1 > y0 else py - y0).astype(F32)
        bx, by = (sx * F32(shape[0])).astype(F32), (sy * F32(shape[1])).astype(F32)
        cx, cy = (bx - F32(0.5)).astype(F32), (by - F32(0.5)).astype(F32)
        cat[(cls == 5) & ((bx == np.floor(bx)) | (by == np.floor(by)))] = 18
        cat[(cls == 5) & ((cx == np.floor(cx)) | (cy == np.floor(cy)))] = 17
    for near, exact, v, b in ((16, 12, py, y1), (15, 11, py, y0), (14, 10, px, x1), (13, 9, px, x0)):      # (where two labels apply the later one stays: x before y, p_min before p_max)
        cat[front & (np.abs(ulps(v, b)) <= 2)] = near
        cat[front & (v == b)] = exact
    for c, b in ((6, step(F32(1), -1)), (7, F32(1)), (8, step(F32(1), 1)), (3, step(f[70], -1)), (4, f[70]), (5, step(f[70], 1))):
        cat[wlz == b] = c
    cat[wlz == 0] = 2
    cat[wlz < 0] = 1
    return cat


def goniometric_candidates(rng, f, n):
    w = []
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    d = (np.round(d * 1024) / 1024) * (0.25 + 4 * grid(rng, (n, 1)).astype(np.float64))
    w.append(world_dirs(f, d[:, 0], d[:, 1], d[:, 2]))                                                          # anywhere, any length
    e = np.concatenate([[0.0], np.arange(1, 33) * 3.0e-5])
    ea, eb = (v.reshape(-1) for v in np.meshgrid(e, e))
    for s in (1.0, -1.0):
        for sa, sb in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            w.append(world_dirs(f, sa * ea[::5], s * np.ones(len(ea[::5])), sb * eb[::5]))                     # the poles (the light's +-y) and their neighbourhood: cos = 1 / sqrt(1 + e^2)
            w.append(world_dirs(f, s * np.ones(len(ea[::5])), sa * ea[::5], sb * eb[::5]))                     # +-x
            w.append(world_dirs(f, sa * ea[::5], sb * eb[::5], s * np.ones(len(ea[::5]))))                     # +-z
    # the seam: the light's z (wp.y after the swap) is -0, every sign of the other two; and phi just below 2 pi
    a = 0.25 + grid(rng, 96, 4).astype(np.float64)
    for sx in (1.0, -1.0):
        for yy in (a, -a, np.zeros(96), -np.zeros(96)):
            for zz in (np.zeros(96), -np.zeros(96)):
                w.append(world_dirs(f, sx * a[::-1], yy, zz))
    tiny = 1e-8 * np.arange(1, 97)
    for xx in (1.0, 2.0, 0.5):
        w.append(world_dirs(f, np.full(96, xx), np.tile([0.0, 0.5, -0.5], 32), -tiny * xx))
        w.append(world_dirs(f, np.full(96, xx), np.tile([0.0, 0.5, -0.5], 32), tiny * xx))
    return np.concatenate(w)


def goniometric_categories(cls, aux):
    wx, wy, wz, phi, theta, s, t = (aux[:, k] for k in range(7))
    one, two_pi = F32(1), (F32(2) * F32(np.pi)).astype(F32)
    cat = np.full(len(cls), 42, np.uint8)
    near = lambda v: (np.abs(ulps(np.abs(v), one)) <= 2) & (np.abs(v) != one)      # noqa: E731
    cat[near(wx) | near(wy)] = 37
    cat[np.abs(wy) == one] = 36
    cat[np.abs(wx) == one] = 35
    cat[near(wz)] = 34
    cat[(phi < two_pi) & (ulps(phi, two_pi) >= -1) | (phi == two_pi)] = 40
    cat[(s == one) | (t == one)] = 41
    cat[wz == -one] = 33      # (theta == pi there, and pi * INV_PI rounds to 1: the pole keeps its own label)
    cat[wz == one] = 32
    neg0 = wy.view(np.uint32) == 0x80000000
    cat[neg0 & (wx < 0)] = 39
    cat[neg0 & (wx > 0)] = 38
    return cat


def admits(kind, k, f, cat):
    """None where light (kind, map k, fields f) can reach category `cat`, else the reason it cannot (committed with the fixture as an exemption)"""
    if kind == PROJ:
        if cat in (17, 18) and k < 0:
            return "no map: st is not computed"
        if f[73] == f[75] and cat in (12, 16, 17, 18, 19):
            return "screen_bounds without extent in y: every inside point has p.y == p_min.y == p_max.y, which is category 11's (and 15's) label"
        if cat == 18 and k >= 0 and maps_shape_is_one(k):
            return "a 1 x 1 map: its only texel borders are the edges st == 0 and st == 1, which carry their own labels"
        return None
    m = f[6:22].reshape(4, 4)[:3, :3]
    if cat in (38, 39):
        # wl.z = m20 x + m21 y + m22 z is -0 only where every term is -0: (+0) + (-0) is +0.  Under a diagonal world_to_light that needs x and y negative (or -0), and wl.x = m00 x
        # then has the sign of -m00: positive only under a mirror of x
        diagonal = not (m - np.diag(np.diag(m))).any()
        if not diagonal:
            return "world_to_light mixes the axes: wl.z is a rounded sum of non-zero terms, not a signed zero"
        x_negative = (m[0, 0] < 0) == (cat == 38)      # the sign of w.x that puts wl.x on the side the category asks for
        if bool(np.signbit(m[2, 0])) == x_negative:
            return "wl.z is -0 only where every term of m[2][0] x + m[2][1] y + m[2][2] z is -0; the sign of this world_to_light's m[2][0] (a zero) then fixes the sign of x, and wl.x gets the other side"
    return None


def maps_shape_is_one(k):
    return MAP_SHAPES[k] == (1, 1)


def map_cases(L, rng, lights, maps, per_cat, n_interior, keep_all=False):
    """the map cases of every light: (rec, w, cat, out) and the exemptions (rec, cat); asserts per_cat cases of every category a light admits"""
    T = _helpers()
    rec, ws, cats, outs, exempt, short = [], [], [], [], [], []
    for r, (kind, k, f) in enumerate(lights):
        lt = light_struct(kind, k, f)
        shape = None if k < 0 else maps.pyramids[k][:2]
        cand = projection_candidates(rng, f, shape, n_interior) if kind == PROJ else goniometric_candidates(rng, f, n_interior)
        out, cls, aux = run_map(L, lt, maps, cand)
        cat = projection_categories(f, shape, cls, aux) if kind == PROJ else goniometric_categories(cls, aux)
        keep = []
        for c in [c for c in list(T.CATS) + [20] if (c < 32) == (kind == PROJ)]:
            idx = np.flatnonzero(cat == c)
            reason = admits(kind, k, f, c)
            if c != 20 and len(idx) < per_cat:
                if reason is None:
                    short.append("light %d reaches only %d cases of category %d (%s)" % (r, len(idx), c, T.CATS[c]))
                exempt.append((r, c))
            elif reason is not None and c != 20:
                short.append("light %d is exempt from category %d (%s) but reaches %d cases: %s" % (r, c, T.CATS[c], len(idx), reason))      # an exemption the text does not need is a wrong reason
            if not keep_all:
                idx = idx[rng.permutation(len(idx))[:2 * per_cat if c in (19, 42) else per_cat]]
            keep.append(idx)
        keep = np.sort(np.concatenate(keep))
        rec.append(np.full(len(keep), r, np.uint8)); ws.append(cand[keep]); cats.append(cat[keep]); outs.append(out[keep])
    assert not short, "\n".join(short)
    return np.concatenate(rec), np.concatenate(ws), np.concatenate(cats), np.concatenate(outs), np.array(exempt, np.int32).reshape(-1, 2)


def sample_li_cases(L, rng, lights, maps, n_generic):
    rec, ps, outs = [], [], []
    for r, (kind, k, f) in enumerate(lights):
        pl = f[0:3].astype(np.float64)
        d = rng.normal(size=(n_generic + 16, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
        dist = np.concatenate([0.5 + 16 * grid(rng, n_generic).astype(np.float64), np.full(8, 1e-20), np.full(8, 1e18)])
        p = np.concatenate([(pl + d * dist[:, None]).astype(F32), np.tile(f[0:3], (4, 1))])
        rec.append(np.full(len(p), r, np.uint8)); ps.append(p); outs.append(run_sample_li(L, light_struct(kind, k, f), maps, p))
    return np.concatenate(rec), np.concatenate(ps), np.concatenate(outs)


CTOR_RES = ((8, 2), (2, 8), (4, 4), (1, 1), (16, 4), (1, 2), (64, 16), (4, 32))      # power-of-two sides (the builder takes no others); both aspect arms and aspect exactly 1


def constructor_cases(L, rng):
    pin, pout = [], []
    for i in range(32):
        frm = (8 * grid(rng, 3, 3) - 4).astype(F32)
        to = (frm + (F32(0.25) + 2 * grid(rng, 3, 3)) * np.where(grid(rng, 3, 1) < 0.5, -1, 1)).astype(F32)
        up = np.array(((0, 1, 0), (0, 0, 1), (1, 0, 0), (0.25, 1, 0.5))[i % 4], F32)
        fov = (1.0, 20.0, 45.0, 90.0, 150.0, 179.0, 30.0, 60.0)[i % 8]
        rx, ry = CTOR_RES[(i // 4) % len(CTOR_RES)]
        pin.append(np.concatenate([frm, to, up, [fov, rx, ry]]).astype(F32)); pout.append(projection_new(L, frm, to, up, fov, rx, ry))
    gin, gout = [], []
    for i in range(16):
        m = rot(rng.normal(size=3), 360 * float(grid(rng, 1)[0])) @ mat(np.diag(0.5 + 2 * grid(rng, 3, 3).astype(np.float64)) if i % 2 else None, t=8 * grid(rng, 3, 3) - 4)
        if i % 5 == 4:
            m = m @ mat(np.diag([1.0, -1.0, 1.0]))
        gin.append(m.astype(F32).reshape(16)); gout.append(goniometric_new(L, m.astype(F32)))
    return np.array(pin, F32), np.array(pout, F32), np.array(gin, F32), np.array(gout, F32)


TABLE_LIGHTS = (      # per scene: projection (from, to, up, fov, map) and goniometric (light_to_world, map) lights inside the world bound of tests' table_scene
    ((((0.3, 3.1, 0.2), (0.5, 0, 1), (0, 0, 1), 50.0, 0), ((-2.1, 2.2, -2.3), (0, 0, 0), (0, 1, 0), 70.0, -1), ((2.2, 4.1, 2.3), (2, 0, 1.5), (1, 0, 0), 30.0, 1)),
     ((mat(t=(1.1, 1.6, 1.2)) @ rot((1, 2, 3), 40.0), 2), (mat(t=(-3.1, 0.6, 3.2)), -1), (mat(t=(3.2, 4.4, -3.1)) @ mat([[1, 0.5, 0], [0, 1, 0.25], [0, 0, 1]]), 4))),
    ((((0.1, 3.6, 3.1), (0, 0, 1.5), (0, 0, 1), 60.0, 4), ((-2.6, 0.4, -1.6), (0, 1, 2), (0, 1, 0), 100.0, -1), ((2.4, 2.1, 4.2), (-1, 0.5, 1), (0, 1, 0), 25.0, 6)),
     ((mat(t=(-1.9, 2.6, 3.3)) @ rot((0, 1, 1), 115.0), 0), (mat(t=(1.3, 0.7, -0.9)), -1), (mat(t=(2.3, 3.3, 1.1)) @ mat(np.diag([-1.0, 1.0, 1.0])), 5))),
)


def table_cases(L, rng, d, lights, maps):
    """the device tables: the scenes' map lights are appended to `lights`; per scene and strategy func, cdf, nvox, voxel at 256 points, and the classes of the spatial run"""
    from oracle import pyoracle
    from rs_pbrt_amd import abi
    T = _helpers()
    pyoracle.build()
    for k, (projs, gonios) in enumerate(TABLE_LIGHTS):
        rows = []
        for frm, to, up, fov, m in projs:
            rx, ry = (1, 1) if m < 0 else maps.pyramids[m][:2]
            f = projection_new(L, frm, to, up, fov, rx, ry)
            f[3:6] = F32(20) + F32(40) * grid(rng, 3, 4)
            rows.append(len(lights)); lights.append((PROJ, m, f))
        for m4, m in gonios:
            f = goniometric_new(L, m4.astype(F32))
            f[3:6] = F32(2) + F32(8) * grid(rng, 3, 4)
            rows.append(len(lights)); lights.append((GONIO, m, f))
        d["tab%d_rows" % k] = np.array(rows, np.int32)
    d["lights"], d["light_kind"], d["light_map"] = np.array([f for _, _, f in lights], F32), np.array([kd for kd, _, _ in lights], np.uint8), np.array([m for _, m, _ in lights], np.int32)
    stats = {}
    for k in range(len(TABLE_LIGHTS)):
        sc = T.table_scene(pyoracle.bvh_build, d, k)
        lo, hi = sc.nodes["bmin"][0].astype(np.float64), sc.nodes["bmax"][0].astype(np.float64)
        kinds = list(sc.lights["kind"])
        ls = np.zeros(len(kinds), T.lightref_dt())
        first = kinds.index(PROJ)
        for j, r in enumerate(d["tab%d_rows" % k]):
            kind, m, f = lights[int(r)]
            assert kinds[first + j] == kind and ((f[0:3] > lo) & (f[0:3] < hi)).all(), "a map light outside the world bound"
            assert np.array_equal(sc.lights[first + j]["p"][:22], T.record_words(kind, f))
            ls[first + j] = (kind, m, f)
        assert kinds.count(abi.LIGHT_DIFFUSE_AREA) == 1 and kinds.count(abi.LIGHT_POINT) == 1 and len(kinds) == 8
        pts = (lo - 0.5 + (hi - lo + 1.0) * grid(rng, (256, 3), 6)).astype(F32)
        d["tab%d_pts" % k] = pts
        for name, strategy in T.STRATEGIES:
            func, cdf, nvox, voxel, counts = run_tables(L, sc, ls, maps, strategy, pts)
            key = "tab%d_%s" % (k, name)
            d[key + "_func"], d[key + "_cdf"], d[key + "_nvox"], d[key + "_voxel"] = func, cdf, nvox, voxel
            assert np.isfinite(func).all() and np.isfinite(cdf).all() and (func > 0).all()
            if strategy == abi.LIGHTS_SPATIAL:
                d["tab%d_counts" % k] = counts
                n_vox = len(np.unique(voxel, axis=0))
                assert counts[15] == 0, "a voxel sample point equals a light position"
                assert all(counts[c] >= 64 for c in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11)), counts      # behind the hither plane, outside each of the four edges, inside, each phi quadrant
                assert counts[:12].sum() == 128 * n_vox * 6
                stats["tab%d" % k] = "%d voxels of %s, classes %s" % (n_vox, nvox.tolist(), counts[:12].tolist())
            else:
                assert (func == func[0]).all() and (voxel == 0).all() and list(nvox) == [1, 1, 1]
    return stats


def reference(L, n_fresh=0, seed=SEED, tables=True, stats=None):
    """inputs and the text's outputs as the fixture's arrays; the generator's own conditions on them are asserted here.  n_fresh: at least that many fresh map cases per
    light kind and sample_li cases, every candidate kept (the fresh-case test)"""
    from rs_pbrt_amd import abi
    assert (PROJ, GONIO) == (abi.LIGHT_PROJECTION, abi.LIGHT_GONIOMETRIC)
    T = _helpers()
    rng = np.random.default_rng(seed)
    d = {}
    maps = make_maps(rng)
    d["map_shapes"] = np.array([(w, h, n) for w, h, n, _ in maps.pyramids], np.int32)
    d["map_texels"] = np.concatenate([t for _, _, _, t in maps.pyramids]).astype(F32)
    d["map_offsets"] = np.concatenate([[0], np.cumsum([len(t) for _, _, _, t in maps.pyramids])]).astype(np.int32)
    lights = make_lights(L, rng, maps)
    n_proj = sum(kd == PROJ for kd, _, _ in lights)
    assert n_proj >= 9 and len(lights) - n_proj >= 6
    if n_fresh:
        d["map_rec"], d["map_w"], d["map_cat"], d["map_out"], ex = map_cases(L, rng, lights, maps, T.MIN_PER_CAT, -(-n_fresh // min(n_proj, len(lights) - n_proj)), keep_all=True)
        d["sli_rec"], d["sli_p"], d["sli_out"] = sample_li_cases(L, rng, lights, maps, -(-n_fresh // min(n_proj, len(lights) - n_proj)))
    else:
        d["map_rec"], d["map_w"], d["map_cat"], d["map_out"], ex = map_cases(L, rng, lights, maps, T.MIN_PER_CAT, 512)
        d["sli_rec"], d["sli_p"], d["sli_out"] = sample_li_cases(L, rng, lights, maps, 48)
        d["ctor_proj_in"], d["ctor_proj_out"], d["ctor_gonio_in"], d["ctor_gonio_out"] = constructor_cases(L, rng)
    d["map_exempt"] = ex
    for c in T.CATS:
        assert (d["map_cat"] == c).sum() >= T.MIN_PER_CAT, T.CATS[c]
    if tables:
        st = table_cases(L, rng, d, lights, maps)
        if stats is not None:
            stats.update(st)
    else:
        d["lights"], d["light_kind"], d["light_map"] = np.array([f for _, _, f in lights], F32), np.array([kd for kd, _, _ in lights], np.uint8), np.array([m for _, m, _ in lights], np.int32)
    pw = np.array([run_power(L, light_struct(kd, m, f), maps) for kd, m, f in lights], F32)
    d["power_out"], d["power_y"] = pw[:, :3].copy(), pw[:, 3].copy()
    if stats is not None:
        for c in sorted(T.CATS):
            stats["category %d (%s)" % (c, T.CATS[c])] = "%d cases over %d lights" % (int((d["map_cat"] == c).sum()), len(np.unique(d["map_rec"][d["map_cat"] == c])))
        stats["exemptions"] = ", ".join("light %d: %s" % (r, T.CATS[c]) for r, c in ex)
    return d


def main():
    L, where = convert()
    for w in where[-len(SOURCES) - 3:]:
        print("compiled from", w)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-only":
        return 0
    stats = {}
    d = reference(L, stats=stats)
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
