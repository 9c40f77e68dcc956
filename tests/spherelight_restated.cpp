// Test helper (compiled by tests/test_spherelight_host.py and tests/test_gpu_sphere_lights.py with g++ into a temporary directory): a hand restatement,
// written from the reference's text, of Sphere::area / sample / sample_with_ref_point / pdf_with_ref_point (src/shapes/sphere.rs:361-504) and of
// DiffuseAreaLight::sample_li / pdf_li / power over that shape (src/lights/diffuse.rs:64-103), over the helpers of tests/sphere_restated.cpp, and over them of
// the three light distributions the path needs (src/core/lightdistrib.rs:127-418) for a scene with sphere lights: the oracle knows no such light, so its own
// tables cannot serve.  sample_li / power below take a DiffuseAreaLight on a sphere primitive themselves and hand every other light to the oracle's.
// f32 throughout with the host libm; build with -ffp-contract=off.
#ifndef RSPT_SPHERELIGHT_NO_BASE   // tests/spherelight_render_restated.cpp has included the helpers already
#include "sphere_restated.cpp"
#endif
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace {

const float SL_PI = 3.14159265358979323846f;
V vsub(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
V vneg(V a) { return V{-a.x, -a.y, -a.z}; }
float vdist2(V a, V b) { const V d = vsub(a, b); return vdot(d, d); }
// geometry.rs:1535-1556 pnt3_offset_ray_origin
V sl_offset_ray_origin(V p, V p_error, V n, V w) {
    const float d = vdot(vabs(n), p_error);
    V offset = mul(n, d);
    if (vdot(w, n) < 0.0f) offset = vneg(offset);
    V po = add(p, offset);
    if (offset.x > 0.0f) po.x = next_float_up(po.x); else if (offset.x < 0.0f) po.x = next_float_down(po.x);
    if (offset.y > 0.0f) po.y = next_float_up(po.y); else if (offset.y < 0.0f) po.y = next_float_down(po.y);
    if (offset.z > 0.0f) po.z = next_float_up(po.z); else if (offset.z < 0.0f) po.z = next_float_down(po.z);
    return po;
}
// transform.rs:490-517 transform_point
V sl_point(const float* m, V p) {
    const float xp = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
    const float yp = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
    const float zp = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
    const float wp = m[12] * p.x + m[13] * p.y + m[14] * p.z + m[15];
    if (wp == 1.0f) return V{xp, yp, zp};
    const float inv = 1.0f / wp;
    return V{inv * xp, inv * yp, inv * zp};
}
// transform.rs:709-769 transform_point_with_abs_error
V sl_point_abs_error(const float* m, V p, V pe, V* abs_error) {
    const float g3 = gamma(3);
    const float xp = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
    const float yp = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
    const float zp = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
    const float wp = m[12] * p.x + m[13] * p.y + m[14] * p.z + m[15];
    float ae[3];
    for (int r = 0; r < 3; r++) {
        const float* row = m + 4 * r;
        ae[r] = (g3 + 1.0f) * (std::fabs(row[0]) * pe.x + std::fabs(row[1]) * pe.y + std::fabs(row[2]) * pe.z) +
                g3 * (std::fabs(row[0] * p.x) + std::fabs(row[1] * p.y) + std::fabs(row[2] * p.z) + std::fabs(row[3]));
    }
    *abs_error = V{ae[0], ae[1], ae[2]};
    if (wp == 1.0f) return V{xp, yp, zp};
    const float inv = 1.0f / wp;
    return V{inv * xp, inv * yp, inv * zp};
}
// geometry.rs:779-794 vec3_coordinate_system (Vector3 / Float multiplies by the reciprocal, :1261-1297)
void sl_coordinate_system(V v1, V* v2, V* v3) {
    if (std::fabs(v1.x) > std::fabs(v1.y)) *v2 = mul(V{-v1.z, 0.0f, v1.x}, 1.0f / std::sqrt(v1.x * v1.x + v1.z * v1.z));
    else *v2 = mul(V{0.0f, v1.z, -v1.y}, 1.0f / std::sqrt(v1.y * v1.y + v1.z * v1.z));
    *v3 = vcross(v1, *v2);
}

struct SlIntr {   // InteractionCommon: p, p_error, n
    V p, p_error, n;
};

float sl_area(const rspt_sphere& s) { return s.phi_max * s.radius * (s.z_max - s.z_min); }   // sphere.rs:361-363

// sphere.rs:364-390
SlIntr sl_sample(const rspt_sphere& s, float u0, float u1, float* pdf) {
    // uniform_sample_sphere (sampling.rs:327-336)
    const float z = 1.0f - 2.0f * u0;
    const float r = std::sqrt(fmax_(0.0f, 1.0f - z * z));
    const float phi = 2.0f * SL_PI * u1;
    const V dir{r * std::cos(phi), r * std::sin(phi), z};
    V p_obj = add(V{0.0f, 0.0f, 0.0f}, mul(dir, s.radius));   // :365
    SlIntr it;
    it.n = vnormalize(xnrm(s.world_to_object, p_obj));         // :367-374
    if (s.reverse_orientation) it.n = mul(it.n, -1.0f);        // :377-379
    const V dd = vsub(p_obj, V{0.0f, 0.0f, 0.0f});
    p_obj = mul(p_obj, s.radius / std::sqrt(vdot(dd, dd)));    // :381
    const V p_obj_error = mul(vabs(p_obj), gamma(5));          // :382
    it.p = sl_point_abs_error(s.object_to_world, p_obj, p_obj_error, &it.p_error);   // :383-387
    *pdf = 1.0f / sl_area(s);                                  // :388
    return it;
}
// the test both ref-point functions open with (sphere.rs:397-401, :469-477)
bool sl_ref_inside(const rspt_sphere& s, const SlIntr& ref, V* p_center) {
    *p_center = sl_point(s.object_to_world, V{0.0f, 0.0f, 0.0f});
    const V p_origin = sl_offset_ray_origin(ref.p, ref.p_error, ref.n, vsub(*p_center, ref.p));
    return vdist2(p_origin, *p_center) <= s.radius * s.radius;
}
// sphere.rs:391-467
SlIntr sl_sample_ref(const rspt_sphere& s, const SlIntr& ref, float u0, float u1, float* pdf) {
    V p_center;
    if (sl_ref_inside(s, ref, &p_center)) {   // :401-416
        const SlIntr intr = sl_sample(s, u0, u1, pdf);
        V wi = vsub(intr.p, ref.p);
        if (vdot(wi, wi) == 0.0f) *pdf = 0.0f;
        else {
            wi = vnormalize(wi);
            *pdf *= vdist2(ref.p, intr.p) / std::fabs(vdot(intr.n, vneg(wi)));
        }
        if (std::isinf(*pdf)) *pdf = 0.0f;
        return intr;
    }
    const V wc = vnormalize(vsub(p_center, ref.p));   // :419-422
    V wc_x, wc_y;
    sl_coordinate_system(wc, &wc_x, &wc_y);
    const float sin_theta_max2 = s.radius * s.radius / vdist2(ref.p, p_center);   // :426-433
    const float cos_theta_max = std::sqrt(fmax_(0.0f, 1.0f - sin_theta_max2));
    const float cos_theta = (1.0f - u0) + u0 * cos_theta_max;
    const float sin_theta = std::sqrt(fmax_(0.0f, 1.0f - cos_theta * cos_theta));
    const float phi = u1 * 2.0f * SL_PI;
    const V dcv = vsub(ref.p, p_center);              // :435-444
    const float dc = std::sqrt(vdot(dcv, dcv));
    const float ds = dc * cos_theta - std::sqrt(fmax_(0.0f, s.radius * s.radius - dc * dc * sin_theta * sin_theta));
    const float cos_alpha = (dc * dc + s.radius * s.radius - ds * ds) / (2.0f * dc * s.radius);
    const float sin_alpha = std::sqrt(fmax_(0.0f, 1.0f - cos_alpha * cos_alpha));
    // spherical_direction_vec3 (geometry.rs:1570-1579) over -wc_x, -wc_y, -wc
    const V n_world = add(add(mul(vneg(wc_x), sin_alpha * std::cos(phi)), mul(vneg(wc_y), sin_alpha * std::sin(phi))), mul(vneg(wc), cos_alpha));   // :446-447
    SlIntr it;
    it.p = add(p_center, mul(n_world, s.radius));     // :448-453
    it.p_error = mul(vabs(it.p), gamma(5));           // :457
    it.n = n_world;
    if (s.reverse_orientation) it.n = mul(it.n, -1.0f);   // :461-463
    *pdf = 1.0f / (2.0f * SL_PI * (1.0f - cos_theta_max));   // :465
    return it;
}
// sphere.rs:468-504
float sl_pdf_ref(const rspt_sphere& s, const SlIntr& ref, V wi) {
    V p_center;
    if (sl_ref_inside(s, ref, &p_center)) {
        Hit h;   // iref.spawn_ray(wi) (interaction.rs:58-80): origin pushed off the error box, t_max = infinity
        if (!sphere_intersect(s, sl_offset_ray_origin(ref.p, ref.p_error, ref.n, wi), wi, INFINITY, true, &h)) return 0.0f;
        float pdf = vdist2(ref.p, h.p) / (std::fabs(vdot(h.n, vneg(wi))) * sl_area(s));
        if (std::isinf(pdf)) pdf = 0.0f;
        return pdf;
    }
    const float sin_theta_max2 = s.radius * s.radius / vdist2(ref.p, p_center);
    const float cos_theta_max = std::sqrt(fmax_(0.0f, 1.0f - sin_theta_max2));
    return 1.0f / (2.0f * SL_PI * (1.0f - cos_theta_max));   // uniform_cone_pdf (sampling.rs:369-371)
}
// DiffuseAreaLight::sample_li (diffuse.rs:64-84) for L = l_emit: l() with the SAMPLED normal (:164-170); out: radiance scale (1 / 0), wi, pdf
bool sl_light_sample(const rspt_sphere& s, bool two_sided, const SlIntr& ref, float u0, float u1, V* wi, float* pdf, SlIntr* light_intr) {
    *light_intr = sl_sample_ref(s, ref, u0, u1, pdf);
    const V d = vsub(light_intr->p, ref.p);
    if (*pdf == 0.0f || vdot(d, d) == 0.0f) { *pdf = 0.0f; return false; }
    *wi = vnormalize(d);
    return two_sided || vdot(light_intr->n, vneg(*wi)) > 0.0f;
}

}  // namespace

extern "C" {
// the layout of rspt_sphere_light (include/rspt.h): 64 floats in, 64 out per element
void sl_hook(const float* x, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; i++) {
        rspt_sphere s;
        std::memcpy(&s, x + 64 * i, sizeof s);
        const float* q = x + 64 * i + 42;
        const bool two_sided = ubits(q[0]) != 0u;
        const SlIntr ref{V{q[1], q[2], q[3]}, V{q[4], q[5], q[6]}, V{q[7], q[8], q[9]}};
        float* r = out + 64 * i;
        for (int k = 0; k < 64; k++) r[k] = 0.0f;
        r[0] = sl_area(s);
        float pdf = 0.0f;
        SlIntr a = sl_sample(s, q[10], q[11], &pdf);
        r[1] = a.p.x; r[2] = a.p.y; r[3] = a.p.z; r[4] = a.p_error.x; r[5] = a.p_error.y; r[6] = a.p_error.z; r[7] = a.n.x; r[8] = a.n.y; r[9] = a.n.z; r[10] = pdf;
        pdf = 0.0f;
        a = sl_sample_ref(s, ref, q[10], q[11], &pdf);
        r[11] = a.p.x; r[12] = a.p.y; r[13] = a.p.z; r[14] = a.p_error.x; r[15] = a.p_error.y; r[16] = a.p_error.z; r[17] = a.n.x; r[18] = a.n.y; r[19] = a.n.z; r[20] = pdf;
        pdf = 0.0f;
        V wi{0.0f, 0.0f, 0.0f};
        const float li = sl_light_sample(s, two_sided, ref, q[10], q[11], &wi, &pdf, &a) ? 1.0f : 0.0f;
        r[21] = li; r[22] = li; r[23] = li; r[24] = wi.x; r[25] = wi.y; r[26] = wi.z; r[27] = pdf;
        r[28] = sl_pdf_ref(s, ref, V{q[12], q[13], q[14]});
    }
}
}

namespace orc {
namespace sl {

static inline ::V tov(V3 a) { return ::V{a.x, a.y, a.z}; }
static inline V3 tov3(::V a) { return V3{a.x, a.y, a.z}; }
static inline ::SlIntr ref_of(const Interaction& it) { return ::SlIntr{tov(it.p), tov(it.p_error), tov(it.n)}; }
// the sphere a light sits on, or null: a DiffuseAreaLight whose primitive is a Sphere
static inline const rspt_sphere* light_sphere(const rspt_scene_desc& d, const rspt_light& lt) {
    if (lt.kind != RSPT_LIGHT_DIFFUSE_AREA || d.prims[lt.prim].mesh != RSPT_MESH_SPHERE) return nullptr;
    return &d.spheres[d.prims[lt.prim].v[0]];
}
// Light::sample_li dispatching on the light's primitive
static inline Spec sample_li(const Scene& sc, const rspt_light& lt, const Interaction& iref, P2 u, V3* wi, Float* pdf, Interaction* light_intr) {
    const rspt_sphere* s = light_sphere(sc.d, lt);
    if (!s) return light_sample_li(sc, lt, iref, u, wi, pdf, light_intr);
    ::SlIntr li;
    ::V w{0.0f, 0.0f, 0.0f};
    const bool lit = ::sl_light_sample(*s, lt.two_sided != 0, ref_of(iref), u.x, u.y, &w, pdf, &li);
    Interaction r;   // InteractionCommon { p, p_error, n, ..Default::default() }
    r.p = tov3(li.p); r.p_error = tov3(li.p_error); r.n = tov3(li.n); r.wo = V3{0, 0, 0}; r.time = 0;
    *light_intr = r;
    if (*pdf == 0.0f) return Spec();   // (diffuse.rs:76-79: wi is left as it was)
    *wi = tov3(w);
    return lit ? S3(lt.L) : Spec(0.0f);
}
// Light::pdf_li of an area light (diffuse.rs:100-103)
static inline Float pdf_li(const Scene& sc, const rspt_light& lt, const Interaction& iref, V3 wi) {
    const rspt_sphere* s = light_sphere(sc.d, lt);
    if (!s) return sc.tri_pdf_ref(sc.d.prims[lt.prim], iref, wi);
    return ::sl_pdf_ref(*s, ref_of(iref), tov(wi));
}
// Light::power (diffuse.rs:85-93 with area = shape.area())
static inline Spec power(const Scene& sc, const rspt_light& lt) {
    const rspt_sphere* s = light_sphere(sc.d, lt);
    if (!s) return light_power(sc, lt);
    const Float factor = lt.two_sided ? 2.0f : 1.0f;
    return S3(lt.L) * factor * ::sl_area(*s) * PI;
}

// One render's (or one query's) light distributions: create_light_sample_distribution (lightdistrib.rs:393-418) over sample_li / power above
struct Dist {
    const Scene* scene;
    int strategy = RSPT_LIGHTS_SPATIAL;
    std::unique_ptr<Distribution1D> fixed;
    int n_voxels[3] = {1, 1, 1};
    std::mutex mu;
    std::map<size_t, std::unique_ptr<Distribution1D>> voxels;   // the reference's hash table is a cache and changes no value (lightdistrib.rs:297-384)

    Dist(const Scene* sc, uint32_t light_strategy) : scene(sc) {
        const uint32_t nl = sc->d.n_lights;
        strategy = (int)light_strategy;
        if (strategy == RSPT_LIGHTS_UNIFORM || nl == 1) {   // :397
            strategy = RSPT_LIGHTS_UNIFORM;
            fixed.reset(new Distribution1D(std::vector<Float>(nl, 1.0f)));
        } else if (strategy == RSPT_LIGHTS_POWER) {
            std::vector<Float> pw;
            for (uint32_t i = 0; i < nl; i++) pw.push_back(power(*sc, sc->d.lights[i]).y());   // integrator.rs:573-584
            fixed.reset(new Distribution1D(pw));
        } else {   // SpatialLightDistribution::new (:127-166)
            strategy = RSPT_LIGHTS_SPATIAL;
            const Bounds3 b = sc->world_bound();
            const V3 diag = b.diagonal();
            const Float bmax = diag[b.maximum_extent()];
            for (int i = 0; i < 3; i++) n_voxels[i] = std::max(1, f2i(std::round(diag[i] / bmax * 64.0f)));   // :140-150
        }
    }
    // SpatialLightDistribution::compute_distribution (lightdistrib.rs:169-269)
    Distribution1D* compute_distribution(const int pi[3]) const {
        const Bounds3 wb = scene->world_bound();
        const V3 p0{(Float)pi[0] / (Float)n_voxels[0], (Float)pi[1] / (Float)n_voxels[1], (Float)pi[2] / (Float)n_voxels[2]};   // :171-185
        const V3 p1{(Float)(pi[0] + 1) / (Float)n_voxels[0], (Float)(pi[1] + 1) / (Float)n_voxels[1], (Float)(pi[2] + 1) / (Float)n_voxels[2]};
        Bounds3 vb; vb.p_min = wb.lerp3(p0); vb.p_max = wb.lerp3(p1);
        const size_t n_samples = 128;   // :196
        const uint32_t nl = scene->d.n_lights;
        std::vector<Float> contrib(nl, 0.0f);
        for (size_t i = 0; i < n_samples; i++) {   // :198-247
            const V3 po = vb.lerp3(V3{radical_inverse(0, i), radical_inverse(1, i), radical_inverse(2, i)});
            Interaction intr; intr.p = po; intr.time = 0; intr.p_error = V3{0, 0, 0}; intr.wo = V3{1, 0, 0}; intr.n = V3{0, 0, 0};   // :202-213
            const P2 u{radical_inverse(3, i), radical_inverse(4, i)};
            for (uint32_t j = 0; j < nl; j++) {
                Float pdf = 0; V3 wi{0, 0, 0}; Interaction li_intr;
                const Spec li = sample_li(*scene, scene->d.lights[j], intr, u, &wi, &pdf, &li_intr);
                if (pdf > 0.0f) contrib[j] += li.y() / pdf;
            }
        }
        Float sum = 0.0f; for (Float c : contrib) sum += c;   // :253-268
        const Float avg = sum / (Float)(n_samples * contrib.size());
        const Float min_contrib = avg > 0.0f ? 0.001f * avg : 1.0f;
        for (Float& c : contrib) c = std::fmax(c, min_contrib);
        return new Distribution1D(contrib);
    }
    // SpatialLightDistribution::lookup (lightdistrib.rs:276-295) for the voxel, then the table built directly
    const Distribution1D* lookup(V3 p, int voxel_out[3] = nullptr) {
        if (strategy != RSPT_LIGHTS_SPATIAL) return fixed.get();
        const V3 off = scene->world_bound().offset(p);
        int pi[3];
        for (int i = 0; i < 3; i++) pi[i] = clamp_t(f2i(off[i] * (Float)n_voxels[i]), 0, n_voxels[i] - 1);
        if (voxel_out) for (int i = 0; i < 3; i++) voxel_out[i] = pi[i];
        const size_t key = ((size_t)pi[2] * n_voxels[1] + pi[1]) * n_voxels[0] + pi[0];
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = voxels.find(key);
            if (it != voxels.end()) return it->second.get();
        }
        std::unique_ptr<Distribution1D> dist(compute_distribution(pi));   // (a pure function of the voxel: which thread builds it cannot show)
        std::lock_guard<std::mutex> g(mu);
        auto it = voxels.emplace(key, std::move(dist)).first;
        return it->second.get();
    }
};

}  // namespace sl
}  // namespace orc

extern "C" {
// The light distribution of (scene, strategy) at p, as rspt_light_distribution reports it: func[n_lights], cdf[n_lights + 1], the grid and p's voxel
int sl_light_distribution(const rspt_scene_desc* sd, uint32_t strategy, const float p[3], float* func_out, float* cdf_out, int32_t nvox_out[3], int32_t voxel_out[3]) {
    if (!sd || !sd->n_lights) return -1;
    orc::Scene sc{*sd};
    orc::sl::Dist v(&sc, strategy);
    int vox[3] = {0, 0, 0};
    const orc::Distribution1D* d = v.lookup(orc::V3{p[0], p[1], p[2]}, vox);
    std::memcpy(func_out, d->func.data(), d->func.size() * sizeof(float));
    std::memcpy(cdf_out, d->cdf.data(), d->cdf.size() * sizeof(float));
    for (int i = 0; i < 3; i++) { nvox_out[i] = v.n_voxels[i]; voxel_out[i] = vox[i]; }
    return 0;
}
}
