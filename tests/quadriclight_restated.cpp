// Test helper (compiled by tests/test_quadriclight_host.py and tests/test_gpu_quadric_lights.py with g++ into a temporary directory): a hand restatement,
// written from the reference's text, of Disk::area / sample / sample_with_ref_point / pdf_with_ref_point (src/shapes/disk.rs:207-280), of the same four of
// Cylinder (src/shapes/cylinder.rs:331-415) and of DiffuseAreaLight::sample_li / pdf_li / power over those shapes (src/lights/diffuse.rs:64-103), over the
// helpers of tests/sphere_restated.cpp, tests/quadric_restated.cpp (the two intersect functions) and tests/spherelight_restated.cpp (the transforms with
// their error terms, the sphere's own light functions), and over them of the three light distributions the path needs (src/core/lightdistrib.rs:127-418)
// for a scene whose disks, cylinders and spheres may emit.  The reference is restated as written, not repaired: Disk::sample knows neither inner_radius
// nor phi_max, both areas are object-space figures, the cylinder's normal comes from the point before the reprojection.
// f32 throughout with the host libm; build with -ffp-contract=off.
#ifndef RSPT_QUADRICLIGHT_NO_BASE   // tests/quadriclight_render_restated.cpp has included the helpers already
#include "quadric_restated.cpp"
#define RSPT_SPHERELIGHT_NO_BASE
#include "spherelight_restated.cpp"
#endif

namespace {

const float QL_PI_OVER_4 = 0.78539816339744830961f, QL_PI_OVER_2 = 1.57079632679489661923f;

float ql_disk_area(const rspt_disk& s) { return s.phi_max * 0.5f * (s.radius * s.radius - s.inner_radius * s.inner_radius); }   // disk.rs:207-211
float ql_cylinder_area(const rspt_cylinder& s) { return (s.z_max - s.z_min) * s.radius * s.phi_max; }                           // cylinder.rs:331-333

// sampling.rs:344-365 concentric_sample_disk
void ql_concentric_sample_disk(float u0, float u1, float* x, float* y) {
    const float ox = u0 * 2.0f - 1.0f, oy = u1 * 2.0f - 1.0f;
    if (ox == 0.0f && oy == 0.0f) { *x = 0.0f; *y = 0.0f; return; }
    float theta, r;
    if (std::fabs(ox) > std::fabs(oy)) {
        r = ox;
        theta = QL_PI_OVER_4 * (oy / ox);
    } else {
        r = oy;
        theta = QL_PI_OVER_2 - QL_PI_OVER_4 * (ox / oy);
    }
    *x = std::cos(theta) * r; *y = std::sin(theta) * r;
}
// disk.rs:212-239
SlIntr ql_disk_sample(const rspt_disk& s, float u0, float u1, float* pdf) {
    float pdx, pdy;
    ql_concentric_sample_disk(u0, u1, &pdx, &pdy);                              // :213
    const V p_obj{pdx * s.radius, pdy * s.radius, s.height};                    // :214-218
    SlIntr it;
    it.n = vnormalize(xnrm(s.world_to_object, V{0.0f, 0.0f, 1.0f}));            // :219-229
    if (s.reverse_orientation) it.n = mul(it.n, -1.0f);                         // :230-232
    it.p = sl_point_abs_error(s.object_to_world, p_obj, V{0.0f, 0.0f, 0.0f}, &it.p_error);   // :233-236
    *pdf = 1.0f / ql_disk_area(s);                                              // :237
    return it;
}
// cylinder.rs:334-374
SlIntr ql_cylinder_sample(const rspt_cylinder& s, float u0, float u1, float* pdf) {
    const float z = s.z_min * (1.0f - u0) + s.z_max * u0;                       // :335, lerp (pbrt.rs:235-245)
    const float phi = u1 * s.phi_max;                                           // :336
    V p_obj{s.radius * std::cos(phi), s.radius * std::sin(phi), z};             // :337-341
    SlIntr it;
    it.n = vnormalize(xnrm(s.world_to_object, V{p_obj.x, p_obj.y, 0.0f}));      // :342-352
    if (s.reverse_orientation) it.n = mul(it.n, -1.0f);                         // :353-355
    const float hit_rad = std::sqrt(p_obj.x * p_obj.x + p_obj.y * p_obj.y);     // :357-359
    p_obj.x *= s.radius / hit_rad;
    p_obj.y *= s.radius / hit_rad;
    const V p_obj_error = mul(vabs(V{p_obj.x, p_obj.y, 0.0f}), gamma(3));       // :360-366
    it.p = sl_point_abs_error(s.object_to_world, p_obj, p_obj_error, &it.p_error);   // :367-371
    *pdf = 1.0f / ql_cylinder_area(s);                                          // :372
    return it;
}
// the tail of both sample_with_ref_point (disk.rs:246-259, cylinder.rs:381-394)
void ql_to_solid_angle(const SlIntr& intr, const SlIntr& ref, float* pdf) {
    V wi = vsub(intr.p, ref.p);
    if (vdot(wi, wi) == 0.0f) *pdf = 0.0f;
    else {
        wi = vnormalize(wi);
        *pdf *= vdist2(ref.p, intr.p) / std::fabs(vdot(intr.n, vneg(wi)));
        if (std::isinf(*pdf)) *pdf = 0.0f;
    }
}
// the tail of both pdf_with_ref_point (disk.rs:269-279, cylinder.rs:404-414) on a hit of iref.spawn_ray(wi)
float ql_hit_pdf(const SlIntr& ref, V wi, const Hit& h, float area) {
    float pdf = vdist2(ref.p, h.p) / (std::fabs(vdot(h.n, vneg(wi))) * area);
    if (std::isinf(pdf)) pdf = 0.0f;
    return pdf;
}

// a shape of any of the three kinds: mesh = RSPT_MESH_SPHERE | _DISK | _CYLINDER
struct QlShape {
    uint32_t mesh;
    const void* rec;
    const rspt_sphere& sphere() const { return *static_cast<const rspt_sphere*>(rec); }
    const rspt_disk& disk() const { return *static_cast<const rspt_disk*>(rec); }
    const rspt_cylinder& cylinder() const { return *static_cast<const rspt_cylinder*>(rec); }
};
float ql_area(const QlShape& q) {
    if (q.mesh == RSPT_MESH_DISK) return ql_disk_area(q.disk());
    if (q.mesh == RSPT_MESH_CYLINDER) return ql_cylinder_area(q.cylinder());
    return sl_area(q.sphere());
}
SlIntr ql_sample(const QlShape& q, float u0, float u1, float* pdf) {
    if (q.mesh == RSPT_MESH_DISK) return ql_disk_sample(q.disk(), u0, u1, pdf);
    if (q.mesh == RSPT_MESH_CYLINDER) return ql_cylinder_sample(q.cylinder(), u0, u1, pdf);
    return sl_sample(q.sphere(), u0, u1, pdf);
}
// disk.rs:240-260, cylinder.rs:375-395; a sphere: sphere.rs:391-467
SlIntr ql_sample_ref(const QlShape& q, const SlIntr& ref, float u0, float u1, float* pdf) {
    if (q.mesh == RSPT_MESH_SPHERE) return sl_sample_ref(q.sphere(), ref, u0, u1, pdf);
    const SlIntr intr = ql_sample(q, u0, u1, pdf);
    ql_to_solid_angle(intr, ref, pdf);
    return intr;
}
// disk.rs:261-280, cylinder.rs:396-415: the shape's own intersect on iref.spawn_ray(wi) (interaction.rs:58-80), t_max = infinity
float ql_pdf_ref(const QlShape& q, const SlIntr& ref, V wi) {
    if (q.mesh == RSPT_MESH_SPHERE) return sl_pdf_ref(q.sphere(), ref, wi);
    const V o = sl_offset_ray_origin(ref.p, ref.p_error, ref.n, wi);
    Hit h;
    if (q.mesh == RSPT_MESH_DISK) {
        if (!disk_intersect(q.disk(), o, wi, INFINITY, true, &h)) return 0.0f;
    } else if (!cylinder_intersect(q.cylinder(), o, wi, INFINITY, true, &h))
        return 0.0f;
    return ql_hit_pdf(ref, wi, h, ql_area(q));
}
// DiffuseAreaLight::sample_li (diffuse.rs:64-84) for L = l_emit: l() with the SAMPLED normal (:164-170); out: radiance scale (1 / 0), wi, pdf
bool ql_light_sample(const QlShape& q, bool two_sided, const SlIntr& ref, float u0, float u1, V* wi, float* pdf, SlIntr* light_intr) {
    *light_intr = ql_sample_ref(q, ref, u0, u1, pdf);
    const V d = vsub(light_intr->p, ref.p);
    if (*pdf == 0.0f || vdot(d, d) == 0.0f) { *pdf = 0.0f; return false; }
    *wi = vnormalize(d);
    return two_sided || vdot(light_intr->n, vneg(*wi)) > 0.0f;
}
// DiffuseAreaLight::power (diffuse.rs:85-93) of L = 1 with area = shape.area()
float ql_power(const QlShape& q, bool two_sided) { return 1.0f * (two_sided ? 2.0f : 1.0f) * ql_area(q) * SL_PI; }

}  // namespace

extern "C" {
// the layout of rspt_quadric_light (include/rspt.h): 64 floats in, 64 out per element
void ql_hook(const float* x, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; i++) {
        rspt_disk dk;
        rspt_cylinder cy;
        std::memcpy(&dk, x + 64 * i, sizeof dk);
        std::memcpy(&cy, x + 64 * i, sizeof cy);
        const uint32_t kind = ubits(x[64 * i + 40]);
        const float* q = x + 64 * i + 42;
        const bool two_sided = ubits(q[0]) != 0u;
        const SlIntr ref{V{q[1], q[2], q[3]}, V{q[4], q[5], q[6]}, V{q[7], q[8], q[9]}};
        float* r = out + 64 * i;
        for (int k = 0; k < 64; k++) r[k] = 0.0f;
        if (kind != RSPT_MESH_DISK && kind != RSPT_MESH_CYLINDER) continue;
        const QlShape sh{kind, kind == RSPT_MESH_DISK ? (const void*)&dk : (const void*)&cy};
        r[0] = ql_area(sh);
        float pdf = 0.0f;
        SlIntr a = ql_sample(sh, q[10], q[11], &pdf);
        r[1] = a.p.x; r[2] = a.p.y; r[3] = a.p.z; r[4] = a.p_error.x; r[5] = a.p_error.y; r[6] = a.p_error.z; r[7] = a.n.x; r[8] = a.n.y; r[9] = a.n.z; r[10] = pdf;
        pdf = 0.0f;
        a = ql_sample_ref(sh, ref, q[10], q[11], &pdf);
        r[11] = a.p.x; r[12] = a.p.y; r[13] = a.p.z; r[14] = a.p_error.x; r[15] = a.p_error.y; r[16] = a.p_error.z; r[17] = a.n.x; r[18] = a.n.y; r[19] = a.n.z; r[20] = pdf;
        pdf = 0.0f;
        V wi{0.0f, 0.0f, 0.0f};
        const float li = ql_light_sample(sh, two_sided, ref, q[10], q[11], &wi, &pdf, &a) ? 1.0f : 0.0f;
        r[21] = li; r[22] = li; r[23] = li; r[24] = wi.x; r[25] = wi.y; r[26] = wi.z; r[27] = pdf;
        r[28] = ql_pdf_ref(sh, ref, V{q[12], q[13], q[14]});
        const float pw = ql_power(sh, two_sided);
        r[29] = pw; r[30] = pw; r[31] = pw;
    }
}
}

namespace orc {
namespace ql {

// the shape a light sits on (a DiffuseAreaLight whose primitive is a Sphere, a Disk or a Cylinder); mesh 0: a triangle or no area light
static inline ::QlShape light_shape(const rspt_scene_desc& d, const rspt_light& lt) {
    if (lt.kind != RSPT_LIGHT_DIFFUSE_AREA) return ::QlShape{0u, nullptr};
    const rspt_prim& pr = d.prims[lt.prim];
    if (pr.mesh == RSPT_MESH_SPHERE) return ::QlShape{pr.mesh, &d.spheres[pr.v[0]]};
    if (pr.mesh == RSPT_MESH_DISK) return ::QlShape{pr.mesh, &d.disks[pr.v[0]]};
    if (pr.mesh == RSPT_MESH_CYLINDER) return ::QlShape{pr.mesh, &d.cylinders[pr.v[0]]};
    return ::QlShape{0u, nullptr};
}
// Light::sample_li dispatching on the light's primitive
static inline Spec sample_li(const Scene& sc, const rspt_light& lt, const Interaction& iref, P2 u, V3* wi, Float* pdf, Interaction* light_intr) {
    const ::QlShape q = light_shape(sc.d, lt);
    if (!q.rec) return light_sample_li(sc, lt, iref, u, wi, pdf, light_intr);
    ::SlIntr li;
    ::V w{0.0f, 0.0f, 0.0f};
    const bool lit = ::ql_light_sample(q, lt.two_sided != 0, sl::ref_of(iref), u.x, u.y, &w, pdf, &li);
    Interaction r;   // InteractionCommon { p, p_error, n, ..Default::default() }
    r.p = sl::tov3(li.p); r.p_error = sl::tov3(li.p_error); r.n = sl::tov3(li.n); r.wo = V3{0, 0, 0}; r.time = 0;
    *light_intr = r;
    if (*pdf == 0.0f) return Spec();   // (diffuse.rs:76-79: wi is left as it was)
    *wi = sl::tov3(w);
    return lit ? S3(lt.L) : Spec(0.0f);
}
// Light::pdf_li of an area light (diffuse.rs:100-103)
static inline Float pdf_li(const Scene& sc, const rspt_light& lt, const Interaction& iref, V3 wi) {
    const ::QlShape q = light_shape(sc.d, lt);
    if (!q.rec) return sc.tri_pdf_ref(sc.d.prims[lt.prim], iref, wi);
    return ::ql_pdf_ref(q, sl::ref_of(iref), sl::tov(wi));
}
// Light::power (diffuse.rs:85-93 with area = shape.area())
static inline Spec power(const Scene& sc, const rspt_light& lt) {
    const ::QlShape q = light_shape(sc.d, lt);
    if (!q.rec) return light_power(sc, lt);
    const Float factor = lt.two_sided ? 2.0f : 1.0f;
    return S3(lt.L) * factor * ::ql_area(q) * PI;
}

// One render's (or one query's) light distributions: sl::Dist (tests/spherelight_restated.cpp) stated again over sample_li / power above
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
        if (strategy == RSPT_LIGHTS_UNIFORM || nl == 1) {   // lightdistrib.rs:397
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

}  // namespace ql
}  // namespace orc

extern "C" {
// The light distribution of (scene, strategy) at p, as rspt_light_distribution reports it: func[n_lights], cdf[n_lights + 1], the grid and p's voxel
int ql_light_distribution(const rspt_scene_desc* sd, uint32_t strategy, const float p[3], float* func_out, float* cdf_out, int32_t nvox_out[3], int32_t voxel_out[3]) {
    if (!sd || !sd->n_lights) return -1;
    orc::Scene sc{*sd};
    orc::ql::Dist v(&sc, strategy);
    int vox[3] = {0, 0, 0};
    const orc::Distribution1D* d = v.lookup(orc::V3{p[0], p[1], p[2]}, vox);
    std::memcpy(func_out, d->func.data(), d->func.size() * sizeof(float));
    std::memcpy(cdf_out, d->cdf.data(), d->cdf.size() * sizeof(float));
    for (int i = 0; i < 3; i++) { nvox_out[i] = v.n_voxels[i]; voxel_out[i] = vox[i]; }
    return 0;
}
}
