// Test helper (compiled by tests/test_maplight_host.py and tests/test_gpu_maplights.py with g++ into a temporary directory): a hand restatement,
// written from the reference's text, of ProjectionLight::{projection, sample_li, power} (src/lights/projection.rs:339-398) and
// GonioPhotometricLight::{scale, sample_li, power} (src/lights/goniometric.rs:233-280), and over them of estimate_direct / uniform_sample_one_light
// (src/core/integrator.rs:359-570), PathIntegrator::li (src/integrators/path.rs:59-282) and the three light distributions the path needs
// (src/core/lightdistrib.rs:127-418) — the oracle knows neither light kind, so its own tables cannot serve.  light_sample_li below takes the two
// new kinds itself and hands every other kind to the oracle's.  The oracle keeps its tile loop, sampler, camera, film, BSDFs and traversal: its
// Scene is built from a copy of the description in which every projection / goniometric light is replaced, in place, by a black point light (the
// light indices of the emissive primitives stay valid and nothing of the oracle's reads kinds it does not know); the real list is kept beside it.
// f32 throughout with the host libm; build with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "orc_render.hpp"

namespace orc {
namespace ml {

static inline bool is_map_light(const rspt_light& lt) { return lt.kind == RSPT_LIGHT_PROJECTION || lt.kind == RSPT_LIGHT_GONIOMETRIC; }

// Transform::transform_point (transform.rs:490-517) with light_projection.m: the matrix Transform::perspective builds (:461-489) is
// scale(s, s, 1) * persp, whose product (mtx_mul, :238-249) has m[0][0], m[1][1], m[2][2], m[2][3] from the record, m[3][2] = 1 and +0 elsewhere
static inline V3 projection_point(const rspt_light& lt, V3 p) {
    const Float m[4][4] = {{lt.p[18], 0.0f, 0.0f, 0.0f}, {0.0f, lt.p[19], 0.0f, 0.0f}, {0.0f, 0.0f, lt.p[20], lt.p[21]}, {0.0f, 0.0f, 1.0f, 0.0f}};
    const Float x = p.x, y = p.y, z = p.z;
    const Float xp = m[0][0] * x + m[0][1] * y + m[0][2] * z + m[0][3];
    const Float yp = m[1][0] * x + m[1][1] * y + m[1][2] * z + m[1][3];
    const Float zp = m[2][0] * x + m[2][1] * y + m[2][2] * z + m[2][3];
    const Float wp = m[3][0] * x + m[3][1] * y + m[3][2] * z + m[3][3];
    if (wp == 1.0f) return V3{xp, yp, zp};   // :503-508
    const Float inv = 1.0f / wp;             // :510-515
    return V3{inv * xp, inv * yp, inv * zp};
}
// ProjectionLight::projection (projection.rs:339-360)
static inline Spec projection(const rspt_scene_desc& d, const rspt_light& lt, V3 w) {
    const V3 wl = mat3_mul(lt.p + 3, w);               // :340 world_to_light.transform_vector (transform.rs:518-527)
    if (wl.z < lt.p[16]) return Spec(0.0f);            // :342-344
    const V3 p = projection_point(lt, wl);             // :346-350
    const Float x0 = lt.p[12], y0 = lt.p[13], x1 = lt.p[14], y1 = lt.p[15];
    if (!(p.x >= x0 && p.x <= x1 && p.y >= y0 && p.y <= y1)) return Spec(0.0f);   // :351-353, pnt2_inside_bnd2f (geometry.rs:990-992)
    if (lt.prim == 0xffffffffu) return Spec(1.0f);     // :357-359
    P2 st{p.x - x0, p.y - y0};                         // :355 Bounds2f::offset (geometry.rs:1891-1900)
    if (x1 > x0) st.x /= x1 - x0;
    if (y1 > y0) st.y /= y1 - y0;
    return env_lookup(d.envmaps[lt.prim], st, 0.0f);   // :356
}
// GonioPhotometricLight::scale (goniometric.rs:233-247)
static inline Spec scale(const rspt_scene_desc& d, const rspt_light& lt, V3 w) {
    V3 wp = normalize(mat3_mul(lt.p + 3, w));          // :234
    std::swap(wp.y, wp.z);                             // :235
    const Float theta = spherical_theta(wp);           // :236
    const Float phi = spherical_phi(wp);               // :237
    if (lt.prim == 0xffffffffu) return Spec(1.0f);     // :244-246
    return env_lookup(d.envmaps[lt.prim], P2{phi * INV_2_PI, theta * INV_PI}, 0.0f);   // :239-243
}
// ProjectionLight::sample_li (projection.rs:362-378), GonioPhotometricLight::sample_li (goniometric.rs:249-265)
static inline Spec map_sample_li(const rspt_scene_desc& d, const rspt_light& lt, const Interaction& iref, V3* wi, Float* pdf, Interaction* light_intr) {
    const V3 pl{lt.p[0], lt.p[1], lt.p[2]};
    *wi = normalize(pl - iref.p);
    *pdf = 1.0f;
    Interaction li;   // InteractionCommon::default(): n = 0, p_error = 0
    li.p_error = V3{0, 0, 0}; li.n = V3{0, 0, 0}; li.wo = V3{0, 0, 0}; li.time = iref.time;
    li.p = pl;
    *light_intr = li;
    const Spec m = lt.kind == RSPT_LIGHT_PROJECTION ? projection(d, lt, -*wi) : scale(d, lt, -*wi);
    return S3(lt.L) * m / distance_squared(pl, iref.p);
}
// ProjectionLight::power (projection.rs:379-398), GonioPhotometricLight::power (goniometric.rs:266-280)
static inline Spec map_power(const rspt_scene_desc& d, const rspt_light& lt) {
    const Spec m = lt.prim == 0xffffffffu ? Spec(1.0f) : env_lookup(d.envmaps[lt.prim], P2{0.5f, 0.5f}, 0.5f);
    if (lt.kind == RSPT_LIGHT_GONIOMETRIC) return m * S3(lt.L) * 4.0f * PI;
    return m * S3(lt.L) * 2.0f * PI * (1.0f - lt.p[17]);
}

// One render's (or one query's) view: the real description, the oracle's Scene over the copy, the light distributions of the real list
struct View {
    const rspt_scene_desc* real;
    std::vector<rspt_light> masked;
    std::unique_ptr<Scene> scene;
    int strategy = RSPT_LIGHTS_SPATIAL;
    std::unique_ptr<Distribution1D> fixed;
    int n_voxels[3] = {1, 1, 1};
    std::mutex mu;
    std::map<size_t, std::unique_ptr<Distribution1D>> voxels;   // the reference's hash table is a cache and changes no value (lightdistrib.rs:297-384)

    explicit View(const rspt_scene_desc* sd) : real(sd) {
        masked.assign(sd->lights, sd->lights + sd->n_lights);
        for (rspt_light& l : masked)
            if (is_map_light(l)) { const float px = l.p[0], py = l.p[1], pz = l.p[2]; l = rspt_light{}; l.kind = RSPT_LIGHT_POINT; l.p[0] = px; l.p[1] = py; l.p[2] = pz; }
        rspt_scene_desc copy = *sd;
        copy.lights = masked.data();
        scene.reset(new Scene{copy});
    }
    const rspt_light& light(uint32_t i) const { return real->lights[i]; }
    uint32_t n_lights() const { return real->n_lights; }
    Spec sample_li(const rspt_light& lt, const Interaction& iref, P2 u, V3* wi, Float* pdf, Interaction* light_intr) const {
        if (is_map_light(lt)) return map_sample_li(*real, lt, iref, wi, pdf, light_intr);
        return light_sample_li(*scene, lt, iref, u, wi, pdf, light_intr);
    }
    static bool is_delta(const rspt_light& lt) { return is_map_light(lt) || light_is_delta(lt); }   // LightFlags::DeltaPosition (projection.rs:189, goniometric.rs:140)
    Spec power(const rspt_light& lt) const { return is_map_light(lt) ? map_power(*real, lt) : light_power(*scene, lt); }

    // create_light_sample_distribution (lightdistrib.rs:393-418), SpatialLightDistribution::new (:127-166)
    void init_distributions(uint32_t light_strategy) {
        const uint32_t nl = n_lights();
        strategy = (int)light_strategy;
        if (strategy == RSPT_LIGHTS_UNIFORM || nl == 1) {   // :397
            strategy = RSPT_LIGHTS_UNIFORM;
            fixed.reset(new Distribution1D(std::vector<Float>(nl, 1.0f)));
        } else if (strategy == RSPT_LIGHTS_POWER) {
            std::vector<Float> pw;
            for (uint32_t i = 0; i < nl; i++) pw.push_back(power(light(i)).y());   // integrator.rs:573-584
            fixed.reset(new Distribution1D(pw));
        } else {
            strategy = RSPT_LIGHTS_SPATIAL;
            const Bounds3 b = scene->world_bound();
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
        const uint32_t nl = n_lights();
        std::vector<Float> contrib(nl, 0.0f);
        for (size_t i = 0; i < n_samples; i++) {   // :198-247
            const V3 po = vb.lerp3(V3{radical_inverse(0, i), radical_inverse(1, i), radical_inverse(2, i)});
            Interaction intr; intr.p = po; intr.time = 0; intr.p_error = V3{0, 0, 0}; intr.wo = V3{1, 0, 0}; intr.n = V3{0, 0, 0};
            const P2 u{radical_inverse(3, i), radical_inverse(4, i)};
            for (uint32_t j = 0; j < nl; j++) {
                Float pdf = 0; V3 wi{0, 0, 0}; Interaction li_intr;
                const Spec li = sample_li(light(j), intr, u, &wi, &pdf, &li_intr);
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
static View* g_view = nullptr;   // the view of the render under way (orc::render hands li no user pointer)

// integrator.rs:407-570
static Spec estimate_direct(View& v, const Interaction& it, const Bsdf& bsdf, P2 u_scattering, uint32_t light_num, P2 u_light, Counters* c) {
    const Scene& sc = *v.scene;
    const rspt_light& light = v.light(light_num);
    const uint8_t bsdf_flags = BSDF_ALL & ~BSDF_SPECULAR;   // :416-420
    Spec ld(0.0f);
    V3 wi{0, 0, 0};
    Float light_pdf = 0.0f, scattering_pdf = 0.0f;
    Interaction light_intr;
    Spec li = v.sample_li(light, it, u_light, &wi, &light_pdf, &light_intr);   // :424-432
    if (light_pdf > 0.0f && !li.is_black()) {
        Spec f = bsdf.f(it.wo, wi, bsdf_flags) * Spec(abs_dot(wi, it.sh_n));   // :437-443
        scattering_pdf = bsdf.pdf(it.wo, wi, bsdf_flags);
        if (!f.is_black()) {
            if (sc.intersect_p(it.spawn_ray_to(light_intr), c)) li = Spec(0.0f);   // VisibilityTester::unoccluded (light.rs:199-206), :456-466
            if (!li.is_black()) {
                if (View::is_delta(light)) ld = ld + f * li / light_pdf;   // :470-471
                else ld = ld + f * li * Spec(power_heuristic(1, light_pdf, 1, scattering_pdf)) / light_pdf;   // :472-476
            }
        }
    }
    if (!View::is_delta(light)) {   // :480
        uint8_t sampled_type = 0;
        Spec f = bsdf.sample_f(it.wo, &wi, u_scattering, &scattering_pdf, bsdf_flags, &sampled_type);   // :486-499
        f = f * Spec(abs_dot(wi, it.sh_n));
        const bool sampled_specular = (sampled_type & BSDF_SPECULAR) != 0;
        if (!f.is_black() && scattering_pdf > 0.0f) {
            Float weight = 1.0f;
            if (!sampled_specular) {   // :520-528
                light_pdf = light.kind == RSPT_LIGHT_INFINITE ? infinite_pdf_li(sc, light, wi) : sc.tri_pdf_ref(sc.d.prims[light.prim], it, wi);
                if (light_pdf == 0.0f) return ld;
                weight = power_heuristic(1, scattering_pdf, 1, light_pdf);
            }
            const Ray ray = it.spawn_ray(wi);   // :530-548
            Spec li2;
            Interaction light_isect;
            if (sc.intersect(ray, &light_isect, c)) {
                const rspt_prim& hp = sc.hit_prim(light_isect);   // (a hit inside an instance under the reference behaviour has lost its primitive: no material, no area light)
                if (light.kind == RSPT_LIGHT_DIFFUSE_AREA && hp.area_light >= 0 && (uint32_t)hp.area_light == light_num)   // :550-558
                    li2 = light_l(light, light_isect.n, -wi);
            } else
                li2 = light.kind == RSPT_LIGHT_INFINITE ? infinite_le(sc, light, ray.d) : Spec();   // :561-563
            if (!li2.is_black()) ld = ld + f * li2 * Spec(1.0f) * weight / scattering_pdf;   // :564-566
        }
    }
    return ld;
}
// integrator.rs:359-403
static Spec uniform_sample_one_light(View& v, const Interaction& it, const Bsdf& bsdf, Sampler& sampler, const Distribution1D& distrib, Counters* c) {
    if (v.n_lights() == 0) return Spec();
    Float pdf = 0.0f;
    const size_t light_num = distrib.sample_discrete(sampler.get_1d(), &pdf);
    if (pdf == 0.0f) return Spec();
    const P2 u_light = sampler.get_2d();
    const P2 u_scattering = sampler.get_2d();
    return ml::estimate_direct(v, it, bsdf, u_scattering, (uint32_t)light_num, u_light, c) / pdf;
}

// path.rs:59-282
static Spec path_li(RenderCtx& cx, const Ray& r, Sampler& sampler, Counters* c) {
    View& v = *g_view;
    const Scene& sc = *v.scene;
    Spec l, beta(1.0f);
    Ray ray = r;
    bool specular_bounce = false;
    uint32_t bounces = 0;
    Float eta_scale = 1.0f;
    for (;;) {
        Interaction isect;
        if (sc.intersect(ray, &isect, c)) {   // :77-81
            const rspt_prim& hp = sc.hit_prim(isect);
            if (bounces == 0 || specular_bounce) {   // :97-101, SurfaceInteraction::le (interaction.rs:475-483)
                if (hp.area_light >= 0) l = l + beta * light_l(v.light(hp.area_light), isect.n, -ray.d);
                else l = l + beta * Spec();
            }
            if (bounces >= cx.rd->max_depth) break;   // :103-105
            if (hp.material == 0xffffffffu) { ray = isect.spawn_ray(ray.d); continue; }   // :109-116
            compute_differentials(&isect, ray);   // compute_scattering_functions (interaction.rs:371-386)
            Bsdf bsdf;
            make_bsdf(sc, isect, hp.material, true, &bsdf);   // :108
            const Distribution1D* distrib = v.n_lights() ? v.lookup(isect.p) : nullptr;   // :118
            if (v.n_lights() && bsdf.num_components(BSDF_ALL & ~BSDF_SPECULAR) > 0)   // :120-139
                l = l + beta * ml::uniform_sample_one_light(v, isect, bsdf, sampler, *distrib, c);
            const V3 wo = -ray.d;   // :141-150
            V3 wi{0, 0, 0};
            Float pdf = 0.0f;
            uint8_t sampled_type = 255;
            const Spec f = bsdf.sample_f(wo, &wi, sampler.get_2d(), &pdf, BSDF_ALL, &sampled_type);
            if (f.is_black() || pdf == 0.0f) break;   // :151-153
            beta = beta * ((f * abs_dot(wi, isect.sh_n)) / pdf);   // :154
            specular_bounce = (sampled_type & BSDF_SPECULAR) != 0;   // :157-158
            if ((sampled_type & BSDF_SPECULAR) && (sampled_type & BSDF_TRANSMISSION)) {   // :159-166
                const Float eta = bsdf.eta;
                if (dot(wo, isect.n) > 0.0f) eta_scale *= eta * eta;
                else eta_scale *= 1.0f / (eta * eta);
            }
            ray = isect.spawn_ray(wi);   // :167
            const Spec rr_beta = beta * eta_scale;   // :251-262
            if (rr_beta.max_component_value() < cx.rd->rr_threshold && bounces > 3) {
                const Float q = std::fmax(0.05f, 1.0f - rr_beta.max_component_value());
                if (sampler.get_1d() < q) break;
                beta = beta / (1.0f - q);
            }
        } else {   // :267-277: the infinite lights in Scene.lights order
            if (bounces == 0 || specular_bounce)
                for (uint32_t i = 0; i < v.n_lights(); i++)
                    if (v.light(i).kind == RSPT_LIGHT_INFINITE) l = l + beta * infinite_le(sc, v.light(i), ray.d);
            break;
        }
        bounces += 1;
    }
    return l;
}

}  // namespace ml
}  // namespace orc

extern "C" {
// orc::render with the path's li replaced by the restatement above; film_xyzw (npix, 4) and li_rgb (npix * spp * 3) as orc_render fills them.
// Every other integrator of the description keeps the oracle's own li (ao reads no lights).
int ml_render(const rspt_scene_desc* sd, const rspt_render_desc* rd, int num_threads, float* film_xyzw, float* li_rgb) {
    if (!sd || !rd) return -1;
    orc::ml::View v(sd);
    v.init_distributions(rd->light_strategy);
    orc::ml::g_view = &v;
    orc::g_li_override = orc::ml::path_li;
    orc::RenderOut out;
    orc::render(*v.scene, *rd, num_threads, film_xyzw, li_rgb, &out);
    orc::g_li_override = nullptr;
    orc::ml::g_view = nullptr;
    return 0;
}
// ProjectionLight::projection(w) (kind 6) / GonioPhotometricLight::scale(w) (kind 7) of light `index`
int ml_map(const rspt_scene_desc* sd, uint32_t index, const float w[3], float out[3]) {
    if (!sd || index >= sd->n_lights || !orc::ml::is_map_light(sd->lights[index])) return -1;
    const rspt_light& lt = sd->lights[index];
    const orc::V3 wv{w[0], w[1], w[2]};
    const orc::Spec s = lt.kind == RSPT_LIGHT_PROJECTION ? orc::ml::projection(*sd, lt, wv) : orc::ml::scale(*sd, lt, wv);
    out[0] = s.c[0]; out[1] = s.c[1]; out[2] = s.c[2];
    return 0;
}
// sample_li of light `index` at the reference point p: out = li (3), wi (3), pdf, the light point (3)
int ml_sample_li(const rspt_scene_desc* sd, uint32_t index, const float p[3], float out[10]) {
    if (!sd || index >= sd->n_lights || !orc::ml::is_map_light(sd->lights[index])) return -1;
    orc::Interaction iref, li;
    iref.p = orc::V3{p[0], p[1], p[2]}; iref.time = 0;
    orc::V3 wi{0, 0, 0};
    orc::Float pdf = 0;
    const orc::Spec s = orc::ml::map_sample_li(*sd, sd->lights[index], iref, &wi, &pdf, &li);
    const float r[10] = {s.c[0], s.c[1], s.c[2], wi.x, wi.y, wi.z, pdf, li.p.x, li.p.y, li.p.z};
    std::memcpy(out, r, sizeof r);
    return 0;
}
// ml_map / ml_sample_li over n directions / reference points (tests/test_reference_light_functions.py runs 2^17 of them): w, p n x 3; out n x 3 / n x 10
int ml_map_n(const rspt_scene_desc* sd, uint32_t index, const float* w, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; i++)
        if (ml_map(sd, index, w + 3 * i, out + 3 * i) != 0) return -1;
    return 0;
}
int ml_sample_li_n(const rspt_scene_desc* sd, uint32_t index, const float* p, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; i++)
        if (ml_sample_li(sd, index, p + 3 * i, out + 10 * i) != 0) return -1;
    return 0;
}
// The light distribution of (scene, strategy) at p, as rspt_light_distribution reports it: func[n_lights], cdf[n_lights + 1], the grid and p's voxel
int ml_light_distribution(const rspt_scene_desc* sd, uint32_t strategy, const float p[3], float* func_out, float* cdf_out, int32_t nvox_out[3], int32_t voxel_out[3]) {
    if (!sd || !sd->n_lights) return -1;
    orc::ml::View v(sd);
    v.init_distributions(strategy);
    int vox[3] = {0, 0, 0};
    const orc::Distribution1D* d = v.lookup(orc::V3{p[0], p[1], p[2]}, vox);
    std::memcpy(func_out, d->func.data(), d->func.size() * sizeof(float));
    std::memcpy(cdf_out, d->cdf.data(), d->cdf.size() * sizeof(float));
    for (int i = 0; i < 3; i++) { nvox_out[i] = v.n_voxels[i]; voxel_out[i] = vox[i]; }
    return 0;
}
}
