// Test helper (compiled by tests/test_quadriclight_host.py and tests/test_gpu_quadric_lights.py with g++ into a temporary directory): PathIntegrator::li
// (src/integrators/path.rs:59-282) and uniform_sample_one_light / estimate_direct (src/core/integrator.rs:359-570) restated over a scene whose disks,
// cylinders and spheres may emit: the two light calls of estimate_direct (Light::sample_li, Light::pdf_li) and Light::power dispatch on the light's
// primitive (tests/quadriclight_restated.cpp), the light distributions are built over those, and intersect / intersect_p / AOIntegrator::li are those of
// tests/quadric_render_restated.cpp.  Run through the oracle's tile loop (sampler, camera, film).  Where no quadric emits, every call lands in the oracle's
// own light functions and the result equals quadric_render_restated.cpp's bit for bit; on a sphere scene whose spheres emit it equals
// spherelight_render_restated.cpp's (tests/test_quadriclight_host.py holds both).
// f32 throughout with the host libm; build with -ffp-contract=off.
#include "quadric_render_restated.cpp"
#define RSPT_SPHERELIGHT_NO_BASE
#include "spherelight_restated.cpp"
#define RSPT_QUADRICLIGHT_NO_BASE
#include "quadriclight_restated.cpp"

namespace orc {
namespace qlr {

static ql::Dist* g_dist = nullptr;   // the distributions of the render under way (orc::render hands li no user pointer)

// integrator.rs:407-570
static Spec estimate_direct(RenderCtx& cx, const Interaction& it, const Bsdf& bsdf, P2 u_scattering, uint32_t light_num, P2 u_light, Counters* c) {
    const Scene& sc = *cx.scene;
    const rspt_light& light = sc.d.lights[light_num];
    const uint8_t bsdf_flags = BSDF_ALL & ~BSDF_SPECULAR;   // :416-420
    Spec ld(0.0f);
    V3 wi{0, 0, 0};
    Float light_pdf = 0.0f, scattering_pdf = 0.0f;
    Interaction light_intr;
    Spec li = ql::sample_li(sc, light, it, u_light, &wi, &light_pdf, &light_intr);   // :424-432
    if (light_pdf > 0.0f && !li.is_black()) {
        Spec f = bsdf.f(it.wo, wi, bsdf_flags) * Spec(abs_dot(wi, it.sh_n));   // :437-443
        scattering_pdf = bsdf.pdf(it.wo, wi, bsdf_flags);
        if (!f.is_black()) {
            if (quadr::intersect_p(sc, it.spawn_ray_to(light_intr), c)) li = Spec(0.0f);   // VisibilityTester::unoccluded (light.rs:199-206), :456-466
            if (!li.is_black()) {
                if (light_is_delta(light)) ld = ld + f * li / light_pdf;   // :470-471
                else ld = ld + f * li * Spec(power_heuristic(1, light_pdf, 1, scattering_pdf)) / light_pdf;   // :472-476
            }
        }
    }
    if (!light_is_delta(light)) {   // :480
        uint8_t sampled_type = 0;
        Spec f = bsdf.sample_f(it.wo, &wi, u_scattering, &scattering_pdf, bsdf_flags, &sampled_type);   // :486-499
        f = f * Spec(abs_dot(wi, it.sh_n));
        const bool sampled_specular = (sampled_type & BSDF_SPECULAR) != 0;
        if (!f.is_black() && scattering_pdf > 0.0f) {
            Float weight = 1.0f;
            if (!sampled_specular) {   // :520-528
                light_pdf = light.kind == RSPT_LIGHT_INFINITE ? infinite_pdf_li(sc, light, wi) : ql::pdf_li(sc, light, it, wi);
                if (light_pdf == 0.0f) return ld;
                weight = power_heuristic(1, scattering_pdf, 1, light_pdf);
            }
            const Ray ray = it.spawn_ray(wi);   // :530-548
            Spec li2;
            Interaction light_isect;
            if (quadr::intersect(sc, ray, &light_isect, c)) {
                const rspt_prim& hp = sc.d.prims[light_isect.prim];
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
static Spec uniform_sample_one_light(RenderCtx& cx, const Interaction& it, const Bsdf& bsdf, Sampler& sampler, const Distribution1D& distrib, Counters* c) {
    if (cx.scene->d.n_lights == 0) return Spec();
    Float pdf = 0.0f;
    const size_t light_num = distrib.sample_discrete(sampler.get_1d(), &pdf);
    if (pdf == 0.0f) return Spec();
    const P2 u_light = sampler.get_2d();
    const P2 u_scattering = sampler.get_2d();
    return qlr::estimate_direct(cx, it, bsdf, u_scattering, (uint32_t)light_num, u_light, c) / pdf;
}

// path.rs:59-282
static Spec path_li(RenderCtx& cx, const Ray& r, Sampler& sampler, Counters* c) {
    const Scene& sc = *cx.scene;
    Spec l, beta(1.0f);
    Ray ray = r;
    bool specular_bounce = false;
    uint32_t bounces = 0;
    Float eta_scale = 1.0f;
    for (;;) {
        Interaction isect;
        if (quadr::intersect(sc, ray, &isect, c)) {   // :77-81
            const rspt_prim& hp = sc.d.prims[isect.prim];
            if (bounces == 0 || specular_bounce) {   // :97-101, SurfaceInteraction::le (interaction.rs:475-483)
                if (hp.area_light >= 0) l = l + beta * light_l(sc.d.lights[hp.area_light], isect.n, -ray.d);
                else l = l + beta * Spec();
            }
            if (bounces >= cx.rd->max_depth) break;   // :103-105
            if (hp.material == 0xffffffffu) { ray = isect.spawn_ray(ray.d); continue; }   // :109-116
            compute_differentials(&isect, ray);   // compute_scattering_functions (interaction.rs:371-386)
            Bsdf bsdf;
            make_bsdf(sc, isect, hp.material, true, &bsdf);   // :108
            const Distribution1D* distrib = sc.d.n_lights ? g_dist->lookup(isect.p) : nullptr;   // :118
            if (sc.d.n_lights && bsdf.num_components(BSDF_ALL & ~BSDF_SPECULAR) > 0)   // :120-139
                l = l + beta * qlr::uniform_sample_one_light(cx, isect, bsdf, sampler, *distrib, c);
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
                for (uint32_t i = 0; i < sc.d.n_lights; i++)
                    if (sc.d.lights[i].kind == RSPT_LIGHT_INFINITE) l = l + beta * infinite_le(sc, sc.d.lights[i], ray.d);
            break;
        }
        bounces += 1;
    }
    return l;
}

}  // namespace qlr
}  // namespace orc

extern "C" {
// orc::render with the path's li replaced by the restatement above and ao's by quadric_render_restated.cpp's; film_xyzw (npix, 4) and li_rgb (npix * spp * 3)
// as orc_render fills them
int qlr_render(const rspt_scene_desc* sd, const rspt_render_desc* rd, int num_threads, float* film_xyzw, float* li_rgb) {
    if (!sd || !rd) return -1;
    orc::Scene sc{*sd};
    orc::ql::Dist dist(&sc, rd->light_strategy);
    orc::qlr::g_dist = &dist;
    orc::g_li_override = orc::qlr::path_li;
    orc::g_ao_li_override = orc::quadr::ao_li;
    // the oracle's own tables are never looked up (path_li above reads `dist`), and its power table would take a quadric light's primitive for a triangle:
    // its setup is given the uniform strategy, which calls no light function
    rspt_render_desc rdu = *rd;
    rdu.light_strategy = RSPT_LIGHTS_UNIFORM;
    orc::RenderOut out;
    orc::render(sc, rdu, num_threads, film_xyzw, li_rgb, &out);
    orc::g_li_override = nullptr;
    orc::g_ao_li_override = nullptr;
    orc::qlr::g_dist = nullptr;
    return 0;
}
}
